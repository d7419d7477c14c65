// Monte-Carlo audit (scp_audit_montecarlo_*): every problem is flown D times closed loop under the disturbance model of the
// covariance audit (audit_flight_one's montecarlo mode, audit_kernel.hpp; the draws of mc_rng.hpp), and the node errors are reduced
// ACROSS THE FLIGHTS, in registers, to per-node sample means and standard deviations.  Nothing of size N D B exists anywhere.
//
// Launch geometry.  One thread per (problem, flight), blocks of one wavefront like audit_tracking_kernel; a problem owns
// W = ceil(D / 64) WHOLE wavefronts: gid = (b W + w) 64 + lane flies d = 64 w + lane + 1.  Lanes with d > D fly flight D again: they
// stay in the loops, so that control flow at a node is uniform and every lane takes part in the cross-lane exchange, and are
// excluded from every sum, count and output.  Unsolved (masked) problems skip by whole wavefronts.
//
// Reduction at node k = 1 .. N.  Each lane holds e = x - xd[:,k] and, for k < N, du / Su.  A lane COUNTS at node k when it is a real
// flight and all of these are finite; a lane that does not count contributes +0.0.  The wavefront reduces NV = 1 + 2 nx + nu values:
// the count, sum e_i, sum e_i^2, sum (du_a / Su_a)^2 (0 at node N).
//
// The tree is FIXED: the butterfly v += xor_exchange(v, s) for s = 1, 2, 4, 8, 16, 32.  Addition is commutative, so both partners of
// an exchange compute the same bits and every lane ends with the same value: that of the balanced binary tree over the lanes
// 0 .. 63 -- ((l0 + l1) + (l2 + l3)) + ... -- which mc_tree64 repeats on the host.  Lane 0 writes the NV partials of the wavefront to
// part[NV, N, W, B]; mc_fold_kernel, one thread per (problem, node), adds the W partials IN WAVEFRONT ORDER from the first, and
// mc_moments_one turns the sums into the node's record of moments[NV, N, B]:
//   [0]            n_k, the flights counted
//   [1 .. nx]      the mean m_i = sum e_i / n_k
//   [nx+1 .. 2nx]  the standard deviation s_i = sqrt(max((sum e_i^2 - (sum e_i)^2 / n_k) / (n_k - 1), 0))
//   [2nx+1 ..]     the effort rms_a = sqrt(sum (du_a / Su_a)^2 / n_k); NaN at node N
// The errors are deviations from the nominal: their mean is of the order of their spread or below, so the one-pass formula loses
// no more than a digit or two to cancellation (it is the textbook formula applied to data that is already centred).  With n_k < 2
// the moments of that node are NaN.  mc_stat_one then folds the node records of a problem, in node order, into
// stat[SCP_MC_STAT_WIDTH] (include/scp_mi355x.h), and the flight records are folded by audit_dispersed_fold, marked 4.0.
// Neither output depends on the batch size, on the place of a problem in the batch or on anything but (the problem, D, seed).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/scp_mi355x.h"
#include "audit_kernel.hpp"
#include "mc_rng.hpp"

namespace scp {

struct McArgs {
    int B, N, steps, D, W;
    unsigned long long seed;
    double viol_tol;
    const double* xd;    // [nx,N,B]
    const double* ud;    // [nu,N,B]
    const double* p;     // [np,B]
    const double* pp;    // [npp,B]
    const double* Sx;    // [nx]
    const double* Su;    // [nu]
    const double* K;     // [nu,nx,N-1,B]
    const double* sig0;  // [nx]
    const double* sigu;  // [nu]
    const double* sigw;  // [nx]
    const int* mask;     // optional [B]
    double* flights;     // [SCP_AUDIT_WIDTH,D,B]
    double* audit;       // [SCP_AUDIT_WIDTH,B]
    double* part;        // [NV,N,W,B]
    double* moments;     // [NV,N,B]
    double* stat;        // [SCP_MC_STAT_WIDTH,B]
};

// mc_api.hip: mc_flight_kernel<M>, mc_fold_kernel and mc_stat_kernel on `stream`
int mc_launch(int model_id, const double* model_par, const McArgs& a, hipStream_t stream);

SCP_DEV constexpr int mc_nv(int nx, int nu) { return 1 + 2 * nx + nu; }

// what one flight contributes at a node: v[NV] = (1, e, e^2, (du / Su)^2), or all +0.0 when it does not count
template <int nx, int nu>
SCP_DEV void mc_node_values(const double (&e)[nx], const double (&dus)[nu], bool counts, double (&v)[1 + 2 * nx + nu])
{
    v[0] = counts ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) { v[1 + i] = counts ? e[i] : 0.0; v[1 + nx + i] = counts ? e[i] * e[i] : 0.0; }
#pragma unroll
    for (int a = 0; a < nu; a++) v[1 + 2 * nx + a] = counts ? dus[a] * dus[a] : 0.0;
}

// the tree of the header over the 64 lane values of one quantity (host twin); v is overwritten
inline double mc_tree64(double (&v)[64])
{
    for (int s = 1; s < 64; s *= 2)
        for (int i = 0; i < 64; i += 2 * s) v[i] = v[i] + v[i + s];
    return v[0];
}

// sums[NV] of ONE node over all flights -> rec[NV]
SCP_DEV void mc_moments_one(int nx, int nu, bool last_node, const double* sums, double* rec)
{
    const double n = sums[0];
    rec[0] = n;
    for (int i = 0; i < nx; i++) {
        const double s1 = sums[1 + i], s2 = sums[1 + nx + i];
        rec[1 + i] = n >= 2.0 ? s1 / n : NAN;
        rec[1 + nx + i] = n >= 2.0 ? sqrt(fmax((s2 - s1 * s1 / n) / (n - 1.0), 0.0)) : NAN;
    }
    for (int a = 0; a < nu; a++) rec[1 + 2 * nx + a] = (n >= 2.0 && !last_node) ? sqrt(sums[1 + 2 * nx + a] / n) : NAN;
}

// the node records mom[NV, N] of ONE problem, in node order -> stat[SCP_MC_STAT_WIDTH].  Strict comparisons from -Inf, the node
// loop outside the index loop: ties go to the smallest node, then the smallest index; NaN moments take no part.  A maximum that
// no node contributes to is NaN with the indices 0.
SCP_DEV void mc_stat_one(int nx, int nu, int N, const double* mom, const double* Sx, double* stat)
{
    const int nv = mc_nv(nx, nu);
    double smax = -INFINITY, ks = 0.0, is = 0.0, mmax = -INFINITY, km = 0.0, rmax = -INFINITY, kr = 0.0, nmin = INFINITY;
    for (int k = 0; k < N; k++) {
        const double* r = mom + (long)k * nv;
        if (r[0] < nmin) nmin = r[0];
        for (int i = 0; i < nx; i++) {
            const double s = r[1 + nx + i] / Sx[i], m = fabs(r[1 + i]) / Sx[i];
            if (s > smax) { smax = s; ks = (double)(k + 1); is = (double)(i + 1); }
            if (m > mmax) { mmax = m; km = (double)(k + 1); }
        }
        if (k < N - 1)
            for (int a = 0; a < nu; a++)
                if (r[1 + 2 * nx + a] > rmax) { rmax = r[1 + 2 * nx + a]; kr = (double)(k + 1); }
    }
    stat[0] = ks > 0.0 ? smax : NAN; stat[1] = ks; stat[2] = is;
    stat[3] = km > 0.0 ? mmax : NAN; stat[4] = km;
    stat[5] = kr > 0.0 ? rmax : NAN; stat[6] = kr;
    stat[7] = nmin;
}

// ---- the `mc` of audit_flight_one on the device: the draws' coordinates and the wavefront reduction at a node ----
template <int nx, int nu>
struct McWave {
    unsigned long long seed;
    int d;
    const double *sig0, *sigu, *sigw;
    bool real;          // d <= D before the clamp: the lane counts
    double* part;       // this wavefront's partials [NV, N]
    __device__ __forceinline__ void node(int k, int, const double (&e)[nx], const double (&dus)[nu], bool finite) const
    {
        constexpr int nv = 1 + 2 * nx + nu;
        double v[nv];
        mc_node_values<nx, nu>(e, dus, real && finite, v);
#pragma unroll
        for (int j = 0; j < nv; j++) {
#pragma unroll
            for (int s = 1; s < 64; s *= 2) v[j] = v[j] + __shfl_xor(v[j], s, 64);
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < nv; j++) part[(long)(k - 1) * nv + j] = v[j];
        }
    }
};

// one thread per (problem, flight), W whole wavefronts per problem
template <class M>
__global__ __launch_bounds__(64) void mc_flight_kernel(McArgs a, typename M::Params par)
{
    constexpr int nv = 1 + 2 * M::nx + M::nu;
    const long wave = blockIdx.x;                         // b W + w
    const int b = (int)(wave / a.W), w = (int)(wave % a.W);
    if (b >= a.B) return;
    const int d0 = 64 * w + (int)threadIdx.x + 1;
    const bool real = d0 <= a.D;
    const int d = real ? d0 : a.D;
    double* rec = a.flights + ((long)b * a.D + (d - 1)) * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {            // the whole wavefront: b is uniform
        if (real) {
#pragma unroll
            for (int i = 0; i < SCP_AUDIT_WIDTH; i++) rec[i] = NAN;
        }
        return;
    }
    McWave<M::nx, M::nu> mc{a.seed, d, a.sig0, a.sigu, a.sigw, real, a.part + wave * a.N * nv};
    double out[SCP_AUDIT_WIDTH];
    audit_flight_one<M, AuditFlight::montecarlo>(par, a.N, a.steps, a.viol_tol, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu,
                                                 a.p + (long)b * np_total<M>(a.N), a.pp + (long)b * M::npp, a.Sx, out, nullptr, nullptr,
                                                 nullptr, a.Su, a.K + (long)b * (a.N - 1) * M::nu * M::nx, mc);
    if (real) {
#pragma unroll
        for (int i = 0; i < SCP_AUDIT_WIDTH; i++) rec[i] = out[i];
    }
}

}  // namespace scp
