// Time-varying discrete LQR gains on the discretisation of discretize! (scp_lqr_gains_*, include/scp_mi355x.h): per problem, with
// Q = diag(qx), R = diag(ru), P <- diag(qf), for k = N-1 down to 1
//     Phi = A_k, Gam = B-_k + B+_k;  H = R + Gam' P Gam;  K_k = H^-1 Gam' P Phi;  P <- Q + Phi' P (Phi - Gam K_k);  P <- (P + P') / 2
// A chain of N-1 dependent small dense steps: latency-bound like the horizon sweeps of K3, nothing to stream but A, B-, B+ once.
//
// Mapping.  One wavefront LANE per ENTRY of P (the four auditable models have nx^2 <= 64), floor(64 / nx^2) problems packed
// into a wavefront (16 double integrators, one of every other model).  A step is a sequence of PHASES; in a phase entry e computes
// ITS element of one or two small matrices from matrices earlier phases left in the work area (LDS on the device), and no phase
// reads an array it writes.  The device runs a phase on all lanes and then meets at a barrier (blocks of one wavefront); the host
// twin runs the same phase functions entry after entry.  Lqr<NX, NU>::chain is that one body.  What a lane computes depends on its
// problem's data and on its entry index only, so a problem's result is independent of B and of its place in the batch bit for bit.
//
// The nu x nu Cholesky factor (nu <= 4) is recomputed by each of the nu nx lanes of K in registers (compile-time indices only:
// no scratch); a lane then solves for its column of K and keeps its row.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/scp_mi355x.h"
#include "models/model_common.hpp"

namespace scp {

struct LqrArgs {
    int B, N;
    const double* A;    // [nx,nx,N-1,B]
    const double* Bm;   // [nx,nu,N-1,B]
    const double* Bp;   // [nx,nu,N-1,B]
    const double* qx;   // [nx]
    const double* ru;   // [nu]
    const double* qf;   // [nx]
    const int* mask;    // optional [B]: problems with mask[b] == 0 are skipped, their K and info are NaN
    double* K;          // [nu,nx,N-1,B]
    double* info;       // [SCP_LQR_INFO_WIDTH,B]
};

// lqr_api.hip: lqr_riccati_kernel<nx, nu> on `stream`; SCP_ERR_UNSUPPORTED for a pair that is not one of the four auditable models'
int lqr_launch(int nx, int nu, const LqrArgs& a, hipStream_t stream);
// qx[nx] >= 0, qf[nx] >= 0, ru[nu] > 0, all present and finite
bool lqr_weights_ok(int nx, int nu, const double* qx, const double* ru, const double* qf);

// the work area of ONE problem, column-major like the arrays of discretize!
template <int NX, int NU>
struct LqrWork {
    double P[NX * NX], Phi[NX * NX], S[NX * NX], W[NX * NX];   // S = P Phi, later the unsymmetrised new P; W = S - G K
    double Gam[NX * NU], G[NX * NU];                           // G = P Gam
    double Y[NU * NX], Kk[NU * NX], kmax[NU * NX];             // Y = Gam' S; K_k; per entry of K the running max |K_k|
    double H[NU * NU];
    int bad;                                                   // set by any entry that met a pivot <= 0 or a non-finite value
};

template <int NX, int NU>
struct Lqr {
    static constexpr int NP = NX * NX, NG = NX * NU, NH = NU * NU;
    static_assert(NP <= 64 && NG <= NP && NH <= NP && NU <= 4 && SCP_LQR_INFO_WIDTH <= NP, "one lane per entry of P carries every phase");
    using Work = LqrWork<NX, NU>;

    SCP_DEV static void init(Work& w, int e, const double* qf)
    {
        if (e < NP) w.P[e] = (e % NX == e / NX) ? qf[e % NX] : 0.0;
        if (e < NG) w.kmax[e] = 0.0;
        if (e == 0) w.bad = 0;
    }
    SCP_DEV static void load(Work& w, int e, const double* A, const double* Bm, const double* Bp)
    {
        if (e < NP) w.Phi[e] = A[e];
        if (e < NG) w.Gam[e] = Bm[e] + Bp[e];
    }
    // S = P Phi [nx,nx], G = P Gam [nx,nu]
    SCP_DEV static void p_times(Work& w, int e)
    {
        if (e < NP) {
            const int i = e % NX, j = e / NX;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.P[i + NX * m] * w.Phi[m + NX * j];
            w.S[e] = s;
        }
        if (e < NG) {
            const int i = e % NX, c = e / NX;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.P[i + NX * m] * w.Gam[m + NX * c];
            w.G[e] = s;
        }
    }
    // H = R + Gam' G [nu,nu], Y = Gam' S [nu,nx]
    SCP_DEV static void gam_t_times(Work& w, int e, const double* ru)
    {
        if (e < NH) {
            const int a = e % NU, c = e / NU;
            double s = a == c ? ru[a] : 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.Gam[m + NX * a] * w.G[m + NX * c];
            w.H[e] = s;
        }
        if (e < NG) {
            const int a = e % NU, j = e / NU;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.Gam[m + NX * a] * w.S[m + NX * j];
            w.Y[e] = s;
        }
    }
    // K_k = H^-1 Y by the Cholesky factor of H: entry (a, j) factors H, solves column j and keeps row a
    SCP_DEV static void gain(Work& w, int e, double* Kout)
    {
        if (e >= NG) return;
        const int a = e % NU, j = e / NU;
        bool bad = false;
        double L[NU][NU], y[NU], x[NU];
#pragma unroll
        for (int c = 0; c < NU; c++) {
            double d = w.H[c + NU * c];
#pragma unroll
            for (int m = 0; m < c; m++) d -= L[c][m] * L[c][m];
            bad = bad || !(d > 0.0) || !__builtin_isfinite(d);
            L[c][c] = sqrt(d);
#pragma unroll
            for (int r = c + 1; r < NU; r++) {
                double s = w.H[r + NU * c];
#pragma unroll
                for (int m = 0; m < c; m++) s -= L[r][m] * L[c][m];
                L[r][c] = s / L[c][c];
            }
        }
#pragma unroll
        for (int r = 0; r < NU; r++) {
            double s = w.Y[r + NU * j];
#pragma unroll
            for (int m = 0; m < r; m++) s -= L[r][m] * y[m];
            y[r] = s / L[r][r];
        }
#pragma unroll
        for (int r = NU - 1; r >= 0; r--) {
            double s = y[r];
#pragma unroll
            for (int m = r + 1; m < NU; m++) s -= L[m][r] * x[m];
            x[r] = s / L[r][r];
        }
        double kv = x[0];
#pragma unroll
        for (int r = 1; r < NU; r++) kv = r == a ? x[r] : kv;
        bad = bad || !__builtin_isfinite(kv);
        w.Kk[e] = kv;
        Kout[e] = kv;
        const double ak = fabs(kv);
        if (ak > w.kmax[e]) w.kmax[e] = ak;
        if (bad) w.bad = 1;
    }
    // W = S - G K_k [nx,nx]
    SCP_DEV static void closed(Work& w, int e)
    {
        if (e >= NP) return;
        const int m = e % NX, j = e / NX;
        double s = w.S[e];
#pragma unroll
        for (int a = 0; a < NU; a++) s -= w.G[m + NX * a] * w.Kk[a + NU * j];
        w.W[e] = s;
    }
    // S <- Q + Phi' W, the new P before it is symmetrised
    SCP_DEV static void phi_t_times(Work& w, int e, const double* qx)
    {
        if (e >= NP) return;
        const int i = e % NX, j = e / NX;
        double s = i == j ? qx[i] : 0.0;
#pragma unroll
        for (int m = 0; m < NX; m++) s += w.Phi[m + NX * i] * w.W[m + NX * j];
        w.S[e] = s;
    }
    SCP_DEV static void symmetrise(Work& w, int e)
    {
        if (e >= NP) return;
        const int i = e % NX, j = e / NX;
        const double v = 0.5 * (w.S[i + NX * j] + w.S[j + NX * i]);
        w.P[e] = v;
        if (!__builtin_isfinite(v)) w.bad = 1;
    }
    // a failed problem: NaN in every K_k; entry 0 writes the info record
    SCP_DEV static void finish(const Work& w, int e, int N, double* K, double* info)
    {
        const bool bad = w.bad != 0;
        if (e < NG && bad)
            for (int k = 0; k < N - 1; k++) K[(long)k * NG + e] = NAN;
        if (e == 0) {
            double kmax = 0.0, tr = 0.0;
#pragma unroll
            for (int i = 0; i < NG; i++) kmax = w.kmax[i] > kmax ? w.kmax[i] : kmax;
#pragma unroll
            for (int i = 0; i < NX; i++) tr += w.P[i + NX * i];
            info[0] = bad ? 1.0 : 0.0; info[1] = bad ? NAN : kmax; info[2] = bad ? NAN : tr; info[3] = 0.0;
        }
    }

    // A[nx,nx,N-1], Bm, Bp[nx,nu,N-1] of ONE problem -> K[nu,nx,N-1], info[SCP_LQR_INFO_WIDTH].  each(f) runs the phase f(e) for
    // every entry e and returns when all of them are done.
    template <class Each>
    SCP_DEV static void chain(Work& w, int N, const double* A, const double* Bm, const double* Bp, const double* qx, const double* ru,
                              const double* qf, double* K, double* info, Each&& each)
    {
        each([&](int e) { init(w, e, qf); });
        for (int k = N - 2; k >= 0; k--) {               // 0-based interval: K_{k+1} of the header
            const double *Ak = A + (long)k * NP, *Bmk = Bm + (long)k * NG, *Bpk = Bp + (long)k * NG;
            double* Kk = K + (long)k * NG;
            each([&](int e) { load(w, e, Ak, Bmk, Bpk); });
            each([&](int e) { p_times(w, e); });
            each([&](int e) { gam_t_times(w, e, ru); });
            each([&](int e) { gain(w, e, Kk); });
            each([&](int e) { closed(w, e); });
            each([&](int e) { phi_t_times(w, e, qx); });
            each([&](int e) { symmetrise(w, e); });
        }
        each([&](int e) { finish(w, e, N, K, info); });
    }
};

// blocks of one wavefront; lane = g * nx^2 + e: entry e of the block's g-th problem (lanes past the last packed problem idle
// but meet every barrier)
template <int NX, int NU>
__global__ __launch_bounds__(64) void lqr_riccati_kernel(LqrArgs a)
{
    using L = Lqr<NX, NU>;
    constexpr int NP = L::NP, NG = L::NG, PACK = 64 / NP;
    __shared__ LqrWork<NX, NU> work[PACK];
    const int g = threadIdx.x / NP, e = threadIdx.x % NP;
    const long b = (long)blockIdx.x * PACK + g;
    const bool mine = g < PACK && b < a.B;
    const bool live = mine && (a.mask == nullptr || a.mask[b] != 0);
    const long bb = mine ? b : 0;
    double* K = a.K + bb * (a.N - 1) * NG;
    double* info = a.info + bb * SCP_LQR_INFO_WIDTH;
    L::chain(work[g < PACK ? g : 0], a.N, a.A + bb * (a.N - 1) * NP, a.Bm + bb * (a.N - 1) * NG, a.Bp + bb * (a.N - 1) * NG, a.qx, a.ru,
             a.qf, K, info, [&](auto f) {
                 if (live) f(e);
                 __syncthreads();
             });
    if (mine && !live) {
        if (e < NG)
            for (int k = 0; k < a.N - 1; k++) K[(long)k * NG + e] = NAN;
        if (e < SCP_LQR_INFO_WIDTH) info[e] = NAN;
    }
}

}  // namespace scp
