// The Monte-Carlo audit's own translation unit: the instantiations of mc_flight_kernel (one per auditable model, models/registry.hpp),
// the fold of the wavefront partials and the per-problem fold (mc_kernel.hpp), their launch for the handle-level entry points of
// audit_entry.hip, and the pure-host twins scp_model_audit_montecarlo_host and scp_mc_draws_host.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/scp_mi355x.h"
#include "audit_host.hpp"
#include "mc_kernel.hpp"
#include "models/registry.hpp"

namespace scp {

// one thread per (problem, node): the W partials in wavefront order -> the node's record of moments
__global__ __launch_bounds__(64) void mc_fold_kernel(McArgs a, int nx, int nu)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long)a.B * a.N) return;
    const int b = (int)(gid / a.N), k = (int)(gid % a.N), nv = mc_nv(nx, nu);
    double* rec = a.moments + gid * nv;
    if (a.mask != nullptr && a.mask[b] == 0) {
        for (int j = 0; j < nv; j++) rec[j] = NAN;
        return;
    }
    // the sums are built in place: rec is this thread's own
    for (int j = 0; j < nv; j++) {
        double s = a.part[(((long)b * a.W + 0) * a.N + k) * nv + j];
        for (int w = 1; w < a.W; w++) s += a.part[(((long)b * a.W + w) * a.N + k) * nv + j];
        rec[j] = s;
    }
    mc_moments_one(nx, nu, k == a.N - 1, rec, rec);
}

// one thread per problem: its node records in node order -> stat, its D flight records in flight order -> the summary, marked 4.0
__global__ __launch_bounds__(64) void mc_stat_kernel(McArgs a, int nx, int nu)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* out = a.audit + (long)b * SCP_AUDIT_WIDTH;
    double* stat = a.stat + (long)b * SCP_MC_STAT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) {
        nan_record<SCP_AUDIT_WIDTH>(out);
        nan_record<SCP_MC_STAT_WIDTH>(stat);
        return;
    }
    mc_stat_one(nx, nu, a.N, a.moments + (long)b * a.N * mc_nv(nx, nu), a.Sx, stat);
    audit_dispersed_fold(a.D, a.flights + (long)b * a.D * SCP_AUDIT_WIDTH, out, 4.0);
}

int mc_launch(int model_id, const double* model_par, const McArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        hipLaunchKernelGGL(mc_flight_kernel<M>, dim3((unsigned)((long)a.B * a.W)), dim3(64), 0, stream, a, M::make_params(model_par));
        if (const int rc = launch_rc()) return rc;
        hipLaunchKernelGGL(mc_fold_kernel, dim3((unsigned)(((long)a.B * a.N + 63) / 64)), dim3(64), 0, stream, a, M::nx, M::nu);
        if (const int rc = launch_rc()) return rc;
        hipLaunchKernelGGL(mc_stat_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, a, M::nx, M::nu);
        return launch_rc();
    });
}

// the `mc` of audit_flight_one in the host twin: the node values of one flight into its lane of the wavefront's table
template <int nx, int nu>
struct McHostLane {
    unsigned long long seed;
    int d;
    const double *sig0, *sigu, *sigw;
    double* table;      // [N, NV, 64] of the wavefront
    int lane;
    void node(int k, int, const double (&e)[nx], const double (&dus)[nu], bool finite) const
    {
        constexpr int nv = 1 + 2 * nx + nu;
        double v[nv];
        mc_node_values<nx, nu>(e, dus, finite, v);
        for (int j = 0; j < nv; j++) table[((size_t)(k - 1) * nv + j) * 64 + lane] = v[j];
    }
};

}  // namespace scp

extern "C" int scp_model_audit_montecarlo_host(int model_id, const double* model_par, int N, const double* xd, const double* ud,
                                               const double* p, const double* pp, const double* Sx, const double* Su, const double* K,
                                               int steps, double viol_tol, int D, uint64_t seed, const double* sig0, const double* sigu,
                                               const double* sigw, double* summary, double* stat, double* moments, double* flights)
{
    if (!model_par || N < 2 || !xd || !ud || !Sx || !Su || !K || !summary || !stat || steps < 1 || D < 2) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        constexpr int nx = M::nx, nu = M::nu, nv = 1 + 2 * nx + nu;
        if ((M::np > 0 && !p) || (M::npp > 0 && !pp)) return (int)SCP_ERR_BAD_ARGUMENT;
        if (!scp::audit_sigmas_ok(nx, nu, sig0, sigu, sigw)) return (int)SCP_ERR_BAD_ARGUMENT;
        const typename M::Params par = M::make_params(model_par);
        std::vector<double> own, own_mom, table((size_t)N * nv * 64), sums((size_t)N * nv, 0.0);
        if (!flights) { own.resize((size_t)SCP_AUDIT_WIDTH * D); flights = own.data(); }
        if (!moments) { own_mom.resize((size_t)N * nv); moments = own_mom.data(); }
        const int W = (D + 63) / 64;
        for (int w = 0; w < W; w++) {
            std::fill(table.begin(), table.end(), 0.0);      // the lanes beyond D contribute +0.0
            for (int lane = 0; lane < 64 && 64 * w + lane < D; lane++) {
                const int d = 64 * w + lane + 1;
                scp::McHostLane<nx, nu> mc{seed, d, sig0, sigu, sigw, table.data(), lane};
                scp::audit_flight_one<M, scp::AuditFlight::montecarlo>(par, N, steps, viol_tol, xd, ud, p, pp, Sx,
                                                                       flights + (size_t)(d - 1) * SCP_AUDIT_WIDTH, nullptr, nullptr, nullptr,
                                                                       Su, K, mc);
            }
            for (size_t q = 0; q < (size_t)N * nv; q++) {
                double v[64];
                for (int lane = 0; lane < 64; lane++) v[lane] = table[q * 64 + lane];
                const double part = scp::mc_tree64(v);
                sums[q] = w == 0 ? part : sums[q] + part;
            }
        }
        for (int k = 0; k < N; k++) scp::mc_moments_one(nx, nu, k == N - 1, sums.data() + (size_t)k * nv, moments + (size_t)k * nv);
        scp::mc_stat_one(nx, nu, N, moments, Sx, stat);
        scp::audit_dispersed_fold(D, flights, summary, 4.0);
        return (int)SCP_OK;
    });
}

extern "C" int scp_mc_draws_host(uint64_t seed, int kind, int k, int d, int n, double* z, unsigned* words)
{
    if (kind < 0 || kind > 2 || k < 0 || d < 1 || n < 1 || !z) return SCP_ERR_BAD_ARGUMENT;
    for (int q = 0; q < (n + 1) / 2; q++) {
        double pair[2];
        uint32_t w[4];
        scp::mc_normal_pair(seed, kind, k, d, q, pair, w);
        z[2 * q] = pair[0];
        if (2 * q + 1 < n) z[2 * q + 1] = pair[1];
        if (words)
            for (int j = 0; j < 4; j++) words[4 * q + j] = w[j];
    }
    return SCP_OK;
}
