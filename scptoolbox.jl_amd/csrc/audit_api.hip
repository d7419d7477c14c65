// The continuous-time audit's own translation unit: per auditable model (models/registry.hpp) the instantiations of audit_foh_kernel,
// of audit_interval_kernel (FOH, and IMPULSE where the model has it) with their fold, of audit_dispersed_kernel with its fold and of
// audit_tracking_kernel with its fold (audit_kernel.hpp), their launches for the handle-level entry points of audit_entry.hip, and the
// pure-host twins scp_model_audit_host, scp_model_audit_intervals_host, scp_model_audit_dispersed_host and
// scp_model_audit_tracking_host.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/scp_mi355x.h"
#include "audit_host.hpp"
#include "audit_kernel.hpp"
#include "models/registry.hpp"

namespace scp {

__global__ void audit_mask_kernel(const int* status, int* mask, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) mask[b] = status[b] == 0 ? 1 : 0;
}

int audit_mask_from_status(const int* status, int* mask, int B, hipStream_t stream)
{
    hipLaunchKernelGGL(audit_mask_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, status, mask, B);
    return launch_rc();
}

int audit_launch(int model_id, const double* model_par, const AuditArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        hipLaunchKernelGGL(audit_foh_kernel<M>, dim3((a.B + 63) / 64), dim3(64), 0, stream, a, M::make_params(model_par));
        return launch_rc();
    });
}

int audit_intervals_launch(int model_id, const double* model_par, int disc_method, const AuditIntervalArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        const typename M::Params par = M::make_params(model_par);
        const dim3 grid((unsigned)(((long)a.B * (a.N - 1) + 63) / 64)), block(64);
        if (disc_method == SCP_IMPULSE) {
            if constexpr (M::has_impulse) hipLaunchKernelGGL((audit_interval_kernel<M, true>), grid, block, 0, stream, a, par);
            else return (int)SCP_ERR_UNSUPPORTED;
        } else {
            hipLaunchKernelGGL((audit_interval_kernel<M, false>), grid, block, 0, stream, a, par);
        }
        if (const int rc = launch_rc()) return rc;
        hipLaunchKernelGGL(audit_interval_fold_kernel<M>, dim3((a.B + 63) / 64), block, 0, stream, a, par);
        return launch_rc();
    });
}

// one thread per problem: its D records in flight order -> the summary record (no model enters: the records carry everything)
__global__ __launch_bounds__(64) void audit_dispersed_fold_kernel(AuditDispersedArgs a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* out = a.audit + (long)b * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) { nan_record<SCP_AUDIT_WIDTH>(out); return; }
    audit_dispersed_fold(a.D, a.flights + (long)b * a.D * SCP_AUDIT_WIDTH, out);
}

// the two launches of a D-flight audit: one thread per (problem, flight), then one per problem
template <class Args, class Params>
static int audit_flights_launch(void (*flight)(Args, Params), void (*fold)(Args), const Args& a, const Params& par, hipStream_t stream)
{
    hipLaunchKernelGGL(flight, dim3((unsigned)(((long)a.B * a.D + 63) / 64)), dim3(64), 0, stream, a, par);
    if (const int rc = launch_rc()) return rc;
    hipLaunchKernelGGL(fold, dim3((a.B + 63) / 64), dim3(64), 0, stream, a);
    return launch_rc();
}

int audit_dispersed_launch(int model_id, const double* model_par, const AuditDispersedArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        return audit_flights_launch(audit_dispersed_kernel<decltype(m)>, audit_dispersed_fold_kernel, a, decltype(m)::make_params(model_par), stream);
    });
}

// the tracking audit's fold: the dispersed fold over [0..11] of the flight records, marked 3.0
__global__ __launch_bounds__(64) void audit_tracking_fold_kernel(AuditTrackingArgs a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* out = a.audit + (long)b * SCP_AUDIT_WIDTH;
    if (a.mask != nullptr && a.mask[b] == 0) { nan_record<SCP_AUDIT_WIDTH>(out); return; }
    audit_dispersed_fold(a.D, a.flights + (long)b * a.D * SCP_AUDIT_WIDTH, out, 3.0);
}

int audit_tracking_launch(int model_id, const double* model_par, const AuditTrackingArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        return audit_flights_launch(audit_tracking_kernel<decltype(m)>, audit_tracking_fold_kernel, a, decltype(m)::make_params(model_par), stream);
    });
}

// the host twin of a D-flight audit: the D flights of ONE problem, with the truth model where one is given, and their fold
template <AuditFlight MODE>
static int audit_flights_host(int model_id, const double* model_par, const double* par_true, int N, const double* xd, const double* ud,
                              const double* p, const double* pp, const double* Sx, const double* Su, const double* K, int res_or_steps, double viol_tol,
                              int D, const double* dx0, const double* ugain, const double* ubias, double marker, double* summary, double* flights)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        if ((M::np > 0 && !p) || (M::npp > 0 && !pp)) return (int)SCP_ERR_BAD_ARGUMENT;
        const typename M::Params par = M::make_params(par_true ? par_true : model_par);
        std::vector<double> own;
        if (!flights) { own.resize((size_t)SCP_AUDIT_WIDTH * D); flights = own.data(); }
        for (int d = 0; d < D; d++)
            audit_flight_one<M, MODE>(par, N, res_or_steps, viol_tol, xd, ud, p, pp, Sx, flights + (size_t)d * SCP_AUDIT_WIDTH,
                                      dx0 ? dx0 + (size_t)d * M::nx : nullptr, ugain ? ugain + (size_t)d * M::nu : nullptr,
                                      ubias ? ubias + (size_t)d * M::nu : nullptr, Su, K);
        audit_dispersed_fold(D, flights, summary, marker);
        return (int)SCP_OK;
    });
}

}  // namespace scp

extern "C" int scp_model_audit_host(int model_id, const double* model_par, int N, const double* xd, const double* ud,
                                    const double* p, const double* pp, const double* Sx, int res, double viol_tol,
                                    double* audit)
{
    if (!model_par || N < 2 || !xd || !ud || !Sx || !audit || res < 2) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        if ((M::np > 0 && !p) || (M::npp > 0 && !pp)) return (int)SCP_ERR_BAD_ARGUMENT;
        scp::audit_flight_one<M, scp::AuditFlight::nominal>(M::make_params(model_par), N, res, viol_tol, xd, ud, p, pp, Sx, audit);
        return (int)SCP_OK;
    });
}

extern "C" int scp_model_audit_intervals_host(int model_id, const double* model_par, int N, int disc_method, const double* xd,
                                              const double* ud, const double* p, const double* pp, const double* Sx, int res,
                                              double viol_tol, double* audit, double* intervals)
{
    if (!model_par || N < 2 || !xd || !ud || !Sx || !audit || res < 2) return SCP_ERR_BAD_ARGUMENT;
    if (disc_method != SCP_FOH && disc_method != SCP_IMPULSE) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        if (disc_method == SCP_IMPULSE && !M::has_impulse) return (int)SCP_ERR_UNSUPPORTED;
        if ((M::np > 0 && !p) || (M::npp > 0 && !pp)) return (int)SCP_ERR_BAD_ARGUMENT;
        const typename M::Params par = M::make_params(model_par);
        const int sub = scp::audit_interval_sub(N, res);
        std::vector<double> own;
        if (!intervals) { own.resize((size_t)SCP_AUDIT_INTERVAL_WIDTH * (N - 1)); intervals = own.data(); }
        for (int k0 = 0; k0 < N - 1; k0++) {
            double* rec = intervals + (size_t)k0 * SCP_AUDIT_INTERVAL_WIDTH;
            if constexpr (M::has_impulse) {
                if (disc_method == SCP_IMPULSE) { scp::audit_interval_one<M, true>(par, N, sub, k0, viol_tol, xd, ud, p, pp, Sx, rec); continue; }
            }
            scp::audit_interval_one<M, false>(par, N, sub, k0, viol_tol, xd, ud, p, pp, Sx, rec);
        }
        scp::audit_interval_fold(N, sub, intervals, scp::audit_par_max<M>(par, p), M::ng > 0, audit);
        return (int)SCP_OK;
    });
}

extern "C" int scp_model_audit_dispersed_host(int model_id, const double* model_par, const double* par_true, int N, const double* xd,
                                              const double* ud, const double* p, const double* pp, const double* Sx, int res,
                                              double viol_tol, int D, const double* dx0, const double* ugain, const double* ubias,
                                              double* summary, double* flights)
{
    if (!model_par || N < 2 || !xd || !ud || !Sx || !summary || res < 2 || D < 1) return SCP_ERR_BAD_ARGUMENT;
    return scp::audit_flights_host<scp::AuditFlight::dispersed>(model_id, model_par, par_true, N, xd, ud, p, pp, Sx, nullptr, nullptr, res,
                                                                viol_tol, D, dx0, ugain, ubias, 2.0, summary, flights);
}

extern "C" int scp_model_audit_tracking_host(int model_id, const double* model_par, const double* par_true, int N, const double* xd,
                                             const double* ud, const double* p, const double* pp, const double* Sx, const double* Su,
                                             const double* K, int steps, double viol_tol, int D, const double* dx0,
                                             const double* ugain, const double* ubias, double* summary, double* flights)
{
    if (!model_par || N < 2 || !xd || !ud || !Sx || !Su || !K || !summary || steps < 1 || D < 1) return SCP_ERR_BAD_ARGUMENT;
    return scp::audit_flights_host<scp::AuditFlight::tracking>(model_id, model_par, par_true, N, xd, ud, p, pp, Sx, Su, K, steps, viol_tol,
                                                               D, dx0, ugain, ubias, 3.0, summary, flights);
}
