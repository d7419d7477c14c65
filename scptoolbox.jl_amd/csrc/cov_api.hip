// The covariance audit's own translation unit: the four instantiations of cov_rows_kernel (one per auditable model) and the four
// of cov_chain_kernel (one per (nx, nu) of them) (cov_kernel.hpp), their launch for the handle-level entry points of scp_api.hip,
// and the pure-host twins scp_model_covariance_rows_host and scp_covariance_host.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/scp_mi355x.h"
#include "cov_kernel.hpp"
#include "models/double_integrator.hpp"
#include "models/quadrotor.hpp"
#include "models/rocket_landing.hpp"
#include "models/starship.hpp"

namespace scp {

// the models the audits are defined for (audit_api.hip): FOH, no node parameters
template <class Fn>
static int with_cov_model(int model_id, Fn&& fn)
{
    switch (model_id) {
        case SCP_MODEL_DOUBLE_INTEGRATOR: return fn(DoubleIntegrator{});
        case SCP_MODEL_QUADROTOR: return fn(Quadrotor{});
        case SCP_MODEL_ROCKET_LANDING: return fn(RocketLanding{});
        case SCP_MODEL_STARSHIP: return fn(Starship{});
        case SCP_MODEL_FREEFLYER: return (int)SCP_ERR_UNSUPPORTED;
        case SCP_MODEL_OSCILLATOR: return (int)SCP_ERR_UNSUPPORTED;
        default: return (int)SCP_ERR_UNKNOWN_MODEL;
    }
}

// the dimension pairs of the double integrator, the quadrotor, the rocket landing and the Starship
template <class Fn>
static int with_cov_dims(int nx, int nu, Fn&& fn)
{
    if (nx == 2 && nu == 1) return fn(Cov<2, 1>{});
    if (nx == 6 && nu == 4) return fn(Cov<6, 4>{});
    if (nx == 7 && nu == 4) return fn(Cov<7, 4>{});
    if (nx == 8 && nu == 3) return fn(Cov<8, 3>{});
    return (int)SCP_ERR_UNSUPPORTED;
}

template <int NX, int NU>
static int cov_chain_launch(Cov<NX, NU>, const CovArgs& a, hipStream_t stream)
{
    constexpr int PACK = 64 / (NX * NX);
    hipLaunchKernelGGL((cov_chain_kernel<NX, NU>), dim3((unsigned)((a.B + PACK - 1) / PACK)), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? (int)SCP_OK : (int)SCP_ERR_HIP;
}

int cov_launch(int model_id, const double* model_par, const CovArgs& a, hipStream_t stream)
{
    return with_cov_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        if (a.nrow[0] != M::ns || a.nrow[1] != M::nl || a.nrow[2] != M::nsoc || a.ntc != M::ntc) return (int)SCP_ERR_BAD_ARGUMENT;
        hipLaunchKernelGGL(cov_rows_kernel<M>, dim3((unsigned)(((long)a.B * a.N + 63) / 64)), dim3(64), 0, stream, a, M::make_params(model_par));
        if (hipGetLastError() != hipSuccess) return (int)SCP_ERR_HIP;
        return with_cov_dims(M::nx, M::nu, [&](auto c) -> int { return cov_chain_launch(c, a, stream); });
    });
}

bool cov_sigmas_ok(int nx, int nu, const double* sig0, const double* sigu, const double* sigw, double nsig)
{
    if (!sig0 || !sigu || !sigw || !std::isfinite(nsig) || !(nsig > 0.0)) return false;
    for (int i = 0; i < nx; i++)
        if (!std::isfinite(sig0[i]) || sig0[i] < 0.0 || !std::isfinite(sigw[i]) || sigw[i] < 0.0) return false;
    for (int i = 0; i < nu; i++)
        if (!std::isfinite(sigu[i]) || sigu[i] < 0.0) return false;
    return true;
}

template <int NX, int NU>
static int cov_host_dims(Cov<NX, NU>, const CovIn& in, double* summary, double* sig, double* nodes)
{
    using C = Cov<NX, NU>;
    typename C::Work w;
    C::chain(w, in, summary, sig, nodes, [&](auto f) {
        for (int e = 0; e < C::NP; e++) f(e);
    });
    return (int)SCP_OK;
}

}  // namespace scp

extern "C" int scp_model_covariance_rows_host(int model_id, const double* model_par, int N, const double* xd, const double* ud,
                                              const double* p, const double* pp, const double* K, double* rows, double* Hf)
{
    if (!model_par || N < 2 || !xd || !ud || !K) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_cov_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        constexpr int nrow = M::ns + M::nl + M::nsoc;
        if ((M::np > 0 && !p) || (M::npp > 0 && !pp) || (nrow > 0 && !rows) || (M::ntc > 0 && !Hf)) return (int)SCP_ERR_BAD_ARGUMENT;
        const typename M::Params par = M::make_params(model_par);
        for (int k = 1; k <= N; k++) scp::cov_rows_one<M>(par, N, k, xd, ud, p, pp, K, rows + (size_t)(k - 1) * nrow * (M::nx + 1), Hf);
        return (int)SCP_OK;
    });
}

extern "C" int scp_covariance_host(int nx, int nu, int N, const double* A, const double* Bm, const double* Bp, const double* K,
                                   const int* nrow, const double* rows, int ntc, const double* Hf, const double* Sx, const double* Su,
                                   const double* sig0, const double* sigu, const double* sigw, double nsig, double* summary,
                                   double* sig, double* nodes)
{
    if (N < 2 || !A || !Bm || !Bp || !K || !nrow || !Sx || !Su || !summary || ntc < 0) return SCP_ERR_BAD_ARGUMENT;
    if (nrow[0] < 0 || nrow[1] < 0 || nrow[2] < 0 || (nrow[0] + nrow[1] + nrow[2] > 0 && !rows) || (ntc > 0 && !Hf)) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_cov_dims(nx, nu, [&](auto c) -> int {
        if (!scp::cov_sigmas_ok(nx, nu, sig0, sigu, sigw, nsig)) return (int)SCP_ERR_BAD_ARGUMENT;
        scp::CovIn in;
        in.N = N; in.nrow[0] = nrow[0]; in.nrow[1] = nrow[1]; in.nrow[2] = nrow[2]; in.ntc = ntc; in.nsig = nsig;
        in.A = A; in.Bm = Bm; in.Bp = Bp; in.K = K; in.rows = rows; in.Hf = Hf;
        in.Sx = Sx; in.Su = Su; in.sig0 = sig0; in.sigu = sigu; in.sigw = sigw;
        return scp::cov_host_dims(c, in, summary, sig, nodes);
    });
}
