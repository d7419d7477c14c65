// The covariance audit's own translation unit: the instantiations of cov_rows_kernel (one per auditable model, models/registry.hpp)
// and of cov_chain_kernel (one per (nx, nu) of them) (cov_kernel.hpp), their launch for the handle-level entry points of
// audit_entry.hip, and the pure-host twins scp_model_covariance_rows_host and scp_covariance_host.
#include <hip/hip_runtime.h>

#include "../../include/scp_mi355x.h"
#include "audit_host.hpp"
#include "cov_kernel.hpp"
#include "models/registry.hpp"

namespace scp {

template <int NX, int NU>
static int cov_chain_launch(Cov<NX, NU>, const CovArgs& a, hipStream_t stream)
{
    return packed_chain_launch(cov_chain_kernel<NX, NU>, NX, a.B, a, stream);
}

int cov_launch(int model_id, const double* model_par, const CovArgs& a, hipStream_t stream)
{
    return with_auditable_model(model_id, [&](auto m) -> int {
        using M = decltype(m);
        if (a.nrow[0] != M::ns || a.nrow[1] != M::nl || a.nrow[2] != M::nsoc || a.ntc != M::ntc) return (int)SCP_ERR_BAD_ARGUMENT;
        hipLaunchKernelGGL(cov_rows_kernel<M>, dim3((unsigned)(((long)a.B * a.N + 63) / 64)), dim3(64), 0, stream, a, M::make_params(model_par));
        if (const int rc = launch_rc()) return rc;
        return cov_chain_launch(Cov<M::nx, M::nu>{}, a, stream);
    });
}

}  // namespace scp

extern "C" int scp_model_covariance_rows_host(int model_id, const double* model_par, int N, const double* xd, const double* ud,
                                              const double* p, const double* pp, const double* K, double* rows, double* Hf)
{
    if (!model_par || N < 2 || !xd || !ud || !K) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_auditable_model(model_id, [&](auto m) -> int {
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
    return scp::with_auditable_dims<scp::Cov>(nx, nu, [&](auto c) -> int {
        using C = decltype(c);
        if (!(nsig > 0.0) || !__builtin_isfinite(nsig) || !scp::audit_sigmas_ok(nx, nu, sig0, sigu, sigw)) return (int)SCP_ERR_BAD_ARGUMENT;
        scp::CovIn in;
        in.N = N; in.nrow[0] = nrow[0]; in.nrow[1] = nrow[1]; in.nrow[2] = nrow[2]; in.ntc = ntc; in.nsig = nsig;
        in.A = A; in.Bm = Bm; in.Bp = Bp; in.K = K; in.rows = rows; in.Hf = Hf;
        in.Sx = Sx; in.Su = Su; in.sig0 = sig0; in.sigu = sigu; in.sigw = sigw;
        typename C::Work w;
        C::chain(w, in, summary, sig, nodes, scp::serial_each<C::NP>());
        return (int)SCP_OK;
    });
}
