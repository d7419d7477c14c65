// The LQR synthesis' own translation unit: the four instantiations of lqr_riccati_kernel (lqr_kernel.hpp), one per (nx, nu) of
// the auditable models, their launch for the handle-level entry points of scp_api.hip, and the pure-host twin scp_lqr_gains_host.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/scp_mi355x.h"
#include "lqr_kernel.hpp"

namespace scp {

// the dimension pairs of the double integrator, the quadrotor, the rocket landing and the Starship
template <class Fn>
static int with_lqr_dims(int nx, int nu, Fn&& fn)
{
    if (nx == 2 && nu == 1) return fn(Lqr<2, 1>{});
    if (nx == 6 && nu == 4) return fn(Lqr<6, 4>{});
    if (nx == 7 && nu == 4) return fn(Lqr<7, 4>{});
    if (nx == 8 && nu == 3) return fn(Lqr<8, 3>{});
    return (int)SCP_ERR_UNSUPPORTED;
}

template <int NX, int NU>
static int lqr_launch_dims(Lqr<NX, NU>, const LqrArgs& a, hipStream_t stream)
{
    constexpr int PACK = 64 / (NX * NX);
    hipLaunchKernelGGL((lqr_riccati_kernel<NX, NU>), dim3((unsigned)((a.B + PACK - 1) / PACK)), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? (int)SCP_OK : (int)SCP_ERR_HIP;
}

int lqr_launch(int nx, int nu, const LqrArgs& a, hipStream_t stream)
{
    return with_lqr_dims(nx, nu, [&](auto l) -> int { return lqr_launch_dims(l, a, stream); });
}

template <int NX, int NU>
static int lqr_host_dims(Lqr<NX, NU>, int N, const double* A, const double* Bm, const double* Bp, const double* qx, const double* ru,
                         const double* qf, double* K, double* info)
{
    using L = Lqr<NX, NU>;
    typename L::Work w;
    L::chain(w, N, A, Bm, Bp, qx, ru, qf, K, info, [&](auto f) {
        for (int e = 0; e < L::NP; e++) f(e);
    });
    return (int)SCP_OK;
}

bool lqr_weights_ok(int nx, int nu, const double* qx, const double* ru, const double* qf)
{
    if (!qx || !ru || !qf) return false;
    for (int i = 0; i < nx; i++)
        if (!std::isfinite(qx[i]) || qx[i] < 0.0 || !std::isfinite(qf[i]) || qf[i] < 0.0) return false;
    for (int i = 0; i < nu; i++)
        if (!std::isfinite(ru[i]) || !(ru[i] > 0.0)) return false;
    return true;
}

}  // namespace scp

extern "C" int scp_lqr_gains_host(int nx, int nu, int N, const double* A, const double* Bm, const double* Bp, const double* qx,
                                  const double* ru, const double* qf, double* K, double* info)
{
    if (N < 2 || !A || !Bm || !Bp || !K || !info) return SCP_ERR_BAD_ARGUMENT;
    return scp::with_lqr_dims(nx, nu, [&](auto l) -> int {
        if (!scp::lqr_weights_ok(nx, nu, qx, ru, qf)) return (int)SCP_ERR_BAD_ARGUMENT;
        return scp::lqr_host_dims(l, N, A, Bm, Bp, qx, ru, qf, K, info);
    });
}
