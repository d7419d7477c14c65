// The LQR synthesis' own translation unit: the instantiations of lqr_riccati_kernel (lqr_kernel.hpp), one per (nx, nu) of the
// auditable models (models/registry.hpp), their launch for the handle-level entry points of audit_entry.hip, and the pure-host twin
// scp_lqr_gains_host.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/scp_mi355x.h"
#include "audit_host.hpp"
#include "lqr_kernel.hpp"
#include "models/registry.hpp"

namespace scp {

template <int NX, int NU>
static int lqr_launch_dims(Lqr<NX, NU>, const LqrArgs& a, hipStream_t stream)
{
    return packed_chain_launch(lqr_riccati_kernel<NX, NU>, NX, a.B, a, stream);
}

int lqr_launch(int nx, int nu, const LqrArgs& a, hipStream_t stream)
{
    return with_auditable_dims<Lqr>(nx, nu, [&](auto l) -> int { return lqr_launch_dims(l, a, stream); });
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
    return scp::with_auditable_dims<scp::Lqr>(nx, nu, [&](auto l) -> int {
        using L = decltype(l);
        if (!scp::lqr_weights_ok(nx, nu, qx, ru, qf)) return (int)SCP_ERR_BAD_ARGUMENT;
        typename L::Work w;
        L::chain(w, N, A, Bm, Bp, qx, ru, qf, K, info, scp::serial_each<L::NP>());
        return (int)SCP_OK;
    });
}
