// Host-side pieces the audit kernel units share (audit_api.hip, lqr_api.hip, cov_api.hip, mc_api.hip).  Static functions only, like the
// helpers of scp_handle.hpp: every unit still links on its own.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/scp_mi355x.h"

namespace scp {

// what the launches since the last look came to
static int launch_rc() { return hipGetLastError() == hipSuccess ? (int)SCP_OK : (int)SCP_ERR_HIP; }

// the launch of a packed chain (lqr_riccati_kernel, cov_chain_kernel): one lane per entry of an NX x NX matrix, floor(64 / NX^2)
// problems per block of one wavefront
template <class Args>
static int packed_chain_launch(void (*kernel)(Args), int NX, int B, const Args& a, hipStream_t stream)
{
    const int pack = 64 / (NX * NX);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + pack - 1) / pack)), dim3(64), 0, stream, a);
    return launch_rc();
}

// the `each` of a packed chain in its host twin: the phase f on the NP entries one after the other
template <int NP>
static auto serial_each()
{
    return [](auto f) {
        for (int e = 0; e < NP; e++) f(e);
    };
}

}  // namespace scp
