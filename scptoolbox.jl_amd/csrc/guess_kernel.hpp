// The straight-line initial guess of a compiled model on the device (guess_api.hip launches it; the structured PTR run keeps its
// result resident).
#pragma once
#include <hip/hip_runtime.h>

#include "models/model_common.hpp"

namespace scp {

// traj.guess(N) for a Monte-Carlo batch on the device (generate_initial_guess, src/solvers/ptr.jl:548-555 ->
// problem.jl:686-700): one thread per (problem, node); the per-problem data pp (initial / terminal conditions)
// is all that crosses PCIe.
struct GuessArgs {
    int B, N;
    const double* pp;   // [npp,B]
    double* xd;         // [nx,N,B]
    double* ud;         // [nu,N,B]
    double* p;          // [np + np_node N,B]
    const int* only = nullptr;   // optional [B]: only the problems with only[b] != 0 are written
};
template <class M>
__global__ __launch_bounds__(256) void ptr_guess_kernel(GuessArgs a, typename M::Params par)
{
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)a.B * a.N) return;
    const int b = (int)(gid / a.N), k = (int)(gid % a.N);
    if (a.only != nullptr && a.only[b] == 0) return;
    double x[M::nx], u[M::nu], pv[M::np > 0 ? M::np : 1], pn[M::np_node > 0 ? M::np_node : 1];
    M::guess(par, a.pp + (long)b * M::npp, a.N, k, x, u, pv, pn);
#pragma unroll
    for (int i = 0; i < M::nx; i++) a.xd[((long)b * a.N + k) * M::nx + i] = x[i];
#pragma unroll
    for (int i = 0; i < M::nu; i++) a.ud[((long)b * a.N + k) * M::nu + i] = u[i];
    double* pb = a.p + (long)b * np_total<M>(a.N);
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < M::np; i++) pb[i] = pv[i];
    }
#pragma unroll
    for (int i = 0; i < M::np_node; i++) pb[M::np + M::np_node * k + i] = pn[i];     // the node's own parameters
}

}  // namespace scp
