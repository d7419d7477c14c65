// Device engine of the generic batched conic solver: owns the uploaded schedule (conic_symbolic.hpp) and the
// interleaved per-problem buffers, launches conic_ipm_kernel (conic_api.hip).  Used by the C ABI of
// include/scp_conic.h and, device-resident, by the generic SCP path (scp_generic.hip: SCvx / GuSTO / PTR q_tr != Inf).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "conic_bind.hpp"

namespace scp {
namespace conic {

constexpr int CONIC_MAX_WAVES = 16;

struct Engine {
    Symbolic sym;
    Sched sched{};           // device pointers
    // Ordering (conic_symbolic.hpp): ONE schedule -- the nested dissection when the program has the chain structure and it is
    // the cheaper one for the launch geometry (5-10x fewer elimination levels = workgroup barriers), the sequential minimum
    // degree otherwise.  SCP_CONIC_ORDER = seq | nd | auto (default auto).  A problem that ends ITERATION_LIMIT /
    // NUMERICAL_ERROR is solved again on the same schedule with a larger static regularisation (launch(): at most two further
    // attempts); fb_mask marks those problems, fb_count counts them.
    int *fb_mask = nullptr, *fb_count = nullptr;
    long long n_fallback = 0, n_launched = 0, n_rescued = 0;   // problems given a further attempt / solved / rescued by one
    int cap = 0, BS = 0;     // batch capacity, interleave stride (cap rounded up to 64)
    int device = 0;
    // worker waves per group of 64 problems (1..16): tuning aid SCP_CONIC_WAVES, default 16 (a full 1024-thread workgroup)
    int waves_per_group = std::getenv("SCP_CONIC_WAVES") ? std::atoi(std::getenv("SCP_CONIC_WAVES")) : 16;
    // sub-workers per wave (1, 4, 16 or 64 -> 64, 16, 4 or 1 problems per wave); 0 = chosen from the batch size (tuning aid
    // SCP_CONIC_SUB; create() refuses any other positive value)
    int sub_workers = std::getenv("SCP_CONIC_SUB") ? std::atoi(std::getenv("SCP_CONIC_SUB")) : 0;
    std::vector<void*> allocs;
    // interleaved inputs [len][BS] and shared copies [len]
    double *c = nullptr, *b = nullptr, *h = nullptr, *Gx = nullptr, *Ax = nullptr, *Px = nullptr;
    double *c_sh = nullptr, *b_sh = nullptr, *h_sh = nullptr, *Gx_sh = nullptr, *Ax_sh = nullptr, *Px_sh = nullptr;
    // interleaved solution [len][BS]
    double *x = nullptr, *y = nullptr, *z = nullptr, *s = nullptr;
    double* work = nullptr;  // everything else
    int *status = nullptr, *iters = nullptr;
    double* info = nullptr;  // [8][BS]
    long long bytes_per_problem = 0;
    std::string err;

    // analyse + upload + allocate; returns scp_status
    int create(int n, int p, int m, int l, const std::vector<int>& q, const Csc& P, const Csc& A, const Csc& G,
               const int* perm, int capacity, int dev);
    void destroy();
    // enqueue the solve of problems [0, B) on `stream`; shared_mask as in scp_conic.h; active: optional int[B]
    // (problems with active[t] == 0 are skipped)
    int launch(hipStream_t stream, int B, const Opts& o, unsigned shared_mask, const int* active = nullptr);
    // worker waves of a launch: waves_per_group within what the kernel has instantiations for
    int waves() const { return waves_per_group < 1 ? 1 : (waves_per_group > CONIC_MAX_WAVES ? CONIC_MAX_WAVES : waves_per_group); }
    // the record of scp_conic_stats (include/scp_conic.h)
    void stats(long long out[16]) const;
};

// [len, B] column-major (batch last) <-> interleaved [len][BS]; device pointers
int transpose_to_interleaved(hipStream_t st, const double* src, double* dst, long len, int B, int BS);
int transpose_from_interleaved(hipStream_t st, const double* src, double* dst, long len, int B, int BS);

}  // namespace conic
}  // namespace scp
