// The structured PTR path of the C-ABI library (include/scp_mi355x.h): formulate (K2), solve (K3) and extract (K4) about the
// resident reference and the PTR run on a problem handle.  Owns h->ptr (scp_handle.hpp).
#include <algorithm>
#include <cmath>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "scp_handle.hpp"
#include "ipm_kernel.hpp"
#include "ipm2_kernel.hpp"
#include "ptr_kernels.hpp"
#include "guess_kernel.hpp"   // GuessArgs
#include "stage_problem.hpp"

using namespace scp;

// ------------------------------------------------------------------------------------------
// PTR
// ------------------------------------------------------------------------------------------

static int ensure_ptr_buffers(scp_problem* h, int hist_iters)
{
    const size_t B = h->cap;
    if (!h->ptr.ptr_ready) {
        int rc = with_structured_model(h->model_id, [&](auto m) -> int {
            using M = decltype(m);
            h->ptr.slab_stride = SP<M>::offsets(h->N).total;
            h->ptr.work_stride = Ipm2Work<M>::offsets(h->N).total;
            return (int)SCP_OK;
        });
        if (rc) return rc;
        const size_t nz = h->info.nx + h->info.nu, npa = h->npt > 0 ? h->npt : 1, N = h->N;
        if (!h->ptr.d_pp) TRY(dalloc(h, &h->ptr.d_pp, (size_t)(h->info.npp > 0 ? h->info.npp : 1) * B));
        TRY(dalloc(h, &h->ptr.prof, 8 * B));
        TRY(dalloc(h, &h->ptr.guess_xd, (size_t)h->info.nx * h->N * B)); TRY(dalloc(h, &h->ptr.guess_ud, (size_t)h->info.nu * h->N * B));
        TRY(dalloc(h, &h->ptr.guess_p, (size_t)(h->npt > 0 ? h->npt : 1) * B));
        TRY(dalloc(h, &h->ptr.slab, (size_t)h->ptr.slab_stride * B));
        TRY(dalloc(h, &h->ptr.work, (size_t)h->ptr.work_stride * B));
        TRY(dalloc(h, &h->ptr.z_out, nz * N * B)); TRY(dalloc(h, &h->ptr.p_out, npa * B)); TRY(dalloc(h, &h->ptr.ipm_info, 8 * B));
        TRY(dalloc(h, &h->ptr.cost, 4 * B)); TRY(dalloc(h, &h->ptr.dev, B)); TRY(dalloc(h, &h->ptr.eta, (2 * N + 1) * B));
        TRY(dalloc(h, &h->ptr.Jaug_ref, B));
        TRY(dalloc(h, &h->ptr.vd, (size_t)h->info.nx * (N - 1) * B)); TRY(dalloc(h, &h->ptr.vs, (size_t)(h->info.ns > 0 ? h->info.ns : 1) * N * B));
        TRY(dalloc(h, &h->ptr.vic, (size_t)(h->info.nic > 0 ? h->info.nic : 1) * B)); TRY(dalloc(h, &h->ptr.vtc, (size_t)(h->info.ntc > 0 ? h->info.ntc : 1) * B));
        TRY(dalloc(h, &h->ptr.Ppen, N * B)); TRY(dalloc(h, &h->ptr.Pf, 2 * B));
        TRY(dalloc(h, &h->ptr.ipm_status, B)); TRY(dalloc(h, &h->ptr.ipm_iters, B)); TRY(dalloc(h, &h->ptr.active, B));
        TRY(dalloc(h, &h->ptr.scp_status, B)); TRY(dalloc(h, &h->ptr.iters_done, B)); TRY(dalloc(h, &h->ptr.n_active, 1));
        TRY(dalloc(h, &h->ptr.cold_iters, B));
        TRY(dalloc(h, &h->ptr.snap, B));
        h->ptr.ptr_ready = true;
    }
    if (hist_iters > h->ptr.hist_cap) {
        TRY(dalloc(h, &h->ptr.hist, (size_t)hist_iters * B * H_N));  // (older, smaller buffer is freed at destroy)
        h->ptr.hist_cap = hist_iters;
    }
    return SCP_OK;
}

static int check_pars(const scp_ptr_params* p)
{
    if (!p || p->iter_max < 1 || !(p->wvc > 0) || !(p->wtr > 0)) return SCP_ERR_BAD_ARGUMENT;
    if (!std::isinf(p->q_tr) || !std::isinf(p->q_exit)) return SCP_ERR_UNSUPPORTED;  // reference tests use Inf only
    if (p->ipm_max_iter < 1) return SCP_ERR_BAD_ARGUMENT;
    if (p->ipm_warm != 0 && !(p->ipm_warm_mu > 0.0)) return SCP_ERR_BAD_ARGUMENT;
    return SCP_OK;
}

// ---- the argument blocks of K2, K3 and K4a ----
static AsmArgs asm_args(const scp_problem* h, int B)
{
    AsmArgs aa;
    aa.B = B; aa.N = h->N; aa.wvc = h->ptr.pars.wvc; aa.wtr = h->ptr.pars.wtr;
    aa.xd = h->traj.ref_xd; aa.ud = h->traj.ref_ud; aa.p = h->traj.ref_p; aa.pp = h->ptr.d_pp;
    aa.A = h->traj.ref_dyn.A; aa.Bm = h->traj.ref_dyn.Bm; aa.Bp = h->traj.ref_dyn.Bp; aa.F = h->traj.ref_dyn.F; aa.r = h->traj.ref_dyn.r;
    aa.Sx = h->d_Sx; aa.cx = h->d_cx; aa.Su = h->d_Su; aa.cu = h->d_cu; aa.Sp = h->d_Sp; aa.cp = h->d_cp;
    aa.slab = h->ptr.slab; aa.slab_stride = h->ptr.slab_stride; aa.active = h->ptr.active;
    return aa;
}

// The snapshot levels of the warm start, coarse ... very fine, and THE place of their defaults (<= 0 selects one); the fine
// level (ipm_warm_mu, ipm_warm_dev) has none: it is the caller's, and check_pars refuses ipm_warm_mu <= 0 with the warm start on
static void warm_levels(const scp_ptr_params& q, double (&mu)[4], double (&dev)[4])
{
    auto dflt = [](double v, double d) { return v > 0.0 ? v : d; };
    mu[0] = dflt(q.ipm_warm_mu_coarse, 1e-1); dev[0] = std::numeric_limits<double>::infinity();
    mu[1] = dflt(q.ipm_warm_mu_mid, 1e-5);    dev[1] = dflt(q.ipm_warm_dev_mid, 1e-1);
    mu[2] = q.ipm_warm_mu;                    dev[2] = q.ipm_warm_dev;
    mu[3] = dflt(q.ipm_warm_mu_vfine, 1e-10); dev[3] = dflt(q.ipm_warm_dev_vfine, 1e-6);
}

static IpmArgs ipm_args(const scp_problem* h, int B)
{
    const scp_ptr_params& q = h->ptr.pars;
    IpmArgs ia;
    ia.B = B; ia.N = h->N; ia.max_iter = q.ipm_max_iter; ia.nref = q.ipm_nref; ia.stall = q.ipm_stall;
    ia.feastol = q.ipm_feastol; ia.abstol = q.ipm_abstol; ia.reltol = q.ipm_reltol; ia.reg = q.ipm_reg;
    ia.ref_gap = q.ipm_ref_gap; ia.ref_tol = q.ipm_ref_tol; ia.split_step = q.ipm_split_step;
    ia.slab = h->ptr.slab; ia.slab_stride = h->ptr.slab_stride; ia.work = h->ptr.work; ia.work_stride = h->ptr.work_stride;
    ia.z_out = h->ptr.z_out; ia.p_out = h->ptr.p_out; ia.status = h->ptr.ipm_status; ia.iters = h->ptr.ipm_iters; ia.info = h->ptr.ipm_info;
    ia.active = h->ptr.active; ia.prof = h->ptr.prof;
    // warm start only inside a running PTR loop, from the second iteration on (the workspace then holds the snapshots of the
    // previous subproblem's solve and h->ptr.dev the previous solution's deviation)
    ia.warm_allowed = (h->run.kind == RUN_PTR && h->ptr.iter >= 2 && q.ipm_warm != 0) ? 1 : 0;
    ia.warm_min_cold = q.ipm_warm_min_cold;
    warm_levels(q, ia.warm_mu, ia.warm_dev);
    ia.prev_dev = h->ptr.dev; ia.cold_iters = h->ptr.cold_iters; ia.snap = h->ptr.snap;
    return ia;
}

static ExtractArgs extract_args(const scp_problem* h, int B)
{
    ExtractArgs ea;
    ea.B = B; ea.N = h->N; ea.slab = h->ptr.slab; ea.slab_stride = h->ptr.slab_stride; ea.z = h->ptr.z_out; ea.ph = h->ptr.p_out;
    ea.Sx = h->d_Sx; ea.cx = h->d_cx; ea.Su = h->d_Su; ea.cu = h->d_cu; ea.Sp = h->d_Sp; ea.cp = h->d_cp;
    ea.active = h->ptr.active; ea.xd = h->traj.sol_xd; ea.ud = h->traj.sol_ud; ea.p = h->traj.sol_p; ea.cost = h->ptr.cost; ea.dev = h->ptr.dev;
    ea.eta = h->ptr.eta;
    ea.Eref = h->traj.ref_dyn.E; ea.vd = h->ptr.vd; ea.vs = h->ptr.vs; ea.vic = h->ptr.vic; ea.vtc = h->ptr.vtc; ea.Ppen = h->ptr.Ppen; ea.Pf = h->ptr.Pf;
    ea.wvc = h->ptr.pars.wvc;
    return ea;
}

// formulate (K2) + solve (K3), with the extraction (K4a) in the tail of the solving wave, about (ref trajectory, ref_dyn);
// results in sol_*
static int subproblem_dev(scp_problem* h, int B)
{
    return with_structured_model(h->model_id, [&](auto m) -> int {
        using M = decltype(m);
        typename M::Params P = M::make_params(h->par.data());
        const long nthreads = (long)B * (h->N + 1);
        TRY(stamp_begin(h, 1));
        hipLaunchKernelGGL(ptr_assemble_kernel<M>, dim3((unsigned)((nthreads + 63) / 64)), dim3(64), 0, h->stream, asm_args(h, B), P);
        TRY(stamp_end(h));
        HIP_TRY(h, hipGetLastError());
        int wpe = (B > 4 * h->num_cus) ? 2 : 1;   // more problems than SIMDs: two problems per SIMD
        if (h->ptr.pars.ipm_wpe == 1 || h->ptr.pars.ipm_wpe == 2) wpe = h->ptr.pars.ipm_wpe;
        const IpmArgs ia = ipm_args(h, B);
        const ExtractArgs ea = extract_args(h, B);
        TRY(stamp_begin(h, 2));
        if (wpe >= 2) hipLaunchKernelGGL((ipm2_solve_kernel<M, 2>), dim3(B), dim3(64), 0, h->stream, ia, ea);
        else hipLaunchKernelGGL((ipm2_solve_kernel<M, 1>), dim3(B), dim3(64), 0, h->stream, ia, ea);
        TRY(stamp_end(h));
        HIP_TRY(h, hipGetLastError());
        h->ptr.sub_ready = true;
        return (int)SCP_OK;
    });
}

static int ptr_start_dev(scp_problem* h)
{
    const int B = h->ptr.B;
    const auto cp = copy_d2d(h, B);
    TRY(copy_traj(h, traj_ref(h), traj_guess(h), cp));
    // until the first iteration has run, the "solution" returned by scp_ptr_get_host is the guess itself
    TRY(copy_traj(h, traj_sol(h), traj_guess(h), cp));
    h->ptr.iter = 0;
    // generate_initial_guess: discretize!(guess)  (ptr.jl:548-555); J_aug of the guess is NaN (ptr.jl:350)
    TRY(discretize_dev(h, B, h->traj.ref_xd, h->traj.ref_ud, h->traj.ref_p, h->traj.ref_dyn, h->traj.d_feas_new, nullptr));
    // scp_ptr_get_host straight after init / restart returns the guess: its feasibility flag and defects are the guess's
    HIP_TRY(h, hipMemcpyAsync(h->traj.d_feas, h->traj.d_feas_new, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    TRY(cp(h->traj.sol_dyn.defect, h->traj.ref_dyn.defect, (size_t)h->info.nx * (h->N - 1)));
    std::vector<double> nan(B, std::numeric_limits<double>::quiet_NaN());
    HIP_TRY(h, hipMemcpyAsync(h->ptr.Jaug_ref, nan.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ptr.scp_status, 0, (size_t)B * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ptr.iters_done, 0, (size_t)B * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ptr.cold_iters, 0, (size_t)B * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ptr.snap, 0, (size_t)B * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ptr.hist, 0, (size_t)h->ptr.pars.iter_max * B * H_N * sizeof(double), h->stream));
    TRY(set_active_all(h, h->ptr.active, B));
    return SCP_OK;
}

// What scp_ptr_init_host, scp_ptr_init_guess_host and scp_ptr_solve_subproblem_batch_host share: argument checks, buffers, run
// state, uploads.  The inits take the trajectory buffers over for a structured run; the stand-alone solve reuses them for its
// one subproblem, so any run on the handle ends there (iterate / restart / get_host are refused until the next init).
enum PtrBegin { PTR_BEGIN_HOST_GUESS, PTR_BEGIN_DEVICE_GUESS, PTR_BEGIN_SINGLE_SOLVE };
static int ptr_begin(scp_problem* h, PtrBegin what, int B, const scp_ptr_params* pars, const double* xd, const double* ud,
                     const double* p, const double* pp)
{
    const bool traj = what != PTR_BEGIN_DEVICE_GUESS, run = what != PTR_BEGIN_SINGLE_SOLVE;
    if (!h || B < 1 || (traj && (!xd || !ud))) return SCP_ERR_BAD_ARGUMENT;
    if (B > h->cap) return SCP_ERR_BATCH_TOO_LARGE;
    if (traj && h->npt > 0 && !p) return SCP_ERR_BAD_ARGUMENT;
    if (h->info.npp > 0 && !pp) return SCP_ERR_BAD_ARGUMENT;
    TRY(check_pars(pars));
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(ensure_ptr_buffers(h, run ? pars->iter_max : 1));
    h->ptr.pars = *pars; h->ptr.B = B; h->ptr.iter = 0; h->run = Run{run ? RUN_PTR : RUN_NONE, nullptr};
    if (run) h->ptr.sub_ready = false;
    const Traj dst = run ? traj_guess(h) : traj_ref(h);
    if (traj) TRY(upload_traj(h, B, xd, ud, p, dst.xd, dst.ud, dst.p));
    if (h->info.npp > 0)
        HIP_TRY(h, hipMemcpyAsync(h->ptr.d_pp, pp, (size_t)h->info.npp * B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return SCP_OK;
}

extern "C" int scp_ptr_init_host(scp_handle h, int B, const scp_ptr_params* pars, const double* xd, const double* ud,
                                 const double* p, const double* pp)
{
    TRY(ptr_begin(h, PTR_BEGIN_HOST_GUESS, B, pars, xd, ud, p, pp));
    return ptr_start_dev(h);
}

extern "C" int scp_ptr_init_guess_host(scp_handle h, int B, const scp_ptr_params* pars, const double* pp)
{
    TRY(ptr_begin(h, PTR_BEGIN_DEVICE_GUESS, B, pars, nullptr, nullptr, nullptr, pp));
    GuessArgs g;
    g.B = B; g.N = h->N; g.pp = h->ptr.d_pp; g.xd = h->ptr.guess_xd; g.ud = h->ptr.guess_ud; g.p = h->ptr.guess_p;
    TRY(guess_dev(h, g));
    return ptr_start_dev(h);
}

extern "C" int scp_ptr_restart(scp_handle h)
{
    TRY(check_run(h, RUN_PTR, nullptr, "scp_ptr_restart"));
    HIP_TRY(h, hipSetDevice(h->device));
    return ptr_start_dev(h);
}

static int copy_sol_to_ref(scp_problem* h, int B)
{
    const size_t nx = h->info.nx, nu = h->info.nu, npF = h->info.npF > 0 ? h->info.npF : 1, M = h->N - 1;
    const auto cp = copy_d2d(h, B);
    TRY(copy_traj(h, traj_ref(h), traj_sol(h), cp));
    TRY(cp(h->traj.ref_dyn.A, h->traj.sol_dyn.A, nx * nx * M)); TRY(cp(h->traj.ref_dyn.Bm, h->traj.sol_dyn.Bm, nx * nu * M));
    TRY(cp(h->traj.ref_dyn.Bp, h->traj.sol_dyn.Bp, nx * nu * M)); TRY(cp(h->traj.ref_dyn.F, h->traj.sol_dyn.F, nx * npF * M));
    TRY(cp(h->traj.ref_dyn.r, h->traj.sol_dyn.r, nx * M));
    TRY(cp(h->traj.ref_dyn.E, h->traj.sol_dyn.E, nx * nx * M));   // ref.dyn.E enters the next subproblem's vd (ptr.jl:805)
    return SCP_OK;
}

// Enqueues one PTR iteration on the handle's stream WITHOUT waiting for it: several handles (sub-batches, one stream each)
// then overlap on the GPU, and several iterations can be in flight per handle -- the straggling problems of one launch no
// longer idle the rest of the chip.  scp_ptr_poll waits and returns the active count.
extern "C" int scp_ptr_iterate_async(scp_handle h)
{
    TRY(check_run(h, RUN_PTR, nullptr, "scp_ptr_iterate"));
    HIP_TRY(h, hipSetDevice(h->device));
    const int B = h->ptr.B;
    h->ptr.iter += 1;
    if (h->ptr.iter > h->ptr.pars.iter_max) return SCP_OK;
    TRY(subproblem_dev(h, B));
    // SCPSubproblemSolution(spbm, ctor) -> SubproblemSolution(x,u,p,...) -> discretize! (ptr.jl:380)
    TRY(discretize_dev(h, B, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p, h->traj.sol_dyn, h->traj.d_feas_new, h->ptr.active));
    TRY(merge_feas_dev(h, B, h->ptr.active));
    HIP_TRY(h, hipMemsetAsync(h->ptr.n_active, 0, sizeof(int), h->stream));
    UpdateArgs ua;
    ua.B = B; ua.iter = h->ptr.iter; ua.iter_max = h->ptr.pars.iter_max; ua.eps_abs = h->ptr.pars.eps_abs; ua.eps_rel = h->ptr.pars.eps_rel;
    ua.cost = h->ptr.cost; ua.dev = h->ptr.dev; ua.feas = h->traj.d_feas; ua.ipm_status = h->ptr.ipm_status; ua.ipm_iters = h->ptr.ipm_iters;
    ua.ipm_info = h->ptr.ipm_info; ua.Jaug_ref = h->ptr.Jaug_ref; ua.active = h->ptr.active; ua.scp_status = h->ptr.scp_status;
    ua.iters_done = h->ptr.iters_done; ua.hist = h->ptr.hist; ua.n_active = h->ptr.n_active;
    TRY(stamp_begin(h, 3));
    hipLaunchKernelGGL(ptr_update_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, ua);
    TRY(stamp_end(h));
    HIP_TRY(h, hipGetLastError());
    // the active count of THIS iteration, readable later without draining the stream (scp_ptr_poll_iteration)
    if (h->ptr.na_cap < h->ptr.pars.iter_max + 2) {     // (first iteration of a run with a longer horizon: nothing of the ring is in flight)
        if (h->ptr.na_ring) { HIP_TRY(h, hipStreamSynchronize(h->stream)); HIP_TRY(h, hipHostFree(h->ptr.na_ring)); h->ptr.na_ring = nullptr; }
        if (h->ptr.na_dev) { HIP_TRY(h, hipFree(h->ptr.na_dev)); h->ptr.na_dev = nullptr; }
        h->ptr.na_cap = h->ptr.pars.iter_max + 2;
        HIP_TRY(h, hipHostMalloc((void**)&h->ptr.na_ring, sizeof(int) * (size_t)h->ptr.na_cap));
        HIP_TRY(h, hipMalloc((void**)&h->ptr.na_dev, sizeof(int) * (size_t)h->ptr.na_cap));
    }
    while ((int)h->ptr.na_ev.size() <= h->ptr.iter) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ptr.na_ev.push_back(e);
    }
    HIP_TRY(h, hipMemcpyAsync(&h->ptr.na_dev[h->ptr.iter], h->ptr.n_active, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&h->ptr.na_ring[h->ptr.iter], h->ptr.n_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipEventRecord(h->ptr.na_ev[h->ptr.iter], h->stream));
    // ref = spbm.sol (ptr.jl:509).  Whole-batch copy: problems that stopped are never read again as `ref`.
    TRY(copy_sol_to_ref(h, B));
    return SCP_OK;
}

extern "C" int scp_ptr_poll(scp_handle h, int* n_active)
{
    TRY(check_run(h, RUN_PTR, nullptr, "scp_ptr_poll"));
    HIP_TRY(h, hipSetDevice(h->device));
    int na = 0;
    if (h->ptr.iter >= 1 && h->ptr.iter <= h->ptr.pars.iter_max)   // n_active of the last enqueued iteration (0 once iter_max is passed)
        HIP_TRY(h, hipMemcpyAsync(&na, h->ptr.n_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    if (n_active) *n_active = na;
    return SCP_OK;
}

// Active count at the end of iteration `iteration` (1-based, already enqueued) WITHOUT waiting for later work on the stream: the
// caller enqueues window k + 1, then reads the count of window k (multi-GPU loop: the queue never drains at a window boundary).
extern "C" int scp_ptr_poll_iteration(scp_handle h, int iteration, int* n_active)
{
    TRY(check_run(h, RUN_PTR, nullptr, "scp_ptr_poll_iteration"));
    if (!n_active || iteration < 1 || iteration > h->ptr.iter) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    if (iteration > h->ptr.pars.iter_max) { *n_active = 0; return SCP_OK; }     // nothing was enqueued beyond iter_max
    if (!h->ptr.na_ring || (int)h->ptr.na_ev.size() <= iteration) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipEventSynchronize(h->ptr.na_ev[iteration]));
    *n_active = h->ptr.na_ring[iteration];
    stamps_collect_ready(h);      // fold the kernel time stamps that have completed (without waiting) -- the pending list stays short
    return SCP_OK;
}

extern "C" int scp_ptr_iterate(scp_handle h, int* n_active)
{
    TRY(scp_ptr_iterate_async(h));
    return scp_ptr_poll(h, n_active);
}

extern "C" int scp_ptr_get_host(scp_handle h, double* xd, double* ud, double* p, int32_t* status, int32_t* iterations,
                                double* cost, uint8_t* feas, double* defect, double* hist)
{
    TRY(check_run(h, RUN_PTR, nullptr, "scp_ptr_get_host"));
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t D = sizeof(double), b = h->ptr.B;
    TRY(download_traj(h, h->ptr.B, true, xd, ud, p, defect));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, h->ptr.scp_status, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations, h->ptr.iters_done, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (cost) HIP_TRY(h, hipMemcpyAsync(cost, h->ptr.cost, 4 * b * D, hipMemcpyDeviceToHost, h->stream));
    if (hist) HIP_TRY(h, hipMemcpyAsync(hist, h->ptr.hist, (size_t)h->ptr.pars.iter_max * b * H_N * D, hipMemcpyDeviceToHost, h->stream));
    TRY(feas_out(h, h->ptr.B, h->traj.d_feas, feas));
    return SCP_OK;
}

extern "C" int scp_ptr_solve_batch_host(scp_handle h, int B, const scp_ptr_params* pars, const double* xd,
                                        const double* ud, const double* p, const double* pp, double* xd_out,
                                        double* ud_out, double* p_out, int32_t* status, int32_t* iterations,
                                        double* cost, uint8_t* feas, double* seconds)
{
    if (!h) return SCP_ERR_BAD_ARGUMENT;
    TRY(scp_ptr_init_host(h, B, pars, xd, ud, p, pp));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    int na = B;
    while (na > 0) TRY(scp_ptr_iterate(h, &na));
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    TRY(scp_ptr_get_host(h, xd_out, ud_out, p_out, status, iterations, cost, feas, nullptr, nullptr));
    return elapsed_out(h, seconds);
}

extern "C" int scp_ptr_solve_subproblem_batch_host(scp_handle h, int B, const scp_ptr_params* pars,
                                                   const double* xd_ref, const double* ud_ref, const double* p_ref,
                                                   const double* pp, double* x, double* u, double* p, double* cost,
                                                   double* eta, int32_t* solver_status, int32_t* solver_iters,
                                                   double* info, double* defect, uint8_t* feas, double* seconds)
{
    TRY(ptr_begin(h, PTR_BEGIN_SINGLE_SOLVE, B, pars, xd_ref, ud_ref, p_ref, pp));
    TRY(set_active_all(h, h->ptr.active, B));
    TRY(discretize_dev(h, B, h->traj.ref_xd, h->traj.ref_ud, h->traj.ref_p, h->traj.ref_dyn, h->traj.d_feas_new, nullptr));
    HIP_TRY(h, hipEventRecord(h->timing.ev0, h->stream));
    TRY(subproblem_dev(h, B));
    HIP_TRY(h, hipEventRecord(h->timing.ev1, h->stream));
    TRY(discretize_dev(h, B, h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p, h->traj.sol_dyn, h->traj.d_feas_new, nullptr));
    const size_t N = h->N, D = sizeof(double), b = B;
    TRY(download_traj(h, B, true, x, u, p, defect));
    if (cost) HIP_TRY(h, hipMemcpyAsync(cost, h->ptr.cost, 4 * b * D, hipMemcpyDeviceToHost, h->stream));
    if (eta) HIP_TRY(h, hipMemcpyAsync(eta, h->ptr.eta, (2 * N + 1) * b * D, hipMemcpyDeviceToHost, h->stream));
    if (solver_status) HIP_TRY(h, hipMemcpyAsync(solver_status, h->ptr.ipm_status, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (solver_iters) HIP_TRY(h, hipMemcpyAsync(solver_iters, h->ptr.ipm_iters, b * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (info) HIP_TRY(h, hipMemcpyAsync(info, h->ptr.ipm_info, 8 * b * D, hipMemcpyDeviceToHost, h->stream));
    TRY(feas_out(h, B, h->traj.d_feas_new, feas));
    return elapsed_out(h, seconds);
}

extern "C" int scp_ptr_get_virtual_controls_host(scp_handle h, double* vd, double* vs, double* vic, double* vtc, double* P,
                                                 double* Pf)
{
    if (!h || !h->ptr.ptr_ready || !h->ptr.sub_ready || h->ptr.B < 1) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nx = h->info.nx, ns = h->info.ns, nic = h->info.nic, ntc = h->info.ntc, N = h->N, D = sizeof(double), b = h->ptr.B;
    if (vd) HIP_TRY(h, hipMemcpyAsync(vd, h->ptr.vd, nx * (N - 1) * b * D, hipMemcpyDeviceToHost, h->stream));
    if (vs && ns > 0) HIP_TRY(h, hipMemcpyAsync(vs, h->ptr.vs, ns * N * b * D, hipMemcpyDeviceToHost, h->stream));
    if (vic && nic > 0) HIP_TRY(h, hipMemcpyAsync(vic, h->ptr.vic, nic * b * D, hipMemcpyDeviceToHost, h->stream));
    if (vtc && ntc > 0) HIP_TRY(h, hipMemcpyAsync(vtc, h->ptr.vtc, ntc * b * D, hipMemcpyDeviceToHost, h->stream));
    if (P) HIP_TRY(h, hipMemcpyAsync(P, h->ptr.Ppen, N * b * D, hipMemcpyDeviceToHost, h->stream));
    if (Pf) HIP_TRY(h, hipMemcpyAsync(Pf, h->ptr.Pf, 2 * b * D, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stamps_collect(h);
    return SCP_OK;
}

extern "C" int scp_debug_get_ipm_profile(scp_handle h, int b, long long* ticks8)
{
    if (!h || !h->ptr.ptr_ready || b < 0 || b >= h->cap || !ticks8) return SCP_ERR_BAD_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(ticks8, h->ptr.prof + (long)b * 8, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return SCP_OK;
}

extern "C" int scp_debug_get_stage_problem(scp_handle h, int b, double* buf, long* n_doubles)
{
    if (!h || !h->ptr.ptr_ready || b < 0 || b >= h->cap) return SCP_ERR_BAD_ARGUMENT;
    if (n_doubles) *n_doubles = h->ptr.slab_stride;
    if (buf) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpy(buf, h->ptr.slab + (long)b * h->ptr.slab_stride, (size_t)h->ptr.slab_stride * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SCP_OK;
}
