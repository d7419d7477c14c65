// The problem handle of the C-ABI library (include/scp_mi355x.h) as its translation units share it: internal, not installed.
//
//   scp_api.hip      model queries, handle life cycle, kernel time stamps, discretize! and propagate (K1)
//   audit_entry.hip  scp_audit_* and scp_lqr_gains_* (their kernels live in audit_api.hip, lqr_api.hip, cov_api.hip and mc_api.hip)
//   ptr_api.hip      structured PTR path (K2-K4)
//   guess_api.hip    initial guesses (every model's straight line, the Starship reference guess)
//   scp_generic.hip  subproblem handles (scp_sub) and the SCvx / GuSTO / generic-PTR loops
//   comm_api.hip     RCCL communicator and scp_ptr_run_sharded
//
// scp_problem groups its state by the unit that WRITES it; every unit may read every group.  The units are built with
// different -D flags (SCP_IPM_PROF*, CONIC_PROF): nothing in this file may depend on one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/scp_mi355x.h"
#include "models/registry.hpp"

struct DynBuf {  // one DLTV + defect on the device
    double *A = nullptr, *Bm = nullptr, *Bp = nullptr, *F = nullptr, *r = nullptr, *E = nullptr, *defect = nullptr;
};

struct StarshipGuessState;   // guess_api.hip
struct scp_sub;              // scp_generic.hip

// What owns a problem handle's trajectory buffers (h->traj): the structured PTR run and every subproblem handle created on the
// problem (scp_generic.hip) write into the same set, so at most one run is alive per handle.
// An init takes them over and thereby ends whatever ran before; the stand-alone subproblem solves leave them to nobody.
enum RunKind { RUN_NONE = 0, RUN_PTR, RUN_SCVX, RUN_GUSTO, RUN_PTR_GENERIC };
struct Run {
    RunKind kind = RUN_NONE;
    const scp_sub* sub = nullptr;   // the subproblem handle whose loop it is (RUN_SCVX, RUN_GUSTO, RUN_PTR_GENERIC)
};

struct scp_problem {
    // ---- the problem description: written by scp_api.hip at create (par also by scp_problem_set_model_par), read by every unit ----
    int model_id = -1;
    scp_model_info info{};
    int N = 0, Nsub = 0, method = 0, cap = 0, device = 0;
    int npt = 0;   // length of the parameter vector: info.np global + info.np_node per node (model_common.hpp)
    double feas_tol = 0;
    std::vector<double> par;
    std::vector<double> Sx, cx, Su, cu, Sp, cp;
    double *d_iSx = nullptr, *d_Sx = nullptr, *d_cx = nullptr, *d_Su = nullptr, *d_cu = nullptr, *d_Sp = nullptr,
           *d_cp = nullptr;
    int num_cus = 256;      // multiProcessorCount of the device (set at create)
    hipStream_t stream = nullptr;   // replaced by scp_set_stream_priority only
    std::vector<void*> allocs;      // every unit's dalloc appends; freed at destroy
    std::string err;                // the failing call's message, whichever unit it is in
    // who may continue a run on h->traj: set by the inits (ptr_begin in ptr_api.hip, loop_begin in scp_generic.hip), cleared by the
    // stand-alone solves and scp_sub_destroy, checked by check_run.  RUN_PTR: scp_ptr_init_host / scp_ptr_init_guess_host
    Run run;

    // ---- scp_api.hip: per-kernel timing, events recorded around every launch (stamp_begin / stamp_end, called from every unit)
    // and accumulated at the next stream sync; ev0 / ev1 bracket what an entry point reports as its device seconds ----
    struct Timing {
        struct Stamp { hipEvent_t a, b; int kind; };
        std::vector<Stamp> stamps_free, stamps_pending;
        double t_kernel[4] = {0, 0, 0, 0};
        long n_kernel[4] = {0, 0, 0, 0};
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
    } timing;

    // ---- scp_api.hip: the form discretize! (K1) takes ----
    struct Disc {
        int* d_mvar = nullptr;   // [2 cap] per-problem choice of the discretize! form (disc_split_kernel)
        // debugging / parity aid: force the reference formulation of discretize! (K1) for const-Jacobian models too
        bool reference_form = std::getenv("SCP_DISC_REFERENCE_FORM") != nullptr;
        int bits = 64;     // arithmetic of discretize! (scp_set_discretize_precision): 64 = reference, 32 = tolerance check
    } disc;

    // ---- audit_entry.hip: continuous-time audit (scp_audit_*): records [SCP_AUDIT_WIDTH cap], mask [cap], the host variant's pp
    // [npp cap]; lazily built ----
    struct Audit {
        double *rec = nullptr, *pp = nullptr;
        double* intervals = nullptr;   // [SCP_AUDIT_INTERVAL_WIDTH (N-1) cap], scp_audit_intervals_*; lazily built
        int* mask = nullptr;
        // scp_audit_dispersed_*: flight records [SCP_AUDIT_WIDTH disp_D cap] and the staged dispersions dx0 [nx disp_D cap],
        // ugain, ubias [nu disp_D cap]; built on first use and rebuilt when a call asks for more flights than disp_D.  Not in
        // h->allocs: flights_reserve frees what it replaces, audit_release the last set
        double *flights = nullptr, *dx0 = nullptr, *ugain = nullptr, *ubias = nullptr;
        int disp_D = 0;
    } audit;

    // ---- audit_entry.hip: LQR gains (scp_lqr_gains_*) and the gains a tracking audit is handed (scp_audit_tracking_*).  dyn / feas:
    // a discretisation of its own, so that no run's buffer is written; K [nu nx (N-1) cap] the resident gains, made for batch B
    // (0 = none); Kin the same size for gains passed by the caller; info [SCP_LQR_INFO_WIDTH cap]; w = qx [nx], ru [nu], qf [nx],
    // uploaded from w_host.  Built on first use (Kin by the first tracking audit that is handed gains, the rest together by the first
    // gains call), not in h->allocs: audit_release frees them ----
    struct Lqr {
        DynBuf dyn;
        int* feas = nullptr;
        double *K = nullptr, *Kin = nullptr, *info = nullptr, *w = nullptr;
        std::vector<double> w_host;
        int B = 0;
    } lqr;

    // ---- audit_entry.hip: covariance audit (scp_audit_covariance_*): the row table rows [(nx+1) nrow N cap], Hf [ntc nx cap], the
    // records rec [SCP_COV_WIDTH cap], sig [nx N cap], nodes [SCP_COV_NODE_WIDTH N cap] and w = sig0 [nx], sigu [nu], sigw [nx],
    // uploaded from w_host.  Built together on first use, not in h->allocs: audit_release frees them.  The discretisation and the
    // gains are h->lqr's ----
    struct Cov {
        double *rows = nullptr, *Hf = nullptr, *rec = nullptr, *sig = nullptr, *nodes = nullptr, *w = nullptr;
        std::vector<double> w_host;
    } cov;

    // ---- audit_entry.hip: Monte-Carlo audit (scp_audit_montecarlo_*): the wavefront partials part [NV N W cap] with NV = 1 + 2 nx + nu,
    // the node records moments [NV N cap], stat [SCP_MC_STAT_WIDTH cap] and w = sig0 [nx], sigu [nu], sigw [nx], uploaded from
    // w_host.  Built together on first use and rebuilt when a call needs more than W wavefronts per problem, not in h->allocs:
    // audit_release frees them.
    // The flight records are h->audit's, the gains h->lqr's ----
    struct Mc {
        double *part = nullptr, *moments = nullptr, *stat = nullptr, *w = nullptr;
        std::vector<double> w_host;
        int W = 0;
    } mc;

    // ---- trajectories: allocated by scp_api.hip at create; written by the run that owns them (h->run: ptr_api.hip or
    // scp_generic.hip) and, between runs, by the stand-alone entry points of every unit (sol_* as their staging buffers) ----
    struct Trajectories {
        double *ref_xd = nullptr, *ref_ud = nullptr, *ref_p = nullptr;
        double *sol_xd = nullptr, *sol_ud = nullptr, *sol_p = nullptr;
        DynBuf ref_dyn, sol_dyn;
        int *d_feas_new = nullptr, *d_feas = nullptr;
    } traj;

    // ---- guess_api.hip: scp_guess_batch_host ----
    struct Guess {
        double *q_pp = nullptr, *q_xd = nullptr, *q_ud = nullptr, *q_p = nullptr;   // scratch of scp_guess_batch_host (a pure query)
        StarshipGuessState* sg = nullptr;   // device-side reference guess of the Starship model (starship_guess.hpp), lazily built
        int failures = 0;                   // instances of the last scp_guess_batch_host call that fell back to the straight line
    } guess;

    // ---- ptr_api.hip: the structured PTR path.  comm_api.hip reads iter, pars.iter_max and na_dev, and advances iter only through
    // scp_ptr_iterate_async ----
    struct Ptr {
        double* d_pp = nullptr;
        double *guess_xd = nullptr, *guess_ud = nullptr, *guess_p = nullptr;   // the run's resident guess: what a restart returns to
        long long* prof = nullptr;
        // subproblem
        double *slab = nullptr, *work = nullptr, *z_out = nullptr, *p_out = nullptr, *ipm_info = nullptr, *cost = nullptr,
               *dev = nullptr, *eta = nullptr, *Jaug_ref = nullptr, *hist = nullptr;
        double *vd = nullptr, *vs = nullptr, *vic = nullptr, *vtc = nullptr, *Ppen = nullptr, *Pf = nullptr;   // ptr.jl:399-432
        int *ipm_status = nullptr, *ipm_iters = nullptr, *active = nullptr, *scp_status = nullptr, *iters_done = nullptr,
            *n_active = nullptr, *cold_iters = nullptr, *snap = nullptr;
        long slab_stride = 0, work_stride = 0;
        bool ptr_ready = false;   // subproblem buffers allocated
        bool sub_ready = false;   // a subproblem has been solved (virtual controls available)
        // PTR run state
        scp_ptr_params pars{};
        int B = 0, iter = 0, hist_cap = 0;
        int na_cap = 0;
        int* na_ring = nullptr;              // pinned host copy of n_active after every enqueued iteration (scp_ptr_poll_iteration)
        int* na_dev = nullptr;               // the same ring ON THE DEVICE: what the multi-GPU all-reduce sums (scp_ptr_run_sharded)
        std::vector<hipEvent_t> na_ev;       // na_ev[k]: recorded behind the copy of iteration k
    } ptr;
};

#define HIP_TRY(h, call)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            if (h) (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);             \
            return SCP_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

struct Traj { double *xd, *ud, *p; };   // one trajectory triple on the device

#pragma GCC visibility push(hidden)
namespace scp {

template <class T>
static int dalloc(scp_problem* h, T** p, size_t count)
{
    void* v = nullptr;
    HIP_TRY(h, hipMalloc(&v, (count > 0 ? count : 1) * sizeof(T)));
    h->allocs.push_back(v);
    *p = (T*)v;
    return SCP_OK;
}

static Traj traj_guess(scp_problem* h) { return {h->ptr.guess_xd, h->ptr.guess_ud, h->ptr.guess_p}; }
static Traj traj_ref(scp_problem* h) { return {h->traj.ref_xd, h->traj.ref_ud, h->traj.ref_p}; }
static Traj traj_sol(scp_problem* h) { return {h->traj.sol_xd, h->traj.sol_ud, h->traj.sol_p}; }
// dst <- src for a trajectory triple: cp(dst, src, doubles per problem) copies one array; a model without parameters has no p
template <class Copy>
static int copy_traj(scp_problem* h, const Traj& dst, const Traj& src, Copy&& cp)
{
    const size_t nx = h->info.nx, nu = h->info.nu, np = h->npt, N = h->N;
    TRY(cp(dst.xd, src.xd, nx * N)); TRY(cp(dst.ud, src.ud, nu * N));
    if (np > 0) TRY(cp(dst.p, src.p, np));
    return SCP_OK;
}
// the `cp` of the structured path: the whole batch, device to device, on the handle's stream
static auto copy_d2d(scp_problem* h, int B)
{
    return [h, B](double* dst, const double* src, size_t n) -> int {
        HIP_TRY(h, hipMemcpyAsync(dst, src, n * (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        return SCP_OK;
    };
}

// ---- handle services, defined in scp_api.hip ----
int check_run(scp_problem* h, RunKind kind, const scp_sub* sub, const char* who);
int stamp_begin(scp_problem* h, int kind);
int stamp_end(scp_problem* h);
void stamps_collect(scp_problem* h);
void stamps_collect_ready(scp_problem* h);
int elapsed_out(scp_problem* h, double* seconds);
int discretize_dev(scp_problem* h, int B, const double* xd, const double* ud, const double* p, const DynBuf& d, int* feas,
                   const int* mask);
int merge_feas_dev(scp_problem* h, int B, const int* active);
int copy_dyn_out(scp_problem* h, int B, const DynBuf& d, double* A, double* Bm, double* Bp, double* F, double* r, double* E,
                 double* defect);
int upload_traj(scp_problem* h, int B, const double* xd, const double* ud, const double* p, double* dxd, double* dud, double* dp);
int download_traj(scp_problem* h, int B, bool from_sol, double* xd, double* ud, double* p, double* defect);
int feas_out(scp_problem* h, int B, const int* dfeas, uint8_t* feas);
int set_active_all(scp_problem* h, int* active, int B);

// ---- audit_entry.hip: every buffer of h->audit outside h->allocs and of h->lqr, h->cov and h->mc freed (scp_problem_destroy) ----
void audit_release(scp_problem* h);

// ---- guess_api.hip: traj.guess(N) of the handle's model on the device (guess_kernel.hpp); the end of h->guess.sg (scp_problem_destroy) ----
struct GuessArgs;
int guess_dev(scp_problem* h, const GuessArgs& g);
void starship_guess_free(StarshipGuessState* g);

// ---- scp_generic.hip: what the resident audit reads of the loop that owns the handle (h->run.sub) ----
struct SubRun {
    int B;                // batch size of the run
    bool iterated;        // false until the first iteration: get_host still returns the reference
    const double* d_pp;   // the run's per-problem parameters
    const int* status;    // [B] outer-loop status
};
SubRun sub_run(const scp_sub* s);

}  // namespace scp
#pragma GCC visibility pop
