/*
 * scp_mi355x.h -- C ABI of the MI355X-native SCP inner loop.
 *
 * Drop-in boundary for the two functions on the hot path of UW-ACL/SCPToolbox.jl
 * (paths relative to the reference root):
 *
 *   discretize!(ref, pbm)                 src/solvers/discretization.jl:160-217
 *   solve_subproblem!(spbm, constructor)  src/solvers/scp.jl:942-950
 *
 * plus the PTR iteration that strings them together (src/solvers/ptr.jl:448-532)
 * so that a Monte-Carlo batch can stay resident in HBM between iterations.
 *
 * Conventions
 *  - plain C, no torch types; all arrays are IEEE fp64, COLUMN-MAJOR exactly as
 *    Julia lays out Array{Float64} (a Julia array can be passed with `pointer`).
 *    A trailing batch dimension B is appended to every per-problem array.
 *  - every entry point returns an scp_status (0 = ok); nothing throws or aborts
 *    across this boundary (mirrors SCPStatus, src/utils/globals.jl:34-42).
 *  - `scp_handle` owns device scratch and one HIP stream; it is re-entrant per
 *    handle, there is no global state.  Caller owns every buffer it passes.
 *  - *_host entry points take host pointers (copies in/out, PCIe inclusive);
 *    *_dev entry points take device pointers and are asynchronous on the
 *    handle's stream (call scp_sync before reading results).
 *
 * The user closures f/A/B/F/s/C/D/G/gic/... of `TrajectoryProblem`
 * (src/parser/problem.jl:64-121) cannot cross an FFI; they are replaced by a
 * registry of compiled device models selected by `model_id` plus a POD
 * parameter blob.
 */
#ifndef SCP_MI355X_H
#define SCP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#include "scp_conic.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scp_problem *scp_handle;

typedef enum {
    SCP_OK = 0,
    SCP_ERR_BAD_ARGUMENT = 1,
    SCP_ERR_UNKNOWN_MODEL = 2,
    SCP_ERR_NO_DEVICE = 3,
    SCP_ERR_HIP = 4,
    SCP_ERR_ALLOC = 5,
    SCP_ERR_BATCH_TOO_LARGE = 6,
    SCP_ERR_UNSUPPORTED = 7,
    SCP_ERR_PEER = 8            /* scp_ptr_run_sharded: another rank failed inside a window (it says so through the window's all-reduce;
                                   every rank leaves the loop, no collective is left unmatched) */
} scp_status;

/* model registry (replaces traj.f/A/B/F..., src/parser/problem.jl:432-450) */
typedef enum {
    SCP_MODEL_DOUBLE_INTEGRATOR = 0, /* builder-defined, see DESIGN.md       */
    SCP_MODEL_QUADROTOR = 1,         /* test/examples/quadrotor              */
    SCP_MODEL_ROCKET_LANDING = 2,    /* builder-defined over rocket_landing  */
    SCP_MODEL_STARSHIP = 3,          /* test/examples/starship_flip          */
    SCP_MODEL_FREEFLYER = 4,         /* test/examples/freeflyer: p = [t_f; delta(6, N)] (np = 1 global + np_node = 6) */
    SCP_MODEL_OSCILLATOR = 5         /* test/examples/oscillator: actuator deadband, p = l1r(N) (np = 0, np_node = 1), ntc = 0 */
} scp_model_id;

/* DiscretizationType, src/parser/problem.jl:52 */
typedef enum { SCP_FOH = 0, SCP_IMPULSE = 1 } scp_disc_method;

/* Static description of a model (dimensions the caller needs to size buffers).
 *
 * PARAMETER VECTOR.  p = [global parameters (np); node parameters (np_node, N) column-major]: its length is
 * np + np_node * N.  Two models have node parameters: the free-flyer (p = [t_f; delta(6, N)], one room-SDF slack per room and
 * node, test/examples/freeflyer/parameters.jl:121-128) and the oscillator (p = l1r(N), one position one-norm slack
 * per node, test/examples/oscillator/parameters.jl:79, whose slacks also enter the running cost).  Dynamics, boundary conditions and parameter-only rows see the
 * global parameters; the constraints of node k (X rows, s) additionally see that node's own np_node parameters, and their
 * parameter Jacobians are COMPACT: np + np_node columns, column j < np = global parameter j, column np + i = entry
 * np + np_node (k - 1) + i of p. */
typedef struct {
    int nx, nu, np;   /* state / input / GLOBAL parameter dims (problem_set_dims!)   */
    int npF;          /* number of structurally non-zero columns of F (F8)      */
    int Fcols[8];     /* their 0-based column indices into p                    */
    int ns;           /* rows of the non-convex path constraint s               */
    int nic, ntc;     /* rows of the initial / terminal boundary conditions     */
    int npar;         /* doubles in the shared model parameter blob             */
    int npp;          /* doubles of per-problem data (Monte-Carlo ICs)          */
    int nl, nsoc, ng; /* convex-set rows: linear, second-order cones (dim 4), p-only */
    int structured;   /* 1: the stage-structured PTR fast path (scp_ptr_*) exists for this model; 0: subproblems run  */
                      /* through the generic conic path only (scp_sub_*, scp_scvx_*, scp_gusto_*)                  */
    int has_subproblem; /* 0: only discretize! / propagate / the initial guess exist; the subproblem entry points return
                           SCP_ERR_UNSUPPORTED (no such model at present) */
    int np_node;      /* parameters per node (see above): free-flyer 6, oscillator 1, every other model 0           */
    int global_rows_in_X; /* 1: the parameter-only rows are members of the convex STATE set X (soft under GuSTO and repeated
                           at every node, freeflyer/definition.jl:318-331), 0: of the input set U (hard, kept once)   */
    int linf_groups, linf_rows; /* the first linf_groups * linf_rows linear rows are LINF cones lowered to rows (MOI's
                           NormInfinity bridge); the rows of one cone share one cone indicator under GuSTO             */
    int s_input_free; /* 1: s(t, k, x, p) does not depend on the input -- admissible for GuSTO (gusto.jl:757-792)      */
} scp_model_info;

/* SCPScaling, src/solvers/scp.jl:39-49 (diagonals only; the reference's
 * Sx/Su/Sp are diagonal matrices, scp.jl:489-511). */
typedef struct {
    const double *Sx, *cx; /* [nx] */
    const double *Su, *cu; /* [nu] */
    const double *Sp, *cp; /* [np + np_node N] */
} scp_scaling;

typedef struct {
    int model_id;            /* scp_model_id                                    */
    const double *model_par; /* [npar] what the reference keeps in traj.mdl: every vehicle / environment constant of the
                                model, shared by the batch (layouts: the model headers in csrc/models) */
    int N;                   /* temporal grid nodes (pars.N)                     */
    int Nsub;                /* sub-interval integration nodes (pars.Nsub)       */
    int disc_method;         /* scp_disc_method (pars.disc_method)               */
    double feas_tol;         /* dynamic feasibility tolerance (pars.feas_tol)    */
    scp_scaling scale;       /* variable scaling (pbm.common.scale)              */
    int batch_capacity;      /* max problems per call                            */
    int device;              /* HIP device ordinal                               */
} scp_problem_desc;

int scp_model_query(int model_id, scp_model_info *info);

/*
 * Model constants that may change after scp_problem_create.  The reference keeps the model as mutable user data (traj.mdl) and
 * its homotopy examples change one constant between warm-started solves of ONE problem object (oscillator/tests.jl:60-77:
 * mdl.traj.kappa1).  Here a model marks the entries of its parameter blob that enter device-evaluated closures only (dynamics, s,
 * boundary conditions): mask[npar], 1 = may change.  Entries the host formulation froze into a template, the scaling or the cost
 * constant are never marked.  Oscillator: kappa1 (index 5); every other model: none.
 *
 * scp_problem_set_model_par replaces the handle's copy of the blob.  It returns SCP_ERR_BAD_ARGUMENT (message in scp_last_error)
 * and changes nothing if an unmarked entry differs from the handle's.  Every kernel receives the model constants BY VALUE at its
 * launch, so the new values hold for everything enqueued after the call and the change is ordered with the handle's stream: no
 * synchronisation is needed, before or after.
 */
int scp_model_par_mutable(int model_id, int *mask /* [npar], 1 = may change after create */);
int scp_problem_set_model_par(scp_handle h, const double *model_par /* [npar] */);

/*
 * Host-side evaluation of a compiled model's convex path constraints and cost at node k (1-based, t_k =
 * LinRange(0,1,N)[k]) -- what the reference obtains by calling the closures traj.X / traj.U (problem_set_X!/U!,
 * src/parser/problem.jl:500-542) and the cost (problem_set_terminal_cost!/running_cost!, :553-600) inside its
 * formulation code (src/solvers/scp.jl:685-734, 552-601).  With z = [x; u], npc = np + np_node (compact parameter
 * columns: the global parameters, then node k's own):
 *   L[nl,nz], Lp[nl,npc], l[nl]  (row-major)   L z + Lp [p_glob; p_node_k] + l <= 0
 *   Mm[4 nsoc,nz], m[4 nsoc]                    Mm z + m in Q^4 per cone (first row >= norm of the other three)
 *   Lg[ng,np], lg[ng]                           Lg p_glob + lg <= 0 (parameter-only rows)
 *   cost = [Qu[nu], lu[nu], lx[nx], tx[nx], tp[npc], Qp[npc]]:  Gamma = sum Qu_i u_i^2 + lu'u + lx'x,
 *          phi = tx'x_N + sum_j tp_j p_j + Qp_j p_j^2 over the global parameters + the same with the node entries of
 *          tp / Qp over the node parameters of EVERY node (free-flyer: -eps_sdf sum(delta))
 * Any pointer may be NULL.  Pure host code (no device needed): used by the host-side subproblem formulation.
 */
int scp_model_rows(int model_id, const double *model_par, int N, int k, double *L, double *Lp, double *l,
                   double *Mm, double *m, double *Lg, double *lg, double *cost);

/*
 * Number of cone indicators of the convex state set X per node -- define_conic_constraint! in its GuSTO mode
 * (src/parser/problem.jl:686-807): one per second-order cone and per linear row without an input column, one per LINF
 * group, and the parameter-only rows when global_rows_in_X.  A GuSTO template penalises nst = *nq + ns quantities per node.
 */
int scp_model_state_indicators(int model_id, const double *model_par, int N, int *nq);

/*
 * Host-side evaluation of a compiled model's closures at node k (1-based) and the point (x[nx], u[nu], p[np + np_node N]) --
 * what Julia obtains by calling traj.f / A / B / F (src/parser/problem.jl:432-450), traj.s / C / D / G (:560-600) and the
 * numerical mode of define_conic_constraint! (:783-803): f[nx], A[nx,nx], B[nx,nu] (column-major), F[nx,npF] (the
 * structurally non-zero columns), s[ns], C[ns,nx], D[ns,nu], G[ns,np + np_node] (row-major, compact parameter columns),
 * q[*nq] = the cone indicators of X.  Any output may be NULL.  No device needed: a maintainer checks a compiled model
 * against the closures it replaces with this call, and so do the CPU tests.
 */
int scp_model_eval_host(int model_id, const double *model_par, int N, int k, const double *x, const double *u,
                        const double *p, double *f, double *A, double *B, double *F, double *s, double *C, double *D,
                        double *G, double *q, int *nq);

int scp_problem_create(const scp_problem_desc *desc, scp_handle *out);
int scp_problem_destroy(scp_handle h);
int scp_sync(scp_handle h);
const char *scp_last_error(scp_handle h);
/*
 * Priority of the handle's HIP stream: level 0 = default, > 0 = higher, < 0 = lower (clamped to the device's range).  A caller that
 * splits a batch over several handles (sub-batches on their own streams) gives them DIFFERENT priorities so that the sub-batches do
 * not run in lockstep: with equal priorities the concurrent K3 launches share the chip evenly, finish together, and the short
 * kernels between two K3 launches (extract, discretize!, assemble) of all sub-batches then run on a nearly idle chip; with a
 * priority order the high-priority sub-batch's short kernels are dispatched ahead of the other's pending K3 workgroups and the chip
 * stays full.  The stream is drained and re-created; call it before a run is started.
 */
int scp_set_stream_priority(scp_handle h, int level);

/*
 * discretize!(ref, pbm) for a batch of B reference trajectories
 * (src/solvers/discretization.jl:160-217; FOH).  Reads
 *   xd[nx,N,B], ud[nu,N,B], p[np,B]
 * writes ref.dyn and the defects:
 *   A[nx,nx,N-1,B], Bm/Bp[nx,nu,N-1,B] (dyn.B[1], dyn.B[2]), F[nx,npF,N-1,B]
 *   (only the npF structurally non-zero columns, in Fcols order),
 *   r[nx,N-1,B], E[nx,nx,N-1,B], defect[nx,N-1,B], feas[B] (ref.feas),
 *   *seconds = device time of the call (ref.dyn.timing, :162,:214).
 * Any output pointer may be NULL to skip the copy-out (host variant).  The call stages its input in the handle's solution
 * buffers: during a run it overwrites the last solution that run's get_host returns.
 */
int scp_discretize_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p,
                              double *A, double *Bm, double *Bp, double *F, double *r, double *E,
                              double *defect, uint8_t *feas, double *seconds);

/*
 * Arithmetic of discretize! on this handle: bits = 64 (default; the reference's Float64, src/utils/basic_types.jl:31)
 * or 32 -- the "fp64 vs fp32 tolerance check" of the Starship configuration: state, Phi, the cooperative LU of
 * Phi \ [..] (discretization.jl:267), the RK4 accumulators and the model evaluation all run in fp32 inside K1; inputs
 * and outputs stay fp64 arrays.  SCP_ERR_UNSUPPORTED for IMPULSE and for models without an fp32 evaluation.
 */
int scp_set_discretize_precision(scp_handle h, int bits);

/* Same on device pointers owned by the caller; asynchronous on the handle's stream.
 * feas is int32[B] on the device. */
int scp_discretize_batch_dev(scp_handle h, int B, const double *xd, const double *ud, const double *p,
                             double *A, double *Bm, double *Bp, double *F, double *r, double *E,
                             double *defect, int32_t *feas);

/*
 * propagate(sol, pbm; res) for a batch (src/solvers/discretization.jl:515-562).  FOH (:536-541): integrates the nonlinear
 * dynamics from xd[:,1,b] over LinRange(0,1,res) with the inputs linearly interpolated between the nodes and returns the
 * continuous-time state samples xc[nx,res,B] (the values of the reference's `Trajectory(tc, xc_vals, :linear)`).
 * IMPULSE (:542-560, handles created with SCP_IMPULSE): every interval restarts from its node with the model's impulse
 * response applied, x0 = xd[:,k] + f(t_k, -k, xd[:,k], ud[:,k], p), and coasts with idle inputs over LinRange(t_k, t_{k+1},
 * subres), subres = ceil(res / (N - 1)); xc[nx, 1 + (N-1) subres, B]: sample 0 = xd[:,1], then the intervals' samples (the
 * reference's sample times are those grids with the first time of every interval shifted by sqrt(eps)).  Host pointers.
 * Like scp_discretize_batch_host it stages its input in the handle's solution buffers and so overwrites a run's last solution.
 */
int scp_propagate_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, int res,
                             double *xc);

/*
 * Continuous-time audit of a batch of solutions: what a user asks of SCPSolution(history) (src/solvers/scp.jl:196-245) once
 * xc = propagate(last_sol, pbm; res) is there -- did it arrive, did it stay inside the constraints BETWEEN the grid nodes,
 * what did it cost -- answered on the device, fused into the propagation: no sample of xc is stored or copied.
 *
 * Samples tc = LinRange(0,1,res), res >= 2; xc_j = the single-shooting RK4 propagation of scp_propagate_batch_host (FOH);
 * uc_j = the first-order-hold input at tc_j.  The model functions are called with t = tc_j and the node index k_j = the
 * 1-based index of the last grid node <= tc_j (N at t = 1).  One record audit[SCP_AUDIT_WIDTH, B] per problem:
 *   [0], [1]   max over the samples and rows of s(tc_j, k_j, xc_j, uc_j, p), and the tc_j where it is attained
 *   [2], [3]   the same for the linear rows L z + Lp p + l of the convex sets X and U together, z = [xc_j; uc_j]
 *   [4], [5]   the same for the second-order cones, as ||z_1..3|| - z_0
 *   [6]        max_i (Lg p + lg)_i, the parameter-only rows
 *   [7]        ||g_tc(xc(1), p, pp)||_inf, the open-loop residual of the terminal boundary condition
 *   [8]        ||Sx^-1 (xc(1) - xd[:,N])||_inf, the open-loop drift from the discrete terminal state
 *   [9]        the cost flown, phi(xc(1), p) + trapz over tc of Gamma(xc_j, uc_j)  (normalised time, like the discrete J)
 *   [10]       number of samples at which any of [0], [2], [4]'s families exceeds viol_tol
 *   [11]       1 if any sample or quantity was not finite, else 0
 *   [12..15]   0 (reserved)
 * On ties the first sample wins; a family without rows reports -Inf and the time 0.
 *
 * SCP_ERR_UNSUPPORTED (with an error text where there is a handle) for IMPULSE handles and for models with node parameters
 * (np_node > 0, the free-flyer): a row of X at node k reads that node's own slack there, and between the nodes no such
 * slack exists.  SCP_ERR_BAD_ARGUMENT for res < 2, a NULL audit and a missing p / pp where the model has one;
 * SCP_ERR_BATCH_TOO_LARGE for B above the handle's capacity.
 */
#define SCP_AUDIT_WIDTH 16
/*
 * The audit of B trajectories given on the host (xd[nx,N,B], ud[nu,N,B], p[np,B], pp[npp,B]); *seconds = device time of the
 * kernel.  Like scp_propagate_batch_host it stages its input in the handle's solution buffers and so overwrites a run's last
 * solution (the run's pp is left alone).
 */
int scp_audit_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                         int res, double viol_tol, double *audit, double *seconds);
/*
 * The audit of the batch RESIDENT in the handle: exactly the trajectories the owning run's *_get_host would return at this
 * moment (structured PTR, SCvx, GuSTO or generic PTR) with that run's pp; problems whose SCP status is not "solved" (0) are
 * skipped and their record is NaN.  Only SCP_AUDIT_WIDTH * B doubles cross PCIe and no buffer of the run is modified:
 * get_host and further iterations behave as if the call had not been made.  SCP_ERR_BAD_ARGUMENT, with an error text,
 * when no run owns the handle.
 */
int scp_audit_resident(scp_handle h, int res, double viol_tol, double *audit, double *seconds);
/*
 * The same record for ONE problem computed on the host by the same code (no device needed): xd[nx,N], ud[nu,N], p[np],
 * pp[npp], Sx[nx] = the diagonal of the state scaling -> audit[SCP_AUDIT_WIDTH].  The counterpart of scp_model_eval_host
 * for the audit: lets a maintainer and the CPU tests check it against the closures it replaces.
 */
int scp_model_audit_host(int model_id, const double *model_par, int N, const double *xd, const double *ud,
                         const double *p, const double *pp, const double *Sx, int res, double viol_tol, double *audit);

/*
 * Interval-parallel audit (multiple shooting).  The single-shooting audit above accumulates its drift over the whole
 * horizon; SCP's own feasibility criterion, the defect of discretize!, is per interval.  Here every interval k = 1 .. N-1 of
 * the grid t_k = LinRange(0,1,N)[k] is flown from ITS OWN node over sub = max(2, ceil(res / (N - 1))) samples
 * tc_j = LinRange(t_k, t_{k+1}, sub)[j] (the reference's subres, at least one RK4 step), one device thread per
 * (problem, interval), and handles created with SCP_IMPULSE are audited too:
 *   FOH      x0 = xd[:,k]; u(t) = c ud[:,k] + (1 - c) ud[:,k+1], c = (t_{k+1} - t) / (t_{k+1} - t_k), t clamped to the interval
 *   IMPULSE  x0 = xd[:,k] + f(t_k, -k, xd[:,k], ud[:,k], p) as in scp_propagate_batch_host; the dynamics coast with u = 0; the
 *            row families and Gamma see z_j = [xc_j; ud[:,k]], the impulse that opened the interval; ud[:,N] is never flown
 * The model functions get the node index k at every sample but the last one, which gets k+1.  Sample 0 of an interval and
 * the last sample of the interval before it are at the same time; both are evaluated and both count.
 *
 * Per-interval record intervals[SCP_AUDIT_INTERVAL_WIDTH, N-1, B]:
 *   [0], [1]   max over the interval's samples and rows of s, and the tc_j where it is attained (first sample wins; no
 *              rows: -Inf, 0);  [2], [3] the same for the linear rows of X and U;  [4], [5] for the cones, ||z_1..3|| - z_0
 *   [6]        the defect ||Sx^-1 (x(t_{k+1}) - xd[:,k+1])||_inf of the flown end state
 *   [7]        trapz of Gamma over the interval's samples
 *   [8]        samples of this interval at which any family exceeds viol_tol
 *   [9]        1 if anything of this interval was not finite
 *   [10], [11] in the record of interval N-1 only: ||g_tc(x_end, p, pp)||_inf and phi(x_end, p); 0 elsewhere
 *   [12..15]   0
 * Summary record audit[SCP_AUDIT_WIDTH, B], the fold of the interval records IN INTERVAL ORDER (so that both outputs are
 * independent of B, of the place of a problem in the batch and of the launch geometry), in the layout of the record above:
 *   [0..5] the maxima with their times (strict >: the earliest interval wins a tie), [6] the parameter-only rows, [7] = [10] of
 *   the last interval, [8] the LARGEST DEFECT over the intervals, [9] phi + (((I_1 + I_2) + ...) + I_{N-1}), [10] the sum of
 *   the counts, [11] the OR of the flags (and of a non-finite [6] or [9]), [12] the 1-based interval of the largest defect (the first
 *   wins), [13] 1.0 = a multiple-shooting record (single-shooting records hold 0 there), [14] sub, [15] 0.
 * mask / failed problems: the summary and all interval records of the problem are NaN.
 *
 * `intervals` may be NULL: then only SCP_AUDIT_WIDTH * B doubles come back (the interval records are 128 (N-1) B bytes).
 * Staging, ownership, masking and the error codes are those of scp_audit_batch_host / scp_audit_resident, except that IMPULSE
 * handles are accepted; *seconds = device time of the two kernels without the copies.
 */
#define SCP_AUDIT_INTERVAL_WIDTH 16
int scp_audit_intervals_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                                   int res, double viol_tol, double *audit, double *intervals /* may be NULL */, double *seconds);
int scp_audit_intervals_resident(scp_handle h, int res, double viol_tol, double *audit, double *intervals /* may be NULL */,
                                 double *seconds);
/*
 * The same two outputs for ONE problem on the host by the same code: audit[SCP_AUDIT_WIDTH], intervals[SCP_AUDIT_INTERVAL_WIDTH,
 * N-1] or NULL.  disc_method = SCP_FOH or SCP_IMPULSE; SCP_ERR_UNSUPPORTED for SCP_IMPULSE with a model without an
 * impulsive-input form and for models with node parameters.
 */
int scp_model_audit_intervals_host(int model_id, const double *model_par, int N, int disc_method, const double *xd, const double *ud,
                                   const double *p, const double *pp, const double *Sx, int res, double viol_tol,
                                   double *audit, double *intervals /* [16, N-1] or NULL */);

/*
 * Dispersed-flight audit.  Every flight above happens in a perfect world: it starts at exactly xd[:,1], flies exactly the
 * optimised input and uses exactly the constants the optimiser used.  Here every problem b is flown D times off-nominal in ONE
 * launch, one device thread per (problem, flight); FOH handles of the four auditable models.  Flight d = 1 .. D is the
 * single-shooting audit of scp_audit_batch_host -- same samples, same RK4, same k_j rule -- with three changes:
 *   initial state  x(0) = xd[:,1,b] + dx0[:,d,b], in physical units
 *   actuators      at every time, stage times included, the flown input is u'(t) = ugain[:,d,b] o u_foh(t) + ubias[:,d,b]
 *                  (component-wise); the dynamics, the row families of U, the cones and Gamma all see u': the flight is
 *                  audited as flown
 *   truth model    par_true[npar], one per call, or NULL = the handle's own constants: the blob, taken as given like the one of
 *                  scp_problem_create, replaces the handle's constants for everything the flight evaluates (dynamics, s, rows,
 *                  cost, g_tc); any entry may differ, the handle is not changed
 * p and pp are not dispersed, and the drift [8] is measured against the undispersed xd[:,N,b].  dx0[nx,D,B], ugain[nu,D,B],
 * ubias[nu,D,B]; NULL means 0, 1 and 0.  flags = SCP_DISP_SHARED: the three arrays carry no batch dimension ([., D]) and every
 * problem flies the same D dispersions.
 *
 * flights[SCP_AUDIT_WIDTH, D, B]: one record per flight in exactly the single-shooting layout ([12..15] = 0).  May be NULL:
 * then the records stay on the device.
 * summary[SCP_AUDIT_WIDTH, B]: the fold of a problem's flight records IN FLIGHT ORDER by one thread per problem, so that both
 * outputs are independent of B, of the place of a problem in the batch and of the launch geometry.  A flight whose record
 * [11] != 0 is counted in [11] and takes no part in any other field; m = the number of counted flights:
 *   [0], [1]   max over the counted flights of the s maximum, and the 1-based flight attaining it (strict >: the first wins;
 *              no finite value: -Inf, 0);  [2], [3] the same for the linear rows;  [4], [5] for the cones
 *   [6]        the parameter-only rows, of the first counted flight (-Inf when m = 0)
 *   [7]        max over the counted flights of ||g_tc||_inf;  [12] the 1-based flight attaining it (the first wins)
 *   [8]        max of the drift
 *   [9]        mean cost (((c_1 + c_2) + ...) + c_m) / m;  [15] max cost
 *   [10]       flights with a violation count > 0
 *   [11]       flights that were not finite
 *   [13]       2.0 (single-shooting records hold 0 there, multiple-shooting ones 1.0)
 *   [14]       D
 * With m = 0: [7], [8], [9], [15] are NaN and [12] = 0.  A masked or failed problem: NaN in its summary and all its flights.
 *
 * Staging, ownership, masking and *seconds (the two kernels without the copies) follow scp_audit_batch_host /
 * scp_audit_resident.  SCP_ERR_UNSUPPORTED (with an error text on a handle) for IMPULSE handles and for models with node
 * parameters; SCP_ERR_BAD_ARGUMENT for D < 1, res < 2, a NULL summary, unknown flag bits and a missing p / pp;
 * SCP_ERR_BATCH_TOO_LARGE for B above the handle's capacity; SCP_ERR_ALLOC when the flight buffer -- 16 D batch_capacity
 * doubles, owned by the handle, allocated on first use and rebuilt when D grows -- cannot be allocated.
 */
#define SCP_DISP_SHARED 1u
int scp_audit_dispersed_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                                   int res, double viol_tol, int D, const double *dx0, const double *ugain, const double *ubias,
                                   unsigned flags, const double *par_true, double *summary, double *flights /* may be NULL */,
                                   double *seconds);
int scp_audit_dispersed_resident(scp_handle h, int res, double viol_tol, int D, const double *dx0, const double *ugain,
                                 const double *ubias, unsigned flags, const double *par_true, double *summary,
                                 double *flights /* may be NULL */, double *seconds);
/*
 * The same two outputs for ONE problem on the host by the same code: dx0[nx,D], ugain[nu,D], ubias[nu,D] (each may be NULL),
 * summary[SCP_AUDIT_WIDTH], flights[SCP_AUDIT_WIDTH, D] or NULL.  model_par plays the handle's blob, par_true (or NULL) the
 * truth model's.  SCP_ERR_UNSUPPORTED for models with node parameters, SCP_ERR_UNKNOWN_MODEL for an unknown model_id.
 */
int scp_model_audit_dispersed_host(int model_id, const double *model_par, const double *par_true, int N, const double *xd,
                                   const double *ud, const double *p, const double *pp, const double *Sx, int res,
                                   double viol_tol, int D, const double *dx0, const double *ugain, const double *ubias,
                                   double *summary, double *flights /* [16, D] or NULL */);

/*
 * LQR gains on the discretisation.  discretize! leaves A_k, B-_k, B+_k of every interval of every problem on the device; a
 * batched time-varying discrete LQR synthesis turns them into sample-and-hold tracking gains at the node rate.  FOH handles of
 * the four auditable models.  For one problem, with Q = diag(qx), R = diag(ru) and P <- diag(qf), for k = N-1 down to 1:
 *   Phi = A_k,  Gam = B-_k + B+_k            the exact map of an input deviation HELD over the interval
 *   H = R + Gam' P Gam                        (Cholesky, nu <= 4)
 *   K_k = H^-1 Gam' P Phi                     [nu, nx]
 *   P <- Q + Phi' P (Phi - Gam K_k),  then P <- (P + P') / 2
 * qx[nx] >= 0, qf[nx] >= 0, ru[nu] > 0 in physical units, shared by the batch.
 *
 * K[nu, nx, N-1, B] (column-major like every array here; may be NULL in the handle-level calls: the gains then stay on the device).
 * info[SCP_LQR_INFO_WIDTH, B]:
 *   [0]  1 when a pivot of H was <= 0 or anything was not finite; the K of that problem is then NaN throughout, [1], [2] too
 *   [1]  max over k of max |K_k|
 *   [2]  trace of P at node 1
 *   [3]  0
 * One wavefront lane per entry of P (nx^2 <= 64), floor(64 / nx^2) problems per wavefront; a problem's result does not depend on
 * B or on its place in the batch, bit for bit.
 *
 * scp_lqr_gains_batch_host stages xd / ud / p like scp_audit_batch_host, runs discretize! into A / B- / B+ buffers the handle
 * owns for this purpose (allocated on first use; SCP_ERR_ALLOC when they cannot be) and then the Riccati kernel.  The gains stay
 * RESIDENT in the handle, together with the B they were made for, until the next gains call.  scp_lqr_gains_resident does the
 * same about the trajectories the owning run's get_host would return; failed problems hold NaN in K and info; no buffer of the
 * run is modified.  *seconds: discretize! and the Riccati kernel without the copies.
 * SCP_ERR_BAD_ARGUMENT for a NULL, negative or non-finite weight (ru: also 0) and a NULL info; SCP_ERR_UNSUPPORTED (with an error
 * text) for IMPULSE handles and models with node parameters; SCP_ERR_BATCH_TOO_LARGE as everywhere.
 */
#define SCP_LQR_INFO_WIDTH 4
int scp_lqr_gains_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *qx,
                             const double *ru, const double *qf, double *K /* may be NULL */, double *info, double *seconds);
int scp_lqr_gains_resident(scp_handle h, const double *qx, const double *ru, const double *qf, double *K /* may be NULL */,
                           double *info, double *seconds);
/*
 * The same recursion for ONE problem on the host by the same code; no model enters it: A[nx,nx,N-1], Bm, Bp[nx,nu,N-1],
 * K[nu,nx,N-1], info[SCP_LQR_INFO_WIDTH].  (nx, nu) is one of the pairs of the four auditable models -- (2,1), (6,4), (7,4),
 * (8,3) -- SCP_ERR_UNSUPPORTED for any other.
 */
int scp_lqr_gains_host(int nx, int nu, int N, const double *A, const double *Bm, const double *Bp, const double *qx,
                       const double *ru, const double *qf, double *K, double *info);

/*
 * Closed-loop tracking audit: the dispersed-flight audit with the loop closed by gains K[nu, nx, N-1, B] (scp_lqr_gains_*, or
 * any others).  dx0 / ugain / ubias / SCP_DISP_SHARED / par_true, the masking, staging, ownership and the flights / summary
 * buffers are those of scp_audit_dispersed_batch_host.  The sampling grid is steps >= 1 RK4 steps per interval,
 * res = steps (N-1) + 1 samples at LinRange(0, 1, res): every step lies inside one interval, node k is sample (k-1) steps.
 * One flight:
 *   1. x = xd[:,1] + dx0; update the hold for k = 1; take sample 0
 *   2. for j = 0 .. res-2: if j > 0 and j mod steps = 0 update the hold for k = j / steps + 1; take the RK4 step; take sample j+1
 * The hold update is du = -K_k (x - xd[:,k]).  The commanded input at any time of the step, stage times included, is
 * u_foh(t) + du; the flown input is ugain o (u_foh(t) + du) + ubias; the dynamics, the U rows, the cones and Gamma all see the
 * flown input.  A sample at a node is audited with the hold that was in force over the step that ended there.  The commanded
 * input is NOT saturated: the U rows and cones report what the feedback asked for.
 *
 * K: a host array, or NULL = the gains resident in the handle (SCP_ERR_BAD_ARGUMENT with an error text when there are none or
 * they were made for another B).
 * flights[SCP_AUDIT_WIDTH, D, B]: the single-shooting layout [0..11], and (strict >: the first occurrence wins a tie)
 *   [12]  max over the hold updates of ||Su^-1 du||_inf, the feedback effort;  [13] the 1-based node attaining it
 *   [14]  max over the nodes 1 .. N of ||Sx^-1 (x(t_k) - xd[:,k])||_inf;      [15] the node attaining it
 * summary[SCP_AUDIT_WIDTH, B]: the fold of scp_audit_dispersed_batch_host over [0..11] of the flights, with [13] = 3.0.
 * Refusals: those of the dispersed audit, and SCP_ERR_BAD_ARGUMENT for steps < 1.
 */
int scp_audit_tracking_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                                  const double *K /* NULL = resident */, int steps, double viol_tol, int D, const double *dx0,
                                  const double *ugain, const double *ubias, unsigned flags, const double *par_true,
                                  double *summary, double *flights /* may be NULL */, double *seconds);
int scp_audit_tracking_resident(scp_handle h, const double *K /* NULL = resident */, int steps, double viol_tol, int D,
                                const double *dx0, const double *ugain, const double *ubias, unsigned flags,
                                const double *par_true, double *summary, double *flights /* may be NULL */, double *seconds);
/* The same two outputs for ONE problem on the host by the same code; Su[nu] scales the effort [12]; K[nu,nx,N-1] is required. */
int scp_model_audit_tracking_host(int model_id, const double *model_par, const double *par_true, int N, const double *xd,
                                  const double *ud, const double *p, const double *pp, const double *Sx, const double *Su,
                                  const double *K, int steps, double viol_tol, int D, const double *dx0, const double *ugain,
                                  const double *ubias, double *summary, double *flights /* [16, D] or NULL */);

/*
 * Closed-loop covariance audit: the linear covariance analysis of every solution with the loop closed by gains K[nu, nx, N-1, B]
 * (scp_lqr_gains_*, or any others) -- what a guidance engineer asks for before spending flights on scp_audit_tracking_*.  FOH
 * handles of the four auditable models.  Shared by the batch, in physical units like the LQR weights: sig0[nx] >= 0 the initial
 * 1-sigma, sigu[nu] >= 0 the 1-sigma of a white input disturbance held over each interval, sigw[nx] >= 0 the 1-sigma of additive
 * state noise per interval; nsig > 0 the sigma level.  For one problem:
 *   Sigma_1 = diag(sig0^2);  for k = 1 .. N-1:  Phi = A_k,  Gam = B-_k + B+_k  (as in scp_lqr_gains_*),  A_cl = Phi - Gam K_k
 *   Sigma_{k+1} = A_cl Sigma_k A_cl' + Gam diag(sigu^2) Gam' + diag(sigw^2),  then Sigma <- (Sigma + Sigma') / 2
 * and at node k (1-based)
 *   state 1-sigma    sigma_{k,i} = sqrt(max(Sigma_k[i,i], 0)),                                  k = 1 .. N
 *   effort 1-sigma   e_{k,a} = sqrt(max((K_k Sigma_k K_k')[a,a], 0)) / Su[a],                   k = 1 .. N-1
 *   sigma margins    of every row of the three sampled families of scp_audit_batch_host (s, the linear rows, the cones; not the
 *                    parameter-only rows), evaluated at the nominal (xd[:,k], ud[:,k], p) with the (t, k) that audit passes at
 *                    the sample coinciding with node k.  A row has a value v and a gradient [g_x, g_u] over z = [x; u]: s rows
 *                    (C_i, D_i); linear rows the row of L; a cone with w = M z + m the value ||w[1:4]|| - w[0] and the gradient
 *                    (w[1:4]' / ||w[1:4]||) M[1:4,:] - M[0,:]  (-M[0,:] when ||w[1:4]|| = 0).  The hold update makes
 *                    dz = [I; -K_k] dx: g = g_x - g_u K_k at k <= N-1, g = g_x at k = N; var = max(g Sigma_k g', 0);
 *                    margin = -v / sqrt(var) when var > 0, else +Inf for v <= 0 and -Inf for v > 0
 *   terminal         tau_i = sqrt(max((H Sigma_N H')[i,i], 0)) with H = d g_tc / dx at xd[:,N]
 *
 * summary[SCP_COV_WIDTH, B]; nodes and indices are 1-based, ties go to the smallest node, then the smallest state:
 *   [0]        1 when anything was not finite ([1..15] are then NaN), else 0
 *   [1..3]     max over k, i of sigma_{k,i} / Sx[i]; the node; the state attaining it
 *   [4], [5]   max over k <= N-1 and a of e_{k,a}; the node
 *   [6], [7]   the smallest margin over the s rows and the nodes; the node (+Inf, 0 when the model has no such rows or no
 *              margin is below +Inf)
 *   [8], [9]   the same for the linear rows;  [10], [11] the same for the cones
 *   [12]       max_i tau_i (0 when ntc = 0)
 *   [13]       trace(Sx^-1 Sigma_N Sx^-1)
 *   [14]       number of (node, row) pairs with margin < nsig
 *   [15]       0
 * Optional outputs, copied only when asked for (NULL otherwise): sig[nx, N, B] the state 1-sigma values, and
 * nodes[SCP_COV_NODE_WIDTH, N, B] per node: [0] max_i sigma / Sx, [1] max_a e (NaN at node N), [2..4] the smallest margin per
 * family at that node, [5] trace(Sx^-1 Sigma_k Sx^-1), [6], [7] 0.
 *
 * Two launches: a node-parallel pre-pass (one thread per (problem, node)) that evaluates the model's rows into a row table the
 * handle owns (allocated on first use; SCP_ERR_ALLOC when it cannot be), and the covariance chain, built like the Riccati kernel:
 * one wavefront lane per entry of Sigma, floor(64 / nx^2) problems per wavefront.  A problem's result does not depend on B or on
 * its place in the batch, bit for bit.
 *
 * scp_audit_covariance_batch_host stages xd / ud / p / pp like scp_audit_batch_host and ALWAYS runs discretize! about them into
 * the A / B- / B+ buffers of scp_lqr_gains_* (the result never depends on an earlier call; resident gains stay as they are).
 * K: a host array, or NULL = the gains resident in the handle, by the rule and with the error texts of scp_audit_tracking_*.
 * scp_audit_covariance_resident does the same about the trajectories the owning run's get_host would return; failed problems hold
 * NaN in every output; no buffer of the run is modified.  *seconds: discretize! and the two kernels without the copies.
 * SCP_ERR_BAD_ARGUMENT for a NULL, negative or non-finite sig0 / sigu / sigw, nsig <= 0 or not finite, and a NULL summary;
 * SCP_ERR_UNSUPPORTED (with the error texts of the other audits) for IMPULSE handles and models with node parameters;
 * SCP_ERR_BATCH_TOO_LARGE as everywhere.
 */
#define SCP_COV_WIDTH 16
#define SCP_COV_NODE_WIDTH 8
int scp_audit_covariance_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                                    const double *K /* NULL = resident */, const double *sig0, const double *sigu,
                                    const double *sigw, double nsig, double *summary, double *sig /* may be NULL */,
                                    double *nodes /* may be NULL */, double *seconds);
int scp_audit_covariance_resident(scp_handle h, const double *K /* NULL = resident */, const double *sig0, const double *sigu,
                                  const double *sigw, double nsig, double *summary, double *sig /* may be NULL */,
                                  double *nodes /* may be NULL */, double *seconds);
/*
 * The pre-pass for ONE problem on the host by the same code: xd[nx,N], ud[nu,N], p[np], pp[npp], K[nu,nx,N-1] (required) ->
 * rows[nx+1, nrow, N] with nrow = ns + nl + nsoc of scp_model_query in family order (s, linear, cone), a row = g[nx] then v, and
 * Hf[ntc, nx].  SCP_ERR_UNSUPPORTED for the models with node parameters.
 */
int scp_model_covariance_rows_host(int model_id, const double *model_par, int N, const double *xd, const double *ud,
                                   const double *p, const double *pp, const double *K, double *rows, double *Hf);
/*
 * The chain for ONE problem on the host by the same code; no model enters it: A[nx,nx,N-1], Bm, Bp[nx,nu,N-1], K[nu,nx,N-1],
 * nrow[3] = the rows per family of rows[nx+1, nrow[0] + nrow[1] + nrow[2], N], Hf[ntc, nx], Sx[nx], Su[nu] ->
 * summary[SCP_COV_WIDTH], sig[nx,N] or NULL, nodes[SCP_COV_NODE_WIDTH,N] or NULL.  (nx, nu) is one of the pairs of the four
 * auditable models -- (2,1), (6,4), (7,4), (8,3) -- SCP_ERR_UNSUPPORTED for any other.
 */
int scp_covariance_host(int nx, int nu, int N, const double *A, const double *Bm, const double *Bp, const double *K,
                        const int *nrow, const double *rows, int ntc, const double *Hf, const double *Sx, const double *Su,
                        const double *sig0, const double *sigu, const double *sigw, double nsig, double *summary,
                        double *sig /* may be NULL */, double *nodes /* may be NULL */);

/*
 * Monte-Carlo audit: D >= 2 NOISY closed-loop flights per problem through the nonlinear dynamics, under exactly the disturbance
 * model of scp_audit_covariance_*, and the sample statistics of the node errors -- the check of that audit's linear prediction.
 * FOH handles of the four auditable models; sig0 / sigu / sigw as there (shared by the batch, physical units), K and steps as
 * in scp_audit_tracking_*.  Flight d = 1 .. D is the tracking flight with ugain = 1, ubias = 0 and
 *   1. x = xd[:,1] + sig0 o xi0
 *   2. at node k < N the hold update du = -K_k (x - xd[:,k]), then w_k = sigu o xiu_k is drawn
 *   3. the flown input is (u_foh(t) + du) + w_k over the whole interval, stage times included; the dynamics, the U rows, the cones
 *      and Gamma see it; the effort is measured on du alone
 *   4. after the last RK4 step of interval k and BEFORE that sample is audited: x += sigw o xiw_{k+1}; the sample at node k+1 and
 *      that node's tracking error see the kicked state
 * Linearised, this is the Sigma recursion of the covariance audit (Gam = B- + B+ is the response to an input offset held over the
 * interval).  The xi are standard normals of a counter-based generator inside the kernel: Philox4x32-10 keyed by the two halves
 * of `seed`, counter (pair index i / 2, node k, d - 1, kind) with kind 0 = xi0 (k = 0), 1 = xiu_k (k = 1 .. N-1), 2 = xiw_k
 * (k = 2 .. N); from the output words r0 .. r3, u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53 and u2 likewise from r2, r3;
 * rho = sqrt(-2 ln u1), component 2q = rho cos(2 pi u2), component 2q+1 = rho sin(2 pi u2).  A draw depends on (seed, kind, k, d,
 * i) only: every problem of a batch sees the same disturbances (common random numbers: the right default for ranking the
 * problems of a batch), and a problem's result does not depend on B or on its place in the batch, bit for bit.
 * scp_mc_draws_host returns the n normals z of one draw and, when asked, the 4 ceil(n / 2) output words behind them.
 *
 * Nothing of size N D B is stored: at every node the errors e = x - xd[:,k] and du / Su of the flights are reduced across the
 * wavefront in registers by a fixed tree (the xor butterfly over the lanes 0 .. 63; a problem owns ceil(D / 64) whole wavefronts,
 * whose partial sums are added in wavefront order).  A flight COUNTS at node k when e and (k < N) du / Su are all finite.
 * moments[1 + 2 nx + nu, N, B] (NULL: not copied), per node k:
 *   [0]            n_k, the flights counted
 *   [1 .. nx]      the sample mean m_i of e_i
 *   [nx+1 .. 2nx]  the sample standard deviation s_i = sqrt(max((sum e_i^2 - (sum e_i)^2 / n_k) / (n_k - 1), 0))
 *   [2nx+1 ..]     rms_a = sqrt(sum (du_a / Su_a)^2 / n_k); NaN at node N
 * all NaN but [0] where n_k < 2.  stat[SCP_MC_STAT_WIDTH, B]; nodes and indices 1-based, ties go to the smallest node, then the
 * smallest index; a maximum to which no node contributes is NaN with the indices 0:
 *   [0..2]     max over k, i of s_i / Sx[i]; its node; its state
 *   [3], [4]   max over k, i of |m_i| / Sx[i]; its node -- the bias that nonlinearity puts on the mean, which the linear analysis
 *              cannot see
 *   [5], [6]   max over k < N and a of rms_a; its node
 *   [7]        min over k of n_k
 * flights[SCP_AUDIT_WIDTH, D, B] (may be NULL): the records of scp_audit_tracking_*, unchanged in layout; summary
 * [SCP_AUDIT_WIDTH, B]: their fold as there, with [13] = 4.0.
 *
 * Staging, masking, the resident gains (K = NULL), the error texts and *seconds (the three kernels without the copies) follow
 * scp_audit_tracking_*; the partial sums live in a buffer the handle owns, allocated on first use and rebuilt when D needs more
 * wavefronts (SCP_ERR_ALLOC when it cannot be).  SCP_ERR_BAD_ARGUMENT for D < 2, steps < 1, a NULL, negative or non-finite
 * sigma and a NULL summary or stat; SCP_ERR_UNSUPPORTED (with the other audits' texts) for IMPULSE handles and the models with node
 * parameters; SCP_ERR_UNKNOWN_MODEL and SCP_ERR_BATCH_TOO_LARGE as everywhere.
 */
#define SCP_MC_STAT_WIDTH 8
int scp_audit_montecarlo_batch_host(scp_handle h, int B, const double *xd, const double *ud, const double *p, const double *pp,
                                    const double *K /* NULL = resident */, int steps, double viol_tol, int D, uint64_t seed,
                                    const double *sig0, const double *sigu, const double *sigw, double *summary, double *stat,
                                    double *moments /* may be NULL */, double *flights /* may be NULL */, double *seconds);
int scp_audit_montecarlo_resident(scp_handle h, const double *K /* NULL = resident */, int steps, double viol_tol, int D,
                                  uint64_t seed, const double *sig0, const double *sigu, const double *sigw, double *summary,
                                  double *stat, double *moments /* may be NULL */, double *flights /* may be NULL */,
                                  double *seconds);
/* The same outputs for ONE problem on the host by the same code and the same tree, no device: summary[16], stat[8],
 * moments[1 + 2 nx + nu, N] or NULL, flights[16, D] or NULL; K[nu,nx,N-1] is required. */
int scp_model_audit_montecarlo_host(int model_id, const double *model_par, int N, const double *xd, const double *ud,
                                    const double *p, const double *pp, const double *Sx, const double *Su, const double *K,
                                    int steps, double viol_tol, int D, uint64_t seed, const double *sig0, const double *sigu,
                                    const double *sigw, double *summary, double *stat, double *moments /* may be NULL */,
                                    double *flights /* [16, D] or NULL */);
/* z[n] of the draw (seed, kind, k, d) and, when words is not NULL, its 4 ceil(n / 2) Philox output words; SCP_ERR_BAD_ARGUMENT
 * for kind outside 0 .. 2, k < 0, d < 1, n < 1 or a NULL z. */
int scp_mc_draws_host(uint64_t seed, int kind, int k, int d, int n, double *z, unsigned *words /* may be NULL */);

/* ------------------------------------------------------------------------ */
/* PTR: solve_subproblem! and the outer loop                                  */
/* ------------------------------------------------------------------------ */

/* PTR.Parameters (src/solvers/ptr.jl:57-71) minus N/Nsub/disc_method/feas_tol
 * (fixed at scp_problem_create) and `solver`/`solver_opts`, which select ECOS
 * in the reference and are replaced by the in-house structured interior-point
 * solver's options. */
typedef struct {
    int iter_max;          /* pars.iter_max                                     */
    double wvc, wtr;       /* virtual-control / trust-region weights            */
    double eps_abs, eps_rel; /* pars.ε_abs, pars.ε_rel                          */
    double q_tr, q_exit;   /* only Inf is implemented (all reference tests)     */
    /* subproblem solver options (ECOS defaults: feastol=abstol=reltol=1e-8, maxit=100) */
    int ipm_max_iter;
    double ipm_feastol, ipm_abstol, ipm_reltol;
    double ipm_reg;        /* static dual regularisation (ECOS: delta); a factorisation that breaks down is repeated with 10x */
    int ipm_nref;          /* iterative-refinement steps per Newton solve       */
    double ipm_ref_gap;    /* ... applied only once relgap < ipm_ref_gap        */
    double ipm_ref_tol;    /* ... and skipped when the residual of the computed  */
                           /* direction is below ipm_ref_tol * ipm_feastol       */
    int ipm_stall;         /* stop after this many non-improving iterations     */
    int ipm_split_step;    /* != 0: separate primal / dual step lengths when the  */
                           /* subproblem has no quadratic cost term (default 0:   */
                           /* -10 % iterations but more iteration-limit exits)   */
    /* Warm start of the subproblem solver inside scp_ptr_iterate (PTR iteration >= 2).  Every solve leaves two SNAPSHOTS in the
     * workspace: the iterates at which its complementarity measure mu = gap / degree first fell below ipm_warm_mu_coarse and
     * below ipm_warm_mu (interior points close to the central path).  The next solve of that problem starts from the fine one
     * when the previous solution moved less than ipm_warm_dev (scaled inf-norm deviation, scp.jl:909-931), from the coarse one
     * otherwise (the coarse one only if the last COLD solve of that problem needed at least ipm_warm_min_cold iterations: it
     * pays where cold solves are slow), instead of the two-solve cold start -- provided the previous solve succeeded; a
     * warm-started solve that fails is repeated cold.  Same optimum
     * (DESIGN.md section 2.1); 0 disables.  Round 6 added two more levels (fields at the end of this struct). */
    int ipm_warm;
    double ipm_warm_mu, ipm_warm_dev;
    int ipm_warm_min_cold;
    int ipm_wpe;           /* kernel variant of the subproblem solver: 0 = chosen from this handle's batch size, 1 = one */
                           /* wave per SIMD (512 registers, batches that cannot fill the chip twice), 2 = two waves per */
                           /* SIMD (callers that run several handles concurrently pass 2: the chip is shared)           */
    double ipm_warm_mu_coarse;   /* coarse snapshot level of the warm start (<= 0: 1e-1); appended in round 4 */
    /* Round 6: FOUR snapshot levels.  A solve keeps the iterates at which mu first fell below ipm_warm_mu_coarse > ipm_warm_mu_mid >
     * ipm_warm_mu > ipm_warm_mu_vfine, and the next solve of the problem starts from the FINEST level whose deviation bound covers the
     * deviation d of the previous solution: d <= ipm_warm_dev_vfine -> very fine, d <= ipm_warm_dev -> fine, d <= ipm_warm_dev_mid -> mid,
     * otherwise coarse (a level whose snapshot was never taken falls through to the next coarser one).  The right level is a matter of
     * scale: the new problem's residual at an old iterate is of the order of d; an iterate at mu = 1e-10 is the best start when the
     * reference moved by 1e-8 (the solve then needs 1 ... 3 iterations) and a trap when it moved by 1e-4 (steps of 0.01 until the
     * iteration limit of a warm attempt, then the cold repeat).  <= 0: the defaults 1e-5, 1e-1, 1e-10, 1e-6 of these four fields.  The
     * fine level itself has NO default in the library: ipm_warm_mu <= 0 with ipm_warm != 0 is SCP_ERR_BAD_ARGUMENT and ipm_warm_dev is
     * taken as given (the levels above were tuned together with ipm_warm_mu = 1e-8, ipm_warm_dev = 1e-3).
     * Two fixed rules keep the levels honest: a level is refreshed only by an iterate within two decades below it (a warm solve that
     * starts far below a level leaves that snapshot alone), and after a solve that ended ALMOST_OPTIMAL the very fine level is not used. */
    double ipm_warm_mu_mid, ipm_warm_dev_mid, ipm_warm_mu_vfine, ipm_warm_dev_vfine;
} scp_ptr_params;

/* per-problem subproblem solver exit status (MOI.TerminationStatusCode subset) */
typedef enum { SCP_SOLVER_OPTIMAL = 0, SCP_SOLVER_ALMOST_OPTIMAL = 1, SCP_SOLVER_ITERATION_LIMIT = 2,
               SCP_SOLVER_NUMERICAL_ERROR = 3 } scp_solver_status;

/* width of one history record (doubles): J, J_tr, J_vc, J_aug, deviation, improv_rel, feas,
 * solver status, solver iterations, active, gap, pres, dres, (3 reserved) */
#define SCP_HIST_WIDTH 16

/*
 * Start a batched PTR solve (PTR.solve, src/solvers/ptr.jl:448-466): uploads the initial
 * guesses xd[nx,N,B], ud[nu,N,B], p[np,B] (traj.guess) and the per-problem data
 * pp[npp,B] (Monte-Carlo initial/terminal conditions), then discretises the guess
 * (generate_initial_guess -> SubproblemSolution -> discretize!, ptr.jl:548-555).
 */
int scp_ptr_init_host(scp_handle h, int B, const scp_ptr_params *pars, const double *xd, const double *ud,
                      const double *p, const double *pp);

/*
 * Same, with the initial guesses generated ON THE DEVICE by the model's own guess rule (traj.guess,
 * src/parser/problem.jl:686-700: straight-line state, nominal input and parameter -- see csrc/models): only
 * pp[npp,B] crosses PCIe, a Monte-Carlo batch never touches the host.
 */
int scp_ptr_init_guess_host(scp_handle h, int B, const scp_ptr_params *pars, const double *pp);

/*
 * One PTR iteration for every still-active problem (ptr.jl:468-523): formulate (K2) ->
 * solve_subproblem! (K3, scp.jl:942-950) -> extract + discretize! of the new point (K1) ->
 * stopping criterion / reference update (K4).  *n_active = problems that continue; the caller
 * all-reduces it across GPUs (the only collective on the path).
 */
int scp_ptr_iterate(scp_handle h, int *n_active);

/*
 * The same iteration split in two: scp_ptr_iterate_async only ENQUEUES it on the handle's stream (several iterations may
 * be in flight; problems that have stopped are skipped on the device), scp_ptr_poll waits for the stream and returns the
 * active count of the last enqueued iteration.  A caller that splits its batch over several handles (one stream each)
 * and enqueues ahead keeps the GPU full while the slowest problems of one launch finish (the subproblem solver's
 * iteration count varies 3x between problems); scp_ptr_iterate == async + poll.
 * scp_ptr_poll_iteration returns the active count at the end of iteration `iteration` (1-based, already enqueued; 0 beyond
 * iter_max) and waits for THAT iteration only: a multi-GPU caller enqueues window k + 1, then reads and all-reduces the count of
 * window k, so the stream never drains at a window boundary (scptoolbox.jl_amd/ptr.py::group_run_resident(pipelined=True)).
 */
int scp_ptr_iterate_async(scp_handle h);
int scp_ptr_poll(scp_handle h, int *n_active);
int scp_ptr_poll_iteration(scp_handle h, int iteration, int *n_active);

/*
 * Results of the batch: final discrete trajectories (SCPSolution.xd/ud/p, scp.jl:105-119),
 * status[B] (0 = "SCP_SOLVED", 1 = "SCP_FAILED"), iterations[B], cost[4,B] = (J, J_tr, J_vc,
 * J_aug) of the last subproblem, feas[B], defect[nx,N-1,B], and the per-iteration history
 * hist[SCP_HIST_WIDTH, B, iter_max].  Any pointer may be NULL.
 */
int scp_ptr_get_host(scp_handle h, double *xd, double *ud, double *p, int32_t *status, int32_t *iterations,
                     double *cost, uint8_t *feas, double *defect, double *hist);

/* Convenience: init + iterate until no problem is active + get (single GPU). */
int scp_ptr_solve_batch_host(scp_handle h, int B, const scp_ptr_params *pars, const double *xd, const double *ud,
                             const double *p, const double *pp, double *xd_out, double *ud_out, double *p_out,
                             int32_t *status, int32_t *iterations, double *cost, uint8_t *feas, double *seconds);

/*
 * solve_subproblem!(spbm, constructor) for a batch (scp.jl:942-950 with the PTR subproblem of
 * ptr.jl:213-293): given reference trajectories, formulates and solves the convex subproblem about
 * them and returns the un-scaled solution x[nx,N,B], u[nu,N,B], p[np,B], the cost split
 * cost[4,B] = (J, J_tr, J_vc, J_aug), trust-region radii eta[2N+1,B] = (ηx, ηu, ηp), the solver
 * status / iteration count and info[8,B] = (pcost, dcost, gap, pres, dres, relgap, merit, best_it).
 * Like the reference it then discretises the new point (defect[nx,N-1,B], feas[B]).
 */
int scp_ptr_solve_subproblem_batch_host(scp_handle h, int B, const scp_ptr_params *pars, const double *xd_ref,
                                        const double *ud_ref, const double *p_ref, const double *pp, double *x,
                                        double *u, double *p, double *cost, double *eta, int32_t *solver_status,
                                        int32_t *solver_iters, double *info, double *defect, uint8_t *feas,
                                        double *seconds);

/*
 * Virtual controls and penalty epigraph variables of the LAST solved subproblem (after
 * scp_ptr_solve_subproblem_batch_host or scp_ptr_iterate) -- what the reference's SubproblemSolution(spbm) reads with
 * value(...) (src/solvers/ptr.jl:399-432): vd[nx,N-1,B] (E_k vd_k = linearised dynamics defect, with the reference's
 * discretised E_k = ref.dyn.E, ptr.jl:805), vs[ns,N,B], vic[nic,B], vtc[ntc,B], P[N,B] (P_k = ||E_k vd_k||_1 +
 * ||vs_k||_1, ptr.jl:813-887), Pf[2,B] = (||vic||_1, ||vtc||_1).  They are eliminated analytically from the reduced
 * subproblem the device solves and re-evaluated from its solution.  Any pointer may be NULL.
 */
int scp_ptr_get_virtual_controls_host(scp_handle h, double *vd, double *vs, double *vic, double *vtc, double *P,
                                      double *Pf);

/*
 * `traj.guess(N)` (src/parser/problem.jl:686-700) of the compiled model for a Monte-Carlo batch, evaluated on the device
 * (§8(f)4): pp[npp,B] -> xd[nx,N,B], ud[nu,N,B], p[np,B] on the host.  Any registered model: straight-line guesses
 * (quadrotor/definition.jl:60-90 and the builder-defined problems), the free-flyer's axis-by-axis path with SLERP attitude
 * (freeflyer/definition.jl:84-186, quaternion.jl:483-490), and -- since round 4 -- the Starship's own guess
 * (starship_flip/definition.jl:97-445) for every instance: bang-bang flip simulated with RK4 (one thread per instance), the
 * terminal-descent programs of all candidate durations as one batch of the conic engine, reconstruction of attitude / thrust /
 * rate / mass on the device.  An instance for which the reference would raise an error (no velocity crossing, no feasible descent
 * duration) gets the straight-line guess instead; scp_guess_failures returns how many of the last call did.
 */
int scp_guess_batch_host(scp_handle h, int B, const double *pp, double *xd, double *ud, double *p);
int scp_guess_failures(scp_handle h);

/* Restart the batch from the initial guesses uploaded by the last scp_ptr_init_host, entirely on the
 * device (D2D copy + discretize! of the guess): the inputs stay resident in HBM. */
int scp_ptr_restart(scp_handle h);

/* Cumulative device seconds (HIP events on the handle's stream) and launch counts per kernel since the
 * last reset: index 0 discretize (K1), 1 assemble (K2), 2 structured IPM (K3), 3 extract+update (K4).
 * reset != 0 clears the counters after reading. */
int scp_get_kernel_timing(scp_handle h, double seconds[4], long launches[4], int reset);

/* Diagnostic: phase counters of the last structured-IPM launch for problem b (100 MHz wall-clock ticks):
 * G, G', factor, rhs+forward, backward, aux recovery, -, total. */
int scp_debug_get_ipm_profile(scp_handle h, int b, long long *ticks8);

/* Diagnostic: copy out the assembled stage-form subproblem data of problem b (layout of
 * csrc/stage_problem.hpp) after scp_ptr_solve_subproblem_batch_host / scp_ptr_iterate.
 * *n_doubles returns the slab length; buf may be NULL to query it. */
int scp_debug_get_stage_problem(scp_handle h, int b, double *buf, long *n_doubles);

/* ------------------------------------------------------------------------ */
/* Generic subproblem pipeline: any SCP subproblem as a conic template        */
/* (PTR with q_tr in {1,2,4,Inf}, SCvx, correct_convex!, ...)                 */
/* ------------------------------------------------------------------------ */

/*
 * The reference formulates a new JuMP model per iteration (`Subproblem(pbm, iter, ref)` + add_dynamics! ... add_cost!,
 * src/solvers/ptr.jl:213-293,467-480; scvx.jl:225-303,483-490; scp.jl:657-895).  Every coefficient it writes is affine
 * in a few per-problem numbers -- ref.dyn, the reference trajectory, the Jacobians of s and of the boundary conditions
 * about it, the trust-region radius.  The host formulates ONCE (scptoolbox.jl_amd/subproblem.py) and hands over
 *   - the sparsity pattern of the standard form of include/scp_conic.h, and
 *   - for each value array an affine map  value[i] = val0[i] + sum_{t = ptr[i]}^{ptr[i+1]-1} coef[t] * src[sidx[t]]
 * over the per-problem SOURCE VECTOR the device fills (layout: scp_sub_source_layout).
 */
typedef struct {
    int len;
    const double *val0; /* [len]                */
    const int *ptr;     /* [len + 1]            */
    const int *sidx;    /* [ptr[len]]           */
    const double *coef; /* [ptr[len]]           */
} scp_affine_map;

typedef struct {
    int n, p, m, l, ncones;     /* standard form sizes, m = l + sum(q)                                   */
    const int *q;
    const int *Pp, *Pi, *Ap, *Ai, *Gp, *Gi; /* CSC patterns (P: upper triangle)                           */
    scp_affine_map c, b, h, Gx, Ax, Px;     /* value maps over the source vector                          */
    int nsrc, nscal;            /* source vector length / trailing algorithm scalars (SCvx: eta)          */
    const int *ix, *iu, *ip;    /* positions of the scaled variables xh[nx,N], uh[nu,N], ph[np] in x      */
    int nfun;                   /* linear functionals of the conic solution reported per problem           */
    scp_affine_map fun;         /* fun[j] = val0[j] + sum coef * x[sidx]  (e.g. trapz(P) + sum(Pf))        */
} scp_sub_template;

typedef struct scp_sub *scp_sub_handle;

/* offsets[0..20] of the 20 source segments (doubles, per problem; every segment column-major):
 * xref(nx,N) uref(nu,N) pref(np + np_node N) A(nx,nx,N-1) Bm Bp(nx,nu,N-1) F(nx,npF,N-1) r(nx,N-1) E(nx,nx,N-1) C(ns,nx,N)
 * D(ns,nu,N) Gs(ns,np + np_node,N) rs(ns,N) H0(nic,nx) K0(nic,np) l0(nic) Hf(ntc,nx) Kf(ntc,np) lf(ntc) scal(nscal);
 * *nsrc = total.  Gs is the COMPACT parameter Jacobian of s at its node (scp_model_info). */
int scp_sub_source_layout(scp_handle h, int nscal, int *offsets, int *nsrc);

int scp_sub_create(scp_handle h, const scp_sub_template *T, scp_sub_handle *out);
int scp_sub_destroy(scp_sub_handle s);
/* statistics of the subproblem's conic engine: the 16 values of scp_conic_stats (include/scp_conic.h) */
int scp_sub_stats(scp_sub_handle s, long long stats[16]);
const char *scp_sub_last_error(scp_sub_handle s);

/*
 * solve_subproblem!(spbm, constructor) (src/solvers/scp.jl:942-950) for a batch and ANY template: discretises the
 * reference trajectories xd_ref[nx,N,B], ud_ref[nu,N,B], p_ref[np,B] (discretize!), linearises the non-convex
 * constraints / boundary conditions about them, fills the conic values (gather), solves (conic_ipm_kernel), un-scales
 * x[nx,N,B], u[nu,N,B], p[np,B] (value(blk), block.jl:368-394) and discretises the new point (defect[nx,N-1,B],
 * feas[B]).  scal[nscal,B]: algorithm scalars; fun[nfun,B]; xconic[n,B]: the whole conic solution (virtual controls,
 * epigraph variables, ...); status/iters/info[8,B] as scp_conic_solve_batch_host.  Any output may be NULL.
 */
int scp_sub_solve_batch_host(scp_sub_handle s, int B, const double *xd_ref, const double *ud_ref, const double *p_ref,
                             const double *pp, const double *scal, const scp_conic_opts *opts, double *x, double *u,
                             double *p, double *fun, double *xconic, int32_t *status, int32_t *iters, double *info,
                             double *defect, uint8_t *feas, double *seconds);

/* SCvx.Parameters (src/solvers/scvx.jl:60-81) minus N/Nsub/disc_method/feas_tol (fixed at scp_problem_create) and
 * q_tr (fixed by the template). */
typedef struct {
    int iter_max;
    double lam;                       /* λ: virtual-control penalty weight                  */
    double rho_0, rho_1, rho_2;       /* ρ thresholds of the update rule (scvx.jl:1000-1045) */
    double beta_sh, beta_gr;          /* shrink / growth factors                             */
    double eta_init, eta_lb, eta_ub;  /* trust-region radius                                 */
    double eps_abs, eps_rel;
    double q_exit;                    /* norm of solution_deviation (scp.jl:909-931): any q >= 1 or Inf */
    scp_conic_opts solver;            /* subproblem solver options (pars.solver_opts)        */
} scp_scvx_params;

/* width of one SCvx history record: L, L_pen, L_aug, J_ref, J_sol, pre_improv, act_improv, rho, eta, eta_next, accepted,
 * stop, deviation, feas, solver status, solver iterations */
#define SCP_SCVX_HIST_WIDTH 16

/*
 * SCvx.solve (src/solvers/scvx.jl:459-540) for a batch, resident on the device.  `sub`: an SCvx subproblem template
 * (nscal = 1: eta; fun[0] = trapz(P) + sum(Pf)); `proj`: a correct_convex! template of the same problem handle or NULL
 * (generate_initial_guess projects the guess, scvx.jl:555-565, scp.jl:275-361).  init uploads the guesses and pp[npp,B];
 * iterate = formulate + solve_subproblem! + discretize! + check_stopping_criterion! + update_trust_region!
 * (scvx.jl:711-770, 924-1045) for every active problem; get returns the LAST subproblem solution of every problem
 * (SCPSolution(history), scp.jl:196-245), status[B] (0 solved, 1 failed, 2 guess projection failed), iterations[B],
 * cost[2,B] = (J of the reference, J of the last solution), feas[B], defect, hist[SCP_SCVX_HIST_WIDTH, B, iter_max].
 */
int scp_scvx_init_host(scp_sub_handle sub, scp_sub_handle proj, int B, const scp_scvx_params *pars, const double *xd,
                       const double *ud, const double *p, const double *pp);
int scp_scvx_iterate(scp_sub_handle sub, int *n_active);
int scp_scvx_get_host(scp_sub_handle sub, double *xd, double *ud, double *p, int32_t *status, int32_t *iterations,
                      double *cost, uint8_t *feas, double *defect, double *hist);

/* GuSTO.Parameters (src/solvers/gusto.jl:59-85) minus N/Nsub/disc_method/feas_tol (fixed at scp_problem_create).  pen / hom must
 * be those the template was built with (:softplus = exponential cones in the template).  q_tr must be the norm the template was built with: the update rule
 * measures the trust-region violation of the new point in it (gusto.jl:1172-1185, 1318-1340). */
typedef struct {
    int iter_max;
    double lam_init, lam_max;         /* soft-penalty weight: initial value, failure threshold                     */
    double rho_0, rho_1;              /* model-accuracy thresholds of the update rule (gusto.jl:1310-1427)          */
    double beta_sh, beta_gr;          /* trust-region shrink / growth factors                                       */
    double gamma_fail;                /* lambda growth factor after an infeasible / trust-violating step            */
    double eta_init, eta_lb, eta_ub;  /* trust-region radius                                                        */
    double mu;                        /* eta *= mu^(1 + k - iter_mu) for k >= iter_mu (kappa, gusto.jl:264)          */
    int iter_mu;
    double eps_abs, eps_rel;
    double q_tr, q_exit;              /* trust-region norm / norm of solution_deviation: q >= 1 or Inf                */
    int nst;                          /* soft-penalised quantities per node in the template: the cone indicators of X
                                         (scp_model_state_indicators) + ns; anything else is refused                  */
    scp_conic_opts solver;
    int pen;                          /* soft penalty (gusto.jl:79-80, 966-1031): 0 = :quad, lambda max(0, f)^2 (default); 1 = :softplus,
                                         lambda log(1 + exp(hom f)) / hom through exponential cones (the template's penalty
                                         variables are then the w of gusto.jl:1000-1029).  Appended in round 4. */
    double hom;                       /* homotopy parameter of :softplus                                              */
} scp_gusto_params;

/* columns of one GuSTO history record (width SCP_SCVX_HIST_WIDTH): L, L_st, L_tr, J_aug, J_st, rho, eta, lambda, eta_next,
 * lambda_next, flags (1 accepted | 2 stop | 4 trust region violated | 8 constraints feasible | 16 dynamically feasible),
 * deviation, solver status, solver iterations, dynamics error, its normalisation */

/*
 * GuSTO.solve (src/solvers/gusto.jl:425-502) for a batch, resident on the device.  `sub`: a GuSTO template (nscal = 2:
 * eta, lambda -- lambda weights the QUADRATIC cost, i.e. the P values are per problem; fun = the penalty variables
 * v_tr[N] then v_st[nst, N]); `proj`: a correct_convex! template or NULL (generate_initial_guess, gusto.jl:516-521).
 * iterate = formulate + solve_subproblem! + discretize! + solution costs (:391-407) + check_stopping_criterion!
 * (:1203-1230) + update_trust_region! (:1245-1293, 1310-1427).  get: as scp_scvx_get_host with cost[2,B] = (J_aug of the
 * reference, J_aug of the last solution) and the GuSTO history columns.
 */
int scp_gusto_init_host(scp_sub_handle sub, scp_sub_handle proj, int B, const scp_gusto_params *pars, const double *xd,
                        const double *ud, const double *p, const double *pp);
int scp_gusto_iterate(scp_sub_handle sub, int *n_active);
int scp_gusto_get_host(scp_sub_handle sub, double *xd, double *ud, double *p, int32_t *status, int32_t *iterations,
                       double *cost, uint8_t *feas, double *defect, double *hist);

/* PTR.Parameters (src/solvers/ptr.jl:57-71) for the generic path: minus N/Nsub/disc_method/feas_tol (fixed at scp_problem_create)
 * and q_tr (fixed by the template); cost_const = the constant the template's objective omits (cost of the scaling offsets). */
typedef struct {
    int iter_max;
    double wvc, wtr;
    double eps_abs, eps_rel;
    double q_exit;                    /* norm of solution_deviation (scp.jl:909-931): any q >= 1 or Inf */
    double cost_const;
    scp_conic_opts solver;
} scp_ptr_generic_params;

/*
 * PTR.solve (src/solvers/ptr.jl:448-532) for a batch, resident on the device, over ANY PTR template (build_ptr: q_tr in
 * {1, 2, 4, Inf}; fun[0] = trapz(P) + sum(Pf), fun[1] = trapz(eta_x) + trapz(eta_u) + eta_p) -- the loop of the models
 * without the stage-structured fast path (Starship, free-flyer) and of the non-Inf trust-region norms.  iterate = formulate +
 * solve_subproblem! + discretize! + cost split (:753-895) + check_stopping_criterion! (:908-932) + ref = sol (:509) for
 * every active problem.  get: as scp_ptr_get_host (cost[4,B] = J, J_tr, J_vc, J_aug of the last subproblem; hist with the
 * SCP_HIST_WIDTH columns).
 */
int scp_ptr_generic_init_host(scp_sub_handle sub, int B, const scp_ptr_generic_params *pars, const double *xd, const double *ud,
                              const double *p, const double *pp);
int scp_ptr_generic_iterate(scp_sub_handle sub, int *n_active);
int scp_ptr_generic_get_host(scp_sub_handle sub, double *xd, double *ud, double *p, int32_t *status, int32_t *iterations,
                             double *cost, uint8_t *feas, double *defect, double *hist);
/*
 * Device-resident continuation: what PTR.solve(pbm, warm) does with warm = the run's own last solutions (ptr.jl:448-466,
 * scp.jl:532-539), without the batch leaving the device.  Every instance's last solution -- of the last iteration it ran,
 * failed instances included -- becomes its reference; status, iteration count, history and cost records are cleared, J_aug of
 * the reference is NaN and every instance is active again; the reference is discretised under the handle's CURRENT model
 * constants (scp_problem_set_model_par).  pars: the parameters of the new stage, or NULL to keep the run's.  iterate / get_host
 * work afterwards as after init and get_host reports the current stage.  SCP_ERR_BAD_ARGUMENT unless a generic PTR run of `sub`
 * owns the problem handle.
 */
int scp_ptr_generic_continue(scp_sub_handle sub, const scp_ptr_generic_params *pars /* NULL: as before */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Multi-GPU behind the boundary (reference: the sequential Monte-Carlo loop `for trial = 1:num_trials`,
 * test/examples/quadrotor/tests.jl:171-184, is the axis that is sharded).  One process per GPU; every rank owns a contiguous
 * shard of the batch (scp_shard_range) in one or more handles (sub-batches on their own HIP streams); the ONLY collective is the
 * per-window all-reduce (SUM, one int64) of the number of still-active problems, issued by RCCL ON THE DEVICE: the count never
 * visits the host between the update kernel that produces it and the collective that sums it.
 *
 *   rank 0:  scp_comm_unique_id(id)  ->  ship the 128 bytes to the other ranks (MPI.bcast, a file, torch.distributed ...)
 *   all   :  scp_comm_create(id, rank, world, device, &comm)            (ncclCommInitRank; librccl.so is loaded at this call)
 *            scp_ptr_init_guess_host(part[i], B_i, &pars, pp_i)         (this rank's shard, as on one GPU)
 *            scp_ptr_run_sharded(comm, part, nparts, lookahead, &iterations, &collectives)
 *            scp_ptr_get_host(part[i], ...)
 *
 * scp_ptr_run_sharded enqueues WINDOWS of `lookahead` PTR iterations on every handle's stream; behind each window a one-thread
 * kernel sums the handles' device-resident active counts and ncclAllReduce adds the ranks' sums on a separate high-priority
 * stream (ordered by events, no stream is drained), the result lands in a pinned ring.  The host enqueues window w + 1 BEFORE it
 * reads the global count of window w, so neither the compute streams nor the host wait for a collective; every rank reads the
 * same sequence of global counts, hence all ranks enqueue the same number of windows (lockstep) -- one more than needed, whose
 * launches skip the stopped problems on the device.  comm == NULL (or world == 1): the same loop without RCCL.
 * *iterations = PTR iterations executed until no problem was active on any rank (<= iter_max), *collectives = all-reduces issued.
 * ------------------------------------------------------------------------------------------------------------------------- */
#define SCP_COMM_ID_BYTES 128
typedef struct scp_comm *scp_comm_handle;
int scp_comm_unique_id(unsigned char id[SCP_COMM_ID_BYTES]);
/* the LOCAL steps scp_comm_create takes before its collective part (load RCCL, select the device, create a stream), without the collective:
 * a host calls it on every rank and agrees on the results (MPI.Allreduce, torch.distributed ...) BEFORE scp_comm_create, whose
 * ncclCommInitRank would otherwise wait for ever for a rank that failed locally; the error text is in scp_comm_last_error(NULL) */
int scp_comm_preflight(int device);
int scp_comm_create(const unsigned char id[SCP_COMM_ID_BYTES], int rank, int world, int device, scp_comm_handle *out);
void scp_comm_destroy(scp_comm_handle c);
const char *scp_comm_last_error(scp_comm_handle c);
/* blocking helper on the communicator's stream (tests, final reductions of scalar statistics): *value <- SUM over ranks */
int scp_comm_all_reduce_sum_i64(scp_comm_handle c, long long *value);
/* contiguous shard [lo, hi) of a global batch of n_total problems owned by `rank` of `world` (sizes differ by at most one) */
void scp_shard_range(long n_total, int rank, int world, long *lo, long *hi);
int scp_ptr_run_sharded(scp_comm_handle c, scp_handle *parts, int nparts, int lookahead, int *iterations, int *collectives);

#ifdef __cplusplus
}
#endif
#endif /* SCP_MI355X_H */
