// Forced harmonic oscillator with an actuator deadband, test/examples/oscillator/{parameters,definition}.jl:
// x = [r; v], u = [aa; ar; l1aa; l1adiff] (actual and reference acceleration, two one-norm slacks), dynamics
// r' = v, v' = aa - w0^2 r - 2 zeta w0 v, all times the fixed duration t_f (definition.jl:161-236).  The deadband
// aa = ar if |ar| > a_db else 0 is the non-convex constraint s, smoothed by the logical OR of src/utils/helper.jl:623-807
// with the sharpness kappa1 -- the constant the reference's homotopy sweeps between warm-started solves (tests.jl:60-77).
//
// PARAMETERS.  p = l1r(N): one position one-norm slack per node (np = 0 global, np_node = 1).  The slack of node k appears
// in the X rows of its node and, unlike the free-flyer's slacks, in the RUNNING cost (definition.jl:116-142):
// node_par_in_running_cost.  No terminal condition (ntc = 0) and no terminal cost.
//
// DISCRETISATION.  A is constant but not nilpotent (eigenvalues t_f w0 (-zeta +- i sqrt(1 - zeta^2))), so the variational
// form (K1v) and the reference form (K1) are two different RK4 recurrences.  Measured on the CPU against the restatement of
// derivs_foh (tests/oscillator_util.py: variational_vs_reference) on perturbed trajectories, largest relative difference of
// A, B-, B+, r, E:  1.6e-8 at the reference's grid N = 30, Nsub = 10 (normalised step 3.8e-3), 3.1e-10 at 1.4e-3 (Nsub = 25),
// 6.8e-11 at 9.9e-4 (Nsub = 36), 6.4e-12 at 5.5e-4 (Nsub = 64) -- fourth order in the step, but also growing with the length
// of the interval: the same step 1.0e-3 gives 3.3e-10 at N = 6 and 2.3e-11 at N = 100.  The largest step that meets 1e-10
// whatever N is about 7e-4 (N = 2: 4.2e-10 at 1.0e-3, 5.4e-11 at 6.0e-4), i.e. Nsub >= 51 at N = 30.  No grid anybody uses
// is that fine, and the reference-form kernel costs nothing at nx = 2: var_form_max_step = 0.
#pragma once
#include "model_common.hpp"

namespace scp {

struct Oscillator : ModelDefaults {
    static constexpr int id = 5;
    static constexpr int nx = 2, nu = 4, np = 0, npF = 0;
    static constexpr int np_node = 1;                 // l1r_k >= |r_k|
    static constexpr bool node_par_in_running_cost = true;
    static constexpr bool const_jacobian = true;
    static constexpr double var_form_max_step = 0.0;  // see DISCRETISATION above: no K1v, hence no Amul / Bcol either
    static constexpr bool has_subproblem = true;
    static constexpr bool structured = false;
    static constexpr bool s_input_free = false;       // s is a function of the input alone
    // [zeta, w0, a_db, a_max, tf, kappa1, alpha, gamma, r_nrml] (parameters.jl:69-115; r_nrml = the reference's traj.r0 in
    // the cost normalisation, a constant of the batch while r0 itself is per-problem data)
    static constexpr int npar = 9;
    // entries of the blob that enter device-evaluated closures only (here: s) and may therefore change after
    // scp_problem_create (scp_problem_set_model_par): kappa1.  Everything else is frozen into the host's template
    // (rows, cost), the scaling or the dynamics' discretisation the caller already holds
    static constexpr bool par_mutable(int i) { return i == 5; }

    struct Params {
        double zeta, w0, a_db, a_max, tf, kappa1, alpha, gamma, r_nrml;
    };
    static Params make_params(const double* par)
    {
        return Params{par[0], par[1], par[2], par[3], par[4], par[5], par[6], par[7], par[8]};
    }
    static constexpr int Fcol(int) { return 0; }

    // f, A (col-major nx*nx), B (nx*nu), Fc (unused: no parameter enters the dynamics)
    SCP_DEV static void dyn(const Params& P, double, int, const double (&x)[nx], const double (&u)[nu], const double*,
                            double (&f)[nx], double (&A)[nx * nx], double (&B)[nx * nu], double (&Fc)[nx])
    {
        f[0] = P.tf * x[1];
        f[1] = P.tf * (u[0] - P.w0 * P.w0 * x[0] - 2.0 * P.zeta * P.w0 * x[1]);
        A[0] = 0.0; A[1] = -P.tf * P.w0 * P.w0; A[2] = P.tf; A[3] = -2.0 * P.tf * P.zeta * P.w0;
        zero(B);
        B[1] = P.tf;                                   // B[v, aa]
        Fc[0] = 0.0; Fc[1] = 0.0;
    }
    SCP_DEV static void action(double (&)[nx]) {}
    static constexpr bool has_fp32 = false;
    // IMPULSE (definition.jl:170-186, 216-227: the k < 0 branch): dx = [0; aa], B[v, aa] = 1, neither scaled by t_f
    static constexpr bool has_impulse = true;
    SCP_DEV static void impulse(const Params&, double, int, const double (&)[nx], const double (&u)[nu], const double*,
                                double (&dx)[nx], double (&B)[nx * nu])
    {
        dx[0] = 0.0; dx[1] = u[0];
        zero(B);
        B[1] = 1.0;
    }

    SCP_DEV static double lin(double a, double b, int n, int j)
    {
        const double t = (double)j / (double)(n - 1);
        return (1.0 - t) * a + t * b;
    }
    SCP_DEV static void free_step(const Params& P, double (&x)[nx], double h)
    {
        auto F = [&](const double (&y)[nx], double (&d)[nx]) {
            d[0] = P.tf * y[1];
            d[1] = P.tf * (0.0 - P.w0 * P.w0 * y[0] - 2.0 * P.zeta * P.w0 * y[1]);
        };
        double k1[nx], k2[nx], k3[nx], k4[nx], y[nx];
        F(x, k1);
        for (int i = 0; i < nx; i++) y[i] = x[i] + h / 2 * k1[i];
        F(y, k2);
        for (int i = 0; i < nx; i++) y[i] = x[i] + h / 2 * k2[i];
        F(y, k3);
        for (int i = 0; i < nx; i++) y[i] = x[i] + h * k3[i];
        F(y, k4);
        for (int i = 0; i < nx; i++) x[i] = x[i] + h / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    }
    // initial guess at node k (0-based) of N (definition.jl:71-114): the free response from pp = [r0, v0], flown by RK4 on
    // LinRange(0, 1, 1000) (helper.jl:411-424) and sampled linearly at the node's time (linterp, helper.jl:107-118, with
    // get_interval :84-90: the interval whose left end is the last grid point strictly below t) -- every node integrates up
    // to its own time; idle inputs; l1r_k = |r_k|
    static constexpr int guess_grid = 1000;
    SCP_DEV static void guess(const Params& P, const double* pp, int N, int k, double (&x)[nx], double (&u)[nu], double*, double* pn)
    {
        const double tau = lin(0.0, 1.0, N, k);
        double xa[nx] = {pp[0], pp[1]};
        int i = 0;
        while (i < guess_grid - 2 && tau > lin(0.0, 1.0, guess_grid, i + 1)) {
            free_step(P, xa, lin(0.0, 1.0, guess_grid, i + 1) - lin(0.0, 1.0, guess_grid, i));
            i++;
        }
        const double ta = lin(0.0, 1.0, guess_grid, i), tb = lin(0.0, 1.0, guess_grid, i + 1);
        double xb[nx] = {xa[0], xa[1]};
        free_step(P, xb, tb - ta);
        const double c = (tb - tau) / (tb - ta);
        for (int j = 0; j < nx; j++) x[j] = c * xa[j] + (1.0 - c) * xb[j];
        for (int j = 0; j < nu; j++) u[j] = 0.0;
        pn[0] = fabs(x[0]);
    }

    // ---- subproblem side ----
    static constexpr int ns = 2, nl = 10, nsoc = 0, ng = 0, nic = 2, ntc = 0, npp = 2;

    // smooth logical OR of the two predicates (helper.jl:775-807: or -> indicator :724-749 -> sigmoid :672-701 -> logsumexp
    // :623-651) with kappa = kappa1, match = normalize = a_max - a_db, and its derivative with respect to ar.  The order of
    // the operations is the reference's: it is what keeps every value finite at kappa1 = 4.6e8, where sigma is exactly 0 or 1
    // and c = exp(kappa L + 2 log(1 - sigma)) is exactly 0 through exp(-Inf).
    SCP_DEV static void smooth_or(const Params& P, double ar, double& OR, double& dOR)
    {
        const double nrm = P.a_max - P.a_db, kap = P.kappa1;
        const double f[2] = {(ar - P.a_db) / nrm, (-P.a_db - ar) / nrm}, g[2] = {1.0 / nrm, -1.0 / nrm};
        // logsumexp(f, grad; t = kappa)
        const double a = fmax(kap * f[0], kap * f[1]);
        const double e0 = exp(kap * f[0] - a), e1 = exp(kap * f[1] - a), E = e0 + e1;
        const double L = (a + log(E)) / kap;
        const double dL = g[0] * (e0 / E) + g[1] * (e1 / E);
        // sigmoid
        const double sig = 1.0 - 1.0 / (1.0 + exp(kap * L));
        const double c = exp(kap * L + 2.0 * log(1.0 - sig));
        // indicator: shifted so that the value is exactly one where a predicate equals `match` (scaled: 1)
        const double am = kap * 1.0;
        const double Lm = (am + log(exp(kap * 1.0 - am))) / kap;
        const double off = 1.0 - 1.0 / (1.0 + exp(kap * Lm));
        OR = sig + (1.0 - off);
        dOR = kap * c * dL;
    }
    // s = [aa - OR ar; OR ar - aa] (definition.jl:370-444); C = 0, G = 0 (ns x (np + np_node))
    SCP_DEV static void s_eval(const Params& P, double, int, const double*, const double* u, const double*, double* s,
                               double* C, double* Dm, double* G)
    {
        const double aa = u[0], ar = u[1];
        double OR, dOR;
        smooth_or(P, ar, OR, dOR);
        const double dORar = dOR * ar + OR;
        s[0] = aa - OR * ar;
        s[1] = OR * ar - aa;
        for (int i = 0; i < ns * nx; i++) C[i] = 0.0;
        for (int i = 0; i < ns * nu; i++) Dm[i] = 0.0;
        for (int i = 0; i < ns * (np + np_node); i++) G[i] = 0.0;
        Dm[0 * nu + 0] = 1.0; Dm[0 * nu + 1] = -dORar;
        Dm[1 * nu + 0] = -1.0; Dm[1 * nu + 1] = dORar;
    }
    // U: |aa| <= a_max, |ar| <= a_max, |aa| <= l1aa, |aa - ar| <= l1adiff; X: |r| <= l1r_k (definition.jl:238-368).  The
    // reference states the last three as L1 cones of a SCALAR argument; they are lowered directly to the two rows +-y - t <= 0
    // (same feasible set in (y, t) as MOI's NormOne bridge, which adds one auxiliary variable: DESIGN.md section 7).
    // Lp is COMPACT (nl x (np + np_node)): column 0 = this node's l1r_k.
    SCP_DEV static void lin_rows(const Params& P, double, int, double* L, double* Lp, double* l)
    {
        constexpr int nz = nx + nu, npc = np + np_node;
        for (int i = 0; i < nl * nz; i++) L[i] = 0.0;
        for (int i = 0; i < nl * npc; i++) Lp[i] = 0.0;
        for (int i = 0; i < nl; i++) l[i] = 0.0;
        constexpr int iaa = nx + 0, iar = nx + 1, il1aa = nx + 2, il1ad = nx + 3;
        L[0 * nz + iaa] = 1.0; l[0] = -P.a_max;
        L[1 * nz + iaa] = -1.0; l[1] = -P.a_max;
        L[2 * nz + iar] = 1.0; l[2] = -P.a_max;
        L[3 * nz + iar] = -1.0; l[3] = -P.a_max;
        L[4 * nz + iaa] = 1.0; L[4 * nz + il1aa] = -1.0;
        L[5 * nz + iaa] = -1.0; L[5 * nz + il1aa] = -1.0;
        L[6 * nz + iaa] = 1.0; L[6 * nz + iar] = -1.0; L[6 * nz + il1ad] = -1.0;
        L[7 * nz + iaa] = -1.0; L[7 * nz + iar] = 1.0; L[7 * nz + il1ad] = -1.0;
        L[8 * nz + 0] = 1.0; Lp[8 * npc + np] = -1.0;
        L[9 * nz + 0] = -1.0; Lp[9 * npc + np] = -1.0;
    }
    SCP_DEV static void soc_rows(const Params&, double, int, double*, double*) {}
    SCP_DEV static void glin_rows(const Params&, double*, double*) {}
    SCP_DEV static void bc_ic(const Params&, const double* x, const double*, const double* pp, double* g, double* H, double*)
    {
        g[0] = x[0] - pp[0]; g[1] = x[1] - pp[1];
        H[0] = 1; H[1] = 0; H[2] = 0; H[3] = 1;
    }
    SCP_DEV static void bc_tc(const Params&, const double*, const double*, const double*, double*, double*, double*) {}
    // Gamma = l1r_k / r_nrml + alpha l1aa / a_max + gamma l1adiff / a_max (definition.jl:116-142), no terminal cost.  The node
    // entry of tp is a coefficient of GAMMA (node_par_in_running_cost): node k's term carries the trapezoid weight w_k
    SCP_DEV static void cost_terms(const Params& P, double* Qu, double* lu, double* lx, double* tx, double* tp, double* Qp)
    {
        for (int i = 0; i < nu; i++) { Qu[i] = 0.0; lu[i] = 0.0; }
        lu[2] = P.alpha / P.a_max; lu[3] = P.gamma / P.a_max;
        for (int i = 0; i < nx; i++) { lx[i] = 0.0; tx[i] = 0.0; }
        tp[np] = 1.0 / P.r_nrml; Qp[np] = 0.0;
    }
};

}  // namespace scp
