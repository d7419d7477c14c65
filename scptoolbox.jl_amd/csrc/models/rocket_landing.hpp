// Mars rocket landing as a free-final-time TrajectoryProblem (builder-defined,
// SURVEY.md F6) over the physical model of
// test/examples/rocket_landing/parameters.jl:77-146:
//   x=[r;v;z=ln m], u=[a;xi], p=[tf];  xdot = tf*(A_c x + B_c u + p_c)
//   A_c = [0 I 0; -(w^x)^2 -2 w^x 0; 0 0 0], B_c = [0; I 0; 0 -alpha], p_c=[0;g;0]
#pragma once
#include "model_common.hpp"

namespace scp {

struct RocketLanding : ModelDefaults {
    static constexpr int id = 2;
    static constexpr int nx = 7, nu = 4, np = 1, npF = 1;
    // Jacobians A, B, F do not depend on (t, x, u) inside an interval -> variational discretize! kernel (K1v)
    static constexpr bool const_jacobian = true;
    static constexpr bool has_subproblem = true;
    static constexpr bool structured = true;   // stage-structured PTR fast path available (stage_problem.hpp, ipm2_*.hpp)
    // largest normalised RK4 step 1/((N-1)(Nsub-1)) for which K1v matches the reference formulation to < 1e-10
    // (Coriolis terms: the two RK4 forms differ by O((tf h)^4) ~ 1e-13 at h = 1e-2, tf = 150 s (measured)); coarser grids use the reference-form kernel K1
    static constexpr double var_form_max_step = 1e-2;
    // the whole model is DATA (src/parser/problem.jl:64-121): the physical constants of
    // test/examples/rocket_landing/parameters.jl:86-106 and the builder-defined problem constants cross the ABI in the blob:
    //   [g(3), omega(3), alpha, m_dry, m_wet, rho_min, rho_max, glide-slope angle (rad), pointing angle (rad), v_max,
    //    tf_min, tf_max, cost_weight]
    static constexpr int npar = 17;
    struct Params {
        double g[3];
        double S2[9];  // -(w^x)^2, col-major
        double S[9];   // -2 w^x,   col-major
        double alpha;
        double m_dry, m_wet, rho_min, rho_max;
        double cos_gs, sin_gs, cos_p, v_max;
        double tf_min, tf_max, cost_weight;
    };
    static Params make_params(const double* par)
    {
        Params P;
        const double* w = par + 3;
        const double K[9] = {0, w[2], -w[1], -w[2], 0, w[0], w[1], -w[0], 0};  // skew(w) col-major
        for (int i = 0; i < 3; i++) P.g[i] = par[i];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double a = 0;
                for (int l = 0; l < 3; l++) a += K[i + 3 * l] * K[l + 3 * j];
                P.S2[i + 3 * j] = -a;
                P.S[i + 3 * j] = -2.0 * K[i + 3 * j];
            }
        P.alpha = par[6];
        P.m_dry = par[7]; P.m_wet = par[8]; P.rho_min = par[9]; P.rho_max = par[10];
        P.cos_gs = cos(par[11]); P.sin_gs = sin(par[11]); P.cos_p = cos(par[12]); P.v_max = par[13];
        P.tf_min = par[14]; P.tf_max = par[15]; P.cost_weight = par[16];
        return P;
    }
    static constexpr int Fcol(int) { return 0; }

    SCP_DEV static void dyn(const Params& P, double, int, const double (&x)[nx], const double (&u)[nu],
                            const double* p, double (&f)[nx], double (&A)[nx * nx], double (&B)[nx * nu],
                            double (&Fc)[nx])
    {
        const double tf = p[0];
        zero(A);
#pragma unroll
        for (int i = 0; i < 3; i++) A[i + nx * (3 + i)] = 1.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                A[(3 + i) + nx * j] = P.S2[i + 3 * j];
                A[(3 + i) + nx * (3 + j)] = P.S[i + 3 * j];
            }
        double f0[nx];
#pragma unroll
        for (int i = 0; i < nx; i++) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < nx; j++) a += A[i + nx * j] * x[j];
            f0[i] = a;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) f0[3 + i] += u[i] + P.g[i];
        f0[6] += -P.alpha * u[3];
#pragma unroll
        for (int i = 0; i < nx; i++) f[i] = f0[i] * tf;
#pragma unroll
        for (int i = 0; i < nx * nx; i++) A[i] *= tf;
        zero(B);
        B[3 + nx * 0] = tf; B[4 + nx * 1] = tf; B[5 + nx * 2] = tf;
        B[6 + nx * 3] = -P.alpha * tf;
#pragma unroll
        for (int i = 0; i < nx; i++) Fc[i] = f[i] / tf;
    }
    // structured products for the variational discretize! kernel: out = A v ; column j of B
    SCP_DEV static void Amul(const Params& P, const double* p, const double (&v)[nx], double (&out)[nx])
    {
        const double tf = p[0];
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] = tf * v[3 + i];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 3; j++) acc += P.S2[i + 3 * j] * v[j] + P.S[i + 3 * j] * v[3 + j];
            out[3 + i] = tf * acc;
        }
        out[6] = 0.0;
    }
    SCP_DEV static void Bcol(const Params& P, const double* p, int j, double (&out)[nx])
    {
#pragma unroll
        for (int i = 0; i < nx; i++) out[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) if (j == i) out[3 + i] = p[0];
        if (j == 3) out[6] = -P.alpha * p[0];
    }
    SCP_DEV static void action(double (&)[nx]) {}
    static constexpr bool has_fp32 = false;    // fp32 variant of K1 (scp_set_discretize_precision): Starship only
    static constexpr bool has_impulse = false;   // no impulsive-input form of this model (IMPULSE -> SCP_ERR_UNSUPPORTED)
    // initial guess at node k of N: straight line from (r0, v0, ln m_wet) to (0, 0, ln m_dry), hover input, tf = 75 s
    SCP_DEV static void guess(const Params& P, const double* pp, int N, int k, double (&x)[nx], double (&u)[nu], double* p, double*)
    {
        const double t = (double)k / (double)(N - 1), tg = (1.0 - t) * 0.0 + t * 1.0, c = (1.0 - tg) / (1.0 - 0.0);
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = c * pp[i] + (1.0 - c) * 0.0;
        x[6] = c * log(P.m_wet) + (1.0 - c) * log(P.m_dry);
        const double g = -P.g[2];
        const double hov[4] = {0.0, 0.0, g, g};
#pragma unroll
        for (int i = 0; i < nu; i++) u[i] = c * hov[i] + (1.0 - c) * hov[i];
        p[0] = 75.0;
    }

    // ---- subproblem side (builder-defined) over definition.jl:84-130 ----
    static constexpr int ns = 2, nl = 6, nsoc = 2, ng = 2, nic = 7, ntc = 6, npp = 6;  // pp = [r0 v0]
    // pattern of Kl (ModelDefaults): the columns s_eval / lin_rows / soc_rows below can write, at most two per row; Kp = 0
    static constexpr int kl_width = 2;
    static constexpr bool has_kp = false;
    static constexpr int kl_col(int row, int slot)
    {
        constexpr int z = 6, a0 = nx, a1 = nx + 1, a2 = nx + 2, xi = nx + 3;
        constexpr int T[ns + nl + 4 * nsoc][kl_width] = {
            {z, xi}, {z, xi},                                   // thrust bounds: (ln m, xi)
            {0, 2}, {0, 2}, {1, 2}, {1, 2}, {z, -1}, {a2, xi},  // glide slope (r), ln m >= ln m_dry, pointing (a_z, xi)
            {-1, -1}, {3, -1}, {4, -1}, {5, -1},                // ||v|| <= v_max
            {xi, -1}, {a0, -1}, {a1, -1}, {a2, -1}};            // ||a|| <= xi
        return T[row][slot];
    }
    // exact thrust bounds in log-mass form: rho_min e^-z - xi <= 0, xi - rho_max e^-z <= 0
    SCP_DEV static void s_eval(const Params& P, double, int, const double* x, const double* u, const double*,
                               double* s, double* C, double* Dm, double* G)
    {
        const double ez = exp(-x[6]);
        s[0] = P.rho_min * ez - u[3];
        s[1] = u[3] - P.rho_max * ez;
        for (int i = 0; i < ns * nx; i++) C[i] = 0.0;
        for (int i = 0; i < ns * nu; i++) Dm[i] = 0.0;
        C[0 * nx + 6] = -P.rho_min * ez; C[1 * nx + 6] = P.rho_max * ez;
        Dm[0 * nu + 3] = -1.0; Dm[1 * nu + 3] = 1.0;
        G[0] = 0.0; G[1] = 0.0;
    }
    // X: glide slope (4 rows, definition.jl:105-114), z >= ln m_dry (:130);  U: xi cos(gamma_p) <= a_z (:103)
    // At the terminal node (t = 1) the terminal condition pins r_N = 0, the APEX of the glide-slope cone: all four rows
    // would be active with non-unique multipliers and no strictly feasible point; they are redundant there and are
    // replaced by the trivially satisfied 0*x - 1 <= 0 (same row count; same rule in oracle/models.py).
    SCP_DEV static void lin_rows(const Params& P, double t, int, double* L, double* Lp, double* l)
    {
        constexpr int nz = nx + nu;
        for (int i = 0; i < nl * nz; i++) L[i] = 0.0;
        for (int i = 0; i < nl; i++) { Lp[i] = 0.0; l[i] = 0.0; }
        if (t >= 1.0) {
            for (int i = 0; i < 4; i++) l[i] = -1.0;
        } else {
            L[0 * nz + 0] = P.cos_gs; L[0 * nz + 2] = -P.sin_gs;
            L[1 * nz + 0] = -P.cos_gs; L[1 * nz + 2] = -P.sin_gs;
            L[2 * nz + 1] = P.cos_gs; L[2 * nz + 2] = -P.sin_gs;
            L[3 * nz + 1] = -P.cos_gs; L[3 * nz + 2] = -P.sin_gs;
        }
        L[4 * nz + 6] = -1.0; l[4] = log(P.m_dry);
        L[5 * nz + nx + 3] = P.cos_p; L[5 * nz + nx + 2] = -1.0;
    }
    // X: ||v|| <= v_max (:116);  U: ||a|| <= xi (:100)
    SCP_DEV static void soc_rows(const Params& P, double, int, double* Mm, double* m)
    {
        constexpr int nz = nx + nu;
        for (int i = 0; i < 8 * nz; i++) Mm[i] = 0.0;
        for (int i = 0; i < 8; i++) m[i] = 0.0;
        m[0] = P.v_max; Mm[1 * nz + 3] = 1.0; Mm[2 * nz + 4] = 1.0; Mm[3 * nz + 5] = 1.0;
        Mm[4 * nz + nx + 3] = 1.0; Mm[5 * nz + nx + 0] = 1.0; Mm[6 * nz + nx + 1] = 1.0; Mm[7 * nz + nx + 2] = 1.0;
    }
    SCP_DEV static void glin_rows(const Params& P, double* Lp, double* lp)
    {
        Lp[0] = 1.0; lp[0] = -P.tf_max;
        Lp[1] = -1.0; lp[1] = P.tf_min;
    }
    SCP_DEV static void bc_ic(const Params& P, const double* x, const double*, const double* pp, double* g, double* H,
                              double* K)
    {
        for (int i = 0; i < 7; i++) { K[i] = 0.0; for (int j = 0; j < 7; j++) H[i * 7 + j] = (i == j); }
        for (int i = 0; i < 6; i++) g[i] = x[i] - pp[i];
        g[6] = x[6] - log(P.m_wet);
    }
    SCP_DEV static void bc_tc(const Params&, const double* x, const double*, const double*, double* g, double* H,
                              double* K)
    {
        for (int i = 0; i < 6; i++) { g[i] = x[i]; K[i] = 0.0; for (int j = 0; j < 7; j++) H[i * 7 + j] = (i == j); }
    }
    // maximise final mass: phi = -cost_weight * z_N
    SCP_DEV static void cost_terms(const Params& P, double* Qu, double* lu, double* lx, double* tx, double* tp, double* Qp)
    {
        for (int i = 0; i < nu; i++) { Qu[i] = 0.0; lu[i] = 0.0; }
        for (int i = 0; i < nx; i++) { lx[i] = 0.0; tx[i] = 0.0; }
        tx[6] = -P.cost_weight;
        tp[0] = 0.0; Qp[0] = 0.0;
    }
};

}  // namespace scp
