// Generic batched conic interior-point solver: the NUMERIC phase.
//
// Replaces the reference's `solve!(prg)` -> JuMP.optimize! -> ECOS for ARBITRARY conic programs of a batch that
// share one sparsity pattern (src/parser/program.jl:63-76,419-424; SURVEY.md section 8b `socp_solve_batch`):
//
//     min 1/2 x'Px + c'x   s.t.  A x = b,   G x + s = h,   s in R+^l x Q^{q_1} x ... x Q^{q_nc}
//
// Algorithm (same class as ECOS; restated for the tests in oracle/ipm.py): Mehrotra predictor-corrector with
// Nesterov-Todd scaling, Newton systems solved through an LDL' factorisation of the SCALED quasi-definite KKT matrix
// [P+dI A' Gt'; A -dI 0; Gt 0 -(1+d)I], Gt = W^-1 G, with static +-d regularisation, ECOS-style dynamic
// regularisation of wrong-signed pivots and iterative refinement against the unregularised matrix.
//
// MI355X mapping.  All problems of the batch replay the SAME static schedule (conic_symbolic.hpp):
//   * LANE = PROBLEM: every per-problem array is INTERLEAVED across the batch (element e of problem t at
//     base[e * stride + t]), so each load/store of a wavefront is one fully coalesced 512-byte line; there is no
//     cross-lane traffic and no divergence except the per-problem iteration count;
//   * WAVE = WORKER: a workgroup of NW wavefronts owns 64 problems; the independent items of every phase -- the
//     columns / entries of one elimination LEVEL of the factorisation, the rows of one level of the triangular solves,
//     rows of the mat-vecs, cones -- are dealt round-robin to the waves, with a workgroup barrier between dependent
//     phases.  A wave's inner loops are latency chains (load, load, FMA); the other waves of the CU hide them;
//   * the schedule (pair lists, row lists, pattern indices) is wave-uniform: scalar loads, shared by all workgroups
//     through L2; inner loops fetch 4 index pairs and 8 operands before the first FMA;
//   * per-problem scalars (step lengths, residual norms) are reduced across the waves through LDS, in a fixed order, so
//     every wave holds bit-identical copies and results do not depend on the launch geometry.
// The kernel is memory-latency / L2-bandwidth bound (16 B per multiply-add); the specialised stage-structured solver
// (ipm2_*.hpp) stays the fast path for the PTR subproblem -- this one is the general seam (SCvx, GuSTO, q_tr != Inf,
// compute_scaling, correct_convex!, user programs).
//
// The solver body is plain `__host__ __device__` C++ templated on an execution context: the tests instantiate it with a
// single-worker host context (oracle/conic_host.cpp, test infrastructure) and compare with oracle/ipm.py; the product
// only launches the kernel (conic_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define CONIC_HD __host__ __device__ __forceinline__
#ifdef CONIC_DEBUG
#include <stdio.h>
#define CONIC_DBG(...) printf(__VA_ARGS__)
#else
#define CONIC_DBG(...) ((void)0)
#endif

// -DCONIC_PROF (device diagnostic build): wall-clock ticks (100 MHz) per phase kind, printed by worker 0 of problem 0 at the end of run()
#if defined(CONIC_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define CPROF_T() ((long long)wall_clock64())
#define CPROF_ADD(i, t0) (prof_[i] += CPROF_T() - (t0))
#else
#define CPROF_T() (0LL)
#define CPROF_ADD(i, t0) ((void)(t0))
#endif

namespace scp {
namespace conic {

struct int2_ { int a, b; };

// static schedule (device pointers on the GPU, host pointers in the host harness)
struct Sched {
    int n, p, m, l, nk, ncone;
    int nnzG, nnzGt, nnzA, nnzP, nnzL, njob, nlp, nlev, nrlev;
    const int *q, *cone_off;
    // cone kinds (round 4): ctype[c] = 0 second-order cone, 1 EXPONENTIAL cone {(x, y, w): y exp(x / y) <= w, y > 0} (dimension 3,
    // src/parser/cone.jl:45); cexp[c] = index of cone c among the nexp exponential ones (-1 otherwise).  NULL / 0: all second-order.
    const int *ctype, *cexp;
    int nexp;
    const int *Gp, *Gi;                       // G (CSC)
    const int *Gr_p, *Gr_j, *Gr_pos;          // G by rows
    const int *Gtp, *Gti;                     // Gt (CSC)
    const int *Gtr_p, *Gtr_j, *Gtr_pos;       // Gt by rows
    const int *Ap, *Ai, *Ar_p, *Ar_j, *Ar_pos;
    const int *Pf_p, *Pf_j, *Pf_pos;          // symmetric expansion of P by rows
    const int *kk_p, *kk_src, *kk_idx, *kk_col;   // rows of the unregularised KKT matrix as one list per row (Symbolic::kk_p)
    const int* kk_long; int nkk_long, kk_long_thr;   // rows longer than kk_long_thr terms
    const int *job_gt0, *job_cone, *job_src_p, *job_src_row, *job_src_g;
    const int *lp_gt, *lp_g;
    const int *perm;
    const int *Lp, *Li, *l_src, *l_src_idx, *d_src, *d_src_idx, *d_kind;
    const long long* pair_p;
    const int2_* pairs;
    const int *row_p, *row_k, *row_pos;
    const int *lev_p, *lev_cols, *lev_ent_p, *lev_ent, *ent_col, *rlev_p, *rlev_cols;
    // long rows / pair lists cut into chunks (conic_symbolic.hpp, Symbolic): short items first inside a level
    const int *lev_nshort, *rchunk_p, *rchunk_r0, *rchunk_r1, *col_c0, *col_c1;
    const int *lev_ent_nshort, *echunk_p, *ent_c0, *ent_c1;
    const long long *echunk_q0, *echunk_q1;
    int max_chunks;
};

struct Opts {
    int max_iter;
    double feastol, abstol, reltol;
    double reg;         // static regularisation d (the entry points replace a negative value by auto_reg(n_free))
    double dyn_eps, dyn_delta;   // dynamic regularisation: pivot with sign*D <= dyn_eps becomes sign*dyn_delta
    int nref;           // max iterative-refinement steps per solve
    double ref_tol;     // stop refining when |res|_2 <= ref_tol (1 + |rhs|_2)
    double step;        // fraction of the step to the boundary (0.99)
    // set by the entry points together with an AUTOMATIC regularisation of 1e-10 (conic_symbolic.hpp auto_reg), never by a
    // caller: the small regularisation comes with a finer ladder when a factorisation breaks (x 10 per attempt instead of x 100) and
    // with the accuracy check of the refined solves (run(): `sloppy`).  0: the behaviour of rounds 3 - 4, bit for bit.
    int fine;
};
CONIC_HD Opts default_opts()
{
    Opts o;
    o.max_iter = 100; o.feastol = 1e-8; o.abstol = 1e-8; o.reltol = 1e-8;
    o.reg = -1.0 /* automatic: conic_symbolic.hpp auto_reg */; o.dyn_eps = 1e-13; o.dyn_delta = 2e-7; o.nref = 10; o.ref_tol = 1e-11; o.step = 0.99; o.fine = 0;
    return o;
}

enum { ST_OPTIMAL = 0, ST_ALMOST = 1, ST_ITERLIM = 2, ST_NUMERR = 3, ST_PINF = 4, ST_DINF = 5 };

// interleaved per-problem vector: element e at p[e * es] (p already offset by the problem's lane)
struct BV {
    double* p;
    long es;
    CONIC_HD double& operator[](long e) const { return p[e * es]; }
};
struct CBV {
    const double* p;
    long es;
    CONIC_HD double operator[](long e) const { return p[e * es]; }
};

// all per-problem arrays of one problem
struct Prob {
    CBV c, b, h, Gx, Ax, Px;               // data
    BV x, y, z, s;                         // solution (in/out)
    BV Gt, Lx, Ux, Dinv;                   // factor
    BV rhs, sol, res, cor, tmp;            // KKT-sized vectors [nk]
    BV part;                               // [max_chunks] partial sums of the long items of one level
    BV lam, wsc, ds, dz, corr, rz;         // cone-sized vectors [m]  (wsc: w (R+ rows) / w-bar (SOC rows))
    BV eta;                                // [ncone + 9 nexp]: eta of the second-order cones, then per exponential cone L^-1 (6) | grad F* (3)
    BV rx, ry;                             // [n], [p]
};

struct Result {
    int status, iters, nreg, nrefine;
    double pcost, dcost, gap, pres, dres, relgap;
    double pinf, dinf;   // residuals of the normalised infeasibility certificates at the last iterate (1e300: none)
};

// ---------------- exponential cone (GuSTO's softplus penalty, src/solvers/gusto.jl:996-1031) ----------------
// Method of ECOS's exponential-cone extension (S. Akle Serrano, 2015), restated in oracle/ipm.py::solve_exp: the pair (s, z) of an
// exponential cone, s in K, z in the dual cone K* = {(u, v, w): u < 0, psi = v - u + u log(-u / w) >= 0}, enters the Newton
// system through mu H with H the Hessian of the dual barrier F*(u, v, w) = -log psi - log(-u) - log w at z, and its centrality
// condition is s + mu grad F*(z) = 0 (first order, no Mehrotra correction); the step is found by backtracking.
CONIC_HD bool exp_primal_interior(double x, double y, double w) { return y > 0.0 && w > 0.0 && y * log(w / y) - x > 0.0; }
CONIC_HD bool exp_dual_interior(double u, double v, double w) { return u < 0.0 && w > 0.0 && v - u + u * log(-u / w) > 0.0; }
// g[3] = grad F*, H = lower triangle of the Hessian in the order 00, 10, 11, 20, 21, 22
CONIC_HD void exp_dual_grad_hess(double u, double v, double w, double* g, double* H)
{
    const double L = log(-u / w), psi = v - u + u * L, ip = 1.0 / psi, ip2 = ip * ip;
    const double d0 = L, d1 = 1.0, d2 = -u / w;          // grad psi
    g[0] = -L * ip - 1.0 / u; g[1] = -ip; g[2] = (u / w) * ip - 1.0 / w;
    H[0] = d0 * d0 * ip2 - (1.0 / u) * ip + 1.0 / (u * u);
    H[1] = d1 * d0 * ip2;
    H[2] = d1 * d1 * ip2;
    H[3] = d2 * d0 * ip2 + (1.0 / w) * ip;
    H[4] = d2 * d1 * ip2;
    H[5] = d2 * d2 * ip2 - (u / (w * w)) * ip + 1.0 / (w * w);
}
// Cholesky M = L L' of the SPD 3 x 3 matrix given by its lower triangle, then Li = L^-1 (same packing).  false: not positive
CONIC_HD bool chol3_inverse(const double* M, double* Li)
{
    const double l00s = M[0];
    if (!(l00s > 0.0)) return false;
    const double l00 = sqrt(l00s), l10 = M[1] / l00, l20 = M[3] / l00;
    const double l11s = M[2] - l10 * l10;
    if (!(l11s > 0.0)) return false;
    const double l11 = sqrt(l11s), l21 = (M[4] - l20 * l10) / l11;
    const double l22s = M[5] - l20 * l20 - l21 * l21;
    if (!(l22s > 0.0)) return false;
    const double l22 = sqrt(l22s);
    Li[0] = 1.0 / l00; Li[2] = 1.0 / l11; Li[5] = 1.0 / l22;
    Li[1] = -l10 * Li[0] * Li[2];
    Li[4] = -l21 * Li[2] * Li[5];
    Li[3] = -(l20 * Li[0] + l21 * Li[1]) * Li[5];
    return true;
}
#ifndef CONIC_EXP_MARGIN
#define CONIC_EXP_MARGIN 1.25  /* an accepted step must keep the exponential pairs inside their cones this much further along */
#endif
#define CONIC_EXP_C0 (-1.051383945322714)   /* the point with s = z = -grad F*(z) (mu = 1), in the order (x, y, w) */
#define CONIC_EXP_C1 (0.556409619469370)
#define CONIC_EXP_C2 (1.258967884768947)

// Execution context of the single-worker (host) instantiation; the device context lives in conic_api.hip.
// wid / nw: this worker and the number of workers sharing the problem; barrier(): all workers reach it;
// sum / min: combine one value per worker, every worker gets the (bit-identical) result; any(): true if the predicate
// holds for any problem of the group (decides how long the group keeps iterating).
struct SerialCtx {
    static constexpr bool COOP = false;                      // cooperative item groups (see Solver::pfor_coop): device, SUB = 64 only
    static constexpr bool COOP_EMU = false;
    CONIC_HD int coop_workers() const { return 1; }
    CONIC_HD double gsum(double v, int) const { return v; }
    CONIC_HD int wid() const { return 0; }
    CONIC_HD int nw() const { return 1; }
    CONIC_HD void barrier() const {}
    CONIC_HD double sum(double v) const { return v; }
    CONIC_HD double min(double v) const { return v; }
    CONIC_HD bool any(bool v) const { return v; }
};

template <class Ctx>
struct Solver {
    const Sched& S;
    const Prob& Q;
    const Opts& O;
    Ctx& cx;
    int nreg = 0, nrefine = 0;
    double lin_worst = 0.0;     // largest relative residual |rhs - K sol| / (1 + |rhs|) a refined solve of the current direction was left with
    mutable long long prof_[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // CONIC_PROF: 0 factor, 1 forward, 2 backward, 3 residual, 4 scaling + Gt, 5 total, 6 solves, 7 residual calls
    double reg = 0.0;    // static regularisation of THIS problem (starts at O.reg, escalated by run() when a factorisation fails)
    // Objective scale of THIS problem: the solver works on osc * (1/2 x'Px + c'x).  1 unless the largest cost coefficient
    // exceeds OBJ_MAX; then it is brought down to OBJ_MAX (run()).  GuSTO multiplies its penalty weight by 5 after every
    // rejected step: at lambda = 6e6 the P values are 1e5 ... 1e7 next to unit constraint rows, the factorisation needs
    // 100+ dynamic regularisations and the run ends NUMERICAL_ERROR with a dual residual of 1e-2 -- where the same program with
    // its objective divided by lambda / 1e4 is OPTIMAL in 18-21 iterations (the oracle's dense pivoting solver does not
    // care).  The absolute-gap tests (abstol and the reduced tolerance 5e-5) are evaluated in the units of the ORIGINAL objective,
    // the relative gap does not depend on the scale, the dual residual is relative to the normalised cost vector (run()); y, z, the
    // costs and the gap are returned unscaled.
    static constexpr double OBJ_MAX = 1e4;
    double osc = 1.0;
    CONIC_HD Solver(const Sched& s, const Prob& q, const Opts& o, Ctx& c) : S(s), Q(q), O(o), cx(c), reg(o.reg) {}

    // parallel loop over [lo, hi): items dealt round-robin to the workers; barrier at the end
    template <class F>
    CONIC_HD void pfor(int lo, int hi, F&& f) const
    {
        for (int i = lo + cx.wid(); i < hi; i += cx.nw()) f(i);
        cx.barrier();
    }
    // same without the trailing barrier (caller combines several loops that touch disjoint data)
    template <class F>
    CONIC_HD void pfor_nb(int lo, int hi, F&& f) const
    {
        for (int i = lo + cx.wid(); i < hi; i += cx.nw()) f(i);
    }

    // ---- cooperative items (round 5; Ctx::COOP: one workgroup per problem, 1 024 workers) ----
    // A worker owning a whole row / pair list walks it four terms per memory round trip, and most levels of a time-staged program
    // hold FEWER items than the workgroup has workers (Starship N = 100: ~100 columns with rows of 20 ... 150 terms on the mid
    // levels, single columns with 8 800-term rows cut into ~190-term chunks on the last eleven): the phase then lasts as long as
    // its longest item while 900 workers idle -- 19 k dependent terms per factorisation, ~20 of the 34 ms of an IPM iteration.
    // With fewer items than workers an item is therefore summed by a GROUP of G = 2 ... 64 consecutive workers (lanes of one wave):
    // lane gl takes the terms gl, gl + G, ... (4 in flight per lane), the partial sums are added by a butterfly of shuffles
    // (fixed order), lane 0 of the group stores the result.  G = 1 is the per-worker code above, bit for bit (host build, the
    // chip-filling geometries).  The summation ORDER of an item depends on G, i.e. on the launch geometry -- round-off only.
    CONIC_HD int coop_width(int nitems) const
    {
        if (!Ctx::COOP || nitems <= 0) return 1;
        int G = 1;
        const int nwk = cx.coop_workers();
        while (G < 64 && (long)nitems * (2 * G) <= nwk) G *= 2;
        return G;
    }
    template <class Fp, class Fd>
    CONIC_HD void pfor_coop(int lo, int hi, int G, Fp&& part, Fd&& done) const
    {
        if constexpr (Ctx::COOP_EMU) {      // host emulation of the device's summation order: the G lanes of a group one after another
            for (int i = lo; i < hi; i++) {
                double pl[64];
                for (int gl = 0; gl < G; gl++) pl[gl] = part(i, gl, G);
                for (int msk = G >> 1; msk > 0; msk >>= 1) {     // the shuffle butterfly of DevCtx::gsum, as lane 0 sees it
                    double nx[64];
                    for (int gl = 0; gl < G; gl++) nx[gl] = pl[gl] + pl[gl ^ msk];
                    for (int gl = 0; gl < G; gl++) pl[gl] = nx[gl];
                }
                done(i, pl[0]);
            }
            return;
        }
        const int gid = cx.wid() / G, ng = cx.nw() / G, gl = cx.wid() % G;
        for (int i = lo + gid; i < hi; i += ng) {
            const double sgm = cx.gsum(part(i, gl, G), G);
            if (gl == 0) done(i, sgm);
        }
    }
    // strided partial sums of the four item kinds (lane gl of a group of G): 4 terms in flight per lane
    CONIC_HD double row_sq_part(int r, int r1, int gl, int G) const       // sum Ux[pos] Lx[pos]
    {
        double a = 0.0;
        int t = r + gl;
        for (; t + 3 * G < r1; t += 4 * G) {
            const int p0 = S.row_pos[t], p1 = S.row_pos[t + G], p2 = S.row_pos[t + 2 * G], p3 = S.row_pos[t + 3 * G];
            const double u0 = Q.Ux[p0], l0 = Q.Lx[p0], u1 = Q.Ux[p1], l1 = Q.Lx[p1], u2 = Q.Ux[p2], l2 = Q.Lx[p2], u3 = Q.Ux[p3], l3 = Q.Lx[p3];
            a += u0 * l0; a += u1 * l1; a += u2 * l2; a += u3 * l3;
        }
        for (; t < r1; t += G) { const int pos = S.row_pos[t]; a += Q.Ux[pos] * Q.Lx[pos]; }
        return a;
    }
    CONIC_HD double pair_part(long long q0, long long q1, int gl, int G) const     // sum Ux[a] Lx[b]
    {
        double a = 0.0;
        long long t = q0 + gl;
        for (; t + 3 * G < q1; t += 4 * G) {
            const int2_ p0 = S.pairs[t], p1 = S.pairs[t + G], p2 = S.pairs[t + 2 * G], p3 = S.pairs[t + 3 * G];
            const double u0 = Q.Ux[p0.a], l0 = Q.Lx[p0.b], u1 = Q.Ux[p1.a], l1 = Q.Lx[p1.b];
            const double u2 = Q.Ux[p2.a], l2 = Q.Lx[p2.b], u3 = Q.Ux[p3.a], l3 = Q.Lx[p3.b];
            a += u0 * l0; a += u1 * l1; a += u2 * l2; a += u3 * l3;
        }
        for (; t < q1; t += G) { const int2_ pr = S.pairs[t]; a += Q.Ux[pr.a] * Q.Lx[pr.b]; }
        return a;
    }
    CONIC_HD double row_tmp_part(int r, int r1, int gl, int G) const      // sum Lx[pos] tmp[k]  (forward substitution)
    {
        double a = 0.0;
        int t = r + gl;
        for (; t + 3 * G < r1; t += 4 * G) {
            const int p0 = S.row_pos[t], p1 = S.row_pos[t + G], p2 = S.row_pos[t + 2 * G], p3 = S.row_pos[t + 3 * G];
            const int k0 = S.row_k[t], k1 = S.row_k[t + G], k2 = S.row_k[t + 2 * G], k3 = S.row_k[t + 3 * G];
            const double l0 = Q.Lx[p0], l1 = Q.Lx[p1], l2 = Q.Lx[p2], l3 = Q.Lx[p3];
            const double t0 = Q.tmp[k0], t1 = Q.tmp[k1], t2 = Q.tmp[k2], t3 = Q.tmp[k3];
            a += l0 * t0; a += l1 * t1; a += l2 * t2; a += l3 * t3;
        }
        for (; t < r1; t += G) a += Q.Lx[S.row_pos[t]] * Q.tmp[S.row_k[t]];
        return a;
    }
    CONIC_HD double col_tmp_part(int e, int e1, int gl, int G) const      // sum Lx[e] tmp[Li[e]]  (backward substitution)
    {
        double a = 0.0;
        int t = e + gl;
        for (; t + 3 * G < e1; t += 4 * G) {
            const int i0 = S.Li[t], i1 = S.Li[t + G], i2 = S.Li[t + 2 * G], i3 = S.Li[t + 3 * G];
            const double l0 = Q.Lx[t], l1 = Q.Lx[t + G], l2 = Q.Lx[t + 2 * G], l3 = Q.Lx[t + 3 * G];
            const double t0 = Q.tmp[i0], t1 = Q.tmp[i1], t2 = Q.tmp[i2], t3 = Q.tmp[i3];
            a += l0 * t0; a += l1 * t1; a += l2 * t2; a += l3 * t3;
        }
        for (; t < e1; t += G) a += Q.Lx[t] * Q.tmp[S.Li[t]];
        return a;
    }
    CONIC_HD double part_part(int c, int c1, int k0, int gl, int G) const  // sum of the chunk partials part[c - k0]
    {
        double a = 0.0;
        for (int t = c + gl; t < c1; t += G) a += Q.part[t - k0];
        return a;
    }

    // ---------------- cone algebra (oracle/ipm.py: Cone) ----------------
    // v <- W v  or  W^-1 v  (in place, m-vector)
    // Exponential cones: W = L' with mu H = L L' is not symmetric -- inverse && !trans: W^-1 v = L^-T v; inverse && trans:
    // W^-T v = L^-1 v (rows / right-hand sides); !inverse: unchanged (only the Mehrotra term of the symmetric cones uses W v)
    CONIC_HD bool is_exp(int c) const { return S.nexp > 0 && S.ctype[c] != 0; }
    CONIC_HD void apply_W(const BV& v, bool inverse, bool trans = false) const
    {
        pfor_nb(0, S.l, [&](int i) { v[i] = inverse ? v[i] / Q.wsc[i] : v[i] * Q.wsc[i]; });
        pfor(0, S.ncone, [&](int c) {
            const int o = S.cone_off[c], d = S.q[c];
            if (is_exp(c)) {
                if (!inverse) return;
                const long e = S.ncone + 9L * S.cexp[c];
                const double a0 = v[o], a1 = v[o + 1], a2 = v[o + 2];
                const double L00 = Q.eta[e], L10 = Q.eta[e + 1], L11 = Q.eta[e + 2], L20 = Q.eta[e + 3], L21 = Q.eta[e + 4], L22 = Q.eta[e + 5];
                if (trans) { v[o] = L00 * a0; v[o + 1] = L10 * a0 + L11 * a1; v[o + 2] = L20 * a0 + L21 * a1 + L22 * a2; }
                else { v[o] = L00 * a0 + L10 * a1 + L20 * a2; v[o + 1] = L11 * a1 + L21 * a2; v[o + 2] = L22 * a2; }
                return;
            }
            const double eta = Q.eta[c], w0 = Q.wsc[o];
            const double v0 = v[o];
            double dot = 0.0;
            for (int r = 1; r < d; r++) dot += Q.wsc[o + r] * v[o + r];
            if (!inverse) {
                const double cf = v0 + dot / (1.0 + w0);
                v[o] = eta * (w0 * v0 + dot);
                for (int r = 1; r < d; r++) v[o + r] = eta * (v[o + r] + cf * Q.wsc[o + r]);
            } else {
                const double cf = -v0 + dot / (1.0 + w0);
                v[o] = (w0 * v0 - dot) / eta;
                for (int r = 1; r < d; r++) v[o + r] = (v[o + r] + cf * Q.wsc[o + r]) / eta;
            }
        });
    }
    // largest alpha >= 0 with s + alpha ds in K (1e300 if unbounded)
    CONIC_HD double max_step(const BV& s, const BV& ds) const
    {
        double a = 1e300;
        pfor_nb(0, S.l, [&](int i) {
            const double d = ds[i];
            if (d < 0.0) a = fmin(a, -s[i] / d);
        });
        pfor_nb(0, S.ncone, [&](int c) {
            if (is_exp(c)) return;       // exponential cones: backtracking (interior_step, exp_neighbourhood)
            const int o = S.cone_off[c], dm = S.q[c];
            const double s0 = s[o], d0 = ds[o];
            double s1s1 = 0.0, d1d1 = 0.0, s1d1 = 0.0;
            for (int r = 1; r < dm; r++) { const double sv = s[o + r], dv = ds[o + r]; s1s1 += sv * sv; d1d1 += dv * dv; s1d1 += sv * dv; }
            const double qa = d0 * d0 - d1d1, qb = 2.0 * (s0 * d0 - s1d1), qc = s0 * s0 - s1s1;
            double r1 = -1.0, r2 = -1.0;
            if (fabs(qa) <= 1e-14 * (d0 * d0 + d1d1 + 1e-300)) {
                if (qb < 0.0) r1 = -qc / qb;
            } else {
                const double disc = qb * qb - 4.0 * qa * qc;
                if (disc >= 0.0) {
                    const double sq = sqrt(disc);
                    const double qq = -0.5 * (qb + (qb >= 0.0 ? sq : -sq));
                    r1 = qq / qa;
                    if (qq != 0.0) r2 = qc / qq;
                }
            }
            if (r1 > 0.0 && s0 + r1 * d0 >= -1e-12 * (fabs(s0) + fabs(r1 * d0))) a = fmin(a, r1);
            if (r2 > 0.0 && s0 + r2 * d0 >= -1e-12 * (fabs(s0) + fabs(r2 * d0))) a = fmin(a, r2);
        });
        return cx.min(a);
    }
    CONIC_HD bool interior_step(const BV& s, const BV& ds, double a, bool dual = false, bool exp_only = false) const
    {
        double ok = 1.0;
        pfor_nb(0, exp_only ? 0 : S.l, [&](int i) { if (!(s[i] + a * ds[i] > 0.0)) ok = 0.0; });
        pfor_nb(0, S.ncone, [&](int c) {
            const int o = S.cone_off[c], d = S.q[c];
            if (exp_only && !is_exp(c)) return;
            if (is_exp(c)) {
                const double v0 = s[o] + a * ds[o], v1 = s[o + 1] + a * ds[o + 1], v2 = s[o + 2] + a * ds[o + 2];
                if (!(dual ? exp_dual_interior(v0, v1, v2) : exp_primal_interior(v0, v1, v2))) ok = 0.0;
                return;
            }
            double t = 0.0;
            for (int r = 1; r < d; r++) { const double v = s[o + r] + a * ds[o + r]; t += v * v; }
            if (!(s[o] + a * ds[o] > sqrt(t))) ok = 0.0;
        });
        return cx.min(ok) > 0.5;
    }
    // cvxopt-style shift into the interior: if v is not in int K add (1 - min) e
    CONIC_HD void shift_interior(const BV& v, bool write = true) const
    {
        if (S.m == 0) return;
        double mn = 1e300;
        pfor_nb(0, S.l, [&](int i) { mn = fmin(mn, v[i]); });
        pfor_nb(0, S.ncone, [&](int c) {
            if (is_exp(c)) return;       // set on the central ray afterwards (run())
            const int o = S.cone_off[c], d = S.q[c];
            double t = 0.0;
            for (int r = 1; r < d; r++) t += v[o + r] * v[o + r];
            mn = fmin(mn, v[o] - sqrt(t));
        });
        mn = cx.min(mn);
        const double sh = (write && mn <= 0.0 && mn < 1e299) ? 1.0 - mn : 0.0;
        pfor_nb(0, S.l, [&](int i) { if (write) v[i] += sh; });
        pfor(0, S.ncone, [&](int c) { if (write && !is_exp(c)) v[S.cone_off[c]] += sh; });
    }
    // Nesterov-Todd scaling from (s, z): fills wsc, eta, lam.  false if not finite.
    CONIC_HD bool nt_scaling(double mu_exp = 1.0) const
    {
        double ok = 1.0;
        pfor_nb(0, S.l, [&](int i) {
            const double s = Q.s[i], z = Q.z[i];
            const double w = sqrt(s / z), lm = sqrt(s * z);
            Q.wsc[i] = w; Q.lam[i] = lm;
            if (!(isfinite(w) && isfinite(lm) && w > 0.0)) ok = 0.0;
        });
        pfor_nb(0, S.ncone, [&](int c) {
            const int o = S.cone_off[c], d = S.q[c];
            if (is_exp(c)) {      // mu H(z) = L L', store L^-1 and grad F*(z)
                const long e = S.ncone + 9L * S.cexp[c];
                double g[3], H[6], Li[6];
                const double u = Q.z[o], v = Q.z[o + 1], w = Q.z[o + 2];
                if (!exp_dual_interior(u, v, w)) { ok = 0.0; return; }
                exp_dual_grad_hess(u, v, w, g, H);
                for (int i = 0; i < 6; i++) H[i] *= mu_exp;
                if (!chol3_inverse(H, Li)) {
                    // psi -> 0: the rank-one part (1 / psi^2) swamps the rest in double precision; a relative jitter of 1e-14
                    const double jit = 1e-14 * (H[0] + H[2] + H[5]);
                    H[0] += jit; H[2] += jit; H[5] += jit;
                    if (!chol3_inverse(H, Li)) { ok = 0.0; return; }
                }
                for (int i = 0; i < 6; i++) { Q.eta[e + i] = Li[i]; if (!isfinite(Li[i])) ok = 0.0; }
                for (int i = 0; i < 3; i++) { Q.eta[e + 6 + i] = g[i]; Q.wsc[o + i] = 1.0; Q.lam[o + i] = 0.0; }
                return;
            }
            const double s0 = Q.s[o], z0 = Q.z[o];
            double ss = 0.0, zz = 0.0, sz = 0.0;
            for (int r = 1; r < d; r++) { const double sv = Q.s[o + r], zv = Q.z[o + r]; ss += sv * sv; zz += zv * zv; sz += sv * zv; }
            const double sres = sqrt(s0 * s0 - ss), zres = sqrt(z0 * z0 - zz);
            const double gamma = sqrt((1.0 + (s0 * z0 + sz) / (sres * zres)) / 2.0);
            const double w0 = (s0 / sres + z0 / zres) / (2.0 * gamma);
            const double eta = sqrt(sres / zres);
            Q.wsc[o] = w0;
            for (int r = 1; r < d; r++) Q.wsc[o + r] = (Q.s[o + r] / sres - Q.z[o + r] / zres) / (2.0 * gamma);
            Q.eta[c] = eta;
            if (!(isfinite(w0) && isfinite(eta) && eta > 0.0 && isfinite(gamma))) ok = 0.0;
            // lam = W z
            double dot = 0.0;
            for (int r = 1; r < d; r++) dot += Q.wsc[o + r] * Q.z[o + r];
            const double cf = z0 + dot / (1.0 + w0);
            Q.lam[o] = eta * (w0 * z0 + dot);
            for (int r = 1; r < d; r++) Q.lam[o + r] = eta * (Q.z[o + r] + cf * Q.wsc[o + r]);
        });
        return cx.min(ok) > 0.5;   // (the reduction is also the barrier that publishes wsc / eta / lam)
    }
    CONIC_HD void nt_identity() const
    {
        pfor_nb(0, S.l, [&](int i) { Q.wsc[i] = 1.0; });
        pfor(0, S.ncone, [&](int c) {
            const int o = S.cone_off[c], d = S.q[c];
            Q.wsc[o] = 1.0;
            for (int r = 1; r < d; r++) Q.wsc[o + r] = 0.0;
            Q.eta[c] = 1.0;
            if (is_exp(c)) {
                const long e = S.ncone + 9L * S.cexp[c];
                for (int i = 0; i < 9; i++) Q.eta[e + i] = 0.0;
                Q.eta[e] = 1.0; Q.eta[e + 2] = 1.0; Q.eta[e + 5] = 1.0;
                Q.wsc[o + 1] = 1.0; Q.wsc[o + 2] = 1.0;
            }
        });
    }

    // ---------------- KKT: Gt = W^-1 G, numeric LDL', solves ----------------
    CONIC_HD void build_Gt() const
    {
        pfor_nb(0, S.nlp, [&](int t) { const int g = S.lp_gt[t]; Q.Gt[g] = Q.Gx[S.lp_g[t]] / Q.wsc[S.Gti[g]]; });
        pfor(0, S.njob, [&](int jb) {
            const int cn = S.job_cone[jb], g0 = S.job_gt0[jb], o = S.cone_off[cn], d = S.q[cn];
            if (is_exp(cn)) {      // rows of Gt = W^-T G = L^-1 (rows of G)
                const long e = S.ncone + 9L * S.cexp[cn];
                double a[3] = {0.0, 0.0, 0.0};
                for (int t = S.job_src_p[jb]; t < S.job_src_p[jb + 1]; t++) a[S.job_src_row[t]] = Q.Gx[S.job_src_g[t]];
                Q.Gt[g0] = Q.eta[e] * a[0];
                Q.Gt[g0 + 1] = Q.eta[e + 1] * a[0] + Q.eta[e + 2] * a[1];
                Q.Gt[g0 + 2] = Q.eta[e + 3] * a[0] + Q.eta[e + 4] * a[1] + Q.eta[e + 5] * a[2];
                return;
            }
            const double eta = Q.eta[cn], w0 = Q.wsc[o];
            double v0 = 0.0, dot = 0.0;
            for (int t = S.job_src_p[jb]; t < S.job_src_p[jb + 1]; t++) {
                const int rr = S.job_src_row[t];
                const double v = Q.Gx[S.job_src_g[t]];
                if (rr == 0) v0 = v; else dot += Q.wsc[o + rr] * v;
            }
            const double cf = -v0 + dot / (1.0 + w0);
            Q.Gt[g0] = (w0 * v0 - dot) / eta;
            for (int r = 1; r < d; r++) Q.Gt[g0 + r] = cf * Q.wsc[o + r] / eta;
            for (int t = S.job_src_p[jb]; t < S.job_src_p[jb + 1]; t++) {
                const int rr = S.job_src_row[t];
                if (rr > 0) Q.Gt[g0 + rr] += Q.Gx[S.job_src_g[t]] / eta;
            }
        });
    }
    CONIC_HD double src_val(int kind, int idx) const
    {
        switch (kind) {
            case 1: return osc * Q.Px[idx];
            case 2: return Q.Ax[idx];
            case 3: return Q.Gt[idx];
            default: return 0.0;
        }
    }
    // acc - sum_t Ux[a_t] Lx[b_t] over the pair list [q0, q1): 4 index pairs / 8 operands in flight, and the NEXT group's
    // index pairs are fetched while the current group's operands are in flight (software pipeline): a group then costs one
    // memory round trip instead of two dependent ones (index -> operand), which is what these latency-bound chains pay for.
    // The order of the subtractions is unchanged (bit-identical results).
    CONIC_HD double pair_dot(double acc, long long q0, long long q1) const
    {
        long long qq = q0;
        if (qq + 4 <= q1) {
            int2_ p0 = S.pairs[qq], p1 = S.pairs[qq + 1], p2 = S.pairs[qq + 2], p3 = S.pairs[qq + 3];
            for (;;) {
                const long long nx = qq + 4;
                const bool more = nx + 4 <= q1;
                const long long pf = more ? nx : qq;          // clamped: the prefetch is unconditional
                const double u0 = Q.Ux[p0.a], l0 = Q.Lx[p0.b], u1 = Q.Ux[p1.a], l1 = Q.Lx[p1.b];
                const double u2 = Q.Ux[p2.a], l2 = Q.Lx[p2.b], u3 = Q.Ux[p3.a], l3 = Q.Lx[p3.b];
                const int2_ n0 = S.pairs[pf], n1 = S.pairs[pf + 1], n2 = S.pairs[pf + 2], n3 = S.pairs[pf + 3];
                acc -= u0 * l0; acc -= u1 * l1; acc -= u2 * l2; acc -= u3 * l3;
                qq = nx;
                if (!more) break;
                p0 = n0; p1 = n1; p2 = n2; p3 = n3;
            }
        }
        for (; qq < q1; qq++) { const int2_ pr = S.pairs[qq]; acc -= Q.Ux[pr.a] * Q.Lx[pr.b]; }
        return acc;
    }
    // d - sum_r Ux[pos_r] Lx[pos_r] over the row-list range [r, r1), subtracted in order: 4 terms in flight, next indices
    // fetched under the operands
    CONIC_HD double row_sub_sq(double d, int r, int r1) const
    {
        if (r + 4 <= r1) {
            int a0 = S.row_pos[r], a1 = S.row_pos[r + 1], a2 = S.row_pos[r + 2], a3 = S.row_pos[r + 3];
            for (;;) {
                const int nx = r + 4;
                const bool more = nx + 4 <= r1;
                const int pf = more ? nx : r;
                const double u0 = Q.Ux[a0], l0 = Q.Lx[a0], u1 = Q.Ux[a1], l1 = Q.Lx[a1];
                const double u2 = Q.Ux[a2], l2 = Q.Lx[a2], u3 = Q.Ux[a3], l3 = Q.Lx[a3];
                const int b0 = S.row_pos[pf], b1 = S.row_pos[pf + 1], b2 = S.row_pos[pf + 2], b3 = S.row_pos[pf + 3];
                d -= u0 * l0; d -= u1 * l1; d -= u2 * l2; d -= u3 * l3;
                r = nx;
                if (!more) break;
                a0 = b0; a1 = b1; a2 = b2; a3 = b3;
            }
        }
        for (; r < r1; r++) { const int pos = S.row_pos[r]; d -= Q.Ux[pos] * Q.Lx[pos]; }
        return d;
    }
    // level-scheduled LDL': per level (a) the pivots of its columns, (b) the entries of its columns.  Long rows / pair
    // lists are summed in chunks by different workers and combined in a second phase (Symbolic::LONG_ITEM).
    CONIC_HD bool factor()
    {
        double ok = 1.0;
        auto pivot = [&](int j, double d) {     // d = K(j,j) +- reg - sum: sign test, dynamic regularisation, 1 / d
            const int kind = S.d_kind[j];
            const double sg = kind == 0 ? 1.0 : -1.0;
            if (!(d * sg > O.dyn_eps)) {   // wrong sign, tiny or NaN: ECOS-style dynamic regularisation
                if (!(d == d)) ok = 0.0;
                CONIC_DBG("dynreg col %d kind %d d %.3e\n", j, kind, d);
                d = sg * O.dyn_delta; nreg++;
            }
            Q.Dinv[j] = 1.0 / d;
        };
        auto diag0 = [&](int j) {
            const int kind = S.d_kind[j];
            double d = kind == 0 ? reg : (kind == 1 ? -reg : -(1.0 + reg));
            if (S.d_src[j] == 1) d += osc * Q.Px[S.d_src_idx[j]];
            return d;
        };
        for (int lv = 0; lv < S.nlev; lv++) {
            const int c0 = S.lev_p[lv], c1 = S.lev_p[lv + 1], cs = c0 + S.lev_nshort[lv];
            const int k0 = S.rchunk_p[lv], k1 = S.rchunk_p[lv + 1];
            const int Ga = coop_width((cs - c0) + (k1 - k0));       // items of the pivot phase: short columns + chunks
            if (Ga == 1) {
                pfor_nb(c0, cs, [&](int t) {
                    const int j = S.lev_cols[t];
                    pivot(j, row_sub_sq(diag0(j), S.row_p[j], S.row_p[j + 1]));
                });
                if (k1 > k0) {
                    pfor(k0, k1, [&](int t) { Q.part[t - k0] = -row_sub_sq(0.0, S.rchunk_r0[t], S.rchunk_r1[t]); });
                    pfor_nb(cs, c1, [&](int t) {
                        const int j = S.lev_cols[t];
                        double d = diag0(j);
                        for (int c = S.col_c0[t]; c < S.col_c1[t]; c++) d -= Q.part[c - k0];
                        pivot(j, d);
                    });
                }
            } else {
                pfor_coop(c0, cs, Ga, [&](int t, int gl, int G) { const int j = S.lev_cols[t]; return row_sq_part(S.row_p[j], S.row_p[j + 1], gl, G); },
                          [&](int t, double sg) { const int j = S.lev_cols[t]; pivot(j, diag0(j) - sg); });
                if (k1 > k0) {
                    pfor_coop(k0, k1, Ga, [&](int t, int gl, int G) { return row_sq_part(S.rchunk_r0[t], S.rchunk_r1[t], gl, G); },
                              [&](int t, double sg) { Q.part[t - k0] = sg; });
                    cx.barrier();
                    const int Gc = coop_width(c1 - cs);
                    pfor_coop(cs, c1, Gc, [&](int t, int gl, int G) { return part_part(S.col_c0[t], S.col_c1[t], k0, gl, G); },
                              [&](int t, double sg) { const int j = S.lev_cols[t]; pivot(j, diag0(j) - sg); });
                }
            }
            cx.barrier();
            const int e0 = S.lev_ent_p[lv], e1 = S.lev_ent_p[lv + 1], es = e0 + S.lev_ent_nshort[lv];
            const int h0 = S.echunk_p[lv], h1 = S.echunk_p[lv + 1];
            const int Ge = coop_width((es - e0) + (h1 - h0));
            auto put = [&](int e, double acc) { Q.Ux[e] = acc; Q.Lx[e] = acc * Q.Dinv[S.ent_col[e]]; };
            if (Ge == 1) {
                pfor_nb(e0, es, [&](int t) {
                    const int e = S.lev_ent[t];
                    put(e, pair_dot(src_val(S.l_src[e], S.l_src_idx[e]), S.pair_p[e], S.pair_p[e + 1]));
                });
                if (h1 > h0) {
                    pfor(h0, h1, [&](int t) { Q.part[t - h0] = -pair_dot(0.0, S.echunk_q0[t], S.echunk_q1[t]); });
                    pfor_nb(es, e1, [&](int t) {
                        const int e = S.lev_ent[t];
                        double acc = src_val(S.l_src[e], S.l_src_idx[e]);
                        for (int c = S.ent_c0[t]; c < S.ent_c1[t]; c++) acc -= Q.part[c - h0];
                        put(e, acc);
                    });
                }
            } else {
                pfor_coop(e0, es, Ge, [&](int t, int gl, int G) { const int e = S.lev_ent[t]; return pair_part(S.pair_p[e], S.pair_p[e + 1], gl, G); },
                          [&](int t, double sg) { const int e = S.lev_ent[t]; put(e, src_val(S.l_src[e], S.l_src_idx[e]) - sg); });
                if (h1 > h0) {
                    pfor_coop(h0, h1, Ge, [&](int t, int gl, int G) { return pair_part(S.echunk_q0[t], S.echunk_q1[t], gl, G); },
                              [&](int t, double sg) { Q.part[t - h0] = sg; });
                    cx.barrier();
                    const int Gc = coop_width(e1 - es);
                    pfor_coop(es, e1, Gc, [&](int t, int gl, int G) { return part_part(S.ent_c0[t], S.ent_c1[t], h0, gl, G); },
                              [&](int t, double sg) { const int e = S.lev_ent[t]; put(e, src_val(S.l_src[e], S.l_src_idx[e]) - sg); });
                }
            }
            cx.barrier();
        }
        return cx.min(ok) > 0.5;
    }
    // acc - sum_r Lx[pos_r] tmp[k_r] over the row-list range [r, r1) (forward substitution), subtracted in order,
    // software-pipelined like pair_dot
    CONIC_HD double row_sub_tmp(double acc, int r, int r1) const
    {
        if (r + 4 <= r1) {
            int a0 = S.row_pos[r], a1 = S.row_pos[r + 1], a2 = S.row_pos[r + 2], a3 = S.row_pos[r + 3];
            int k0 = S.row_k[r], k1 = S.row_k[r + 1], k2 = S.row_k[r + 2], k3 = S.row_k[r + 3];
            for (;;) {
                const int nx = r + 4;
                const bool more = nx + 4 <= r1;
                const int pf = more ? nx : r;
                const double l0 = Q.Lx[a0], l1 = Q.Lx[a1], l2 = Q.Lx[a2], l3 = Q.Lx[a3];
                const double t0 = Q.tmp[k0], t1 = Q.tmp[k1], t2 = Q.tmp[k2], t3 = Q.tmp[k3];
                const int b0 = S.row_pos[pf], b1 = S.row_pos[pf + 1], b2 = S.row_pos[pf + 2], b3 = S.row_pos[pf + 3];
                const int m0 = S.row_k[pf], m1 = S.row_k[pf + 1], m2 = S.row_k[pf + 2], m3 = S.row_k[pf + 3];
                acc -= l0 * t0; acc -= l1 * t1; acc -= l2 * t2; acc -= l3 * t3;
                r = nx;
                if (!more) break;
                a0 = b0; a1 = b1; a2 = b2; a3 = b3; k0 = m0; k1 = m1; k2 = m2; k3 = m3;
            }
        }
        for (; r < r1; r++) acc -= Q.Lx[S.row_pos[r]] * Q.tmp[S.row_k[r]];
        return acc;
    }
    // out = K^-1 in  (in, out in the original [x; y; z] numbering; uses tmp)
    // Software-pipelined substitution sweeps (round 5; device, one workgroup per problem).  A sweep is ~2 x 118 barrier-separated
    // phases and a phase was a chain of FOUR dependent memory round trips (level bounds -> column -> row bounds -> term indices ->
    // operands) before its only arithmetic.  Everything but the operand tmp[k] is independent of the solve -- the schedule, the
    // factor entries Lx, the right-hand side -- so a lane fetches, BEFORE the barrier that ends level lv - 1, its item of level lv:
    // column, bounds, its first four strided terms (index, Lx) and the right-hand side.  After the barrier a phase is one round
    // trip (tmp[k]), the group's butterfly sum and a store.  Levels with chunked items or more items than groups take the
    // unpipelined path.  Same arithmetic, in the same order, as pfor_coop.
    // backward substitution of one column by ONE worker (4 terms in flight, next indices under the operands)
    CONIC_HD void bwd_col(int j, const BV& out) const
    {
        double acc = Q.tmp[j] * Q.Dinv[j];
        int e = S.Lp[j];
        const int e1 = S.Lp[j + 1];
        if (e + 4 <= e1) {
            int i0 = S.Li[e], i1 = S.Li[e + 1], i2 = S.Li[e + 2], i3 = S.Li[e + 3];
            for (;;) {
                const int nx = e + 4;
                const bool more = nx + 4 <= e1;
                const int pf = more ? nx : e;
                const double l0 = Q.Lx[e], l1 = Q.Lx[e + 1], l2 = Q.Lx[e + 2], l3 = Q.Lx[e + 3];
                const double t0 = Q.tmp[i0], t1 = Q.tmp[i1], t2 = Q.tmp[i2], t3 = Q.tmp[i3];
                const int n0 = S.Li[pf], n1 = S.Li[pf + 1], n2 = S.Li[pf + 2], n3 = S.Li[pf + 3];
                acc -= l0 * t0; acc -= l1 * t1; acc -= l2 * t2; acc -= l3 * t3;
                e = nx;
                if (!more) break;
                i0 = n0; i1 = n1; i2 = n2; i3 = n3;
            }
        }
        for (; e < e1; e++) acc -= Q.Lx[e] * Q.tmp[S.Li[e]];
        Q.tmp[j] = acc;
        out[S.perm[j]] = acc;
    }
    struct PreF { int G, has, j, r0, r1, k[4], simple; double l[4], rhs; };
    CONIC_HD void prep_fwd(int lv, const BV& in, PreF& P) const
    {
        P.simple = 0; P.has = 0; P.G = 1;
        if (lv >= S.nlev) return;
        const int c0 = S.lev_p[lv], cs = c0 + S.lev_nshort[lv];
        const int k0 = S.rchunk_p[lv], k1 = S.rchunk_p[lv + 1];
        const int G = coop_width((cs - c0) + (k1 - k0));
        P.G = G;
        if (G <= 1 || k1 > k0 || (cs - c0) > cx.nw() / G) return;
        P.simple = 1;
        const int t = c0 + cx.wid() / G, gl = cx.wid() % G;
        if (t >= cs) return;
        P.has = 1;
        const int j = S.lev_cols[t];
        P.j = j; P.r0 = S.row_p[j]; P.r1 = S.row_p[j + 1];
        P.rhs = in[S.perm[j]];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int tt = P.r0 + gl + u * G;
            const int tc = tt < P.r1 ? tt : (P.r1 > P.r0 ? P.r1 - 1 : P.r0);      // clamped: the loads are unconditional
            const bool okk = tt < P.r1;
            P.k[u] = okk ? S.row_k[tc] : -1;
            P.l[u] = okk ? Q.Lx[S.row_pos[tc]] : 0.0;
        }
    }
    struct PreB { int G, has, j, e0, e1, i[4], simple; double l[4], dj; };
    CONIC_HD void prep_bwd(int lv, PreB& P) const
    {
        P.simple = 0; P.has = 0; P.G = 1;
        if (lv >= S.nrlev) return;
        const int c0 = S.rlev_p[lv], c1 = S.rlev_p[lv + 1];
        const int G = coop_width(c1 - c0);
        P.G = G;
        if (G <= 1 || (c1 - c0) > cx.nw() / G) return;
        P.simple = 1;
        const int t = c0 + cx.wid() / G, gl = cx.wid() % G;
        if (t >= c1) return;
        P.has = 1;
        const int j = S.rlev_cols[t];
        P.j = j; P.e0 = S.Lp[j]; P.e1 = S.Lp[j + 1];
        P.dj = Q.Dinv[j];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int tt = P.e0 + gl + u * G;
            const int tc = tt < P.e1 ? tt : (P.e1 > P.e0 ? P.e1 - 1 : P.e0);
            const bool okk = tt < P.e1;
            P.i[u] = okk ? S.Li[tc] : -1;
            P.l[u] = okk ? Q.Lx[tc] : 0.0;
        }
    }
    CONIC_HD void solve_raw_pipelined(const BV& in, const BV& out) const
    {
        PreF P;
        const long long tf_ = CPROF_T();
        prof_[6] += 1;
        prep_fwd(0, in, P);
        for (int lv = 0; lv < S.nlev; lv++) {
            PreF N;
            if (P.simple) {
                const int G = P.G, gl = cx.wid() % G;
                double a = 0.0;
                if (P.has) {
                    double tv[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) tv[u] = P.k[u] >= 0 ? Q.tmp[P.k[u]] : 0.0;
                    prep_fwd(lv + 1, in, N);       // the next level's fetches fly under this level's operands
#pragma unroll
                    for (int u = 0; u < 4; u++) a += P.l[u] * tv[u];
                    if (P.r1 - P.r0 > 4 * G) a += row_tmp_part(P.r0 + 4 * G, P.r1, gl, G);
                } else {
                    prep_fwd(lv + 1, in, N);
                }
                const double sg = cx.gsum(a, G);
                if (P.has && gl == 0) Q.tmp[P.j] = P.rhs - sg;
            } else {
                const int c0 = S.lev_p[lv], c1 = S.lev_p[lv + 1], cs = c0 + S.lev_nshort[lv];
                const int k0 = S.rchunk_p[lv], k1 = S.rchunk_p[lv + 1];
                const int Ga = P.G;
                if (Ga == 1) {
                    pfor_nb(c0, cs, [&](int t) {
                        const int j = S.lev_cols[t];
                        Q.tmp[j] = row_sub_tmp(in[S.perm[j]], S.row_p[j], S.row_p[j + 1]);
                    });
                    if (k1 > k0) {
                        pfor(k0, k1, [&](int t) { Q.part[t - k0] = -row_sub_tmp(0.0, S.rchunk_r0[t], S.rchunk_r1[t]); });
                        pfor_nb(cs, c1, [&](int t) {
                            const int j = S.lev_cols[t];
                            double acc = in[S.perm[j]];
                            for (int c = S.col_c0[t]; c < S.col_c1[t]; c++) acc -= Q.part[c - k0];
                            Q.tmp[j] = acc;
                        });
                    }
                } else {
                    pfor_coop(c0, cs, Ga, [&](int t, int gl, int G) { const int j = S.lev_cols[t]; return row_tmp_part(S.row_p[j], S.row_p[j + 1], gl, G); },
                              [&](int t, double sg) { const int j = S.lev_cols[t]; Q.tmp[j] = in[S.perm[j]] - sg; });
                    if (k1 > k0) {
                        pfor_coop(k0, k1, Ga, [&](int t, int gl, int G) { return row_tmp_part(S.rchunk_r0[t], S.rchunk_r1[t], gl, G); },
                                  [&](int t, double sg) { Q.part[t - k0] = sg; });
                        cx.barrier();
                        const int Gc = coop_width(c1 - cs);
                        pfor_coop(cs, c1, Gc, [&](int t, int gl, int G) { return part_part(S.col_c0[t], S.col_c1[t], k0, gl, G); },
                                  [&](int t, double sg) { const int j = S.lev_cols[t]; Q.tmp[j] = in[S.perm[j]] - sg; });
                    }
                }
                prep_fwd(lv + 1, in, N);
            }
            cx.barrier();
            P = N;
        }
        CPROF_ADD(1, tf_);
        const long long tb_ = CPROF_T();
        PreB B_;
        prep_bwd(0, B_);
        for (int lv = 0; lv < S.nrlev; lv++) {
            PreB N;
            if (B_.simple) {
                const int G = B_.G, gl = cx.wid() % G;
                double a = 0.0, tj = 0.0;
                if (B_.has) {
                    double tv[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) tv[u] = B_.i[u] >= 0 ? Q.tmp[B_.i[u]] : 0.0;
                    tj = Q.tmp[B_.j];
                    prep_bwd(lv + 1, N);
#pragma unroll
                    for (int u = 0; u < 4; u++) a += B_.l[u] * tv[u];
                    if (B_.e1 - B_.e0 > 4 * G) a += col_tmp_part(B_.e0 + 4 * G, B_.e1, gl, G);
                } else {
                    prep_bwd(lv + 1, N);
                }
                const double sg = cx.gsum(a, G);
                if (B_.has && gl == 0) { const double acc = tj * B_.dj - sg; Q.tmp[B_.j] = acc; out[S.perm[B_.j]] = acc; }
            } else {
                const int Gb = B_.G;
                if (Gb > 1) {
                    pfor_coop(S.rlev_p[lv], S.rlev_p[lv + 1], Gb, [&](int t, int gl, int G) { const int j = S.rlev_cols[t]; return col_tmp_part(S.Lp[j], S.Lp[j + 1], gl, G); },
                              [&](int t, double sg) { const int j = S.rlev_cols[t]; const double acc = Q.tmp[j] * Q.Dinv[j] - sg; Q.tmp[j] = acc; out[S.perm[j]] = acc; });
                } else {
                    pfor_nb(S.rlev_p[lv], S.rlev_p[lv + 1], [&](int t) { bwd_col(S.rlev_cols[t], out); });
                }
                prep_bwd(lv + 1, N);
            }
            cx.barrier();
            B_ = N;
        }
        CPROF_ADD(2, tb_);
    }
    CONIC_HD void solve_raw(const BV& in, const BV& out) const
    {
        if constexpr (Ctx::COOP && !Ctx::COOP_EMU) { solve_raw_pipelined(in, out); return; }
        for (int lv = 0; lv < S.nlev; lv++) {
            const int c0 = S.lev_p[lv], c1 = S.lev_p[lv + 1], cs = c0 + S.lev_nshort[lv];
            const int k0 = S.rchunk_p[lv], k1 = S.rchunk_p[lv + 1];
            const int Ga = coop_width((cs - c0) + (k1 - k0));
            if (Ga == 1) {
                pfor_nb(c0, cs, [&](int t) {
                    const int j = S.lev_cols[t];
                    Q.tmp[j] = row_sub_tmp(in[S.perm[j]], S.row_p[j], S.row_p[j + 1]);
                });
                if (k1 > k0) {
                    pfor(k0, k1, [&](int t) { Q.part[t - k0] = -row_sub_tmp(0.0, S.rchunk_r0[t], S.rchunk_r1[t]); });
                    pfor_nb(cs, c1, [&](int t) {
                        const int j = S.lev_cols[t];
                        double acc = in[S.perm[j]];
                        for (int c = S.col_c0[t]; c < S.col_c1[t]; c++) acc -= Q.part[c - k0];
                        Q.tmp[j] = acc;
                    });
                }
            } else {
                pfor_coop(c0, cs, Ga, [&](int t, int gl, int G) { const int j = S.lev_cols[t]; return row_tmp_part(S.row_p[j], S.row_p[j + 1], gl, G); },
                          [&](int t, double sg) { const int j = S.lev_cols[t]; Q.tmp[j] = in[S.perm[j]] - sg; });
                if (k1 > k0) {
                    pfor_coop(k0, k1, Ga, [&](int t, int gl, int G) { return row_tmp_part(S.rchunk_r0[t], S.rchunk_r1[t], gl, G); },
                              [&](int t, double sg) { Q.part[t - k0] = sg; });
                    cx.barrier();
                    const int Gc = coop_width(c1 - cs);
                    pfor_coop(cs, c1, Gc, [&](int t, int gl, int G) { return part_part(S.col_c0[t], S.col_c1[t], k0, gl, G); },
                              [&](int t, double sg) { const int j = S.lev_cols[t]; Q.tmp[j] = in[S.perm[j]] - sg; });
                }
            }
            cx.barrier();
        }
        for (int lv = 0; lv < S.nrlev; lv++) {
            const int Gb = coop_width(S.rlev_p[lv + 1] - S.rlev_p[lv]);
            if (Gb > 1) {
                pfor_coop(S.rlev_p[lv], S.rlev_p[lv + 1], Gb, [&](int t, int gl, int G) { const int j = S.rlev_cols[t]; return col_tmp_part(S.Lp[j], S.Lp[j + 1], gl, G); },
                          [&](int t, double sg) { const int j = S.rlev_cols[t]; const double acc = Q.tmp[j] * Q.Dinv[j] - sg; Q.tmp[j] = acc; out[S.perm[j]] = acc; });
                cx.barrier();
                continue;
            }
            pfor(S.rlev_p[lv], S.rlev_p[lv + 1], [&](int t) {
                const int j = S.rlev_cols[t];
                double acc = Q.tmp[j] * Q.Dinv[j];
                int e = S.Lp[j];
                const int e1 = S.Lp[j + 1];
                if (e + 4 <= e1) {     // software pipeline: the next group's row indices under the current operands
                    int i0 = S.Li[e], i1 = S.Li[e + 1], i2 = S.Li[e + 2], i3 = S.Li[e + 3];
                    for (;;) {
                        const int nx = e + 4;
                        const bool more = nx + 4 <= e1;
                        const int pf = more ? nx : e;
                        const double l0 = Q.Lx[e], l1 = Q.Lx[e + 1], l2 = Q.Lx[e + 2], l3 = Q.Lx[e + 3];
                        const double t0 = Q.tmp[i0], t1 = Q.tmp[i1], t2 = Q.tmp[i2], t3 = Q.tmp[i3];
                        const int n0 = S.Li[pf], n1 = S.Li[pf + 1], n2 = S.Li[pf + 2], n3 = S.Li[pf + 3];
                        acc -= l0 * t0; acc -= l1 * t1; acc -= l2 * t2; acc -= l3 * t3;
                        e = nx;
                        if (!more) break;
                        i0 = n0; i1 = n1; i2 = n2; i3 = n3;
                    }
                }
                for (; e < e1; e++) acc -= Q.Lx[e] * Q.tmp[S.Li[e]];
                Q.tmp[j] = acc;
                out[S.perm[j]] = acc;
            });
        }
    }
    // res = rhs - Ktrue sol  (unregularised scaled KKT matrix); returns |res|_2^2
    CONIC_HD double kkt_residual(const BV& rhs, const BV& sol, const BV& res) const
    {
        const int n = S.n, p = S.p, m = S.m;
        double nrm = 0.0;
        const long long tr_ = CPROF_T();
        prof_[7] += 1;
        // Rows of the globally coupled variables -- thousands of terms -- are left to whole waves below (Symbolic::kk_long): one
        // worker walking such a row kept the other 1 023 at the barrier for 0.9 ms per call, more than a whole substitution sweep
        // (profiles/r05_k5_phase_profile.txt).  (A unified, software-pipelined row list for ALL rows was measured slower: most rows
        // have fewer than four terms.)
        auto is_long = [&](int r) { return Ctx::COOP && S.kk_p[r + 1] - S.kk_p[r] > S.kk_long_thr; };
        pfor_nb(0, n, [&](int i) {
            if (is_long(i)) return;
            double acc = rhs[i];
            for (int t = S.Pf_p[i]; t < S.Pf_p[i + 1]; t++) acc -= osc * Q.Px[S.Pf_pos[t]] * sol[S.Pf_j[t]];
            for (int e = S.Ap[i]; e < S.Ap[i + 1]; e++) acc -= Q.Ax[e] * sol[n + S.Ai[e]];
            for (int e = S.Gtp[i]; e < S.Gtp[i + 1]; e++) acc -= Q.Gt[e] * sol[n + p + S.Gti[e]];
            res[i] = acc; nrm += acc * acc;
        });
        pfor_nb(0, p, [&](int r) {
            if (is_long(n + r)) return;
            double acc = rhs[n + r];
            for (int t = S.Ar_p[r]; t < S.Ar_p[r + 1]; t++) acc -= Q.Ax[S.Ar_pos[t]] * sol[S.Ar_j[t]];
            res[n + r] = acc; nrm += acc * acc;
        });
        pfor_nb(0, m, [&](int r) {
            if (is_long(n + p + r)) return;
            double acc = rhs[n + p + r] + sol[n + p + r];
            for (int t = S.Gtr_p[r]; t < S.Gtr_p[r + 1]; t++) acc -= Q.Gt[S.Gtr_pos[t]] * sol[S.Gtr_j[t]];
            res[n + p + r] = acc; nrm += acc * acc;
        });
        if (Ctx::COOP) {
            pfor_coop(0, S.nkk_long, 64, [&](int q_, int gl, int G) {
                const int r = S.kk_long[q_];
                double a = 0.0;
                int t = S.kk_p[r] + gl;
                const int t1 = S.kk_p[r + 1];
                for (; t + 3 * G < t1; t += 4 * G) {
                    const double v0 = src_val(S.kk_src[t], S.kk_idx[t]), v1 = src_val(S.kk_src[t + G], S.kk_idx[t + G]);
                    const double v2 = src_val(S.kk_src[t + 2 * G], S.kk_idx[t + 2 * G]), v3 = src_val(S.kk_src[t + 3 * G], S.kk_idx[t + 3 * G]);
                    const double x0 = sol[S.kk_col[t]], x1 = sol[S.kk_col[t + G]], x2 = sol[S.kk_col[t + 2 * G]], x3 = sol[S.kk_col[t + 3 * G]];
                    a += v0 * x0; a += v1 * x1; a += v2 * x2; a += v3 * x3;
                }
                for (; t < t1; t += G) a += src_val(S.kk_src[t], S.kk_idx[t]) * sol[S.kk_col[t]];
                return a;
            }, [&](int q_, double sg) {
                const int r = S.kk_long[q_];
                const double acc = rhs[r] + (r >= n + p ? sol[r] : 0.0) - sg;
                res[r] = acc; nrm += acc * acc;
            });
        }
        CPROF_ADD(5, tr_);          // the rows alone
        const double out_ = cx.sum(nrm);
        CPROF_ADD(3, tr_);
        return out_;
    }
    // sol = Ktrue^-1 rhs by the regularised factor + iterative refinement (oracle/ipm.py: kkt_factor.solve_)
    CONIC_HD void solve_refined(const BV& rhs, const BV& sol)
    {
        double rn = 0.0;
        pfor_nb(0, S.nk, [&](int i) { rn += rhs[i] * rhs[i]; });
        rn = cx.sum(rn);
        const double tol = O.ref_tol * (1.0 + sqrt(rn));
        solve_raw(rhs, sol);
        double prev = 1e300, last_rel = 0.0;
        bool refining = true;
        for (int it = 0; it < O.nref; it++) {
            const double r2 = sqrt(kkt_residual(rhs, sol, Q.res));
            if (refining) last_rel = r2 / (1.0 + sqrt(rn));   // (the residual the last correction starts from)
            if (r2 <= tol || !(r2 < prev)) refining = false;   // converged, or refinement stopped helping
            if (!cx.any(refining)) break;
            prev = r2;
            solve_raw(Q.res, Q.cor);
            if (refining) { pfor_nb(0, S.nk, [&](int i) { sol[i] += Q.cor[i]; }); nrefine++; }
            cx.barrier();
        }
        lin_worst = fmax(lin_worst, last_rel);
    }
    // Newton step for the complementarity right-hand side d_s (stored in Q.corr on entry):
    //   rhs = [-rx; -ry; -rz - W (lam \ d_s)], scaled solve, dz = W^-1 dzt, ds = -rz - G dx
    // results: sol[0:n] = dx, sol[n:n+p] = dy, Q.dz, Q.ds
    CONIC_HD void newton()
    {
        const int n = S.n, p = S.p, m = S.m;
        // t = lam \ d_s  (in place in corr)
        pfor_nb(0, S.l, [&](int i) { Q.corr[i] = Q.corr[i] / Q.lam[i]; });
        pfor_nb(0, S.ncone, [&](int c) {
            if (is_exp(c)) return;      // corr holds q = s + sigma mu grad F*(z) of the exponential rows (unscaled): see below
            const int o = S.cone_off[c], d = S.q[c];
            const double l0 = Q.lam[o], d0 = Q.corr[o];
            double l1l1 = 0.0, l1d1 = 0.0;
            for (int r = 1; r < d; r++) { l1l1 += Q.lam[o + r] * Q.lam[o + r]; l1d1 += Q.lam[o + r] * Q.corr[o + r]; }
            const double u0 = (l0 * d0 - l1d1) / (l0 * l0 - l1l1);
            Q.corr[o] = u0;
            for (int r = 1; r < d; r++) Q.corr[o + r] = (Q.corr[o + r] - u0 * Q.lam[o + r]) / l0;
        });
        // rhs third block (already scaled by W^-T): W^-T (-rz - W' t) = -W^-T rz - t; exponential rows: W^-T (-rz + q)
        pfor(0, m, [&](int r) { Q.dz[r] = -Q.rz[r]; });
        if (S.nexp > 0) {
            pfor(0, S.ncone, [&](int c) {
                if (!is_exp(c)) return;
                const int o = S.cone_off[c];
                for (int r = 0; r < 3; r++) { Q.dz[o + r] += Q.corr[o + r]; Q.corr[o + r] = 0.0; }
            });
        }
        apply_W(Q.dz, true, true);
        pfor_nb(0, n, [&](int i) { Q.rhs[i] = -Q.rx[i]; });
        pfor_nb(0, p, [&](int r) { Q.rhs[n + r] = -Q.ry[r]; });
        pfor(0, m, [&](int r) { Q.rhs[n + p + r] = Q.dz[r] - Q.corr[r]; });
        solve_refined(Q.rhs, Q.sol);
        pfor(0, m, [&](int r) { Q.dz[r] = Q.sol[n + p + r]; });
        apply_W(Q.dz, true);   // dz = W^-1 dzt
        pfor(0, m, [&](int r) {
            double acc = -Q.rz[r];
            for (int t = S.Gr_p[r]; t < S.Gr_p[r + 1]; t++) acc -= Q.Gx[S.Gr_pos[t]] * Q.sol[S.Gr_j[t]];
            Q.ds[r] = acc;
        });
    }

    CONIC_HD void jordan_sq_neg(const BV& out) const
    {
        pfor_nb(0, S.l, [&](int i) { out[i] = -Q.lam[i] * Q.lam[i]; });
        pfor(0, S.ncone, [&](int c) {
            const int o = S.cone_off[c], d = S.q[c];
            if (is_exp(c)) { for (int r = 0; r < 3; r++) out[o + r] = Q.s[o + r]; return; }     // affine: q = s
            double ll0 = 0.0;
            for (int r = 0; r < d; r++) ll0 += Q.lam[o + r] * Q.lam[o + r];
            const double l0 = Q.lam[o];
            for (int r = 1; r < d; r++) out[o + r] = -2.0 * l0 * Q.lam[o + r];
            out[o] = -ll0;
        });
    }
    // exponential pairs of the trial point (s + a ds, z + a dz): each keeps at least a tenth of the average complementarity
    CONIC_HD bool exp_neighbourhood(double a, int deg) const
    {
        double tot = 0.0;
        pfor_nb(0, S.m, [&](int r) { tot += (Q.s[r] + a * Q.ds[r]) * (Q.z[r] + a * Q.dz[r]); });
        tot = cx.sum(tot);
        const double mu_t = tot / (double)deg;
        double ok = 1.0;
        pfor_nb(0, S.ncone, [&](int c) {
            if (!is_exp(c)) return;
            const int o = S.cone_off[c];
            double sz = 0.0;
            for (int r = 0; r < 3; r++) sz += (Q.s[o + r] + a * Q.ds[o + r]) * (Q.z[o + r] + a * Q.dz[o + r]);
            if (!(sz / 3.0 >= 0.1 * mu_t)) ok = 0.0;
        });
        return cx.min(ok) > 0.5;
    }

    // `live`: false for the padding lanes of a ragged last group (they run the same control flow, their results are
    // discarded)
    CONIC_HD Result run(bool live = true)
    {
        const int n = S.n, p = S.p, m = S.m;
        Result R;
        R.status = ST_ITERLIM; R.iters = 0;
        R.pcost = R.dcost = R.gap = R.pres = R.dres = R.relgap = 0.0;
        R.pinf = R.dinf = 1e300;
        const int deg = S.l + S.ncone + 2 * S.nexp;      // an exponential cone has degree 3
        bool done = !live;
        // ---- objective scale (see osc) ----
        {
            double mc = 0.0;
            pfor_nb(0, n, [&](int i) { mc = fmax(mc, fabs(Q.c[i])); });
            pfor_nb(0, S.nnzP, [&](int e) { mc = fmax(mc, fabs(Q.Px[e])); });
            mc = -cx.min(-mc);
            osc = mc > OBJ_MAX ? OBJ_MAX / mc : 1.0;
        }
        // ---- initial point (cvxopt coneqp): K(W = I) [x; y; z] = [-c; b; h], s = -z, shift ----
        nt_identity();
        build_Gt();
        const bool fok = factor();
        pfor_nb(0, n, [&](int i) { Q.rhs[i] = -osc * Q.c[i]; });
        pfor_nb(0, p, [&](int r) { Q.rhs[n + r] = Q.b[r]; });
        pfor(0, m, [&](int r) { Q.rhs[n + p + r] = Q.h[r]; });
        solve_refined(Q.rhs, Q.sol);
        // (a problem that is not live keeps the solution it holds: the fallback pass of Engine::launch re-solves a subset)
        pfor_nb(0, n, [&](int i) { if (!done) Q.x[i] = Q.sol[i]; });
        pfor_nb(0, p, [&](int r) { if (!done) Q.y[r] = Q.sol[n + r]; });
        pfor(0, m, [&](int r) { if (!done) { const double zz = Q.sol[n + p + r]; Q.z[r] = zz; Q.s[r] = -zz; } });
        shift_interior(Q.s, !done);
        shift_interior(Q.z, !done);
        if (S.nexp > 0) {
            // exponential pairs start on the central ray (s, z) = (t c, t c), mu = t^2 = the average complementarity of the symmetric part
            double sz = 0.0;
            pfor_nb(0, S.l, [&](int r) { sz += Q.s[r] * Q.z[r]; });
            pfor_nb(0, S.ncone, [&](int c) {
                if (is_exp(c)) return;
                const int o = S.cone_off[c], d = S.q[c];
                for (int r = 0; r < d; r++) sz += Q.s[o + r] * Q.z[o + r];
            });
            sz = cx.sum(sz);
            const int dsym = S.l + S.ncone - S.nexp;
            const double t0 = dsym > 0 ? sqrt(fmax(1.0, sz / (double)dsym)) : 1.0;
            pfor(0, S.ncone, [&](int c) {
                if (!is_exp(c) || done) return;
                const int o = S.cone_off[c];
                Q.s[o] = t0 * CONIC_EXP_C0; Q.s[o + 1] = t0 * CONIC_EXP_C1; Q.s[o + 2] = t0 * CONIC_EXP_C2;
                Q.z[o] = t0 * CONIC_EXP_C0; Q.z[o + 1] = t0 * CONIC_EXP_C1; Q.z[o + 2] = t0 * CONIC_EXP_C2;
            });
        }
        double nb = 0.0, nh = 0.0, nc = 0.0;
        pfor_nb(0, p, [&](int r) { nb += Q.b[r] * Q.b[r]; });
        pfor_nb(0, m, [&](int r) { nh += Q.h[r] * Q.h[r]; });
        pfor_nb(0, n, [&](int i) { nc += osc * Q.c[i] * osc * Q.c[i]; });
        nb = cx.sum(nb); nh = cx.sum(nh); nc = cx.sum(nc);
        // the dual residual is measured on the NORMALISED objective, |osc rx| / max(1, |osc c|): with P values of 1e7 next to a cost
        // vector of order 1 the original-unit test |rx| <= 1e-8 max(1, |c|) asks for 1e-15 relative accuracy of the terms of rx,
        // which no double-precision solver delivers (the oracle's un-normalised solver and, presumably, ECOS end such programs
        // NUMERICAL_ERROR: tests/test_outcomes_cpu.py).  The gap tests below are in the units of the original objective.
        const double nrm_b = fmax(1.0, sqrt(nb)), nrm_h = fmax(1.0, sqrt(nh)), nrm_c = fmax(1.0, sqrt(nc));
        if (!fok && !done) { R.status = ST_NUMERR; done = true; }
        double best_merit = 1e300;
        int best_it = 0;
        // The counters a problem reports are those it had when IT stopped: at the exit tests, or at the end of the iteration that
        // stopped it half way -- where a single-worker run leaves the loop.  A finished problem of a shared workgroup runs along for as
        // long as its neighbours iterate and its factorisations and refinements go on counting: reported as they stood at the end of
        // run(), dyn_regs / refinements of a problem depended on the other problems of its workgroup.
        int nreg_out = 0, nrefine_out = 0;
        bool counted = false;
        auto freeze_counters = [&]() { if (done && !counted) { nreg_out = nreg; nrefine_out = nrefine; counted = true; } };

        for (int it = 0; it <= O.max_iter; it++) {
            if (!cx.any(!done)) break;
            // ---- residuals ----
            double xPx = 0.0, cxv = 0.0, nrx = 0.0, naz = 0.0, nPx = 0.0;
            auto rx_row = [&](int i, double az) {
                double px = 0.0;
                for (int t = S.Pf_p[i]; t < S.Pf_p[i + 1]; t++) px += osc * Q.Px[S.Pf_pos[t]] * Q.x[S.Pf_j[t]];
                const double xi = Q.x[i], ci = osc * Q.c[i];
                const double r = px + az + ci;
                Q.rx[i] = r;
                xPx += xi * px; cxv += ci * xi; nrx += r * r; naz += az * az; nPx += px * px;
            };
            pfor_nb(0, n, [&](int i) {
                if (Ctx::COOP && S.kk_p[i + 1] - S.kk_p[i] > S.kk_long_thr) return;     // long columns: whole waves, below
                double az = 0.0;
                for (int e = S.Ap[i]; e < S.Ap[i + 1]; e++) az += Q.Ax[e] * Q.y[S.Ai[e]];
                for (int e = S.Gp[i]; e < S.Gp[i + 1]; e++) az += Q.Gx[e] * Q.z[S.Gi[e]];
                rx_row(i, az);
            });
            if (Ctx::COOP) {      // the columns of the globally coupled variables (hundreds to thousands of entries of A and G)
                pfor_coop(0, S.nkk_long, 64, [&](int q_, int gl, int G) {
                    const int i = S.kk_long[q_];
                    double a = 0.0;
                    if (i >= n) return a;
                    for (int e = S.Ap[i] + gl; e < S.Ap[i + 1]; e += G) a += Q.Ax[e] * Q.y[S.Ai[e]];
                    for (int e = S.Gp[i] + gl; e < S.Gp[i + 1]; e += G) a += Q.Gx[e] * Q.z[S.Gi[e]];
                    return a;
                }, [&](int q_, double sg) { const int i = S.kk_long[q_]; if (i < n) rx_row(i, sg); });
            }
            double nry = 0.0, yry = 0.0, nAx = 0.0, by = 0.0;
            pfor_nb(0, p, [&](int r) {
                double acc = 0.0;
                for (int t = S.Ar_p[r]; t < S.Ar_p[r + 1]; t++) acc += Q.Ax[S.Ar_pos[t]] * Q.x[S.Ar_j[t]];
                const double br = Q.b[r], res = acc - br;
                Q.ry[r] = res;
                nry += res * res; yry += Q.y[r] * res; nAx += acc * acc; by += br * Q.y[r];
            });
            double nrz = 0.0, zrz = 0.0, gap = 0.0, nGxs = 0.0, hz = 0.0;
            pfor_nb(0, m, [&](int r) {
                double acc = 0.0;
                for (int t = S.Gr_p[r]; t < S.Gr_p[r + 1]; t++) acc += Q.Gx[S.Gr_pos[t]] * Q.x[S.Gr_j[t]];
                const double sr = Q.s[r], zr = Q.z[r], hr = Q.h[r];
                const double res = acc + sr - hr;
                Q.rz[r] = res;
                nrz += res * res; zrz += zr * res; gap += sr * zr; nGxs += (acc + sr) * (acc + sr); hz += hr * zr;
            });
            xPx = cx.sum(xPx); cxv = cx.sum(cxv); nrx = cx.sum(nrx); naz = cx.sum(naz); nPx = cx.sum(nPx);
            nry = cx.sum(nry); yry = cx.sum(yry); nAx = cx.sum(nAx); by = cx.sum(by);
            nrz = cx.sum(nrz); zrz = cx.sum(zrz); gap = cx.sum(gap); nGxs = cx.sum(nGxs); hz = cx.sum(hz);
            const double pcost = 0.5 * xPx + cxv;
            const double dcost = pcost + yry + zrz - gap;
            const double pres = fmax(sqrt(nry) / nrm_b, sqrt(nrz) / nrm_h), dres = sqrt(nrx) / nrm_c;
            double relgap = 1e300;
            if (pcost < 0.0) relgap = gap / -pcost;
            else if (dcost > 0.0) relgap = gap / dcost;
            if (!done) {
                // stall exit (iteration limits above ECOS's default 100, e.g. the reference's maxit = 1000 for the Starship,
                // starship_flip/tests.jl:47, 96): an iterate that meets the REDUCED tolerances and has not improved its merit by 10 %
                // for 15 iterations stops as ALMOST_OPTIMAL instead of crawling to the limit at step lengths of 1e-3
                {
                    const double merit = fmax(fmax(pres, dres) / O.feastol, fmin(gap / (osc * O.abstol), relgap / O.reltol));
                    if (merit < 0.9 * best_merit) { best_merit = merit; best_it = it; }
                    //  only for iteration limits above ECOS's default -- ECOS itself has no such rule, so a default run
                    // (max_iter <= 100) keeps ECOS's exits -- and never in the iteration that passes the OPTIMAL test below
                    const bool opt_now = pres <= O.feastol && dres <= O.feastol && (gap <= osc * O.abstol || relgap <= O.reltol);
                    if (O.max_iter > 100 && !opt_now && it - best_it >= 15 && pres <= 1e-4 && dres <= 1e-4 && (gap / osc <= 5e-5 || relgap <= 5e-5)) {
                        R.iters = it; R.pcost = pcost / osc; R.dcost = dcost / osc; R.gap = gap / osc; R.pres = pres; R.dres = dres; R.relgap = relgap;
                        R.status = ST_ITERLIM; done = true;
                    }
                }
            }
            if (!done) {
                R.iters = it; R.pcost = pcost / osc; R.dcost = dcost / osc; R.gap = gap / osc; R.pres = pres; R.dres = dres; R.relgap = relgap;
                if (!(pres == pres) || !(dres == dres) || !(gap == gap)) { R.status = ST_NUMERR; done = true; }
                else if (pres <= O.feastol && dres <= O.feastol && (gap <= osc * O.abstol || relgap <= O.reltol)) { R.status = ST_OPTIMAL; done = true; }   // gap / osc: the gap of the original objective
                else {
                    // infeasibility certificates on the iterates normalised by the certificate's objective: a Farkas
                    // vector (y, z) with b'y + h'z = -1 and |A'y + G'z| <= feastol, or a ray x with c'x = -1,
                    // |Ax|, |Gx + s|, |Px| <= feastol (the iterates of an infeasible / unbounded program diverge along them)
                    const double bh = by + hz;
                    R.pinf = bh < 0.0 ? sqrt(naz) / -bh : 1e300;
                    R.dinf = cxv < 0.0 ? fmax(fmax(sqrt(nAx), sqrt(nGxs)), sqrt(nPx) / osc) / (-cxv / osc) : 1e300;
                    if (R.pinf <= O.feastol && it > 0) { R.status = ST_PINF; done = true; }
                    else if (R.dinf <= O.feastol && it > 0) { R.status = ST_DINF; done = true; }
                    else if (it == O.max_iter) done = true;
                }
            }
            freeze_counters();
            if (!cx.any(!done)) break;
            // ---- scaling + factorisation (finished problems run along; their state is frozen below) ----
            const long long ts_ = CPROF_T();
            const bool sok = nt_scaling(deg > 0 ? gap / (double)deg : 1.0);
            if (!sok && !done) { R.status = ST_NUMERR; done = true; CONIC_DBG("nt_scaling failed it=%d\n", it); }
            build_Gt();
            CPROF_ADD(4, ts_);
            // The scaled KKT matrix is quasi-definite: in exact arithmetic every pivot has its sign for ANY order.  A wrong-signed
            // pivot is round-off of the cancelling G~'G~ terms (1e12 late in a run) swamping the static regularisation; the dynamic
            // replacement by dyn_delta (ECOS) usually carries the run through, but it puts 1/dyn_delta into the factor and now and
            // then the following pivots overflow (NaN).  Only such a BROKEN factorisation is repeated with a 100x larger static
            // regularisation (kept for the rest of that problem's run; the refinement against the unregularised matrix absorbs it).
            // The same repair applies one step later: a factorisation that "succeeded" with dozens of dynamic regularisations can
            // still return a direction with non-finite entries.  That direction is recomputed ONCE MORE from a factorisation with
            // the larger static regularisation before the run is stopped at the current iterate (Starship N = 31 PTR program in
            // the nested order: OPTIMAL two iterations later instead of ALMOST_OPTIMAL at a gap of 3e-6).
            bool fk = true;
            double a = 1.0;
            // (a retry is decided for the whole group -- its workers share the barriers -- so a problem that does not need it repeats
            //  the same factorisation and solves bit for bit; the counters are those of the LAST attempt, not the sum)
            const int nreg0 = nreg, nrefine0 = nrefine;
            for (int dir_attempt = 0; dir_attempt < 2; dir_attempt++) {
            nrefine = nrefine0; lin_worst = 0.0;
            const int n_attempts = O.fine ? 7 : 3;
            for (int attempt = 0; attempt < n_attempts; attempt++) {
                nreg = nreg0;
                { const long long t0_ = CPROF_T(); fk = factor(); CPROF_ADD(0, t0_); }
                const bool bad = !done && !fk;
                if (!cx.any(bad) || attempt == n_attempts - 1) break;
                if (bad) { reg = fmin(reg * (O.fine ? 10.0 : 100.0), 1e-4); CONIC_DBG("static regularisation -> %.1e it=%d\n", reg, it); }
            }
            if (!fk && !done) { R.status = ST_NUMERR; done = true; CONIC_DBG("factor failed it=%d\n", it); }
            double ll = 0.0;
            pfor_nb(0, m, [&](int r) { ll += Q.lam[r] * Q.lam[r]; });
            ll = cx.sum(ll);
            const double mu = S.nexp > 0 ? gap / (double)deg : (deg > 0 ? ll / deg : 0.0);
            // ---- affine direction: d_s = -lam o lam ----
            jordan_sq_neg(Q.corr);
            newton();
            double a_aff = fmin(1.0, fmin(max_step(Q.s, Q.ds), max_step(Q.z, Q.dz)));
            if (m == 0) a_aff = 1.0;
            if (S.nexp > 0) {      // exponential cones: backtrack the affine step into the cones
                for (int k = 0; k < 60; k++) {
                    const bool in_s = interior_step(Q.s, Q.ds, a_aff), in_z = interior_step(Q.z, Q.dz, a_aff, true);   // (both hold barriers)
                    const bool inside = in_s && in_z;
                    if (!inside) a_aff *= 0.8;
                    if (!cx.any(!inside && !done)) break;
                }
            }
            double sigma = (1.0 - a_aff) * (1.0 - a_aff) * (1.0 - a_aff);
            if (S.nexp > 0) sigma = fmin(1.0, fmax(1e-4, sigma));
            // ---- combined direction: d_s = sigma mu e - lam o lam - (W^-1 ds_a) o (W dz_a) ----
            cx.barrier();
            apply_W(Q.ds, true);
            apply_W(Q.dz, false);
            pfor_nb(0, S.l, [&](int i) { Q.corr[i] = sigma * mu - Q.lam[i] * Q.lam[i] - Q.ds[i] * Q.dz[i]; });
            pfor(0, S.ncone, [&](int c) {
                const int o = S.cone_off[c], d = S.q[c];
                if (is_exp(c)) {      // q = s + sigma mu grad F*(z)
                    const long e = S.ncone + 9L * S.cexp[c];
                    for (int r = 0; r < 3; r++) Q.corr[o + r] = Q.s[o + r] + sigma * mu * Q.eta[e + 6 + r];
                    return;
                }
                double ll0 = 0.0, uv0 = 0.0;
                for (int r = 0; r < d; r++) { ll0 += Q.lam[o + r] * Q.lam[o + r]; uv0 += Q.ds[o + r] * Q.dz[o + r]; }
                const double l0 = Q.lam[o], u0 = Q.ds[o], v0 = Q.dz[o];
                for (int r = 1; r < d; r++) Q.corr[o + r] = -2.0 * l0 * Q.lam[o + r] - (u0 * Q.dz[o + r] + v0 * Q.ds[o + r]);
                Q.corr[o] = sigma * mu - ll0 - uv0;
            });
            newton();
            a = 1.0;
            if (m > 0) a = fmin(1.0, O.step * fmin(max_step(Q.s, Q.ds), max_step(Q.z, Q.dz)));
            if (S.nexp > 0) a = fmin(a, O.step);
            for (int k = 0; k < 80; k++) {   // stay strictly inside the cone despite round-off in max_step
                const bool in_s = interior_step(Q.s, Q.ds, a), in_z = interior_step(Q.z, Q.dz, a, true);   // (every worker calls both: they hold barriers)
                bool inside = in_s && in_z;
                if (S.nexp > 0) {
                    // fraction to the boundary of the exponential cones: the pairs must still be inside 10 % further along the step
                    // (the backtracking alone can stop a hair inside a cone and the following centring steps collapse)
                    const bool m_s = interior_step(Q.s, Q.ds, CONIC_EXP_MARGIN * a, false, true), m_z = interior_step(Q.z, Q.dz, CONIC_EXP_MARGIN * a, true, true);
                    inside = exp_neighbourhood(a, deg) && inside && m_s && m_z;
                }
                if (!inside) a *= 0.8;
                if (!cx.any(!inside && !done)) break;
            }
            CONIC_DBG("it %d gap %.3e pres %.2e dres %.2e mu %.2e sigma %.3f a_aff %.4f a %.4f nreg %d lin %.1e\n", it, gap, pres, dres, mu, sigma, a_aff, a, nreg, lin_worst);
            if (!(a > 0.0) && !done) { R.status = ST_NUMERR; done = true; CONIC_DBG("step failed it=%d\n", it); }
            // a direction with non-finite entries (a late, badly conditioned factorisation): stop at the CURRENT iterate
            // instead of destroying it -- it usually meets the reduced tolerances already (ALMOST_OPTIMAL, like ECOS)
            double mag = 0.0;
            pfor_nb(0, n + p, [&](int i) { mag += fabs(Q.sol[i]); });
            pfor_nb(0, m, [&](int r) { mag += fabs(Q.dz[r]) + fabs(Q.ds[r]); });
            mag = cx.sum(mag);
            // (every exit below is decided for the whole group: the workers of all its problems share the barriers)
            const bool wild = !done && !(mag <= 1e300);
            // (round 5) ... or a finite direction from a factorisation that the refinement could not repair: the residual
            // |rhs - K sol| / (1 + |rhs|) a refined solve is left with is <= 2e-9 on a healthy factorisation and >= 1e-6 on a broken one
            // (free-flyer GuSTO at a static regularisation of 1e-10: 4e8 at the iteration that threw the primal residual from 7e-13
            // back to 2e-3, after which the run ended ALMOST_OPTIMAL 0.7 % off; no pivot had the wrong sign, so neither the dynamic
            // regularisation nor the NaN test saw it).  Same repair: the direction is recomputed once with 100 x the regularisation.
            const bool sloppy = O.fine && !done && !wild && lin_worst > 1e-7 && dir_attempt == 0;
            if (dir_attempt == 1 || !cx.any((wild || sloppy) && reg < 1e-4)) {
                if (wild) { R.status = ST_NUMERR; done = true; CONIC_DBG("non-finite direction it=%d\n", it); }
                break;
            }
            if (wild || sloppy) { reg = fmin(reg * 100.0, 1e-4); CONIC_DBG("%s direction (linear residual %.1e): static regularisation -> %.1e it=%d\n", wild ? "non-finite" : "inaccurate", lin_worst, reg, it); }
            cx.barrier();
            }   // dir_attempt
            cx.barrier();
            if (!done) {
                pfor_nb(0, n, [&](int i) { Q.x[i] += a * Q.sol[i]; });
                pfor_nb(0, p, [&](int r) { Q.y[r] += a * Q.sol[n + r]; });
                pfor_nb(0, m, [&](int r) { Q.z[r] += a * Q.dz[r]; Q.s[r] += a * Q.ds[r]; });
            }
            freeze_counters();
            cx.barrier();
        }
        if (!counted) { nreg_out = nreg; nrefine_out = nrefine; }
        if (R.status == ST_ITERLIM || R.status == ST_NUMERR) {
            // ECOS's reduced tolerances (feastol_inacc 1e-4, abstol_inacc = reltol_inacc = 5e-5): what the reference receives as
            // ALMOST_OPTIMAL from JuMP and treats as a safe solution (scp.jl:965-980)
            if (R.pres <= 1e-4 && R.dres <= 1e-4 && (R.gap <= 5e-5 || R.relgap <= 5e-5) && R.pres == R.pres) R.status = ST_ALMOST;
            // a diverging run that stalled short of the certificate tolerance: reduced-accuracy certificates, like the
            // reduced-accuracy optimality test above (ECOS reports such exits as (in)feasibility "close to" tolerance)
            else if (R.status == ST_ITERLIM && R.dinf <= 1e-5) R.status = ST_DINF;
            else if (R.status == ST_ITERLIM && R.pinf <= 1e-5) R.status = ST_PINF;
        }
        if (osc != 1.0 && live) {     // multipliers of the ORIGINAL objective
            const double back = 1.0 / osc;
            pfor_nb(0, p, [&](int r) { Q.y[r] *= back; });
            pfor_nb(0, m, [&](int r) { Q.z[r] *= back; });
        }
        cx.barrier();
        R.nreg = (int)cx.sum((double)nreg_out); R.nrefine = nrefine_out;
        return R;
    }
};

}  // namespace conic
}  // namespace scp
