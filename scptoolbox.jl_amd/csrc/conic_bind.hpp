// Host-side glue between the symbolic analysis (conic_symbolic.hpp) and the solver body (conic_ipm.hpp), written ONCE for the
// device engine (conic_api.hip) and for the host twin of the tests (oracle/conic_host.cpp): the table of the per-problem work
// arrays, the binding of a Symbolic to a Sched, and the solver options of the C ABI (include/scp_conic.h).
#pragma once
#include <vector>

#include "../../include/scp_conic.h"
#include "conic_ipm.hpp"
#include "conic_symbolic.hpp"

namespace scp {
namespace conic {

// The work arrays of one problem (scaled G, the factor L / U = L D, right-hand sides, ...) in the order they lie in the work
// buffer, each with its length: THE list -- the buffer's size and every carve of it come from here.  P: Prob, or a struct with
// the same field names; take(len) hands out the next array.
template <class P, class Take>
void carve_work(const Sched& D, P& Q, Take&& take)
{
    Q.Gt = take(D.nnzGt); Q.Lx = take(D.nnzL); Q.Ux = take(D.nnzL); Q.Dinv = take(D.nk);
    Q.rhs = take(D.nk); Q.sol = take(D.nk); Q.res = take(D.nk); Q.cor = take(D.nk); Q.tmp = take(D.nk);
    Q.part = take(D.max_chunks);
    Q.lam = take(D.m); Q.wsc = take(D.m); Q.ds = take(D.m); Q.dz = take(D.m); Q.corr = take(D.m); Q.rz = take(D.m);
    Q.eta = take(D.ncone + 9L * D.nexp); Q.rx = take(D.n); Q.ry = take(D.p);
}
// doubles of work buffer per problem: the carve itself, counting
inline long work_len(const Sched& D)
{
    long total = 0;
    Prob Q;
    carve_work(D, Q, [&](long len) { total += len; return BV{nullptr, 0}; });
    return total;
}

inline Csc make_csc(int nrow, int ncol, const int* p, const int* i)
{
    Csc M;
    M.nrow = nrow; M.ncol = ncol;
    if (p == nullptr) { M.p.assign(ncol + 1, 0); return M; }
    M.p.assign(p, p + ncol + 1);
    const int nnz = M.p[ncol] > 0 ? M.p[ncol] : 0;
    if (nnz > 0 && i != nullptr) M.i.assign(i, i + nnz);
    return M;
}

// q[c] > 0: second-order cone of that dimension; q[c] = -3: exponential cone (include/scp_conic.h).  For the symbolic
// analysis (`q`) an exponential cone is a dense 3-row block like a second-order cone of dimension 3.
struct ConeKinds {
    std::vector<int> q, ctype, cexp;   // Sched::ctype / cexp
    int nexp = 0;
    explicit ConeKinds(const std::vector<int>& q_in) : q(q_in), ctype(q_in.size(), 0), cexp(q_in.size(), -1)
    {
        for (size_t c = 0; c < q.size(); c++) if (q[c] == -3) { q[c] = 3; ctype[c] = 1; cexp[c] = nexp++; }
    }
};

// what a Sched points to that a Symbolic does not hold in that form; alive while `place` of bind_schedule needs its vectors
struct SchedAux {
    CsrView Gr;
    std::vector<int2_> pairs;
    std::vector<long long> pair_p, echunk_q0, echunk_q1;
    explicit SchedAux(const Symbolic& S)
        : Gr(csr_view(S.G)), pairs(S.pair_a.size()), pair_p(S.pair_p.begin(), S.pair_p.end()),
          echunk_q0(S.echunk_q0.begin(), S.echunk_q0.end()), echunk_q1(S.echunk_q1.begin(), S.echunk_q1.end())
    {
        for (size_t i = 0; i < pairs.size(); i++) { pairs[i].a = S.pair_a[i]; pairs[i].b = S.pair_b[i]; }
    }
};

// Every field of a Sched from its Symbolic.  place(const std::vector<T>&) -> const T*: where the solver will read that vector
// (the device: an uploaded copy; the host twin: the vector itself).
template <class Place>
void bind_schedule(const Symbolic& S, const ConeKinds& K, const SchedAux& X, Sched& D, Place&& place)
{
    D.n = S.n; D.p = S.p; D.m = S.m; D.l = S.l; D.nk = S.nk; D.ncone = (int)S.q.size(); D.nexp = K.nexp;
    D.nnzG = S.G.nnz(); D.nnzGt = S.Gt.nnz(); D.nnzA = S.A.nnz(); D.nnzP = S.P.nnz(); D.nnzL = S.Lp[S.nk];
    D.njob = (int)S.job_gt0.size(); D.nlp = (int)S.lp_gt.size();
    D.nlev = (int)S.lev_p.size() - 1; D.nrlev = (int)S.rlev_p.size() - 1;
    D.nkk_long = (int)S.kk_long.size(); D.kk_long_thr = Symbolic::KK_LONG; D.max_chunks = S.max_chunks;
    // the program's pattern
    D.q = place(S.q); D.cone_off = place(S.cone_off); D.ctype = place(K.ctype); D.cexp = place(K.cexp);
    D.Gp = place(S.G.p); D.Gi = place(S.G.i); D.Gr_p = place(X.Gr.p); D.Gr_j = place(X.Gr.j); D.Gr_pos = place(X.Gr.pos);
    D.Gtp = place(S.Gt.p); D.Gti = place(S.Gt.i); D.Gtr_p = place(S.Gtr.p); D.Gtr_j = place(S.Gtr.j); D.Gtr_pos = place(S.Gtr.pos);
    D.Ap = place(S.A.p); D.Ai = place(S.A.i); D.Ar_p = place(S.Ar.p); D.Ar_j = place(S.Ar.j); D.Ar_pos = place(S.Ar.pos);
    D.Pf_p = place(S.Pfull.p); D.Pf_j = place(S.Pfull.j); D.Pf_pos = place(S.Pfull.pos);
    D.kk_p = place(S.kk_p); D.kk_src = place(S.kk_src); D.kk_idx = place(S.kk_idx); D.kk_col = place(S.kk_col);
    D.kk_long = place(S.kk_long);
    D.job_gt0 = place(S.job_gt0); D.job_cone = place(S.job_cone); D.job_src_p = place(S.job_src_p);
    D.job_src_row = place(S.job_src_row); D.job_src_g = place(S.job_src_g); D.lp_gt = place(S.lp_gt); D.lp_g = place(S.lp_g);
    // the factorisation (everything that depends on the ordering)
    D.perm = place(S.perm);
    D.Lp = place(S.Lp); D.Li = place(S.Li); D.l_src = place(S.l_src); D.l_src_idx = place(S.l_src_idx);
    D.d_src = place(S.d_src); D.d_src_idx = place(S.d_src_idx); D.d_kind = place(S.d_kind);
    D.pair_p = place(X.pair_p); D.pairs = place(X.pairs);
    D.row_p = place(S.row_p); D.row_k = place(S.row_k); D.row_pos = place(S.row_pos);
    D.lev_p = place(S.lev_p); D.lev_cols = place(S.lev_cols); D.lev_ent_p = place(S.lev_ent_p); D.lev_ent = place(S.lev_ent);
    D.ent_col = place(S.ent_col); D.rlev_p = place(S.rlev_p); D.rlev_cols = place(S.rlev_cols);
    D.lev_nshort = place(S.lev_nshort); D.rchunk_p = place(S.rchunk_p); D.rchunk_r0 = place(S.rchunk_r0); D.rchunk_r1 = place(S.rchunk_r1);
    D.col_c0 = place(S.col_c0); D.col_c1 = place(S.col_c1);
    D.lev_ent_nshort = place(S.lev_ent_nshort); D.echunk_p = place(S.echunk_p); D.ent_c0 = place(S.ent_c0); D.ent_c1 = place(S.ent_c1);
    D.echunk_q0 = place(X.echunk_q0); D.echunk_q1 = place(X.echunk_q1);
}

// solver options of the C ABI <-> Opts (NULL: the defaults)
inline Opts opts_from_abi(const scp_conic_opts* a)
{
    Opts o = default_opts();
    if (a) {
        o.max_iter = a->max_iter; o.feastol = a->feastol; o.abstol = a->abstol; o.reltol = a->reltol; o.reg = a->reg;
        o.dyn_eps = a->dyn_eps; o.dyn_delta = a->dyn_delta; o.nref = a->nref; o.ref_tol = a->ref_tol; o.step = a->step;
    }
    return o;
}
inline void opts_to_abi(const Opts& o, scp_conic_opts* a)
{
    a->max_iter = o.max_iter; a->feastol = o.feastol; a->abstol = o.abstol; a->reltol = o.reltol; a->reg = o.reg;
    a->dyn_eps = o.dyn_eps; a->dyn_delta = o.dyn_delta; a->nref = o.nref; a->ref_tol = o.ref_tol; a->step = o.step;
}
// a negative (or NaN) reg leaves the static regularisation to the solver: auto_reg of the pattern, and with 1e-10 the
// safety nets of Opts::fine
inline Opts resolve_auto_reg(Opts o, const Symbolic& S, int nexp)
{
    o.fine = 0;
    if (!(o.reg >= 0.0)) { o.reg = auto_reg(S.n_free, S.n, S.m, S.q.empty() && S.P.i.empty(), nexp > 0); o.fine = o.reg < 1e-9; }
    return o;
}

}  // namespace conic
}  // namespace scp
