// Closed-loop covariance audit (scp_audit_covariance_*, include/scp_mi355x.h): the linear covariance analysis of a solution under
// the sample-and-hold gains K_k of lqr_kernel.hpp (or any others).  Per problem
//     Sigma_1 = diag(sig0^2);  for k = 1 .. N-1:  Phi = A_k, Gam = B-_k + B+_k, A_cl = Phi - Gam K_k,
//     Sigma_{k+1} = A_cl Sigma_k A_cl' + Gam diag(sigu^2) Gam' + diag(sigw^2),  then Sigma <- (Sigma + Sigma') / 2
// and at every node the 1-sigma of the states, of the feedback effort, of the terminal conditions, and the distance of every
// constraint row from its boundary in sigmas.  Two launches:
//
// Row pre-pass (cov_rows_kernel<M>), node-parallel, one thread per (problem, node): the three sampled row families of
// audit_sample (audit_kernel.hpp) at the nominal node, as value v and gradient g = g_x - g_u K_k over the state alone (the hold
// update makes dz = [I; -K_k] dx; g = g_x at node N), into the row table rows[nx+1, nrow, N, B] in family order (s, linear, cone);
// H = d g_tc / dx at node N into Hf[ntc, nx, B].  Like the audits it reads its local arrays with compile-time indices only.
//
// Covariance chain (cov_chain_kernel<NX, NU>), the forward twin of Lqr<NX, NU>::chain: one wavefront LANE per ENTRY of Sigma,
// floor(64 / nx^2) problems per wavefront, a node is a sequence of PHASES separated by barriers, the work area in LDS, and ONE body
// for the device and the pure-host twin through each(f).  No phase reads an array it writes.  What a lane computes depends on its
// problem's data and its entry index only, and every fold runs in a fixed order: a problem's result is independent of B and of its
// place in the batch bit for bit.  Row r of the table belongs to entry r mod nx^2.  No model enters the chain.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/scp_mi355x.h"
#include "audit_kernel.hpp"
#include "models/model_common.hpp"

namespace scp {

struct CovArgs {
    int B, N;
    int nrow[3];         // rows per family: s, linear, cone (their sum is the row count of the table)
    int ntc;
    double nsig;
    const double* xd;    // [nx,N,B]       (pre-pass)
    const double* ud;    // [nu,N,B]       (pre-pass)
    const double* p;     // [np,B]         (pre-pass)
    const double* pp;    // [npp,B]        (pre-pass)
    const double* A;     // [nx,nx,N-1,B]
    const double* Bm;    // [nx,nu,N-1,B]
    const double* Bp;    // [nx,nu,N-1,B]
    const double* K;     // [nu,nx,N-1,B]
    const double* Sx;    // [nx]
    const double* Su;    // [nu]
    const double* sig0;  // [nx]
    const double* sigu;  // [nu]
    const double* sigw;  // [nx]
    const int* mask;     // optional [B]: problems with mask[b] == 0 are skipped, everything of theirs is NaN
    double* rows;        // [nx+1,nrow,N,B]: g[nx] then v
    double* Hf;          // [ntc,nx,B]
    double* summary;     // [SCP_COV_WIDTH,B]
    double* sig;         // optional [nx,N,B]
    double* nodes;       // optional [SCP_COV_NODE_WIDTH,N,B]
};

// cov_api.hip: cov_rows_kernel<M> then cov_chain_kernel<nx, nu> on `stream` (SCP_ERR_UNSUPPORTED for models with node parameters)
int cov_launch(int model_id, const double* model_par, const CovArgs& a, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// The rows of ONE node k (1-based) of ONE problem: xd[nx,N], ud[nu,N], p[np], pp[npp], Kg[nu,nx,N-1] -> rows_k[nx+1,nrow] and, at
// k = N, Hf[ntc,nx].  The model functions get (t, k) = (LinRange(0,1,N)[k], k): what the single-shooting audit passes at the
// sample that coincides with the node.
// ------------------------------------------------------------------------------------------------
template <class M>
SCP_DEV void cov_rows_one(const typename M::Params& par, int N, int k, const double* xd, const double* ud, const double* pb,
                          const double* pp, const double* Kg, double* rows_k, double* Hf)
{
    static_assert(M::np_node == 0, "a row of node k would read that node's own parameters");
    constexpr int nx = M::nx, nu = M::nu, nz = nx + nu, np = M::np, npa = np > 0 ? np : 1, nw = nx + 1;
    constexpr int ns = M::ns, nsa = ns > 0 ? ns : 1, nl = M::nl, nla = nl > 0 ? nl : 1, nsoc = M::nsoc, nsoca = nsoc > 0 ? nsoc : 1;
    constexpr int ntc = M::ntc, ntca = ntc > 0 ? ntc : 1;
    const double t = linrange(0.0, 1.0, N, k - 1);
    const bool hold = k < N;
    double x[nx], u[nu], z[nz], Kk[nu * nx];
#pragma unroll
    for (int i = 0; i < nx; i++) { x[i] = xd[(long)(k - 1) * nx + i]; z[i] = x[i]; }
#pragma unroll
    for (int i = 0; i < nu; i++) { u[i] = ud[(long)(k - 1) * nu + i]; z[nx + i] = u[i]; }
#pragma unroll
    for (int i = 0; i < nu * nx; i++) Kk[i] = hold ? Kg[(long)(k - 1) * nu * nx + i] : 0.0;
    // row r: the value and g = g_x - g_u K_k (g_x alone at node N: 0 * Inf must not enter there)
    auto emit = [&](int r, double v, const double* gx, const double* gu) {
        double* row = rows_k + (long)r * nw;
#pragma unroll
        for (int j = 0; j < nx; j++) {
            double g = gx[j];
            if (hold) {
#pragma unroll
                for (int a = 0; a < nu; a++) g -= gu[a] * Kk[a + nu * j];
            }
            row[j] = g;
        }
        row[nx] = v;
    };
    if constexpr (ns > 0) {
        double s[nsa], C[nsa * nx], Dm[nsa * nu], G[nsa * npa];
        M::s_eval(par, t, k, x, u, pb, s, C, Dm, G);
#pragma unroll
        for (int i = 0; i < ns; i++) emit(i, s[i], &C[i * nx], &Dm[i * nu]);
    }
    if constexpr (nl > 0) {
        double L[nla * nz], Lp[nla * npa], l[nla];
#pragma unroll
        for (int i = 0; i < nl * npa; i++) Lp[i] = 0.0;
        M::lin_rows(par, t, k, L, Lp, l);
#pragma unroll
        for (int i = 0; i < nl; i++) {
            double a = l[i];
#pragma unroll
            for (int j = 0; j < nz; j++) a += L[i * nz + j] * z[j];
#pragma unroll
            for (int j = 0; j < np; j++) a += Lp[i * npa + j] * pb[j];
            emit(ns + i, a, &L[i * nz], &L[i * nz + nx]);
        }
    }
    if constexpr (nsoc > 0) {
        double Mm[nsoca * 4 * nz], m[nsoca * 4];
        M::soc_rows(par, t, k, Mm, m);
#pragma unroll
        for (int c = 0; c < nsoc; c++) {
            double w[4], gz[nz];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double a = m[4 * c + r];
#pragma unroll
                for (int j = 0; j < nz; j++) a += Mm[(4 * c + r) * nz + j] * z[j];
                w[r] = a;
            }
            const double nrm = sqrt(w[1] * w[1] + w[2] * w[2] + w[3] * w[3]);
#pragma unroll
            for (int j = 0; j < nz; j++) {
                const double d = (w[1] * Mm[(4 * c + 1) * nz + j] + w[2] * Mm[(4 * c + 2) * nz + j] + w[3] * Mm[(4 * c + 3) * nz + j]) / nrm;
                gz[j] = (nrm == 0.0 ? 0.0 : d) - Mm[(4 * c) * nz + j];
            }
            emit(ns + nl + c, nrm - w[0], &gz[0], &gz[nx]);
        }
    }
    if constexpr (ntc > 0) {
        if (!hold) {
            double g[ntca], H[ntca * nx], Kt[ntca * npa];
            M::bc_tc(par, x, pb, pp, g, H, Kt);            // only H survives dead-code elimination
#pragma unroll
            for (int i = 0; i < ntc; i++)
#pragma unroll
                for (int j = 0; j < nx; j++) Hf[i + ntc * j] = H[i * nx + j];
        }
    }
}

// one thread per (problem, node), gid = b N + (k - 1), blocks of one wavefront: the mapping of audit_interval_kernel
template <class M>
__global__ __launch_bounds__(64) void cov_rows_kernel(CovArgs a, typename M::Params par)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long)a.B * a.N) return;
    const int b = (int)(gid / a.N), k = (int)(gid % a.N) + 1;
    if (a.mask != nullptr && a.mask[b] == 0) return;       // the chain writes the NaN of a skipped problem
    constexpr int nrow = M::ns + M::nl + M::nsoc;
    cov_rows_one<M>(par, a.N, k, a.xd + (long)b * a.N * M::nx, a.ud + (long)b * a.N * M::nu, a.p + (long)b * np_total<M>(a.N),
                    a.pp + (long)b * M::npp, a.K + (long)b * (a.N - 1) * M::nu * M::nx, a.rows + gid * nrow * (M::nx + 1),
                    a.Hf + (long)b * M::ntc * M::nx);
}

// ------------------------------------------------------------------------------------------------
// the chain
// ------------------------------------------------------------------------------------------------

// what one problem's chain reads besides the work area
struct CovIn {
    int N, nrow[3], ntc;
    double nsig;
    const double *A, *Bm, *Bp, *K;       // this problem's
    const double *rows, *Hf;             // this problem's
    const double *Sx, *Su, *sig0, *sigu, *sigw;
};

// the work area of ONE problem, column-major like the arrays of discretize!
template <int NX, int NU>
struct CovWork {
    double Sig[NX * NX], Phi[NX * NX], Acl[NX * NX], T[NX * NX], S[NX * NX];   // T = A_cl Sigma; S = the unsymmetrised new Sigma
    double Gam[NX * NU], Kk[NU * NX], Y[NU * NX];                              // Y = K_k Sigma
    double nm[3][NX * NX];      // per entry: the smallest margin of its rows at this node, per family
    double cnt[NX * NX];        // per entry: its (node, row) pairs with a margin below nsig so far
    double tau[NX * NX];        // per entry: the largest terminal 1-sigma of its rows of H
    double sd[NX], eff[NU];     // this node's sigma_i / Sx_i and e_a
    double rec[SCP_COV_WIDTH];  // the running summary record: every field has ONE writer (measure / fold / step)
    int bad;                    // set by any entry that met a non-finite value
};

template <int NX, int NU>
struct Cov {
    static constexpr int NP = NX * NX, NG = NX * NU;
    static_assert(NP <= 64 && NG <= NP && NU <= 4 && NP >= 3, "one lane per entry of Sigma carries every phase");
    using Work = CovWork<NX, NU>;

    SCP_DEV static void init(Work& w, int e, const CovIn& in)
    {
        if (e >= NP) return;
        w.Sig[e] = (e % NX == e / NX) ? in.sig0[e % NX] * in.sig0[e % NX] : 0.0;
        w.cnt[e] = 0.0;
        w.tau[e] = 0.0;
        if (e == 0) {
            w.bad = 0;
#pragma unroll
            for (int i = 0; i < SCP_COV_WIDTH; i++) w.rec[i] = (i == 1 || i == 4) ? -INFINITY : ((i == 6 || i == 8 || i == 10) ? INFINITY : 0.0);
        }
    }
    SCP_DEV static void load(Work& w, int e, const double* A, const double* Bm, const double* Bp, const double* K)
    {
        if (e < NP) w.Phi[e] = A[e];
        if (e < NG) { w.Gam[e] = Bm[e] + Bp[e]; w.Kk[e] = K[e]; }
    }
    // at node k, on Sigma_k: the diagonal lanes take sigma_i; Y = K_k Sigma; every entry takes the margins of its rows; A_cl
    SCP_DEV static void measure(Work& w, int e, const CovIn& in, bool last, const double* rows_k, double* sig_k)
    {
        bool bad = false;
        if (e < NP) {
            const int i = e % NX, j = e / NX;
            if (i == j) {
                const double v = w.Sig[e];
                bad = bad || !__builtin_isfinite(v);
                const double s = sqrt(v > 0.0 ? v : 0.0);
                if (sig_k != nullptr) sig_k[i] = s;
                w.sd[i] = s / in.Sx[i];
                bad = bad || !__builtin_isfinite(w.sd[i]);
            }
            if (!last) {
                double s = w.Phi[e];
#pragma unroll
                for (int a = 0; a < NU; a++) s -= w.Gam[i + NX * a] * w.Kk[a + NU * j];
                w.Acl[e] = s;
            }
            double m0 = INFINITY, m1 = INFINITY, m2 = INFINITY;
            const int n0 = in.nrow[0], n1 = n0 + in.nrow[1], n2 = n1 + in.nrow[2];
            for (int r = e; r < n2; r += NP) {
                const double* row = rows_k + (long)r * (NX + 1);
                double g[NX], var = 0.0;
#pragma unroll
                for (int c = 0; c < NX; c++) g[c] = row[c];
                const double v = row[NX];
                // one row of Sigma at a time, here and in `terminal` (g[c] re-read from the table, so that no index of g is dynamic):
                // with all nx^2 LDS reads in flight the chain needs up to 228 registers and runs slower
#pragma unroll 1
                for (int c = 0; c < NX; c++) {
                    double s = 0.0;
#pragma unroll
                    for (int d = 0; d < NX; d++) s += w.Sig[c + NX * d] * g[d];
                    var += row[c] * s;
                }
                bad = bad || !__builtin_isfinite(var) || !__builtin_isfinite(v);
                const double m = var > 0.0 ? -v / sqrt(var) : (v <= 0.0 ? INFINITY : -INFINITY);
                if (r < n0) m0 = m < m0 ? m : m0;
                else if (r < n1) m1 = m < m1 ? m : m1;
                else m2 = m < m2 ? m : m2;
                if (m < in.nsig) w.cnt[e] += 1.0;
            }
            w.nm[0][e] = m0; w.nm[1][e] = m1; w.nm[2][e] = m2;
        }
        if (e < NG && !last) {
            const int a = e % NU, j = e / NU;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.Kk[a + NU * m] * w.Sig[m + NX * j];
            w.Y[e] = s;
        }
        if (bad) w.bad = 1;
    }
    // the folds of node k (1-based) in a fixed order: entry 0 the states and the trace, the last three entries one family each,
    // the first nu entries e_a = sqrt((K Sigma K')_aa) / Su_a; and T = A_cl Sigma
    SCP_DEV static void fold(Work& w, int e, const CovIn& in, int k, bool last, double* node_k)
    {
        bool bad = false;
        if (e < NU && !last) {
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < NX; j++) q += w.Y[e + NU * j] * w.Kk[e + NU * j];
            const double v = sqrt(q > 0.0 ? q : 0.0) / in.Su[e];
            bad = bad || !__builtin_isfinite(q) || !__builtin_isfinite(v);
            w.eff[e] = v;
        }
        if (e == 0) {
            double m = -INFINITY, arg = 0.0, tr = 0.0;
#pragma unroll
            for (int i = 0; i < NX; i++) {
                if (w.sd[i] > m) { m = w.sd[i]; arg = (double)(i + 1); }
                tr += w.Sig[i + NX * i] / (in.Sx[i] * in.Sx[i]);
            }
            bad = bad || !__builtin_isfinite(tr);
            if (m > w.rec[1]) { w.rec[1] = m; w.rec[2] = (double)k; w.rec[3] = arg; }
            w.rec[13] = tr;
            if (node_k != nullptr) { node_k[0] = m; node_k[5] = tr; node_k[6] = 0.0; node_k[7] = 0.0; }
        }
        if (e >= NP - 3 && e < NP) {
            const int f = e - (NP - 3);
            double m = INFINITY;
            for (int i = 0; i < NP; i++) m = w.nm[f][i] < m ? w.nm[f][i] : m;
            if (m < w.rec[6 + 2 * f]) { w.rec[6 + 2 * f] = m; w.rec[7 + 2 * f] = (double)k; }
            if (node_k != nullptr) node_k[2 + f] = m;
        }
        if (e < NP && !last) {
            const int i = e % NX, j = e / NX;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.Acl[i + NX * m] * w.Sig[m + NX * j];
            w.T[e] = s;
        }
        if (bad) w.bad = 1;
    }
    // S = T A_cl' + Gam diag(sigu^2) Gam' + diag(sigw^2), the new Sigma before it is symmetrised; entry 0 folds the efforts
    SCP_DEV static void step(Work& w, int e, const CovIn& in, int k, double* node_k)
    {
        if (e < NP) {
            const int i = e % NX, j = e / NX;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) s += w.T[i + NX * m] * w.Acl[j + NX * m];
#pragma unroll
            for (int a = 0; a < NU; a++) s += w.Gam[i + NX * a] * (in.sigu[a] * in.sigu[a]) * w.Gam[j + NX * a];
            if (i == j) s += in.sigw[i] * in.sigw[i];
            w.S[e] = s;
        }
        if (e == 0) {
            double m = -INFINITY;
#pragma unroll
            for (int a = 0; a < NU; a++) m = w.eff[a] > m ? w.eff[a] : m;
            if (m > w.rec[4]) { w.rec[4] = m; w.rec[5] = (double)k; }
            if (node_k != nullptr) node_k[1] = m;
        }
    }
    SCP_DEV static void symmetrise(Work& w, int e)
    {
        if (e >= NP) return;
        const int i = e % NX, j = e / NX;
        const double v = 0.5 * (w.S[i + NX * j] + w.S[j + NX * i]);
        w.Sig[e] = v;
        if (!__builtin_isfinite(v)) w.bad = 1;
    }
    // at node N: tau_i = sqrt((H Sigma_N H')_ii), row i of H by entry i mod nx^2
    SCP_DEV static void terminal(Work& w, int e, const CovIn& in, double* node_k)
    {
        if (e >= NP) return;
        bool bad = false;
        for (int i = e; i < in.ntc; i += NP) {
            double q = 0.0;
#pragma unroll 1
            for (int c = 0; c < NX; c++) {
                double s = 0.0;
#pragma unroll
                for (int d = 0; d < NX; d++) s += w.Sig[c + NX * d] * in.Hf[i + in.ntc * d];
                q += in.Hf[i + in.ntc * c] * s;
            }
            bad = bad || !__builtin_isfinite(q);
            const double t = sqrt(q > 0.0 ? q : 0.0);
            if (t > w.tau[e]) w.tau[e] = t;
        }
        if (e == 0 && node_k != nullptr) node_k[1] = NAN;
        if (bad) w.bad = 1;
    }
    // entry 0 writes the summary record: the running fields, the largest tau and the count, both folded in entry order
    SCP_DEV static void finish(const Work& w, int e, double* summary)
    {
        if (e != 0) return;
        const bool bad = w.bad != 0;
        double tau = 0.0, cnt = 0.0;
        for (int i = 0; i < NP; i++) { tau = w.tau[i] > tau ? w.tau[i] : tau; cnt += w.cnt[i]; }
        summary[0] = bad ? 1.0 : 0.0;
#pragma unroll
        for (int i = 1; i < SCP_COV_WIDTH; i++) summary[i] = bad ? NAN : w.rec[i];
        if (!bad) { summary[12] = tau; summary[14] = cnt; summary[15] = 0.0; }
    }

    // ONE problem -> summary[SCP_COV_WIDTH], sig[nx,N] or nullptr, nodes[SCP_COV_NODE_WIDTH,N] or nullptr.  each(f) runs the phase
    // f(e) for every entry e and returns when all of them are done.
    template <class Each>
    SCP_DEV static void chain(Work& w, const CovIn& in, double* summary, double* sig, double* nodes, Each&& each)
    {
        const int N = in.N, nrow = in.nrow[0] + in.nrow[1] + in.nrow[2];
        each([&](int e) { init(w, e, in); });
        for (int k = 0; k < N; k++) {                     // 0-based node
            const bool last = k == N - 1;
            const double* rows_k = in.rows + (long)k * nrow * (NX + 1);
            double* sig_k = sig != nullptr ? sig + (long)k * NX : nullptr;
            double* node_k = nodes != nullptr ? nodes + (long)k * SCP_COV_NODE_WIDTH : nullptr;
            if (!last) {
                const double *Ak = in.A + (long)k * NP, *Bmk = in.Bm + (long)k * NG, *Bpk = in.Bp + (long)k * NG, *Kk = in.K + (long)k * NG;
                each([&](int e) { load(w, e, Ak, Bmk, Bpk, Kk); });
            }
            each([&](int e) { measure(w, e, in, last, rows_k, sig_k); });
            each([&](int e) { fold(w, e, in, k + 1, last, node_k); });
            if (last) {
                each([&](int e) { terminal(w, e, in, node_k); });
            } else {
                each([&](int e) { step(w, e, in, k + 1, node_k); });
                each([&](int e) { symmetrise(w, e); });
            }
        }
        each([&](int e) { finish(w, e, summary); });
    }
};

// blocks of one wavefront; lane = g * nx^2 + e: entry e of the block's g-th problem (lanes past the last packed problem idle
// but meet every barrier), the launch geometry of lqr_riccati_kernel
template <int NX, int NU>
__global__ __launch_bounds__(64) void cov_chain_kernel(CovArgs a)
{
    using C = Cov<NX, NU>;
    constexpr int NP = C::NP, NG = C::NG, PACK = 64 / NP;
    __shared__ CovWork<NX, NU> work[PACK];
    const int g = threadIdx.x / NP, e = threadIdx.x % NP;
    const long b = (long)blockIdx.x * PACK + g;
    const bool mine = g < PACK && b < a.B;
    const bool live = mine && (a.mask == nullptr || a.mask[b] != 0);
    const long bb = mine ? b : 0;
    const int N = a.N, nrow = a.nrow[0] + a.nrow[1] + a.nrow[2];
    CovIn in;
    in.N = N; in.nrow[0] = a.nrow[0]; in.nrow[1] = a.nrow[1]; in.nrow[2] = a.nrow[2]; in.ntc = a.ntc; in.nsig = a.nsig;
    in.A = a.A + bb * (N - 1) * NP; in.Bm = a.Bm + bb * (N - 1) * NG; in.Bp = a.Bp + bb * (N - 1) * NG; in.K = a.K + bb * (N - 1) * NG;
    in.rows = a.rows + bb * N * nrow * (NX + 1); in.Hf = a.Hf + bb * a.ntc * NX;
    in.Sx = a.Sx; in.Su = a.Su; in.sig0 = a.sig0; in.sigu = a.sigu; in.sigw = a.sigw;
    double* summary = a.summary + bb * SCP_COV_WIDTH;
    double* sig = a.sig != nullptr ? a.sig + bb * N * NX : nullptr;
    double* nodes = a.nodes != nullptr ? a.nodes + bb * N * SCP_COV_NODE_WIDTH : nullptr;
    C::chain(work[g < PACK ? g : 0], in, summary, sig, nodes, [&](auto f) {
        if (live) f(e);
        __syncthreads();
    });
    if (mine && !live) {
        for (int i = e; i < SCP_COV_WIDTH; i += NP) summary[i] = NAN;
        if (sig != nullptr)
            for (long i = e; i < (long)N * NX; i += NP) sig[i] = NAN;
        if (nodes != nullptr)
            for (long i = e; i < (long)N * SCP_COV_NODE_WIDTH; i += NP) nodes[i] = NAN;
    }
}

}  // namespace scp
