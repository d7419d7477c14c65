// TEST INFRASTRUCTURE (not product code): host build of the PRODUCT's generic conic solver sources
// (scptoolbox.jl_amd/csrc/conic_symbolic.hpp + conic_ipm.hpp), so that the numerics of the solver body -- which is
// plain `__host__ __device__` C++ -- can be checked on a machine without a GPU against the independent restatement
// oracle/ipm.py (tests/test_conic_cpu.py), and timed as the CPU leg of the generic path.  The product never loads this
// library: scptoolbox.jl_amd/conic.py binds libscp_mi355x.so only and fails without it.
//
// Same memory layout as on the device: every per-problem array interleaved across the batch.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../scptoolbox.jl_amd/csrc/conic_bind.hpp"

using namespace scp::conic;

// Multi-worker emulation of the device context (CONIC_HOST_WORKERS=n): n host threads play the worker waves of one
// problem, with a real barrier and shared reduction slots -- a missing barrier in the solver body shows up as a data
// race (wrong / irreproducible results) on the CPU, without a GPU.
struct ThreadShared {
    int nw;
    std::atomic<int> count{0};
    std::atomic<int> sense{0};
    std::vector<double> red;
    explicit ThreadShared(int n) : nw(n), red(n) {}
};
// Single worker that sums every item in the ORDER the device does when a workgroup owns one problem (CONIC_HOST_COOP=<workers of the
// device group, 1024>): groups of G lanes with strided terms and a butterfly of partial sums (conic_ipm.hpp, Solver::pfor_coop).
struct SerialCoopCtx {
    static constexpr bool COOP = true;
    static constexpr bool COOP_EMU = true;
    int vw = 1024;
    int coop_workers() const { return vw; }
    double gsum(double v, int) const { return v; }
    int wid() const { return 0; }
    int nw() const { return 1; }
    void barrier() const {}
    double sum(double v) const { return v; }
    double min(double v) const { return v; }
    bool any(bool v) const { return v; }
};

struct ThreadCtx {
    static constexpr bool COOP = false;
    static constexpr bool COOP_EMU = false;
    int coop_workers() const { return 1; }
    double gsum(double v, int) const { return v; }
    ThreadShared* sh;
    int w;
    mutable int local_sense = 0;
    int wid() const { return w; }
    int nw() const { return sh->nw; }
    void barrier() const
    {
        local_sense ^= 1;
        if (sh->count.fetch_add(1) == sh->nw - 1) { sh->count.store(0); sh->sense.store(local_sense); }
        else while (sh->sense.load() != local_sense) std::this_thread::yield();
    }
    double sum(double v) const
    {
        sh->red[w] = v; barrier();
        double acc = 0.0;
        for (int i = 0; i < sh->nw; i++) acc += sh->red[i];
        barrier();
        return acc;
    }
    double min(double v) const
    {
        sh->red[w] = v; barrier();
        double acc = sh->red[0];
        for (int i = 1; i < sh->nw; i++) acc = std::fmin(acc, sh->red[i]);
        barrier();
        return acc;
    }
    bool any(bool v) const { const double r = sum(v ? 1.0 : 0.0); return r > 0.0; }
};

static int env_int(const char* name, int unset)
{
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : unset;
}

// The schedule of a pattern under CONIC_HOST_ORDER = seq (default) | nd | best.  "nd" / "best": what Engine::create does
// (analyse_auto: the cheapest dissection; "best" may also keep the sequential order); a caller's perm goes before either.
static Symbolic host_analyse(int n, int p, int m, int l, const std::vector<int>& q, const int* Pp, const int* Pi, const int* Ap,
                             const int* Ai, const int* Gp, const int* Gi, const int* perm)
{
    const char* om = std::getenv("CONIC_HOST_ORDER");
    const std::string order = om ? om : "seq";
    const Csc P = make_csc(n, n, Pp, Pi), A = make_csc(p, n, Ap, Ai), G = make_csc(m, n, Gp, Gi);
    if (perm == nullptr && (order == "nd" || order == "best"))
        return analyse_auto(n, p, m, l, q, P, A, G, env_int("CONIC_HOST_WORKERS", 256), order == "best");
    return analyse(n, p, m, l, q, P, A, G, perm);      // sequential minimum degree, or the caller's order
}

// Work profile of a schedule, per elimination level: [columns, row entries (pivot sums = forward substitution terms), longest
// row, L entries, operand pairs, longest pair list] -- what tools/order_survey.py prices the level-scheduled kernel's critical
// path with (a worker owns a whole row / a whole pair list), then the same with the long items cut into chunks:
// [6] critical path of the level's pivot / forward phase (longest short row, or longest chunk + chunks of a row), [7] the same
// for its entry phase.  prof[nlev][8]; returns nlev (prof may be NULL).
extern "C" int conic_host_schedule_profile(int n, int p, int m, int l, int ncones, const int* q, const int* Pp, const int* Pi,
                                           const int* Ap, const int* Ai, const int* Gp, const int* Gi, long long* prof, int cap)
{
    Symbolic S;
    try {
        S = host_analyse(n, p, m, l, std::vector<int>(q, q + ncones), Pp, Pi, Ap, Ai, Gp, Gi, nullptr);
    } catch (const std::exception&) {
        return -1;
    }
    const int nlev = (int)S.lev_p.size() - 1;
    if (!prof) return nlev;
    for (int lv = 0; lv < nlev && lv < cap; lv++) {
        long long* o = prof + 8LL * lv;
        o[0] = S.lev_p[lv + 1] - S.lev_p[lv]; o[1] = o[2] = 0;
        for (int t = S.lev_p[lv]; t < S.lev_p[lv + 1]; t++) {
            const int j = S.lev_cols[t];
            const long long len = S.row_p[j + 1] - S.row_p[j];
            o[1] += len; o[2] = std::max(o[2], len);
        }
        o[3] = S.lev_ent_p[lv + 1] - S.lev_ent_p[lv]; o[4] = o[5] = 0;
        for (int t = S.lev_ent_p[lv]; t < S.lev_ent_p[lv + 1]; t++) {
            const int e = S.lev_ent[t];
            const long long len = S.pair_p[e + 1] - S.pair_p[e];
            o[4] += len; o[5] = std::max(o[5], len);
        }
        o[6] = o[7] = 0;
        for (int t = S.lev_p[lv]; t < S.lev_p[lv + 1]; t++) {
            const int j = S.lev_cols[t];
            if (t < S.lev_p[lv] + S.lev_nshort[lv]) { o[6] = std::max<long long>(o[6], S.row_p[j + 1] - S.row_p[j]); continue; }
            long long mc = 0;
            for (int c = S.col_c0[t]; c < S.col_c1[t]; c++) mc = std::max<long long>(mc, S.rchunk_r1[c] - S.rchunk_r0[c]);
            o[6] = std::max<long long>(o[6], mc + (S.col_c1[t] - S.col_c0[t]));
        }
        for (int t = S.lev_ent_p[lv]; t < S.lev_ent_p[lv + 1]; t++) {
            const int e = S.lev_ent[t];
            if (t < S.lev_ent_p[lv] + S.lev_ent_nshort[lv]) { o[7] = std::max<long long>(o[7], S.pair_p[e + 1] - S.pair_p[e]); continue; }
            long long mc = 0;
            for (int c = S.ent_c0[t]; c < S.ent_c1[t]; c++) mc = std::max<long long>(mc, S.echunk_q1[c] - S.echunk_q0[c]);
            o[7] = std::max<long long>(o[7], mc + (S.ent_c1[t] - S.ent_c0[t]));
        }
    }
    return nlev;
}

extern "C" int conic_host_solve(int n, int p, int m, int l, int ncones, const int* q, const int* Pp, const int* Pi,
                                const int* Ap, const int* Ai, const int* Gp, const int* Gi, const int* perm, int B,
                                const double* c, const double* b, const double* hvec, const double* Gx, const double* Ax,
                                const double* Px, unsigned shared_mask, const scp_conic_opts* opts, double* x, double* y,
                                double* z, double* s, int32_t* status, int32_t* iters, double* info, long long* stats)
{
    ConeKinds K{std::vector<int>()};
    Symbolic S;
    try {
        K = ConeKinds(std::vector<int>(q, q + ncones));
        S = host_analyse(n, p, m, l, K.q, Pp, Pi, Ap, Ai, Gp, Gi, perm);
    } catch (const std::exception&) {
        return 1;
    }
    const SchedAux aux(S);
    Sched D;
    bind_schedule(S, K, aux, D, [](const auto& v) { return v.data(); });      // the solver reads the vectors where they are
    if (stats) { stats[0] = D.nnzL; stats[1] = S.flops; stats[2] = D.nk; stats[3] = D.nnzGt; stats[4] = S.nd_depth; stats[5] = D.nlev; stats[6] = D.nrlev;
        long mx = 0; for (int j = 0; j < S.nk; j++) mx = std::max<long>(mx, S.row_p[j + 1] - S.row_p[j]);
        stats[7] = mx; }
    if (std::getenv("CONIC_HOST_PERM_HASH")) {      // (test aid: the elimination order as one number, to compare two builds of the ordering code)
        unsigned long long hsh = 1469598103934665603ULL;
        for (int v : S.perm) { hsh ^= (unsigned long long)(unsigned)v; hsh *= 1099511628211ULL; }
        std::fprintf(stderr, "CONIC_HOST_PERM_HASH %016llx nk %d nnzL %d\n", hsh, S.nk, (int)S.Li.size());
    }
    if (B <= 0) return 0;

    const Opts o = resolve_auto_reg(opts_from_abi(opts), S, K.nexp);
    const long BS = B;
    // inputs: [len, B] column-major -> interleaved [len][BS]
    auto interleave = [&](const double* src, long len, bool shared) {
        std::vector<double> v((size_t)std::max<long>(len, 1) * (shared ? 1 : BS), 0.0);
        if (len == 0) return v;
        if (shared) { std::memcpy(v.data(), src, sizeof(double) * len); return v; }
        for (long t = 0; t < B; t++) for (long e = 0; e < len; e++) v[e * BS + t] = src[t * len + e];
        return v;
    };
    std::vector<double> ci = interleave(c, n, shared_mask & SCP_CONIC_SHARED_C), bi = interleave(b, p, shared_mask & SCP_CONIC_SHARED_B),
                        hi = interleave(hvec, m, shared_mask & SCP_CONIC_SHARED_H), Gi_ = interleave(Gx, D.nnzG, shared_mask & SCP_CONIC_SHARED_G),
                        Ai_ = interleave(Ax, D.nnzA, shared_mask & SCP_CONIC_SHARED_A), Pi_ = interleave(Px, D.nnzP, shared_mask & SCP_CONIC_SHARED_P);
    std::vector<double> work((size_t)work_len(D) * BS, 0.0), xs((size_t)std::max(n, 1) * BS), ys((size_t)std::max(p, 1) * BS),
        zs((size_t)std::max(m, 1) * BS), ss((size_t)std::max(m, 1) * BS);
    const int workers = env_int("CONIC_HOST_WORKERS", 1);
#pragma omp parallel for schedule(dynamic) if (workers <= 1)
    for (int t = 0; t < B; t++) {
        Prob Q;
        auto cb = [&](std::vector<double>& v, bool shared) { return shared ? CBV{v.data(), 1} : CBV{v.data() + t, BS}; };
        Q.c = cb(ci, shared_mask & SCP_CONIC_SHARED_C); Q.b = cb(bi, shared_mask & SCP_CONIC_SHARED_B);
        Q.h = cb(hi, shared_mask & SCP_CONIC_SHARED_H); Q.Gx = cb(Gi_, shared_mask & SCP_CONIC_SHARED_G);
        Q.Ax = cb(Ai_, shared_mask & SCP_CONIC_SHARED_A); Q.Px = cb(Pi_, shared_mask & SCP_CONIC_SHARED_P);
        Q.x = BV{xs.data() + t, BS}; Q.y = BV{ys.data() + t, BS}; Q.z = BV{zs.data() + t, BS}; Q.s = BV{ss.data() + t, BS};
        double* w = work.data();
        carve_work(D, Q, [&](long len) { BV v{w + t, BS}; w += len * BS; return v; });
        Result R;
        const int coop = env_int("CONIC_HOST_COOP", 0);
        if (workers <= 1 && coop > 1) {
            SerialCoopCtx cx; cx.vw = coop;
            Solver<SerialCoopCtx> sv(D, Q, o, cx);
            R = sv.run();
        } else if (workers <= 1) {
            SerialCtx cx;
            Solver<SerialCtx> sv(D, Q, o, cx);
            R = sv.run();
        } else {
            ThreadShared sh(workers);
            std::vector<std::thread> th;
            std::vector<Result> rs(workers);
            for (int w = 0; w < workers; w++)
                th.emplace_back([&, w]() {
                    ThreadCtx cx; cx.sh = &sh; cx.w = w;
                    Solver<ThreadCtx> sv(D, Q, o, cx);
                    rs[w] = sv.run();
                });
            for (auto& t_ : th) t_.join();
            R = rs[0];
            for (int w = 1; w < workers; w++)
                if (rs[w].status != R.status || rs[w].iters != R.iters || rs[w].pcost != R.pcost) R.status = 99;   // workers disagree
        }
        if (status) status[t] = R.status;
        if (iters) iters[t] = R.iters;
        if (info) {
            double* io = info + 8L * t;
            io[0] = R.pcost; io[1] = R.dcost; io[2] = R.gap; io[3] = R.pres; io[4] = R.dres; io[5] = R.relgap;
            io[6] = R.nreg; io[7] = R.nrefine;
        }
        if (x) for (long e = 0; e < n; e++) x[(long)t * n + e] = xs[e * BS + t];
        if (y) for (long e = 0; e < p; e++) y[(long)t * p + e] = ys[e * BS + t];
        if (z) for (long e = 0; e < m; e++) z[(long)t * m + e] = zs[e * BS + t];
        if (s) for (long e = 0; e < m; e++) s[(long)t * m + e] = ss[e * BS + t];
    }
    return 0;
}
