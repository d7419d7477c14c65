// Stand-alone sanitizer check of the host twin of the generic conic solver (oracle/conic_host.cpp): conic_host_solve on small
// hand-written programs whose optimal values are known in closed form, with every input and output array on the heap at EXACTLY
// its documented size.  The twin takes its work buffer from the same table of per-problem arrays as the device engine.  What this
// program can catch of a mistake in that table, before anything runs on a GPU: the work buffer is ONE allocation sized by the table, so
// AddressSanitizer reports a carve that runs past the total (in effect the last array) and any overrun of the input and output
// arrays; an array that is too short in the middle spills into its neighbour inside the allocation and shows only as a wrong
// status or cost.  On programs this small the "nd" pass ends with the level counts of the "seq" pass (printed below), so it
// adds the other entry of the order selection, not another schedule.  Not a pytest and not loaded into Python.  Built and run by
// `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS; host code only, no GPU is needed or used).
//
// Exit status 0 and "ok" when every problem ended OPTIMAL within 1e-7 of its closed-form cost (the bound
// tests/test_conic_geometry_gpu.py holds this solver to on the softplus family) and the runs with shared arrays gave the bits
// of the runs with one copy per problem.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/scp_conic.h"

extern "C" int conic_host_solve(int n, int p, int m, int l, int ncones, const int* q, const int* Pp, const int* Pi,
                                const int* Ap, const int* Ai, const int* Gp, const int* Gi, const int* perm, int B,
                                const double* c, const double* b, const double* hvec, const double* Gx, const double* Ax,
                                const double* Px, unsigned shared_mask, const scp_conic_opts* opts, double* x, double* y,
                                double* z, double* s, int32_t* status, int32_t* iters, double* info, long long* stats);

using Vec = std::vector<double>;
using Idx = std::vector<int>;

static int bad = 0;

// one pattern + the values of a batch; every value array [len, B] (batch last) unless its bit is set in `shared`
struct Program {
    const char* name;
    int n, p, m, l;
    Idx q, Ap, Ai, Gp, Gi;
    int B;
    unsigned shared;
    Vec c, b, h, Gx, Ax, cost;
};
struct Out {
    Vec x, y, z, s, info;
    std::vector<int32_t> status, iters;
};

static const int* ptr(const Idx& v) { return v.empty() ? nullptr : v.data(); }
static const double* ptr(const Vec& v) { return v.empty() ? nullptr : v.data(); }

static Out solve(const Program& P, const char* order)
{
    Out o;
    const size_t B = P.B;
    o.x.assign(P.n * B, NAN); o.y.assign(P.p * B, NAN); o.z.assign(P.m * B, NAN); o.s.assign(P.m * B, NAN);
    o.info.assign(8 * B, NAN); o.status.assign(B, -1); o.iters.assign(B, -1);
    std::vector<long long> stats(8, -1);
    const int rc = conic_host_solve(P.n, P.p, P.m, P.l, (int)P.q.size(), ptr(P.q), nullptr, nullptr, ptr(P.Ap), ptr(P.Ai), ptr(P.Gp),
                                    ptr(P.Gi), nullptr, P.B, ptr(P.c), ptr(P.b), ptr(P.h), ptr(P.Gx), ptr(P.Ax), nullptr, P.shared,
                                    nullptr, o.x.data(), o.y.data(), o.z.data(), o.s.data(), o.status.data(), o.iters.data(),
                                    o.info.data(), stats.data());
    if (rc != 0) { std::printf("%s (%s): conic_host_solve returned %d\n", P.name, order, rc); bad++; return o; }
    double worst = 0.0;
    int itmax = 0;
    for (int t = 0; t < P.B; t++) {
        if (o.status[t] != SCP_CONIC_OPTIMAL) { std::printf("%s (%s): problem %d ended with status %d\n", P.name, order, t, o.status[t]); bad++; }
        const double err = std::fabs(o.info[8 * t] - P.cost[t]);
        if (!(err <= 1e-7)) { std::printf("%s (%s): problem %d cost %.12g, closed form %.12g\n", P.name, order, t, o.info[8 * t], P.cost[t]); bad++; }
        worst = std::fmax(worst, err);
        itmax = std::max(itmax, (int)o.iters[t]);
    }
    std::printf("%-28s %-3s  B %d  KKT %lld  nnz(L) %lld  levels %lld  iterations <= %d  cost error %.2e\n", P.name, order, P.B, stats[2],
                stats[0], stats[5], itmax, worst);
    return o;
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static void expect_same(const Out& a, const Out& b, const char* what, const char* order)
{
    if (same_bits(a.x, b.x) && same_bits(a.y, b.y) && same_bits(a.z, b.z) && same_bits(a.s, b.s) && same_bits(a.info, b.info) &&
        same_bits(a.status, b.status) && same_bits(a.iters, b.iters)) return;
    std::printf("%s (%s): shared and per-problem arrays give different bits\n", what, order);
    bad++;
}
static Vec tile(const Vec& v, int B)
{
    Vec r;
    for (int t = 0; t < B; t++) r.insert(r.end(), v.begin(), v.end());
    return r;
}

int main()
{
    // min g x0  s.t.  x1 + x2 = beta,  (x0, x1, x2) in Q^3:   x0 = |beta| / sqrt(2)
    Program soc{"SOCP, h / Gx / Ax shared", 3, 1, 3, 0, {3}, {0, 0, 1, 2}, {0, 0}, {0, 1, 2, 3}, {0, 1, 2}, 3,
                SCP_CONIC_SHARED_H | SCP_CONIC_SHARED_G | SCP_CONIC_SHARED_A,
                {1, 0, 0, 2, 0, 0, 0.5, 0, 0}, {1, -2, 3}, {0, 0, 0}, {-1, -1, -1}, {1, 1}, {}};
    const double g[3] = {1, 2, 0.5}, beta[3] = {1, -2, 3};
    for (int t = 0; t < 3; t++) soc.cost.push_back(g[t] * std::fabs(beta[t]) / std::sqrt(2.0));
    Program soc_all = soc;
    soc_all.name = "SOCP, every array per problem"; soc_all.shared = 0;
    soc_all.h = tile(soc.h, 3); soc_all.Gx = tile(soc.Gx, 3); soc_all.Ax = tile(soc.Ax, 3);

    // min w  s.t.  x = a,  y = r,  (x, y, w) in the exponential cone:   w = r exp(a / r)
    Program ex{"exponential cone", 3, 2, 3, 0, {-3}, {0, 1, 2, 2}, {0, 1}, {0, 1, 2, 3}, {0, 1, 2}, 2, SCP_CONIC_SHARED_C | SCP_CONIC_SHARED_G,
               {0, 0, 1}, {0.5, 1, -1, 2}, {0, 0, 0, 0, 0, 0}, {-1, -1, -1}, {1, 1, 1, 1}, {std::exp(0.5), 2 * std::exp(-0.5)}};

    // min -x0 - 2 x1  s.t.  x0 <= h0,  x1 <= h1,  x0 + x1 <= h2,  x >= 0   (no equality rows, no cones)
    Program lp{"LP, p = 0, no cones", 2, 0, 5, 5, {}, {}, {}, {0, 3, 6}, {0, 2, 3, 1, 2, 4}, 2, SCP_CONIC_SHARED_C | SCP_CONIC_SHARED_G,
               {-1, -2}, {}, {1, 2, 2.5, 0, 0, 3, 1, 3.5, 0, 0}, {1, 1, -1, 1, 1, -1}, {}, {-4.5, -4.5}};

    for (const char* order : {"seq", "nd"}) {
        setenv("CONIC_HOST_ORDER", order, 1);
        const Out a = solve(soc, order), b = solve(soc_all, order);
        expect_same(a, b, "SOCP", order);
        solve(ex, order);
        solve(lp, order);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
