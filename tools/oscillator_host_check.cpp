// Stand-alone sanitizer check of the host compilation of the oscillator model (csrc/models/oscillator.hpp): the functions the
// device kernels call, on heap arrays of EXACTLY the sizes the kernels give them, at the mild and at the extreme sharpness
// kappa1 of the deadband homotopy (where exp overflows to Inf and the reference's order of operations must still give finite
// values).  Not a pytest and not loaded into Python.  Built and run by
// `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and "ok" when every value was finite and the analytic Jacobian of s agrees with central differences.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../scptoolbox.jl_amd/csrc/models/oscillator.hpp"

using M = scp::Oscillator;

static int bad = 0;
static void finite(const std::vector<double>& v, const char* what, double kappa, double ar)
{
    for (double x : v)
        if (!std::isfinite(x)) { std::printf("not finite: %s at kappa1 = %g, ar = %.17g\n", what, kappa, ar); bad++; return; }
}

int main()
{
    const int N = 12;
    for (double kappa : {4.595, 2.1e3, 4.595e8}) {
        std::vector<double> par = {0.5, 1.0, 0.05, 0.3, 10.0, kappa, 0.06, 0.1, 1.0};
        const M::Params P = M::make_params(par.data());
        const double db = P.a_db, am = P.a_max;
        double worst = 0.0;
        for (double ar : {0.0, db, -db, db * (1 + 1e-6), db * (1 - 1e-6), -db * (1 + 1e-6), -db * (1 - 1e-6), am, -am, 0.17, -0.02}) {
            std::vector<double> x = {0.4, -0.1}, u = {0.1, ar, 0.2, 0.3}, p(N, 0.25);
            std::vector<double> s(M::ns), C(M::ns * M::nx), D(M::ns * M::nu), G(M::ns * (M::np + M::np_node));
            M::s_eval(P, 0.5, 3, x.data(), u.data(), p.data(), s.data(), C.data(), D.data(), G.data());
            finite(s, "s", kappa, ar); finite(C, "C", kappa, ar); finite(D, "D", kappa, ar); finite(G, "G", kappa, ar);
            if (kappa < 1e2) {      // smooth enough for a difference quotient
                const double h = 1e-6;
                std::vector<double> up = u, um = u, sp(M::ns), sm(M::ns), c2(C.size()), d2(D.size()), g2(G.size());
                up[1] += h; um[1] -= h;
                M::s_eval(P, 0.5, 3, x.data(), up.data(), p.data(), sp.data(), c2.data(), d2.data(), g2.data());
                M::s_eval(P, 0.5, 3, x.data(), um.data(), p.data(), sm.data(), c2.data(), d2.data(), g2.data());
                for (int i = 0; i < M::ns; i++) worst = std::fmax(worst, std::fabs(D[i * M::nu + 1] - (sp[i] - sm[i]) / (2 * h)));
            }
            double xs[M::nx] = {0.4, -0.1}, us[M::nu] = {0.1, ar, 0.2, 0.3}, f[M::nx], A[M::nx * M::nx], B[M::nx * M::nu], Fc[M::nx], dx[M::nx];
            M::dyn(P, 0.5, 3, xs, us, p.data(), f, A, B, Fc);
            finite(std::vector<double>(f, f + M::nx), "f", kappa, ar);
            M::impulse(P, 0.5, 3, xs, us, p.data(), dx, B);
            finite(std::vector<double>(dx, dx + M::nx), "impulse", kappa, ar);
            int nq = 0;
            scp::for_each_x_indicator<M>(P, 0.5, 3, x.data(), p.data(), N, [&](double q) { if (!std::isfinite(q)) bad++; nq++; });
            if (nq != 2) { std::printf("X indicators: %d, expected 2\n", nq); bad++; }
        }
        if (worst > 1e-6) { std::printf("D against central differences: %g at kappa1 = %g\n", worst, kappa); bad++; }
        constexpr int nz = M::nx + M::nu, npc = M::np + M::np_node;
        std::vector<double> L(M::nl * nz), Lp(M::nl * npc), l(M::nl);
        M::lin_rows(P, 0.0, 1, L.data(), Lp.data(), l.data());
        std::vector<double> Qu(M::nu), lu(M::nu), lx(M::nx), tx(M::nx), tp(npc), Qp(npc);
        M::cost_terms(P, Qu.data(), lu.data(), lx.data(), tx.data(), tp.data(), Qp.data());
        finite(L, "L", kappa, 0); finite(Lp, "Lp", kappa, 0); finite(l, "l", kappa, 0); finite(tp, "tp", kappa, 0); finite(lu, "lu", kappa, 0);
        std::vector<double> pp = {-0.5, -0.1}, g(M::nic), H(M::nic * M::nx), x0 = {0.3, 0.2};
        M::bc_ic(P, x0.data(), nullptr, pp.data(), g.data(), H.data(), nullptr);
        M::bc_tc(P, x0.data(), nullptr, pp.data(), nullptr, nullptr, nullptr);
        finite(g, "g_ic", kappa, 0);
        double r_end = 0.0;
        for (int k = 0; k < N; k++) {
            double x[M::nx], u[M::nu];
            std::vector<double> pn(M::np_node);
            M::guess(P, pp.data(), N, k, x, u, nullptr, pn.data());
            finite({x[0], x[1], u[0], u[3], pn[0]}, "guess", kappa, 0);
            if (k == 0 && (x[0] != pp[0] || x[1] != pp[1])) { std::printf("guess: node 1 is not the initial condition\n"); bad++; }
            r_end = x[0];
        }
        std::printf("kappa1 %-10g  D vs central differences %.2e   free response r(1) = %.6g\n", kappa, worst, r_end);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
