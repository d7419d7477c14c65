// Stand-alone sanitizer check of the two host twins of the closed-loop tracking audit: scp_lqr_gains_host (csrc/lqr_api.hip) for
// the four dimension pairs, N in {2, 9}, with a finite problem, a failing one (a pivot of exactly 0) and a non-finite one; and
// scp_model_audit_tracking_host (csrc/audit_api.hip) for the rocket landing and the quadrotor, N in {2, 9}, D in {1, 3},
// steps in {1, 4}, with and without the flight records and the truth model, flown with the gains the first twin made.  Heap
// arrays of EXACTLY the documented sizes.  Not a pytest and not loaded into Python.  Build and run from the repository root (host
// code only; no GPU is needed or used):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/lqr_tracking_host_check.cpp scptoolbox.jl_amd/csrc/audit_api.hip scptoolbox.jl_amd/csrc/lqr_api.hip \
//         -o build/lqr_tracking_host_check && build/lqr_tracking_host_check
//
// Exit status 0 and one line per call when every call returned what it should.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

struct Case {
    const char* name;
    int id, nx, nu, np, npp;
    std::vector<double> par, par_true, x0, xf, u, p, pp, Sx, Su;
};

// a discretisation that looks like one: A = I + h (a few couplings), B-, B+ = h / 2 (a few entries); [.,.,N-1] column-major
static void make_dyn(int nx, int nu, int N, std::vector<double>& A, std::vector<double>& Bm, std::vector<double>& Bp)
{
    const double h = 1.0 / (N - 1);
    A.assign((size_t)nx * nx * (N - 1), 0.0);
    Bm.assign((size_t)nx * nu * (N - 1), 0.0);
    Bp.assign((size_t)nx * nu * (N - 1), 0.0);
    for (int k = 0; k < N - 1; k++) {
        double* a = A.data() + (size_t)k * nx * nx;
        for (int i = 0; i < nx; i++) a[i + nx * i] = 1.0;
        for (int i = 0; i + nx / 2 < nx; i++) a[i + nx * (i + nx / 2)] = h * (1.0 + 0.1 * k);      // position rows read the velocities
        for (int c = 0; c < nu; c++) {
            const int i = nx / 2 + c % (nx - nx / 2);
            Bm[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 + 0.05 * c);
            Bp[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 - 0.05 * c);
            Bm[(size_t)k * nx * nu + c % nx + nx * c] += 0.1 * h * h;
        }
    }
}

int main()
{
    int bad = 0;
    // ---- scp_lqr_gains_host ----
    const int dims[4][2] = {{2, 1}, {6, 4}, {7, 4}, {8, 3}};
    for (const auto& d : dims) {
        const int nx = d[0], nu = d[1];
        for (int N : {2, 9}) {
            std::vector<double> A, Bm, Bp, qx(nx, 1.0), ru(nu, 0.5), qf(nx, 10.0);
            make_dyn(nx, nu, N, A, Bm, Bp);
            std::vector<double> K((size_t)nu * nx * (N - 1), -5.0), info(SCP_LQR_INFO_WIDTH, -6.0);
            int rc = scp_lqr_gains_host(nx, nu, N, A.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(), info.data());
            bool fin = rc == SCP_OK && info[0] == 0.0 && info[3] == 0.0 && std::isfinite(info[1]) && std::isfinite(info[2]) && info[1] > 0.0;
            for (double v : K) fin = fin && std::isfinite(v);
            std::printf("gains (%d,%d) N %d rc %d failed %g kmax %.6g trace %.6g%s\n", nx, nu, N, rc, info[0], info[1], info[2], fin ? "" : "   <-- BAD");
            bad += fin ? 0 : 1;
            // a non-finite entry in the FIRST interval, the last one met: every K_k is NaN afterwards
            std::vector<double> An(A);
            An[1] = INFINITY;
            rc = scp_lqr_gains_host(nx, nu, N, An.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(), info.data());
            fin = rc == SCP_OK && info[0] == 1.0;
            for (double v : K) fin = fin && std::isnan(v);
            bad += fin ? 0 : 1;
            if (nu > 1) {      // two identical input columns and an R that is lost against Gam' P Gam = 4: a pivot of exactly 0
                std::vector<double> Ai((size_t)nx * nx * (N - 1), 0.0), Bz((size_t)nx * nu * (N - 1), 0.0), r0(nu, 1e-30), q0(nx, 0.0), q1(nx, 1.0);
                for (int k = 0; k < N - 1; k++) {
                    for (int i = 0; i < nx; i++) Ai[(size_t)k * nx * nx + i + nx * i] = 1.0;
                    Bz[(size_t)k * nx * nu + 0] = 1.0;
                    Bz[(size_t)k * nx * nu + nx] = 1.0;
                }
                rc = scp_lqr_gains_host(nx, nu, N, Ai.data(), Bz.data(), Bz.data(), q0.data(), r0.data(), q1.data(), K.data(), info.data());
                fin = rc == SCP_OK && info[0] == 1.0;
                for (double v : K) fin = fin && std::isnan(v);
                std::printf("gains (%d,%d) N %d zero pivot: rc %d failed %g%s\n", nx, nu, N, rc, info[0], fin ? "" : "   <-- BAD");
                bad += fin ? 0 : 1;
            }
        }
    }
    {
        double one[64] = {1.0};
        for (double& v : one) v = 1.0;
        double neg[8] = {-1.0, 1, 1, 1, 1, 1, 1, 1};
        if (scp_lqr_gains_host(13, 6, 5, one, one, one, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, neg, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, one, neg, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, one, one, nullptr, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 1, one, one, one, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    }

    // ---- scp_model_audit_tracking_host ----
    const double d2r = 3.14159265358979323846 / 180.0;
    std::vector<Case> cases;
    cases.push_back({"rocket_landing", SCP_MODEL_ROCKET_LANDING, 7, 4, 1, 6,
                     {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {0, 0, -4.0, 6.1e-5, 0, 3.5e-5, 5.6e-4, 1505, 1905, 4972, 12000, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
                     {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}, {14, 14, 7, 7}});
    cases.push_back({"quadrotor", SCP_MODEL_QUADROTOR, 6, 4, 1, 12,
                     {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {10.3, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
                     {1, 1, 1, 1, 1, 1}, {46, 46, 46, 23}});
    for (const Case& c : cases) {
        for (int N : {2, 9}) {
            for (int D : {1, 3}) {
                for (int steps : {1, 4}) {
                    for (int truth = 0; truth < 2; truth++) {
                        std::vector<double> xd((size_t)c.nx * N), ud((size_t)c.nu * N);
                        for (int k = 0; k < N; k++) {
                            const double t = (double)k / (N - 1);
                            for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
                            for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
                        }
                        std::vector<double> dx0((size_t)c.nx * D), gain((size_t)c.nu * D), bias((size_t)c.nu * D);
                        for (int d = 0; d < D; d++) {
                            for (int i = 0; i < c.nx; i++) dx0[(size_t)d * c.nx + i] = 0.01 * (d + 1) * c.Sx[i] * std::sin(1.0 + i + d);
                            for (int i = 0; i < c.nu; i++) {
                                gain[(size_t)d * c.nu + i] = 1.0 + 0.02 * d * std::cos(2.0 + i);
                                bias[(size_t)d * c.nu + i] = 0.01 * d * std::sin(3.0 + i);
                            }
                        }
                        // gains by Bryson's rule on the synthetic discretisation: small, finite, of the documented size
                        std::vector<double> A, Bm, Bp, qx(c.nx), ru(c.nu), qf(c.nx);
                        make_dyn(c.nx, c.nu, N, A, Bm, Bp);
                        for (int i = 0; i < c.nx; i++) { qx[i] = 1.0 / (c.Sx[i] * c.Sx[i]); qf[i] = 10.0 * qx[i]; }
                        for (int i = 0; i < c.nu; i++) ru[i] = 1.0 / (c.Su[i] * c.Su[i]);
                        std::vector<double> K((size_t)c.nu * c.nx * (N - 1)), info(SCP_LQR_INFO_WIDTH);
                        const int rg = scp_lqr_gains_host(c.nx, c.nu, N, A.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(),
                                                          info.data());
                        std::vector<double> par(c.par), pt(c.par_true), p(c.p), pp(c.pp), Sx(c.Sx), Su(c.Su);
                        std::vector<double> sum(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0), rec((size_t)SCP_AUDIT_WIDTH * D, -9.0);
                        const double* ptrue = truth ? pt.data() : nullptr;
                        const int rc = scp_model_audit_tracking_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                     Sx.data(), Su.data(), K.data(), steps, 0.0, D, dx0.data(), gain.data(),
                                                                     bias.data(), sum.data(), rec.data());
                        const int rc2 = scp_model_audit_tracking_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                      Sx.data(), Su.data(), K.data(), steps, 0.0, D, dx0.data(), gain.data(),
                                                                      bias.data(), only.data(), nullptr);
                        bool fin = rg == SCP_OK && info[0] == 0.0 && rc == SCP_OK && rc2 == SCP_OK && sum[11] == 0.0 && sum[13] == 3.0 && sum[14] == (double)D;
                        for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(sum[i]) && sum[i] == only[i];
                        for (int d = 0; d < D; d++) {
                            const double* r = rec.data() + (size_t)d * SCP_AUDIT_WIDTH;
                            for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(r[i]);
                            fin = fin && r[12] > 0.0 && r[13] >= 1.0 && r[13] <= N - 1 && r[14] > 0.0 && r[15] >= 1.0 && r[15] <= N;
                        }
                        std::printf("%-15s N %d D %d steps %d truth %d rc %d  drift %.6g cost %.6g..%.6g effort %.6g@%g track %.6g@%g%s\n", c.name, N, D,
                                    steps, truth, rc, sum[8], sum[9], sum[15], rec[12], rec[13], rec[14], rec[15], fin ? "" : "   <-- BAD");
                        bad += fin ? 0 : 1;
                    }
                }
            }
        }
    }
    // NULL dispersion arrays, and the refusals, which touch no array
    {
        const Case& c = cases[1];
        const int N = 2;
        std::vector<double> xd(c.x0), ud(c.u), sum(SCP_AUDIT_WIDTH, -7.0), K((size_t)c.nu * c.nx, 0.0);
        xd.insert(xd.end(), c.xf.begin(), c.xf.end());
        ud.insert(ud.end(), c.u.begin(), c.u.end());
        if (scp_model_audit_tracking_host(c.id, c.par.data(), nullptr, N, xd.data(), ud.data(), c.p.data(), c.pp.data(), c.Sx.data(), c.Su.data(),
                                          K.data(), 3, 0.0, 2, nullptr, nullptr, nullptr, sum.data(), nullptr) != SCP_OK || sum[11] != 0.0 ||
            sum[14] != 2.0 || sum[13] != 3.0) bad++;
    }
    double one[SCP_AUDIT_WIDTH] = {0};
    if (scp_model_audit_tracking_host(SCP_MODEL_FREEFLYER, one, nullptr, 5, one, one, one, one, one, one, one, 4, 0.0, 1, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, one, 4, 0.0, 0, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, one, 0, 0.0, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, nullptr, 4, 0.0, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
