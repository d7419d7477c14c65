// Stand-alone sanitizer check of the two host twins of the closed-loop tracking audit: scp_lqr_gains_host (csrc/lqr_api.hip) for
// the four dimension pairs, N in {2, 9}, with a finite problem, a failing one (a pivot of exactly 0) and a non-finite one; and
// scp_model_audit_tracking_host (csrc/audit_api.hip) for the rocket landing and the quadrotor, N in {2, 9}, D in {1, 3},
// steps in {1, 4}, with and without the flight records and the truth model, flown with the gains the first twin made.  Heap
// arrays of EXACTLY the documented sizes.  Not a pytest and not loaded into Python.  Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per call when every call returned what it should.
#include "host_check.hpp"

int main()
{
    // ---- scp_lqr_gains_host ----
    for (const Model& m : models()) {
        const int nx = m.nx, nu = m.nu;
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
        if (scp_lqr_gains_host(13, 6, 5, one, one, one, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, neg, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, one, neg, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 2, one, one, one, one, one, nullptr, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_lqr_gains_host(2, 1, 1, one, one, one, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    }

    // ---- scp_model_audit_tracking_host ----
    for (int id : {SCP_MODEL_ROCKET_LANDING, SCP_MODEL_QUADROTOR}) {
        const Model& c = models()[id];
        for (int N : {2, 9}) {
            for (int D : {1, 3}) {
                for (int steps : {1, 4}) {
                    for (int truth = 0; truth < 2; truth++) {
                        std::vector<double> xd, ud;
                        straight_line(c, N, xd, ud);
                        std::vector<double> dx0((size_t)c.nx * D), gain((size_t)c.nu * D), bias((size_t)c.nu * D);
                        for (int d = 0; d < D; d++) {
                            for (int i = 0; i < c.nx; i++) dx0[(size_t)d * c.nx + i] = 0.01 * (d + 1) * c.Sx[i] * std::sin(1.0 + i + d);
                            for (int i = 0; i < c.nu; i++) {
                                gain[(size_t)d * c.nu + i] = 1.0 + 0.02 * d * std::cos(2.0 + i);
                                bias[(size_t)d * c.nu + i] = 0.01 * d * std::sin(3.0 + i);
                            }
                        }
                        std::vector<double> A, Bm, Bp, K;
                        make_dyn(c.nx, c.nu, N, A, Bm, Bp);
                        const bool gk = gains(c.nx, c.nu, N, A, Bm, Bp, c.Sx, c.Su, K);
                        std::vector<double> par(c.par), pt(c.par_true), p(c.p), pp(c.pp), Sx(c.Sx), Su(c.Su);
                        std::vector<double> sum(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0), rec((size_t)SCP_AUDIT_WIDTH * D, -9.0);
                        const double* ptrue = truth ? pt.data() : nullptr;
                        const int rc = scp_model_audit_tracking_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                     Sx.data(), Su.data(), K.data(), steps, 0.0, D, dx0.data(), gain.data(),
                                                                     bias.data(), sum.data(), rec.data());
                        const int rc2 = scp_model_audit_tracking_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                      Sx.data(), Su.data(), K.data(), steps, 0.0, D, dx0.data(), gain.data(),
                                                                      bias.data(), only.data(), nullptr);
                        bool fin = gk && rc == SCP_OK && rc2 == SCP_OK && sum[11] == 0.0 && sum[13] == 3.0 && sum[14] == (double)D;
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
        const Model& c = models()[SCP_MODEL_QUADROTOR];
        const int N = 2;
        std::vector<double> xd(c.x0), ud(c.u), sum(SCP_AUDIT_WIDTH, -7.0), K((size_t)c.nu * c.nx, 0.0);
        xd.insert(xd.end(), c.xf.begin(), c.xf.end());
        ud.insert(ud.end(), c.u.begin(), c.u.end());
        if (scp_model_audit_tracking_host(c.id, c.par.data(), nullptr, N, xd.data(), ud.data(), c.p.data(), c.pp.data(), c.Sx.data(), c.Su.data(),
                                          K.data(), 3, 0.0, 2, nullptr, nullptr, nullptr, sum.data(), nullptr) != SCP_OK || sum[11] != 0.0 ||
            sum[14] != 2.0 || sum[13] != 3.0) bad++;
    }
    if (scp_model_audit_tracking_host(SCP_MODEL_FREEFLYER, one, nullptr, 5, one, one, one, one, one, one, one, 4, 0.0, 1, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, one, 4, 0.0, 0, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, one, 0, 0.0, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    if (scp_model_audit_tracking_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, one, nullptr, 4, 0.0, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    return verdict();
}
