// Stand-alone sanitizer check of the two host twins of the closed-loop covariance audit: scp_model_covariance_rows_host for the
// rocket landing, the quadrotor and the double integrator, N in {2, 9}, and scp_covariance_host (both csrc/cov_api.hip) on the rows
// the first twin made, with and without the optional outputs, with a non-finite discretisation, and for all four dimension pairs on
// hand-made rows.  The gains come from scp_lqr_gains_host (csrc/lqr_api.hip).  Heap arrays of EXACTLY the documented sizes.  Not a
// pytest and not loaded into Python.  Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per call when every call returned what it should.
#include "host_check.hpp"

int main()
{
    for (int id : {SCP_MODEL_ROCKET_LANDING, SCP_MODEL_QUADROTOR}) {
        const Model& c = models()[id];
        const int nrow = c.nrow[0] + c.nrow[1] + c.nrow[2];
        for (int N : {2, 9}) {
            std::vector<double> xd, ud;
            straight_line(c, N, xd, ud);
            std::vector<double> A, Bm, Bp, K;
            make_dyn(c.nx, c.nu, N, A, Bm, Bp);
            const bool gk = gains(c.nx, c.nu, N, A, Bm, Bp, c.Sx, c.Su, K);
            std::vector<double> par(c.par), p(c.p), pp(c.pp), Sx(c.Sx), Su(c.Su);
            std::vector<double> rows((size_t)(c.nx + 1) * nrow * N, -1.0), Hf((size_t)c.ntc * c.nx, -2.0);
            const int rr = scp_model_covariance_rows_host(c.id, par.data(), N, xd.data(), ud.data(), p.data(), pp.data(), K.data(), rows.data(), Hf.data());
            bool fin = gk && rr == SCP_OK;
            for (double v : rows) fin = fin && std::isfinite(v);
            for (double v : Hf) fin = fin && std::isfinite(v);
            std::vector<double> sig0(c.nx), sigu(c.nu), sigw(c.nx);
            for (int i = 0; i < c.nx; i++) { sig0[i] = 0.01 * Sx[i]; sigw[i] = 1e-3 * Sx[i]; }
            for (int i = 0; i < c.nu; i++) sigu[i] = 0.01 * Su[i];
            std::vector<double> sum(SCP_COV_WIDTH, -7.0), only(SCP_COV_WIDTH, -8.0), sig((size_t)c.nx * N, -9.0), nodes((size_t)SCP_COV_NODE_WIDTH * N, -10.0);
            const int rc = scp_covariance_host(c.nx, c.nu, N, A.data(), Bm.data(), Bp.data(), K.data(), c.nrow, rows.data(), c.ntc, Hf.data(), Sx.data(),
                                               Su.data(), sig0.data(), sigu.data(), sigw.data(), 3.0, sum.data(), sig.data(), nodes.data());
            const int rc2 = scp_covariance_host(c.nx, c.nu, N, A.data(), Bm.data(), Bp.data(), K.data(), c.nrow, rows.data(), c.ntc, Hf.data(), Sx.data(),
                                                Su.data(), sig0.data(), sigu.data(), sigw.data(), 3.0, only.data(), nullptr, nullptr);
            fin = fin && rc == SCP_OK && rc2 == SCP_OK && sum[0] == 0.0 && sum[15] == 0.0;
            for (int i = 0; i < SCP_COV_WIDTH; i++) fin = fin && !std::isnan(sum[i]) && sum[i] == only[i];
            for (int i : {1, 4, 12, 13}) fin = fin && std::isfinite(sum[i]) && sum[i] > 0.0;
            fin = fin && sum[2] >= 1.0 && sum[2] <= N && sum[3] >= 1.0 && sum[3] <= c.nx && sum[5] >= 1.0 && sum[5] <= N - 1;
            for (double v : sig) fin = fin && std::isfinite(v) && v > 0.0;
            for (int k = 0; k < N; k++) fin = fin && nodes[(size_t)k * SCP_COV_NODE_WIDTH] > 0.0 && (k == N - 1) == std::isnan(nodes[(size_t)k * SCP_COV_NODE_WIDTH + 1]);
            std::printf("%-15s N %d rows rc %d chain rc %d  sigma %.6g@%g/%g effort %.6g@%g margins %.4g %.4g %.4g tau %.6g below %g%s\n", c.name, N, rr,
                        rc, sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[8], sum[10], sum[12], sum[14], fin ? "" : "   <-- BAD");
            bad += fin ? 0 : 1;
            // a non-finite entry in the last interval: the record says so and nothing else is claimed
            std::vector<double> An(A);
            An[An.size() - 2] = NAN;
            const int rn = scp_covariance_host(c.nx, c.nu, N, An.data(), Bm.data(), Bp.data(), K.data(), c.nrow, rows.data(), c.ntc, Hf.data(), Sx.data(),
                                               Su.data(), sig0.data(), sigu.data(), sigw.data(), 3.0, sum.data(), sig.data(), nodes.data());
            fin = rn == SCP_OK && sum[0] == 1.0;
            for (int i = 1; i < SCP_COV_WIDTH; i++) fin = fin && std::isnan(sum[i]);
            bad += fin ? 0 : 1;
        }
    }
    // every dimension pair on hand-made rows: more rows than entries of Sigma for (2,1), none at all, and no terminal rows
    for (const Model& m : models()) {
        const int nx = m.nx, nu = m.nu;
        for (int N : {2, 9}) {
            std::vector<double> A, Bm, Bp, K, Sx(nx, 2.0), Su(nu, 3.0), sig0(nx, 0.02), sigu(nu, 0.0), sigw(nx, 0.0);
            make_dyn(nx, nu, N, A, Bm, Bp);
            bool fin = gains(nx, nu, N, A, Bm, Bp, Sx, Su, K);
            const int nrow[3] = {3, 0, 4}, none[3] = {0, 0, 0}, nr = 7, ntc = 1;
            std::vector<double> rows((size_t)(nx + 1) * nr * N, 0.0), Hf((size_t)ntc * nx, 1.0);
            for (int k = 0; k < N; k++)
                for (int r = 0; r < nr; r++) {
                    double* row = rows.data() + ((size_t)k * nr + r) * (nx + 1);
                    row[r % nx] = 1.0 + r;
                    row[nx] = -0.1 * (r + 1);
                }
            std::vector<double> sum(SCP_COV_WIDTH, -7.0), sig((size_t)nx * N, -9.0), nodes((size_t)SCP_COV_NODE_WIDTH * N, -10.0);
            int rc = scp_covariance_host(nx, nu, N, A.data(), Bm.data(), Bp.data(), K.data(), nrow, rows.data(), ntc, Hf.data(), Sx.data(), Su.data(),
                                         sig0.data(), sigu.data(), sigw.data(), 2.0, sum.data(), sig.data(), nodes.data());
            fin = fin && rc == SCP_OK && sum[0] == 0.0 && std::isfinite(sum[6]) && sum[8] == INFINITY && sum[9] == 0.0 && std::isfinite(sum[10]) && sum[12] > 0.0;
            rc = scp_covariance_host(nx, nu, N, A.data(), Bm.data(), Bp.data(), K.data(), none, nullptr, 0, nullptr, Sx.data(), Su.data(), sig0.data(),
                                     sigu.data(), sigw.data(), 2.0, sum.data(), nullptr, nullptr);
            fin = fin && rc == SCP_OK && sum[0] == 0.0 && sum[6] == INFINITY && sum[7] == 0.0 && sum[10] == INFINITY && sum[12] == 0.0 && sum[14] == 0.0;
            std::printf("chain (%d,%d) N %d rc %d%s\n", nx, nu, N, rc, fin ? "" : "   <-- BAD");
            bad += fin ? 0 : 1;
        }
    }
    // the refusals, which touch no array
    {
        const int nrow[3] = {0, 0, 0}, nbad[3] = {0, -1, 0};
        if (scp_covariance_host(13, 6, 5, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, one, one, one, 3.0, one, nullptr, nullptr) != SCP_ERR_UNSUPPORTED) bad++;
        if (scp_covariance_host(2, 1, 2, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, neg, one, one, 3.0, one, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_covariance_host(2, 1, 2, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, one, nullptr, one, 3.0, one, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_covariance_host(2, 1, 2, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, one, one, one, 0.0, one, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_covariance_host(2, 1, 2, one, one, one, one, nbad, nullptr, 0, nullptr, one, one, one, one, one, 3.0, one, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_covariance_host(2, 1, 2, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, one, one, one, 3.0, nullptr, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_covariance_host(2, 1, 1, one, one, one, one, nrow, nullptr, 0, nullptr, one, one, one, one, one, 3.0, one, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_model_covariance_rows_host(SCP_MODEL_FREEFLYER, one, 5, one, one, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (scp_model_covariance_rows_host(SCP_MODEL_OSCILLATOR, one, 5, one, one, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (scp_model_covariance_rows_host(SCP_MODEL_QUADROTOR, one, 5, one, one, one, one, nullptr, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_model_covariance_rows_host(42, one, 5, one, one, one, one, one, one, one) != SCP_ERR_UNKNOWN_MODEL) bad++;
    }
    return verdict();
}
