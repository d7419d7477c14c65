// Stand-alone sanitizer check of the two host twins of the closed-loop covariance audit: scp_model_covariance_rows_host for the
// rocket landing, the quadrotor and the double integrator, N in {2, 9}, and scp_covariance_host (both csrc/cov_api.hip) on the rows
// the first twin made, with and without the optional outputs, with a non-finite discretisation, and for all four dimension pairs on
// hand-made rows.  The gains come from scp_lqr_gains_host (csrc/lqr_api.hip).  Heap arrays of EXACTLY the documented sizes.  Not a
// pytest and not loaded into Python.  Build and run from the repository root (host code only; no GPU is needed or used):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/covariance_host_check.cpp scptoolbox.jl_amd/csrc/cov_api.hip scptoolbox.jl_amd/csrc/lqr_api.hip \
//         -o build/covariance_host_check && build/covariance_host_check
//
// Exit status 0 and one line per call when every call returned what it should.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

struct Case {
    const char* name;
    int id, nx, nu, nrow[3], ntc;
    std::vector<double> par, x0, xf, u, p, pp, Sx, Su;
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
        for (int i = 0; i + nx / 2 < nx; i++) a[i + nx * (i + nx / 2)] = h * (1.0 + 0.1 * k);
        for (int c = 0; c < nu; c++) {
            const int i = nx / 2 + c % (nx - nx / 2);
            Bm[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 + 0.05 * c);
            Bp[(size_t)k * nx * nu + i + nx * c] = 0.5 * h * (1.0 - 0.05 * c);
            Bm[(size_t)k * nx * nu + c % nx + nx * c] += 0.1 * h * h;
        }
    }
}

static bool gains(int nx, int nu, int N, const std::vector<double>& A, const std::vector<double>& Bm, const std::vector<double>& Bp,
                  const std::vector<double>& Sx, const std::vector<double>& Su, std::vector<double>& K)
{
    std::vector<double> qx(nx), ru(nu), qf(nx), info(SCP_LQR_INFO_WIDTH);
    for (int i = 0; i < nx; i++) { qx[i] = 1.0 / (Sx[i] * Sx[i]); qf[i] = 10.0 * qx[i]; }
    for (int i = 0; i < nu; i++) ru[i] = 1.0 / (Su[i] * Su[i]);
    K.assign((size_t)nu * nx * (N - 1), -5.0);
    return scp_lqr_gains_host(nx, nu, N, A.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(), info.data()) == SCP_OK &&
           info[0] == 0.0;
}

int main()
{
    int bad = 0;
    const double d2r = 3.14159265358979323846 / 180.0;
    std::vector<Case> cases;
    cases.push_back({"rocket_landing", SCP_MODEL_ROCKET_LANDING, 7, 4, {2, 6, 2}, 6,
                     {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
                     {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}, {14, 14, 7, 7}});
    cases.push_back({"quadrotor", SCP_MODEL_QUADROTOR, 6, 4, {2, 3, 1}, 6,
                     {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
                     {1, 1, 1, 1, 1, 1}, {46, 46, 46, 23}});
    for (const Case& c : cases) {
        // nrow = (ns, nl, nsoc) and ntc of the model header: were they out of date, the sanitizer would see the pre-pass overrun `rows`
        const int nrow = c.nrow[0] + c.nrow[1] + c.nrow[2];
        for (int N : {2, 9}) {
            std::vector<double> xd((size_t)c.nx * N), ud((size_t)c.nu * N);
            for (int k = 0; k < N; k++) {
                const double t = (double)k / (N - 1);
                for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
                for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
            }
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
    const int dims[4][2] = {{2, 1}, {6, 4}, {7, 4}, {8, 3}};
    for (const auto& d : dims) {
        const int nx = d[0], nu = d[1];
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
        double one[64];
        for (double& v : one) v = 1.0;
        double neg[8] = {-1.0, 1, 1, 1, 1, 1, 1, 1};
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
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
