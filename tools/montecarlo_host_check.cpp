// Stand-alone sanitizer check of the two host twins of the Monte-Carlo audit: scp_model_audit_montecarlo_host for the rocket
// landing and the quadrotor, N in {2, 9}, D in {2, 64, 65} (one padded wavefront, a full one, a second one with a single flight),
// with and without the optional outputs, and scp_mc_draws_host for odd and even n (both csrc/mc_api.hip).  The gains come from
// scp_lqr_gains_host (csrc/lqr_api.hip).  Heap arrays of EXACTLY the documented sizes.  Not a pytest and not loaded into Python.
// Build and run from the repository root (host code only; no GPU is needed or used):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/montecarlo_host_check.cpp scptoolbox.jl_amd/csrc/mc_api.hip scptoolbox.jl_amd/csrc/lqr_api.hip \
//         -o build/montecarlo_host_check && build/montecarlo_host_check
//
// Exit status 0 and one line per call when every call returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

struct Case {
    const char* name;
    int id, nx, nu;
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
        }
    }
}

int main()
{
    int bad = 0;
    const double d2r = 3.14159265358979323846 / 180.0;
    std::vector<Case> cases;
    cases.push_back({"rocket_landing", SCP_MODEL_ROCKET_LANDING, 7, 4,
                     {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
                     {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}, {14, 14, 7, 7}});
    cases.push_back({"quadrotor", SCP_MODEL_QUADROTOR, 6, 4,
                     {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
                     {1, 1, 1, 1, 1, 1}, {46, 46, 46, 23}});
    for (const Case& c : cases) {
        const int nv = 1 + 2 * c.nx + c.nu;
        for (int N : {2, 9}) {
            std::vector<double> xd((size_t)c.nx * N), ud((size_t)c.nu * N);
            for (int k = 0; k < N; k++) {
                const double t = (double)k / (N - 1);
                for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
                for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
            }
            std::vector<double> A, Bm, Bp, K((size_t)c.nu * c.nx * (N - 1), -5.0);
            make_dyn(c.nx, c.nu, N, A, Bm, Bp);
            std::vector<double> qx(c.nx), ru(c.nu), qf(c.nx), info(SCP_LQR_INFO_WIDTH);
            for (int i = 0; i < c.nx; i++) { qx[i] = 1.0 / (c.Sx[i] * c.Sx[i]); qf[i] = 10.0 * qx[i]; }
            for (int i = 0; i < c.nu; i++) ru[i] = 1.0 / (c.Su[i] * c.Su[i]);
            const bool gk = scp_lqr_gains_host(c.nx, c.nu, N, A.data(), Bm.data(), Bp.data(), qx.data(), ru.data(), qf.data(), K.data(),
                                               info.data()) == SCP_OK && info[0] == 0.0;
            std::vector<double> par(c.par), p(c.p), pp(c.pp), Sx(c.Sx), Su(c.Su), sig0(c.nx), sigu(c.nu), sigw(c.nx);
            for (int i = 0; i < c.nx; i++) { sig0[i] = 0.01 * Sx[i]; sigw[i] = 0.002 * Sx[i]; }
            for (int i = 0; i < c.nu; i++) sigu[i] = 0.01 * Su[i];
            for (int D : {2, 64, 65}) {
                std::vector<double> sum(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0), stat(SCP_MC_STAT_WIDTH, -9.0),
                    stat2(SCP_MC_STAT_WIDTH, -10.0), mom((size_t)nv * N, -11.0), fl((size_t)SCP_AUDIT_WIDTH * D, -12.0);
                const uint64_t seed = 0x1234567890ABCDEFull + (uint64_t)D;
                const int rc = scp_model_audit_montecarlo_host(c.id, par.data(), N, xd.data(), ud.data(), p.data(), pp.data(), Sx.data(), Su.data(),
                                                               K.data(), 3, 0.0, D, seed, sig0.data(), sigu.data(), sigw.data(), sum.data(),
                                                               stat.data(), mom.data(), fl.data());
                const int rc2 = scp_model_audit_montecarlo_host(c.id, par.data(), N, xd.data(), ud.data(), p.data(), pp.data(), Sx.data(), Su.data(),
                                                                K.data(), 3, 0.0, D, seed, sig0.data(), sigu.data(), sigw.data(), only.data(),
                                                                stat2.data(), nullptr, nullptr);
                bool fin = gk && rc == SCP_OK && rc2 == SCP_OK && sum[13] == 4.0 && sum[14] == (double)D && sum[11] == 0.0 && stat[7] == (double)D;
                for (int i = 0; i < SCP_AUDIT_WIDTH; i++) fin = fin && !std::isnan(sum[i]) && sum[i] == only[i];
                for (int i = 0; i < SCP_MC_STAT_WIDTH; i++) fin = fin && std::isfinite(stat[i]) && stat[i] == stat2[i];
                fin = fin && stat[0] > 0.0 && stat[1] >= 1.0 && stat[1] <= N && stat[2] >= 1.0 && stat[2] <= c.nx && stat[6] >= 1.0 && stat[6] <= N - 1;
                for (int k = 0; k < N; k++) {
                    const double* r = mom.data() + (size_t)k * nv;
                    fin = fin && r[0] == (double)D;
                    for (int i = 1; i <= 2 * c.nx; i++) fin = fin && std::isfinite(r[i]);
                    for (int i = 2 * c.nx + 1; i < nv; i++) fin = fin && (k == N - 1 ? std::isnan(r[i]) : std::isfinite(r[i]));
                }
                for (double v : fl) fin = fin && !std::isnan(v);
                std::printf("%-15s N %d D %2d rc %d  std %.6g@%g/%g mean %.6g@%g rms %.6g@%g n_min %g%s\n", c.name, N, D, rc, stat[0], stat[1],
                            stat[2], stat[3], stat[4], stat[5], stat[6], stat[7], fin ? "" : "   <-- BAD");
                bad += fin ? 0 : 1;
            }
            // a NaN gain in the last interval: the flights say so, that node counts nobody, nothing aborts
            if (N > 2) {
                std::vector<double> Kn(K);
                Kn[Kn.size() - c.nu] = NAN;      // the first input of the last hold (the last one of the quadrotor enters no dynamics)
                std::vector<double> sum(SCP_AUDIT_WIDTH), stat(SCP_MC_STAT_WIDTH), mom((size_t)nv * N);
                const int rn = scp_model_audit_montecarlo_host(c.id, par.data(), N, xd.data(), ud.data(), p.data(), pp.data(), Sx.data(), Su.data(),
                                                               Kn.data(), 2, 0.0, 3, 1, sig0.data(), sigu.data(), sigw.data(), sum.data(),
                                                               stat.data(), mom.data(), nullptr);
                const bool fin = rn == SCP_OK && sum[11] == 3.0 && stat[7] == 0.0 && mom[(size_t)(N - 2) * nv] == 0.0 && mom[(size_t)(N - 3) * nv] == 3.0 &&
                                 std::isnan(mom[(size_t)(N - 1) * nv + 1]);
                std::printf("%-15s N %d NaN gain rc %d flagged %g n_min %g%s\n", c.name, N, rn, sum[11], stat[7], fin ? "" : "   <-- BAD");
                bad += fin ? 0 : 1;
            }
        }
    }
    // the draws: exactly n doubles and 4 ceil(n / 2) words
    for (int n : {1, 2, 7, 8}) {
        std::vector<double> z(n, -1.0);
        std::vector<unsigned> w((size_t)4 * ((n + 1) / 2), 0u);
        bool fin = scp_mc_draws_host(0xFFFFFFFF00000001ull, 2, 9, 65, n, z.data(), w.data()) == SCP_OK;
        for (double v : z) fin = fin && std::isfinite(v) && std::fabs(v) < 9.0;
        std::vector<double> z2(n, -1.0);
        fin = fin && scp_mc_draws_host(0xFFFFFFFF00000001ull, 2, 9, 65, n, z2.data(), nullptr) == SCP_OK && z2 == z;
        std::printf("draws n %d z0 %.17g%s\n", n, z[0], fin ? "" : "   <-- BAD");
        bad += fin ? 0 : 1;
    }
    {
        std::vector<double> z(2);
        std::vector<unsigned> w(4);
        const bool kat = scp_mc_draws_host(0, 0, 0, 1, 2, z.data(), w.data()) == SCP_OK && w[0] == 0x6627e8d5u && w[1] == 0xe169c58du &&
                         w[2] == 0xbc57ac4cu && w[3] == 0x9b00dbd8u;
        std::printf("known answer %08x %08x %08x %08x%s\n", w[0], w[1], w[2], w[3], kat ? "" : "   <-- BAD");
        bad += kat ? 0 : 1;
    }
    // the refusals, which touch no array
    {
        const int before = bad;
        double one[64];
        for (double& v : one) v = 1.0;
        double neg[8] = {-1.0, 1, 1, 1, 1, 1, 1, 1};
#define MC(id, K, steps, D, s0, su, sw, sum, st) \
    scp_model_audit_montecarlo_host(id, one, 5, one, one, one, one, one, one, K, steps, 0.0, D, 0, s0, su, sw, sum, st, nullptr, nullptr)
        if (MC(SCP_MODEL_FREEFLYER, one, 1, 2, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (MC(SCP_MODEL_OSCILLATOR, one, 1, 2, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
        if (MC(42, one, 1, 2, one, one, one, one, one) != SCP_ERR_UNKNOWN_MODEL) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 1, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 0, 2, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, nullptr, 1, 2, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 1, 2, neg, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 1, 2, one, nullptr, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 1, 2, one, one, one, nullptr, one) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (MC(SCP_MODEL_QUADROTOR, one, 1, 2, one, one, one, one, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
#undef MC
        if (scp_mc_draws_host(0, 3, 0, 1, 2, one, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_mc_draws_host(0, 0, 0, 0, 2, one, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        if (scp_mc_draws_host(0, 0, 0, 1, 2, nullptr, nullptr) != SCP_ERR_BAD_ARGUMENT) bad++;
        std::printf("refusals: %d wrong\n", bad - before);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
