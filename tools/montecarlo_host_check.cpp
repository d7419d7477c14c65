// Stand-alone sanitizer check of the two host twins of the Monte-Carlo audit: scp_model_audit_montecarlo_host for the rocket
// landing and the quadrotor, N in {2, 9}, D in {2, 64, 65} (one padded wavefront, a full one, a second one with a single flight),
// with and without the optional outputs, and scp_mc_draws_host for odd and even n (both csrc/mc_api.hip).  The gains come from
// scp_lqr_gains_host (csrc/lqr_api.hip).  Heap arrays of EXACTLY the documented sizes.  Not a pytest and not loaded into Python.
// Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per call when every call returned what it should.
#include <cstdint>

#include "host_check.hpp"

int main()
{
    for (int id : {SCP_MODEL_ROCKET_LANDING, SCP_MODEL_QUADROTOR}) {
        const Model& c = models()[id];
        const int nv = 1 + 2 * c.nx + c.nu;
        for (int N : {2, 9}) {
            std::vector<double> xd, ud;
            straight_line(c, N, xd, ud);
            std::vector<double> A, Bm, Bp, K;
            make_dyn(c.nx, c.nu, N, A, Bm, Bp, false);
            const bool gk = gains(c.nx, c.nu, N, A, Bm, Bp, c.Sx, c.Su, K);
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
    return verdict();
}
