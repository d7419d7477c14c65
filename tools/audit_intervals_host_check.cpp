// Stand-alone sanitizer check of the host twin of the interval-parallel audit (scp_model_audit_intervals_host,
// csrc/audit_api.hip): the bodies the device kernels run, on heap arrays of EXACTLY the documented sizes, for a FOH case
// (rocket landing) and an IMPULSE case (quadrotor), with and without the interval records.  Not a pytest and not loaded into
// Python.  Build and run from the repository root (host code only; no GPU is needed or used):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/audit_intervals_host_check.cpp scptoolbox.jl_amd/csrc/audit_api.hip -o build/audit_intervals_host_check \
//         && build/audit_intervals_host_check
//
// Exit status 0 and one line per call when every call returned SCP_OK with finite, flag-free records.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

struct Case {
    const char* name;
    int id, method, nx, nu, np, npp;
    std::vector<double> par, x0, xf, u, p, pp, Sx;
};

int main()
{
    const double d2r = 3.14159265358979323846 / 180.0;
    std::vector<Case> cases;
    cases.push_back({"rocket_landing FOH", SCP_MODEL_ROCKET_LANDING, SCP_FOH, 7, 4, 1, 6,
                     {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
                     {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}});
    cases.push_back({"quadrotor IMPULSE", SCP_MODEL_QUADROTOR, SCP_IMPULSE, 6, 4, 1, 12,
                     {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
                     {1, 1, 1, 1, 1, 1}});
    int bad = 0;
    for (const Case& c : cases) {
        for (int N : {2, 9}) {
            for (int res : {2, 3 * (N - 1), 6 * (N - 1) + 1}) {
                std::vector<double> xd((size_t)c.nx * N), ud((size_t)c.nu * N);
                for (int k = 0; k < N; k++) {
                    const double t = (double)k / (N - 1);
                    for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
                    for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
                }
                std::vector<double> par(c.par), p(c.p), pp(c.pp), Sx(c.Sx), audit(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0);
                std::vector<double> rec((size_t)SCP_AUDIT_INTERVAL_WIDTH * (N - 1), -9.0);
                const int rc = scp_model_audit_intervals_host(c.id, par.data(), N, c.method, xd.data(), ud.data(), p.data(), pp.data(),
                                                              Sx.data(), res, 0.0, audit.data(), rec.data());
                const int rc2 = scp_model_audit_intervals_host(c.id, par.data(), N, c.method, xd.data(), ud.data(), p.data(), pp.data(),
                                                               Sx.data(), res, 0.0, only.data(), nullptr);
                bool fin = rc == SCP_OK && rc2 == SCP_OK && audit[11] == 0.0 && audit[13] == 1.0;
                for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(audit[i]) && audit[i] == only[i];
                for (int k = 0; k < N - 1; k++)
                    for (int i = 6; i < SCP_AUDIT_INTERVAL_WIDTH; i++) fin = fin && std::isfinite(rec[(size_t)k * SCP_AUDIT_INTERVAL_WIDTH + i]);
                std::printf("%-20s N %d res %3d rc %d  s %.6g@%.3f lin %.6g@%.3f soc %.6g@%.3f bc %.6g defect %.6g@%g cost %.6g nviol %g sub %g%s\n",
                            c.name, N, res, rc, audit[0], audit[1], audit[2], audit[3], audit[4], audit[5], audit[7], audit[8], audit[12],
                            audit[9], audit[10], audit[14], fin ? "" : "   <-- BAD");
                bad += fin ? 0 : 1;
            }
        }
    }
    // the refusals touch no array
    double one[SCP_AUDIT_WIDTH] = {0};
    if (scp_model_audit_intervals_host(SCP_MODEL_FREEFLYER, one, 5, SCP_FOH, one, one, one, one, one, 4, 0.0, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_intervals_host(SCP_MODEL_ROCKET_LANDING, one, 5, SCP_IMPULSE, one, one, one, one, one, 4, 0.0, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_intervals_host(SCP_MODEL_QUADROTOR, one, 5, SCP_FOH, one, one, one, one, one, 1, 0.0, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
