// Stand-alone sanitizer check of the host twin of the continuous-time audit (scp_model_audit_host, csrc/audit_api.hip): the body
// the device kernel runs, on heap arrays of EXACTLY the documented sizes, for the four supported models.  Not a pytest and not
// loaded into Python.  Build and run from the repository root (host code only; no GPU is needed or used):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/audit_host_check.cpp scptoolbox.jl_amd/csrc/audit_api.hip -o build/audit_host_check && build/audit_host_check
//
// Exit status 0 and one line per model when every call returned SCP_OK with a finite, flag-free record.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/scp_mi355x.h"

struct Case {
    const char* name;
    int id, nx, nu, np, npp;
    std::vector<double> par, x0, xf, u, p, pp, Sx;
};

static std::vector<double> heap(const std::vector<double>& v) { return std::vector<double>(v.begin(), v.end()); }

int main()
{
    const double d2r = 3.14159265358979323846 / 180.0;
    std::vector<Case> cases;
    cases.push_back({"double_integrator", SCP_MODEL_DOUBLE_INTEGRATOR, 2, 1, 0, 4, {0.1, 10.0}, {0, 0}, {47, 0}, {1.5}, {}, {0, 0, 47, 0}, {47, 9.4}});
    cases.push_back({"quadrotor", SCP_MODEL_QUADROTOR, 6, 4, 1, 12,
                     {9.81, 0.6, 23.2, 60 * d2r, 0.0, 2.5, 0.0, 2, 2, 0, 1, 2, 0, 1.5, 1.5, 0, 2, 5, 0},
                     {0, 0, 0, 0, 0, 0}, {2.5, 6, 0, 0, 0, 0}, {0.1, -0.2, 9.81, 9.9}, {1.25}, {0, 0, 0, 0, 0, 0, 2.5, 6, 0, 0, 0, 0},
                     {1, 1, 1, 1, 1, 1}});
    cases.push_back({"rocket_landing", SCP_MODEL_ROCKET_LANDING, 7, 4, 1, 6,
                     {0, 0, -3.7114, 6.1e-5, 0, 3.5e-5, 5.1e-4, 1505, 1905, 4972, 13258, 86 * d2r, 40 * d2r, 138.9, 40, 120, 1},
                     {2000, 0, 1500, 80, 30, -75, std::log(1905.0)}, {0, 0, 0, 0, 0, 0, std::log(1505.0)}, {0.1, 0.1, 3.7, 3.9}, {75},
                     {2000, 0, 1500, 80, 30, -75}, {5000, 5000, 2500, 278, 278, 278, 0.24}});
    cases.push_back({"starship", SCP_MODEL_STARSHIP, 8, 3, 10, 5,
                     {9, 100, 9.81, 120e3, 0.4, 0.45, 2.5e7, 0.2, 880e3, 2210e3, 2640e3, 6630e3, -3.1e-4, 10 * d2r, 20 * d2r, 0.05, 0, 40, 0.5,
                      27 * d2r, 15 * d2r, 0, -0.1, 0.3, 10e3},
                     {100, 600, 0, -85, 90 * d2r, 0, 0, 0}, {0, 0, 0, -0.1, 0, 0, -3e3, 0}, {2.7e6, 0.02, 0.01},
                     {1.0, 1.0, 50, 300, 0, -42, 0.8, 0, -1500, 0}, {100, 600, 0, -85, 90 * d2r}, {200, 600, 20, 85, 1.6, 0.35, 1e3, 0.35}});
    int bad = 0;
    for (const Case& c : cases) {
        const int N = 9;
        for (int res : {2, 4 * (N - 1) + 1, 2 * 15 * (N - 1)}) {
            std::vector<double> xd((size_t)c.nx * N), ud((size_t)c.nu * N);
            for (int k = 0; k < N; k++) {
                const double t = (double)k / (N - 1);
                for (int i = 0; i < c.nx; i++) xd[(size_t)k * c.nx + i] = (1 - t) * c.x0[i] + t * c.xf[i];
                for (int i = 0; i < c.nu; i++) ud[(size_t)k * c.nu + i] = c.u[i] * (1.0 + 0.05 * std::sin(3.0 * k + i));
            }
            std::vector<double> par = heap(c.par), p = heap(c.p), pp = heap(c.pp), Sx = heap(c.Sx), audit(SCP_AUDIT_WIDTH, -7.0);
            const int rc = scp_model_audit_host(c.id, par.data(), N, xd.data(), ud.data(), c.np ? p.data() : nullptr, pp.data(), Sx.data(),
                                                res, 0.0, audit.data());
            bool fin = rc == SCP_OK && audit[11] == 0.0;
            for (int i = 7; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(audit[i]);
            std::printf("%-18s res %3d rc %d  s %.6g@%.3f lin %.6g@%.3f soc %.6g@%.3f par %.6g bc %.6g drift %.6g cost %.6g nviol %g flag %g%s\n", c.name,
                        res, rc, audit[0], audit[1], audit[2], audit[3], audit[4], audit[5], audit[6], audit[7], audit[8], audit[9], audit[10],
                        audit[11], fin ? "" : "   <-- BAD");
            bad += fin ? 0 : 1;
        }
    }
    // the refusals touch no array
    double one[SCP_AUDIT_WIDTH] = {0};
    if (scp_model_audit_host(SCP_MODEL_FREEFLYER, one, 5, one, one, one, one, one, 4, 0.0, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_host(SCP_MODEL_QUADROTOR, one, 5, one, one, one, one, one, 1, 0.0, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
