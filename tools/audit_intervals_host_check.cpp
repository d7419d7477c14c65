// Stand-alone sanitizer check of the host twin of the interval-parallel audit (scp_model_audit_intervals_host,
// csrc/audit_api.hip): the bodies the device kernels run, on heap arrays of EXACTLY the documented sizes, for a FOH case
// (rocket landing) and an IMPULSE case (quadrotor), with and without the interval records.  Not a pytest and not loaded into
// Python.  Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per call when every call returned SCP_OK with finite, flag-free records.
#include <string>

#include "host_check.hpp"

int main()
{
    const struct { int id, method; const char* form; } cases[] = {{SCP_MODEL_ROCKET_LANDING, SCP_FOH, " FOH"}, {SCP_MODEL_QUADROTOR, SCP_IMPULSE, " IMPULSE"}};
    for (const auto& cs : cases) {
        const Model& c = models()[cs.id];
        const std::string name = std::string(c.name) + cs.form;
        for (int N : {2, 9}) {
            for (int res : {2, 3 * (N - 1), 6 * (N - 1) + 1}) {
                std::vector<double> xd, ud;
                straight_line(c, N, xd, ud);
                std::vector<double> par(c.par), p(c.p), pp(c.pp), Sx(c.Sx), audit(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0);
                std::vector<double> rec((size_t)SCP_AUDIT_INTERVAL_WIDTH * (N - 1), -9.0);
                const int rc = scp_model_audit_intervals_host(c.id, par.data(), N, cs.method, xd.data(), ud.data(), p.data(), pp.data(),
                                                              Sx.data(), res, 0.0, audit.data(), rec.data());
                const int rc2 = scp_model_audit_intervals_host(c.id, par.data(), N, cs.method, xd.data(), ud.data(), p.data(), pp.data(),
                                                               Sx.data(), res, 0.0, only.data(), nullptr);
                bool fin = rc == SCP_OK && rc2 == SCP_OK && audit[11] == 0.0 && audit[13] == 1.0;
                for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(audit[i]) && audit[i] == only[i];
                for (int k = 0; k < N - 1; k++)
                    for (int i = 6; i < SCP_AUDIT_INTERVAL_WIDTH; i++) fin = fin && std::isfinite(rec[(size_t)k * SCP_AUDIT_INTERVAL_WIDTH + i]);
                std::printf("%-20s N %d res %3d rc %d  s %.6g@%.3f lin %.6g@%.3f soc %.6g@%.3f bc %.6g defect %.6g@%g cost %.6g nviol %g sub %g%s\n",
                            name.c_str(), N, res, rc, audit[0], audit[1], audit[2], audit[3], audit[4], audit[5], audit[7], audit[8], audit[12],
                            audit[9], audit[10], audit[14], fin ? "" : "   <-- BAD");
                bad += fin ? 0 : 1;
            }
        }
    }
    // the refusals touch no array
    if (scp_model_audit_intervals_host(SCP_MODEL_FREEFLYER, one, 5, SCP_FOH, one, one, one, one, one, 4, 0.0, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_intervals_host(SCP_MODEL_ROCKET_LANDING, one, 5, SCP_IMPULSE, one, one, one, one, one, 4, 0.0, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_intervals_host(SCP_MODEL_QUADROTOR, one, 5, SCP_FOH, one, one, one, one, one, 1, 0.0, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    return verdict();
}
