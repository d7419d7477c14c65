// Stand-alone sanitizer check of the host twin of the continuous-time audit (scp_model_audit_host, csrc/audit_api.hip): the body
// the device kernel runs, on heap arrays of EXACTLY the documented sizes, for the four supported models.  Not a pytest and not
// loaded into Python.  Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per model when every call returned SCP_OK with a finite, flag-free record.
#include "host_check.hpp"

static std::vector<double> heap(const std::vector<double>& v) { return std::vector<double>(v.begin(), v.end()); }

int main()
{
    for (const Model& c : models()) {
        const int N = 9;
        for (int res : {2, 4 * (N - 1) + 1, 2 * 15 * (N - 1)}) {
            std::vector<double> xd, ud;
            straight_line(c, N, xd, ud);
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
    if (scp_model_audit_host(SCP_MODEL_FREEFLYER, one, 5, one, one, one, one, one, 4, 0.0, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_host(SCP_MODEL_QUADROTOR, one, 5, one, one, one, one, one, 1, 0.0, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    return verdict();
}
