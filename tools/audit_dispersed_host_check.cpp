// Stand-alone sanitizer check of the host twin of the dispersed-flight audit (scp_model_audit_dispersed_host,
// csrc/audit_api.hip): the bodies the device kernels run, on heap arrays of EXACTLY the documented sizes, for the rocket landing
// and the quadrotor, N in {2, 9}, D in {1, 3}, with and without the flight records and the truth model.  Not a pytest and not
// loaded into Python.  Built and run by `make -C tools host-checks` (see tools/Makefile, HOST_CHECK_UNITS).
//
// Exit status 0 and one line per call when every call returned SCP_OK with finite, flag-free records whose summary is the same
// with and without the flight records.
#include "host_check.hpp"

int main()
{
    for (int id : {SCP_MODEL_ROCKET_LANDING, SCP_MODEL_QUADROTOR}) {
        const Model& c = models()[id];
        for (int N : {2, 9}) {
            for (int D : {1, 3}) {
                for (int truth = 0; truth < 2; truth++) {
                    const int res = 6 * (N - 1) + 1;
                    std::vector<double> xd, ud;
                    straight_line(c, N, xd, ud);
                    std::vector<double> dx0((size_t)c.nx * D), gain((size_t)c.nu * D), bias((size_t)c.nu * D);
                    for (int d = 0; d < D; d++) {
                        for (int i = 0; i < c.nx; i++) dx0[(size_t)d * c.nx + i] = 0.01 * d * c.Sx[i] * std::sin(1.0 + i + d);
                        for (int i = 0; i < c.nu; i++) {
                            gain[(size_t)d * c.nu + i] = 1.0 + 0.02 * d * std::cos(2.0 + i);
                            bias[(size_t)d * c.nu + i] = 0.01 * d * std::sin(3.0 + i);
                        }
                    }
                    std::vector<double> par(c.par), pt(c.par_true), p(c.p), pp(c.pp), Sx(c.Sx);
                    std::vector<double> sum(SCP_AUDIT_WIDTH, -7.0), only(SCP_AUDIT_WIDTH, -8.0), rec((size_t)SCP_AUDIT_WIDTH * D, -9.0);
                    const double* ptrue = truth ? pt.data() : nullptr;
                    const int rc = scp_model_audit_dispersed_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                  Sx.data(), res, 0.0, D, dx0.data(), gain.data(), bias.data(), sum.data(),
                                                                  rec.data());
                    const int rc2 = scp_model_audit_dispersed_host(c.id, par.data(), ptrue, N, xd.data(), ud.data(), p.data(), pp.data(),
                                                                   Sx.data(), res, 0.0, D, dx0.data(), gain.data(), bias.data(), only.data(),
                                                                   nullptr);
                    bool fin = rc == SCP_OK && rc2 == SCP_OK && sum[11] == 0.0 && sum[13] == 2.0 && sum[14] == (double)D;
                    for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(sum[i]) && sum[i] == only[i];
                    for (int d = 0; d < D; d++)
                        for (int i = 6; i < SCP_AUDIT_WIDTH; i++) fin = fin && std::isfinite(rec[(size_t)d * SCP_AUDIT_WIDTH + i]);
                    std::printf("%-15s N %d D %d truth %d rc %d  s %.6g#%g lin %.6g#%g soc %.6g#%g bc %.6g#%g drift %.6g cost %.6g..%.6g nviol %g%s\n",
                                c.name, N, D, truth, rc, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[7], sum[12], sum[8], sum[9],
                                sum[15], sum[10], fin ? "" : "   <-- BAD");
                    bad += fin ? 0 : 1;
                }
            }
        }
    }
    // NULL dispersion arrays, and the refusals, which touch no array
    {
        const Model& c = models()[SCP_MODEL_QUADROTOR];
        const int N = 2;
        std::vector<double> xd(c.x0), ud(c.u), sum(SCP_AUDIT_WIDTH, -7.0);
        xd.insert(xd.end(), c.xf.begin(), c.xf.end());
        ud.insert(ud.end(), c.u.begin(), c.u.end());
        if (scp_model_audit_dispersed_host(c.id, c.par.data(), nullptr, N, xd.data(), ud.data(), c.p.data(), c.pp.data(), c.Sx.data(), 5, 0.0, 2,
                                           nullptr, nullptr, nullptr, sum.data(), nullptr) != SCP_OK || sum[11] != 0.0 || sum[14] != 2.0) bad++;
    }
    if (scp_model_audit_dispersed_host(SCP_MODEL_FREEFLYER, one, nullptr, 5, one, one, one, one, one, 4, 0.0, 1, one, one, one, one, one) != SCP_ERR_UNSUPPORTED) bad++;
    if (scp_model_audit_dispersed_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, 4, 0.0, 0, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    if (scp_model_audit_dispersed_host(SCP_MODEL_QUADROTOR, one, nullptr, 5, one, one, one, one, one, 1, 0.0, 1, one, one, one, one, one) != SCP_ERR_BAD_ARGUMENT) bad++;
    return verdict();
}
