"""What the interval-parallel audit costs against the single-shooting audit of the same build, on the headline configuration of
bench.py (rocket landing, N = 100, its Nsub, 4 096 Monte-Carlo instances, res = 2 Nsub (N - 1), hence sub = 30) after a converged
PTR run on ONE handle, the batch resident.  Wall time, median of 10 after 2 warm-ups, the stream drained by every call:
  (s) scp_audit_resident: one thread per problem, res - 1 serial RK4 steps each, 16 B doubles come back;
  (m) scp_audit_intervals_resident without the interval records: one thread per (problem, interval), sub - 1 steps each, then the
      ordered fold; 16 B doubles come back;
  (i) the same with the interval records: 16 (N - 1) B doubles more.
Prints one JSON line (and writes it to the file given as the first argument): the three medians, the device time of the kernels
from the library's own event timer, the bytes each variant moves, and the batch's largest defect next to the single-shooting
drift.  No ratio is asserted: the file holds whatever the device gives."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audit_timing import REPS, WARMUP, median_wall  # noqa: E402


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    import bench
    pkg = graft.load_package()
    model, N, Nsub, iters, B = bench.WORKLOADS["rocket_landing"]
    if len(sys.argv) > 2:
        B = int(sys.argv[2])
    traj = pkg.TrajectoryProblem(model)
    pars = pkg.PTR.Parameters(N=N, Nsub=Nsub, iter_max=iters, wvc=1e3, wtr=0.1, eps_abs=1e-5, eps_rel=1e-4, feas_tol=1e-3)
    pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
    pp = bench.mc_pp(traj.mdl, B, 0)
    sol, _ = pkg.PTR.solve(pbm, pp, device_guess=True)
    res = 2 * Nsub * (N - 1)
    ok = np.array([str(st).startswith("SCP_SOLVED") for st in sol.status])      # the audit's own mask (scp.py)
    kern = {"s": [], "m": [], "i": []}

    def run(key, fn):
        def call():
            a = fn()
            kern[key].append(a.seconds)
            return a
        t, tmin, a = median_wall(call)
        return t, tmin, float(np.median(kern[key][WARMUP:])), a
    # alternate the variants once more after the first pass, so that a drift of the machine shows as a difference between the passes
    t_s, min_s, k_s, a_s = run("s", lambda: pkg.audit_resident(pbm, res=res, viol_tol=0.0))
    t_m, min_m, k_m, a_m = run("m", lambda: pkg.audit_intervals_resident(pbm, res=res, viol_tol=0.0, intervals=False))
    t_i, min_i, k_i, a_i = run("i", lambda: pkg.audit_intervals_resident(pbm, res=res, viol_tol=0.0, intervals=True))
    t_s2, _, k_s2, _ = run("s", lambda: pkg.audit_resident(pbm, res=res, viol_tol=0.0))
    t_m2, _, k_m2, _ = run("m", lambda: pkg.audit_intervals_resident(pbm, res=res, viol_tol=0.0, intervals=False))
    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run, res=%d, sub=%d" % (model, N, Nsub, B, res, a_m.sub),
               solved=int(ok.sum()), reps=REPS, warmup=WARMUP,
               s_audit_resident_wall_s=t_s, s_min_s=min_s, s_kernel_s=k_s, s_bytes_to_host=int(a_s.raw.nbytes),
               m_intervals_resident_wall_s=t_m, m_min_s=min_m, m_kernels_s=k_m, m_bytes_to_host=int(a_m.raw.nbytes),
               i_with_records_wall_s=t_i, i_min_s=min_i, i_kernels_s=k_i, i_bytes_to_host=int(a_i.raw.nbytes + a_i.intervals.nbytes),
               second_pass=dict(s_wall_s=t_s2, s_kernel_s=k_s2, m_wall_s=t_m2, m_kernels_s=k_m2),
               threads_single=B, threads_intervals=B * (N - 1), steps_single=res - 1, steps_intervals=a_m.sub - 1,
               summaries_equal_with_and_without_records=bool(a_m.raw.tobytes() == a_i.raw.tobytes()),
               largest_defect_of_the_solved=float(np.max(a_m.defect[ok])) if ok.any() else None,
               largest_single_shooting_drift_of_the_solved=float(np.max(a_s.drift[ok])) if ok.any() else None,
               nonfinite=int(np.nansum(a_m.nonfinite)), summary=a_m.summary(tol_con=1e-6, tol_bc=1e-3))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
