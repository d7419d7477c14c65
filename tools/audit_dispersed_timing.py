"""What the dispersed-flight audit costs against the single-shooting audit of the same build, on the headline configuration of
bench.py (rocket landing, N = 100, its Nsub, 4 096 Monte-Carlo instances, res = 2 Nsub (N - 1)) after a converged PTR run on ONE
handle, the batch resident.  Wall time, median of 10 after 2 warm-ups, the stream drained by every call:
  (a) scp_audit_resident: one thread per problem, one nominal flight each;
  (b) scp_audit_dispersed_resident at D = 1, 16 and 64 without the flight records: one thread per (problem, flight), then the
      ordered fold; the dispersions [B, D, .] go up, 16 B doubles come back;
  (c) D = 16 with the flight records: 16 D B doubles more;
  (d) what a user did before: 16 `audit` calls, each on a host-perturbed copy of the solution (the same 16 dispersions), every
      copy uploaded again.  The single-shooting audit is untouched by the dispersed one, so this is its cost as it was.
(d) stages its copies in the handle's solution buffers and therefore runs last.  Prints one JSON line (and writes it to the file
given as the first argument): the medians, the device time of the kernels from the library's own event timer, the bytes each
variant moves.  No ratio is asserted: the file holds whatever the device gives."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audit_timing import REPS, WARMUP, median_wall  # noqa: E402

DS = (1, 16, 64)


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
    rng = np.random.default_rng(0)
    ub = traj.mdl.scale_advice()[1]
    dmax = max(DS)
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((B, dmax, pbm.nx))
    gain = 1.0 + 0.02 * rng.standard_normal((B, dmax, pbm.nu))
    bias = 0.01 * (ub[:, 1] - ub[:, 0]) * rng.standard_normal((B, dmax, pbm.nu))
    dx0[:, 0], gain[:, 0], bias[:, 0] = 0.0, 1.0, 0.0
    disp = {d: tuple(np.ascontiguousarray(a[:, :d]) for a in (dx0, gain, bias)) for d in DS}
    kern = {}

    def run(key, fn):
        kern[key] = []

        def call():
            a = fn()
            kern[key].append(a.seconds)
            return a
        t, tmin, a = median_wall(call)
        return dict(wall_s=t, min_s=tmin, kernel_s=float(np.median(kern[key][WARMUP:]))), a

    def today():
        """16 audits of host-perturbed copies; .seconds = the sum of the 16 kernels"""
        x0, g, b = disp[16]
        recs, sec = [], 0.0
        for d in range(16):
            xd = sol.xd.copy()
            xd[:, 0] += x0[:, d]
            ud = sol.ud * g[:, d][:, None, :] + b[:, d][:, None, :]
            a = pkg.audit(SimpleNamespace(xd=xd, ud=ud, p=sol.p, status=sol.status), pbm, pp=pp, res=res, viol_tol=0.0)
            recs.append(a.raw)
            sec += a.seconds
        return SimpleNamespace(seconds=sec, raw=np.stack(recs, axis=1))

    dispersed = lambda d, fl: (lambda: pkg.audit_dispersed_resident(pbm, *disp[d], res=res, viol_tol=0.0, flights=fl))      # noqa: E731
    t_a, a_a = run("a", lambda: pkg.audit_resident(pbm, res=res, viol_tol=0.0))
    t_b, a_b = {}, {}
    for d in DS:
        t_b[d], a_b[d] = run("b%d" % d, dispersed(d, False))
    t_c, a_c = run("c", dispersed(16, True))
    # alternate the variants once more after the first pass, so that a drift of the machine shows as a difference between the passes
    t_a2, _ = run("a2", lambda: pkg.audit_resident(pbm, res=res, viol_tol=0.0))
    t_b2 = {d: run("b%d_2" % d, dispersed(d, False))[0] for d in DS}
    t_d, a_d = run("d", today)
    live = ok & (a_c.n_nonfinite == 0)
    dev = np.abs(a_d.raw[live][:, :, 7:10] - a_c.flights[live][:, :, 7:10]).max() if live.any() else None
    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run, res=%d" % (model, N, Nsub, B, res),
               solved=int(ok.sum()), reps=REPS, warmup=WARMUP,
               a_audit_resident=t_a, a_bytes_to_host=int(a_a.raw.nbytes),
               b_dispersed_resident={str(d): t_b[d] for d in DS},
               b_bytes_to_device={str(d): int(sum(x.nbytes for x in disp[d])) for d in DS}, b_bytes_to_host=int(a_b[1].raw.nbytes),
               c_dispersed_16_with_records=t_c, c_bytes_to_host=int(a_c.raw.nbytes + a_c.flights.nbytes),
               d_sixteen_audit_calls=t_d, d_bytes_to_device=int(16 * (sol.xd.nbytes + sol.ud.nbytes + sol.p.nbytes + pp.nbytes)),
               second_pass=dict(a_audit_resident=t_a2, b_dispersed_resident={str(d): t_b2[d] for d in DS}),
               threads={"a": B, **{"b%d" % d: B * d for d in DS}}, steps_per_thread=res - 1,
               flight_1_of_D1_equals_flight_1_of_D16=bool(a_b[1].raw[ok][:, [0, 2, 4, 7, 8, 9]].tobytes()
                                                          == a_c.flights[ok][:, 0][:, [0, 2, 4, 7, 8, 9]].tobytes()),
               summaries_equal_with_and_without_records=bool(a_b[16].raw.tobytes() == a_c.raw.tobytes()),
               largest_difference_d_vs_c_fields_7_to_9=None if dev is None else float(dev),
               flights_violating_per_problem_mean=float(np.mean(a_c.n_violating[ok])) if ok.any() else None,
               nonfinite_flights=int(np.nansum(a_c.n_nonfinite)))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
