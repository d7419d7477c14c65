"""What the device-resident continuation saves on the oscillator's deadband homotopy: the reference's ten-stage run
(oscillator/tests.jl:22-93: N = 30, Nsub = 10, kappa1 = Homotopy(1e-8)(LinRange(0, 1, 10))) on a Monte-Carlo batch of 4 096
instances (r0 in [0.15, 1], v0 in [-0.2, 0.2], seeded), on ONE handle, two ways:
  (c) PTR.solve_homotopy: set_model_par + scp_ptr_generic_continue between the stages; nothing is uploaded after the first
      stage and an intermediate stage reads back 44 bytes per instance (status, iterations, costs);
  (h) a host warm restart per stage: set_model_par, then PTR.solve(pbm, pp, warm = the previous stage's arrays), i.e. get_host
      of the whole batch + init_host with it.
Both start from the model's guess made on the device (scp_guess_batch_host), inside the timed run.  Wall time of the whole ten-stage run
(it ends in a get_host, which drains the stream), median of 10 after one warm-up, the two
variants alternated run by run so that a drift of the machine falls on both.  Prints one JSON line (and writes it to the file
given as the first argument).  No ratio is asserted: the file holds whatever the device gives.

    python tools/oscillator_homotopy_timing.py [out.json] [batch = 4096]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARMUP = 10, 1      # a run lasts 40 s at this size: one warm-up (template, symbolic analysis, code objects), ten timed


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    N, Nsub, S = 30, 10, 10
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    hom = pkg.Homotopy(1e-8)
    kappas = [hom(x) for x in np.linspace(0.0, 1.0, S)]
    traj = pkg.TrajectoryProblem("oscillator")
    pars = pkg.PTR.Parameters(N=N, Nsub=Nsub, iter_max=10, wvc=1e2, wtr=1e-3, eps_abs=-np.inf, eps_rel=1e-3 / 100, feas_tol=5e-3)
    pbm = pkg.PTR.create(pars, traj, batch_capacity=B)
    rng = np.random.default_rng(0)
    pp = np.stack([rng.uniform(0.15, 1.0, B), rng.uniform(-0.2, 0.2, B)], axis=1)

    def by_continue():
        return pkg.PTR.solve_homotopy(pbm, "kappa1", kappas, pp=pp)

    def by_host_restart():
        warm, its = pkg.device_guess(pbm, pp), []      # the same device guess solve_homotopy starts from
        for kap in kappas:
            pbm.set_model_par(kappa1=kap)
            sol, hist = pkg.PTR.solve(pbm, pp, warm=warm)
            warm = (sol.xd, sol.ud, sol.p)
            its.append(sol.iterations)
        return sol, hist, dict(iterations=np.array(its))

    # the two variants alternate run by run, so that a drift of the machine falls on both alike
    ts, last = {"c": [], "h": []}, {}
    for i in range(WARMUP + REPS):
        for key, fn in (("c", by_continue), ("h", by_host_restart)):
            t0 = time.perf_counter()
            last[key] = fn()
            ts[key].append(time.perf_counter() - t0)
            print("%s run %d: %.3f s" % (fn.__name__, i, ts[key][-1]), file=sys.stderr, flush=True)
    t_c, min_c, t_h, min_h = (float(f(ts[k][WARMUP:])) for k in ("c", "h") for f in (np.median, np.min))
    (sol_c, _, sum_c), (sol_h, _, sum_h) = last["c"], last["h"]
    per_stage = 8 * (pbm.nx * N + pbm.nu * N + pbm.np) * B
    out = dict(workload="oscillator deadband homotopy N=%d Nsub=%d, %d stages, batch %d" % (N, Nsub, S, B), reps=REPS, warmup=WARMUP,
               c_continue_wall_s=t_c, c_min_s=min_c, h_host_restart_wall_s=t_h, h_min_s=min_h,
               c_runs_s=ts["c"], h_runs_s=ts["h"],
               solved_last_stage=int(sum(st == "SCP_SOLVED" for st in sol_c.status)), solved_every_stage=int((sum_c["status"] == 0).all(axis=0).sum()),
               ptr_iterations_total=int(sum_c["iterations"].max(axis=1).sum()), ptr_iterations_per_stage=sum_c["iterations"].max(axis=1).tolist(),
               same_iterations_both_ways=bool((sum_c["iterations"] == sum_h["iterations"]).all()),
               same_trajectories_both_ways=bool(sol_c.xd.tobytes() == sol_h.xd.tobytes() and sol_c.ud.tobytes() == sol_h.ud.tobytes()),
               trajectory_bytes_per_stage_each_direction=int(per_stage), J_median=float(np.median(sol_c.J)))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
