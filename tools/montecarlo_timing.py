"""What the Monte-Carlo audit costs, on the headline configuration of bench.py (rocket landing, N = 100, its Nsub, 4 096
Monte-Carlo instances) after a converged PTR run on ONE handle, the batch and the LQR gains resident, steps = 2 Nsub per interval
as in tools/lqr_tracking_timing.py.  Wall time, median of 10 after 2 warm-ups, the stream drained by every call:
  (a) scp_audit_montecarlo_resident at D = 64 (moments and stat come back, no flight records) against
      scp_audit_tracking_resident at the same D and steps, zero dispersions, IN THE SAME BUILD: the ratio of the libraries' own
      device seconds is the price of the draws and the cross-flight reductions;
  (b) the same at D = 256;
  (c) what a user has today for per-node noise is nothing on the device; had they the node errors of every flight on the host
      (an array [D, N, nx] per problem, which no entry point returns), the moments would be numpy's mean / std / rms over the
      flights.  Only that numpy time is reported: on arrays of the right shape for 8 problems, filled with standard normals
      scaled by the sigmas (the time does not depend on the values), scaled to the batch.  It is a lower bound of the host
      alternative: it contains no flight and no copy.
Prints one JSON line (and writes it to the file given as the first argument).  No ratio is asserted: the file holds whatever the
device gives."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audit_timing import REPS, WARMUP, median_wall  # noqa: E402

SEED = 2026


def numpy_moments(E, U):
    """E[P, D, N, nx], U[P, D, N-1, nu] -> the node records [P, N, 1 + 2 nx + nu] of include/scp_mi355x.h"""
    P, D, N, nx = E.shape
    out = np.full((P, N, 1 + 2 * nx + U.shape[3]), np.nan)
    out[:, :, 0] = D
    out[:, :, 1:1 + nx] = E.mean(axis=1)
    out[:, :, 1 + nx:1 + 2 * nx] = E.std(axis=1, ddof=1)
    out[:, :-1, 1 + 2 * nx:] = np.sqrt((U * U).mean(axis=1))
    return out


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
    ok = np.array([str(st).startswith("SCP_SOLVED") for st in sol.status])
    steps = 2 * Nsub
    sig0, sigu, sigw = 0.01 * pbm.scale.Sx, 0.01 * pbm.scale.Su, 0.002 * pbm.scale.Sx
    g = pkg.lqr_gains_resident(pbm)
    kern = {}

    def run(key, fn):
        kern[key] = []

        def call():
            a = fn()
            kern[key].append(a.seconds)
            return a
        t, tmin, a = median_wall(call)
        return dict(wall_s=t, min_s=tmin, kernel_s=float(np.median(kern[key][WARMUP:]))), a

    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run; gains resident, steps=%d" % (model, N, Nsub, B, steps),
               solved=int(ok.sum()), gain_failures=int(np.nansum(g.info[:, 0])), reps=REPS, warmup=WARMUP, seed=SEED)
    for D in (64, 256):
        zero = (np.zeros((D, pbm.nx)), np.ones((D, pbm.nu)), np.zeros((D, pbm.nu)))
        t_mc, a = run("mc%d" % D, lambda: pkg.audit_montecarlo_resident(pbm, None, steps, sig0, sigu, sigw, D, SEED))
        t_tr, tr = run("tr%d" % D, lambda: pkg.audit_tracking_resident(pbm, None, steps, *zero, shared=True))
        # once more, so that a drift of the machine shows as a difference between the passes
        t_mc2, _ = run("mc%d_2" % D, lambda: pkg.audit_montecarlo_resident(pbm, None, steps, sig0, sigu, sigw, D, SEED))
        t_tr2, _ = run("tr%d_2" % D, lambda: pkg.audit_tracking_resident(pbm, None, steps, *zero, shared=True))
        cov = pkg.audit_covariance_resident(pbm, None, sig0, sigu, sigw, per_node=True)
        c = a.compare(cov)
        out["D%d" % D] = dict(montecarlo_resident=t_mc, tracking_resident_same_D_and_steps=t_tr,
                              ratio_kernel=t_mc["kernel_s"] / t_tr["kernel_s"], ratio_wall=t_mc["wall_s"] / t_tr["wall_s"],
                              second_pass=dict(montecarlo_resident=t_mc2, tracking_resident_same_D_and_steps=t_tr2,
                                               ratio_kernel=t_mc2["kernel_s"] / t_tr2["kernel_s"]),
                              bytes_to_host=int(a.raw.nbytes + a.stat.nbytes + a.moments.nbytes),
                              nonfinite_flights=int(np.nansum(a.n_nonfinite)), n_min=float(np.nanmin(a.n_min)),
                              std_over_sig_min=float(np.nanmin(c.ratio_min)), std_over_sig_max=float(np.nanmax(c.ratio_max)),
                              std_over_sig_median=float(np.nanmedian(c.ratio)), z_mean_max=float(np.nanmax(c.z_mean)))
    # (c) numpy moments over node errors that are already on the host, 8 problems, scaled to the batch
    P, D = 8, 64
    rng = np.random.default_rng(SEED)
    E = sig0 * rng.standard_normal((P, D, N, pbm.nx))
    U = 0.01 * rng.standard_normal((P, D, N - 1, pbm.nu))
    ts = []
    for _ in range(WARMUP + REPS):
        t0 = time.perf_counter()
        numpy_moments(E, U)
        ts.append(time.perf_counter() - t0)
    t8 = float(np.median(ts[WARMUP:]))
    out["c_numpy_moments_only"] = dict(problems=P, D=D, seconds_for_8=t8, scaled_to_batch_s=t8 * B / P,
                                       node_error_bytes_per_batch=int(8 * D * N * pbm.nx * B),
                                       ratio_to_montecarlo_wall=t8 * B / P / out["D64"]["montecarlo_resident"]["wall_s"])
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
