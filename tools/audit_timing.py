"""What the continuous-time audit costs against what it replaces, on the headline configuration of bench.py (rocket landing,
N = 100, its Nsub, 4 096 Monte-Carlo instances, res = 2 Nsub (N - 1)) after a converged PTR run on ONE handle.  Wall time, median
of 10 after 2 warm-ups, the stream drained by every call:
  (a) scp_propagate_batch_host alone: nx res B doubles allocated on the device and copied to the host (the yardstick);
  (b) (a) plus the numpy evaluation of the same record from those samples;
  (c) scp_audit_resident: 16 B doubles come back.
Prints one JSON line (and writes it to the file given as the first argument): the three medians, the kernel / copy split of (c)
from the library's own device timer, the bytes each variant moves, and how far (b)'s record is from (c)'s."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REPS, WARMUP = 10, 2


def numpy_record(pkg, pbm, sol, pp, tc, xc):
    """the audit record of the rocket-landing batch from the samples xc[B, res, nx] (vectorised numpy, one pass)"""
    mdl, N = pbm.traj.mdl, pbm.pars.N
    B, res, nx = xc.shape
    mr = pkg.subproblem.ModelRows(mdl)
    tg = pbm.t_grid
    k = np.clip(np.searchsorted(tg, tc, side="left"), 1, N - 1)
    c = (tg[k] - tc) / (tg[k] - tg[k - 1])
    uc = c[None, :, None] * sol.ud[:, k - 1] + (1.0 - c)[None, :, None] * sol.ud[:, k]
    z = np.concatenate([xc, uc], axis=2)
    rec = np.zeros((B, 16))
    ez = np.exp(-xc[:, :, 6])
    s = np.stack([mdl.rho_min * ez - uc[:, :, 3], uc[:, :, 3] - mdl.rho_max * ez], axis=2).max(axis=2)
    L0, _, l0, Mm, m = mr.rows(N, 1)
    LN, _, lN, _, _ = mr.rows(N, N)                               # the rows of t = 1 (the last sample only)
    lin = (z @ L0.T + l0).max(axis=2)
    lin[:, -1] = (z[:, -1] @ LN.T + lN).max(axis=1)
    w = z @ Mm.T + m
    soc = np.stack([np.linalg.norm(w[:, :, 4 * i + 1:4 * i + 4], axis=2) - w[:, :, 4 * i] for i in range(mr.nsoc)], axis=2).max(axis=2)
    for f, v in enumerate((s, lin, soc)):
        j = v.argmax(axis=1)
        rec[:, 2 * f], rec[:, 2 * f + 1] = v[np.arange(B), j], tc[j]
    Lg, lg = mr.global_rows(N)
    rec[:, 6] = (sol.p @ Lg.T + lg).max(axis=1)
    xf = xc[:, -1]
    rec[:, 7] = np.abs(xf[:, 0:6]).max(axis=1)
    rec[:, 8] = np.abs((xf - sol.xd[:, -1]) / pbm.scale.Sx).max(axis=1)
    ct = mr.cost_terms(N)
    gam = (uc * uc) @ ct["Qu"] + uc @ ct["lu"] + xc @ ct["lx"]
    rec[:, 9] = xf @ ct["tx"] + sol.p @ ct["tp"] + (sol.p * sol.p) @ ct["Qp"] + (0.5 * np.diff(tc)[None, :] * (gam[:, 1:] + gam[:, :-1])).sum(axis=1)
    rec[:, 10] = (np.maximum(np.maximum(s, lin), soc) > 0.0).sum(axis=1)
    rec[:, 11] = (~np.isfinite(z).all(axis=(1, 2))).astype(float)
    return rec


def median_wall(fn):
    ts = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[WARMUP:])), float(np.min(ts[WARMUP:])), out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft     # here, not at module level: numpy_record is imported by a CPU test
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
    ok = np.array([st == "SCP_SOLVED" for st in sol.status])
    # (c) first: the run is still resident (the propagate call below stages its input in the solution buffers -- the same data)
    kernel = []

    def run_c():
        a = pkg.audit_resident(pbm, res=res, viol_tol=0.0)
        kernel.append(a.seconds)
        return a
    t_c, tmin_c, a = median_wall(run_c)
    t_a, tmin_a, (tc, xc) = median_wall(lambda: pkg.propagate(sol, pbm, res=res))

    def run_b():
        tc_, xc_ = pkg.propagate(sol, pbm, res=res)
        return numpy_record(pkg, pbm, sol, pp, tc_, xc_)
    t_b, tmin_b, rec = median_wall(run_b)
    k_c = float(np.median(kernel[WARMUP:]))
    scale = np.maximum(1.0, np.abs(rec[ok]))
    dev = np.abs(a.raw[ok][:, [0, 2, 4, 6, 7, 8, 9]] - rec[ok][:, [0, 2, 4, 6, 7, 8, 9]]) / scale[:, [0, 2, 4, 6, 7, 8, 9]]
    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run, res=%d" % (model, N, Nsub, B, res), solved=int(ok.sum()),
               reps=REPS, warmup=WARMUP,
               a_propagate_wall_s=t_a, a_min_s=tmin_a, a_bytes_to_host=int(xc.nbytes), a_device_bytes_allocated=int(xc.nbytes),
               b_propagate_plus_numpy_wall_s=t_b, b_min_s=tmin_b,
               c_audit_resident_wall_s=t_c, c_min_s=tmin_c, c_kernel_s=k_c, c_copy_and_sync_s=t_c - k_c, c_bytes_to_host=int(a.raw.nbytes),
               c_le_a=bool(t_c <= t_a), numpy_vs_device_max_rel=float(dev.max()) if dev.size else None,
               n_viol_equal=bool(np.array_equal(a.raw[ok][:, 10], rec[ok][:, 10])),
               summary=a.summary(tol_con=1e-6, tol_bc=1e-3))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
