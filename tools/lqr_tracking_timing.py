"""What the LQR synthesis and the closed-loop tracking audit cost, on the headline configuration of bench.py (rocket landing,
N = 100, its Nsub, 4 096 Monte-Carlo instances) after a converged PTR run on ONE handle, the batch resident.  Wall time, median
of 10 after 2 warm-ups, the stream drained by every call:
  (a) gains on the device: scp_lqr_gains_resident (discretize! into the handle's own buffers, then the Riccati kernel; K comes
      back to the host) -- and the same with K left on the device;
  (b) what a user could do before: scp_discretize_batch_host with A, B-, B+ copied out, then the Riccati recursion in numpy,
      batched over the problems (one matmul / solve per step for the whole batch);
  (c) tracking flights at D = 16, steps = 2 Nsub per interval, gains resident, without the flight records;
  (d) scp_audit_dispersed_resident at the same D and the same res = steps (N - 1) + 1: the open-loop kernel of the same build.
Prints one JSON line (and writes it to the file given as the first argument): the medians, the device time from the library's
own event timer, the ratios (a)/(b) and (c)/(d), and the largest difference between the device's K and numpy's.  No ratio is
asserted: the file holds whatever the device gives."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audit_timing import REPS, WARMUP, median_wall  # noqa: E402

D = 16


def numpy_riccati(A, Bm, Bp, qx, ru, qf):
    """the recursion of include/scp_mi355x.h for the whole batch: A[B,N-1,nx,nx], Bm, Bp[B,N-1,nu,nx] in the library's memory order"""
    B, M, nx = A.shape[0], A.shape[1], A.shape[2]
    Q, R = np.diag(qx), np.diag(ru)
    P = np.tile(np.diag(qf)[None], (B, 1, 1))
    K = np.zeros((B, M, Bm.shape[2], nx))
    for k in range(M - 1, -1, -1):
        Phi, Gam = np.swapaxes(A[:, k], 1, 2), np.swapaxes(Bm[:, k] + Bp[:, k], 1, 2)
        GtP = np.swapaxes(Gam, 1, 2) @ P
        K[:, k] = np.linalg.solve(R + GtP @ Gam, GtP @ Phi)
        P = Q + np.swapaxes(Phi, 1, 2) @ P @ (Phi - Gam @ K[:, k])
        P = 0.5 * (P + np.swapaxes(P, 1, 2))
    return K


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    import bench
    pkg = graft.load_package()
    L = pkg._lib.lib()
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
    res = steps * (N - 1) + 1
    rng = np.random.default_rng(0)
    ub = traj.mdl.scale_advice()[1]
    dx0 = 0.01 * pbm.scale.Sx * rng.standard_normal((B, D, pbm.nx))
    gain = 1.0 + 0.02 * rng.standard_normal((B, D, pbm.nu))
    bias = 0.01 * (ub[:, 1] - ub[:, 0]) * rng.standard_normal((B, D, pbm.nu))
    dx0[:, 0], gain[:, 0], bias[:, 0] = 0.0, 1.0, 0.0
    qx, ru, qf = 1.0 / pbm.scale.Sx ** 2, 1.0 / pbm.scale.Su ** 2, 10.0 / pbm.scale.Sx ** 2
    kern = {}

    def run(key, fn):
        kern[key] = []

        def call():
            a = fn()
            kern[key].append(a.seconds)
            return a
        t, tmin, a = median_wall(call)
        return dict(wall_s=t, min_s=tmin, kernel_s=float(np.median(kern[key][WARMUP:]))), a

    info = np.zeros((B, 4))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def gains_on_device_only():
        sec = ctypes.c_double(0.0)
        pkg._lib.check(L.scp_lqr_gains_resident(pbm.handle, vp(qx), vp(ru), vp(qf), None, vp(info), ctypes.byref(sec)), pbm.handle)
        return type("R", (), dict(seconds=sec.value))

    split = {}

    def before():
        """discretize! on the device with A, B-, B+ copied out, then numpy; .seconds = the device time of discretize! alone"""
        A, Bm, Bp = (np.zeros((B, N - 1, c, pbm.nx)) for c in (pbm.nx, pbm.nu, pbm.nu))
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        pkg._lib.check(L.scp_discretize_batch_host(pbm.handle, B, vp(sol.xd), vp(sol.ud), vp(sol.p), vp(A), vp(Bm), vp(Bp), None, None, None,
                                                   None, None, ctypes.byref(sec)), pbm.handle)
        t1 = time.perf_counter()
        K = numpy_riccati(A, Bm, Bp, qx, ru, qf)
        split.setdefault("discretize_and_copy_s", []).append(t1 - t0)
        split.setdefault("numpy_riccati_s", []).append(time.perf_counter() - t1)
        return type("R", (), dict(seconds=sec.value, K=K))

    t_a, g = run("a", lambda: pkg.lqr_gains_resident(pbm, qx, ru, qf))
    t_a0, _ = run("a0", gains_on_device_only)
    t_c, a_c = run("c", lambda: pkg.audit_tracking_resident(pbm, None, steps, dx0, gain, bias))
    t_d, a_d = run("d", lambda: pkg.audit_dispersed_resident(pbm, dx0, gain, bias, res=res))
    # once more, so that a drift of the machine shows as a difference between the passes
    t_c2, _ = run("c2", lambda: pkg.audit_tracking_resident(pbm, None, steps, dx0, gain, bias))
    t_d2, _ = run("d2", lambda: pkg.audit_dispersed_resident(pbm, dx0, gain, bias, res=res))
    # (b) stages the solution in the handle's solution buffers and therefore runs last
    t_b, r_b = run("b", before)
    live = ok & ~g.failed & ~g.skipped
    dK = float(np.abs(g.K[live] - r_b.K[live]).max()) if live.any() else None
    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run; tracking: D=%d, steps=%d, res=%d" % (model, N, Nsub, B, D, steps, res),
               solved=int(ok.sum()), reps=REPS, warmup=WARMUP,
               a_gains_resident=t_a, a_gains_resident_K_left_on_device=t_a0, a_bytes_to_host=int(g.raw.nbytes + g.info.nbytes),
               b_discretize_copy_out_then_numpy=t_b, b_discretize_and_copy_s=float(np.median(split["discretize_and_copy_s"][WARMUP:])),
               b_numpy_riccati_s=float(np.median(split["numpy_riccati_s"][WARMUP:])),
               ratio_a_over_b_wall=t_a["wall_s"] / t_b["wall_s"],
               c_tracking_resident=t_c, d_dispersed_resident_same_D_and_res=t_d, ratio_c_over_d_wall=t_c["wall_s"] / t_d["wall_s"],
               ratio_c_over_d_kernel=t_c["kernel_s"] / t_d["kernel_s"],
               second_pass=dict(c_tracking_resident=t_c2, d_dispersed_resident_same_D_and_res=t_d2),
               gain_failures=int(np.nansum(g.info[:, 0])), k_max=float(np.nanmax(g.k_max)) if live.any() else None,
               largest_difference_device_K_vs_numpy=dK,
               drift_open_loop_max_median=float(np.nanmedian(a_d.drift)), drift_closed_loop_max_median=float(np.nanmedian(a_c.drift)),
               nonfinite_flights_open=int(np.nansum(a_d.n_nonfinite)), nonfinite_flights_closed=int(np.nansum(a_c.n_nonfinite)))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
