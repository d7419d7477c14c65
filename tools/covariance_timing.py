"""What the closed-loop covariance audit costs, on the headline configuration of bench.py (rocket landing, N = 100, its Nsub,
4 096 Monte-Carlo instances) after a converged PTR run on ONE handle, the batch and the gains resident.  Wall time, median of 10
after 2 warm-ups, the stream drained by every call:
  (1) scp_audit_covariance_resident, summary only (16 doubles per problem come back): wall time and the library's own
      event time (*seconds: discretize!, the row pre-pass and the chain), and the same with sig and nodes copied out;
  (2) what a user could do before: scp_discretize_batch_host with A, B-, B+ copied out, then the covariance recursion in numpy
      batched over the problems (Sigma chain, state and effort 1-sigma only: no rows, no margins; the gains are those an earlier
      scp_lqr_gains_resident copied out, and that copy is not timed again -- so this is a LOWER bound on the numpy path);
  (3) the Riccati part of scp_lqr_gains_resident on the same build: its *seconds minus the discretize! share that
      scp_get_kernel_timing reports for the same call; the covariance kernels' share of (1) is split off the same way.
Prints one JSON line (and writes it to the file given as the first argument).  No ratio is asserted: the file holds whatever the
device gives."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audit_timing import REPS, WARMUP, median_wall  # noqa: E402


def numpy_covariance(A, Bm, Bp, K, Su, sig0, sigu, sigw):
    """the recursion of include/scp_mi355x.h for the whole batch: A[B,N-1,nx,nx], Bm, Bp, K[B,N-1,nu,nx] in the library's memory
    order -> (sig[B,N,nx], effort[B,N-1,nu])"""
    B, M, nx = A.shape[0], A.shape[1], A.shape[2]
    S = np.tile(np.diag(sig0 ** 2)[None], (B, 1, 1))
    U, Wn = np.diag(sigu ** 2), np.diag(sigw ** 2)
    sig, eff = np.zeros((B, M + 1, nx)), np.zeros((B, M, K.shape[3]))
    for k in range(M):
        Phi, Gam, Kk = np.swapaxes(A[:, k], 1, 2), np.swapaxes(Bm[:, k] + Bp[:, k], 1, 2), np.swapaxes(K[:, k], 1, 2)
        sig[:, k] = np.sqrt(np.maximum(np.diagonal(S, axis1=1, axis2=2), 0.0))
        eff[:, k] = np.sqrt(np.maximum(np.einsum("bai,bij,baj->ba", Kk, S, Kk), 0.0)) / Su
        Acl = Phi - Gam @ Kk
        S = Acl @ S @ np.swapaxes(Acl, 1, 2) + Gam @ U @ np.swapaxes(Gam, 1, 2) + Wn
        S = 0.5 * (S + np.swapaxes(S, 1, 2))
    sig[:, M] = np.sqrt(np.maximum(np.diagonal(S, axis1=1, axis2=2), 0.0))
    return sig, eff


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
    Sx, Su = pbm.scale.Sx, pbm.scale.Su
    sig0, sigu, sigw = 0.01 * Sx, 0.01 * Su, 1e-3 * Sx
    qx, ru, qf = 1.0 / Sx ** 2, 1.0 / Su ** 2, 10.0 / Sx ** 2
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    kern, disc = {}, {}

    def k1_seconds():
        s4, n4 = (ctypes.c_double * 4)(), (ctypes.c_long * 4)()
        pkg._lib.check(L.scp_get_kernel_timing(pbm.handle, s4, n4, 1), pbm.handle)
        return s4[0]

    def run(key, fn):
        kern[key], disc[key] = [], []

        def call():
            k1_seconds()
            a = fn()
            kern[key].append(a.seconds)
            disc[key].append(k1_seconds())
            return a
        t, tmin, a = median_wall(call)
        ks, ds = float(np.median(kern[key][WARMUP:])), float(np.median(disc[key][WARMUP:]))
        return dict(wall_s=t, min_s=tmin, kernel_s=ks, discretize_s=ds, without_discretize_s=ks - ds), a

    info = np.zeros((B, 4))

    def gains_on_device_only():
        sec = ctypes.c_double(0.0)
        pkg._lib.check(L.scp_lqr_gains_resident(pbm.handle, vp(qx), vp(ru), vp(qf), None, vp(info), ctypes.byref(sec)), pbm.handle)
        return type("R", (), dict(seconds=sec.value))

    split = {}

    def before(K):
        A, Bm, Bp = (np.zeros((B, N - 1, c, pbm.nx)) for c in (pbm.nx, pbm.nu, pbm.nu))
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        pkg._lib.check(L.scp_discretize_batch_host(pbm.handle, B, vp(sol.xd), vp(sol.ud), vp(sol.p), vp(A), vp(Bm), vp(Bp), None, None, None,
                                                   None, None, ctypes.byref(sec)), pbm.handle)
        t1 = time.perf_counter()
        sig, eff = numpy_covariance(A, Bm, Bp, K, Su, sig0, sigu, sigw)
        split.setdefault("discretize_and_copy_s", []).append(t1 - t0)
        split.setdefault("numpy_recursion_s", []).append(time.perf_counter() - t1)
        return type("R", (), dict(seconds=sec.value, sig=sig, eff=eff))

    g = pkg.lqr_gains_resident(pbm, qx, ru, qf)
    t_3, _ = run("gains", gains_on_device_only)
    t_1, a = run("cov", lambda: pkg.audit_covariance_resident(pbm, None, sig0, sigu, sigw))
    t_1n, an = run("cov_nodes", lambda: pkg.audit_covariance_resident(pbm, None, sig0, sigu, sigw, per_node=True))
    # (2) stages the solution in the handle's solution buffers and therefore runs last
    t_2, r_2 = run("before", lambda: before(g.raw))
    live = ok & ~g.failed & ~g.skipped & ~a.skipped & ~a.failed
    d_sig = float(np.abs(an.sig[live] - r_2.sig[live]).max()) if live.any() else None
    out = dict(workload="%s N=%d Nsub=%d batch %d after a converged PTR run, gains resident; sig0 = 0.01 Sx, sigu = 0.01 Su, sigw = 1e-3 Sx"
                        % (model, N, Nsub, B),
               solved=int(ok.sum()), reps=REPS, warmup=WARMUP,
               covariance_resident_summary_only=t_1, covariance_resident_with_sig_and_nodes=t_1n,
               bytes_to_host_summary_only=int(a.raw.nbytes), bytes_to_host_with_sig_and_nodes=int(an.raw.nbytes + an.sig.nbytes + an.nodes.nbytes),
               copy_out_then_numpy=t_2, copy_out_discretize_and_copy_s=float(np.median(split["discretize_and_copy_s"][WARMUP:])),
               copy_out_numpy_recursion_s=float(np.median(split["numpy_recursion_s"][WARMUP:])),
               ratio_device_over_numpy_wall=t_1["wall_s"] / t_2["wall_s"],
               lqr_gains_resident_K_left_on_device=t_3,
               ratio_covariance_kernels_over_riccati_kernel=t_1["without_discretize_s"] / t_3["without_discretize_s"] if t_3["without_discretize_s"] > 0 else None,
               covariance_failures=int(np.nansum(a.raw[:, 0])), largest_difference_device_sig_vs_numpy=d_sig,
               sigma_max_median=float(np.nanmedian(a.sigma_max)), margin_lin_median=float(np.nanmedian(a.margin_lin)),
               n_below_3_sigma_total=float(np.nansum(a.n_below)))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")
    pbm.close()


if __name__ == "__main__":
    main()
