"""The LQR gains and the closed-loop tracking audit on the host (scp_lqr_gains_host and scp_model_audit_tracking_host: the bodies
the device kernels run, csrc/lqr_kernel.hpp and csrc/audit_kernel.hpp) against the CPU reference of tests/audit_tracking_util.py:
gain parity, failure reporting, flight records, zero gains = the dispersed audit, the benefit of closing the loop, the summary bit
for bit, and the error codes and exported names that need no device."""
import numpy as np
import pytest

import audit_tracking_util as atu
import audit_util as au

BAD, UNKNOWN, UNSUPPORTED = 1, 2, 7
FIRST3 = au.AUDIT_MODELS[:3]
GAIN_CASES = [(n, N) for n in FIRST3 for N in (2, 5, 9)] + [("starship", 9)]
FLIGHT_CASES = [(n, N, st) for n in FIRST3 for N in (2, 5) for st in (1, 4)] + [("starship", atu.STARSHIP["N"], atu.STARSHIP["steps"])]


def _gains(pkg, A, Bm, Bp, qx, ru, qf, dims=None, N=None):
    nx, nu = (A.shape[1], Bm.shape[1]) if dims is None else dims
    N = A.shape[0] + 1 if N is None else N
    K, info = np.full((max(N - 1, 1), nx, nu), 321.0), np.full(4, 322.0)
    rc = pkg._lib.lib().scp_lqr_gains_host(nx, nu, N, au.vp(A), au.vp(Bm), au.vp(Bp), au.vp(qx), au.vp(ru), au.vp(qf), au.vp(K), au.vp(info))
    return rc, np.swapaxes(K, -1, -2), info


def _fly(pkg, name, N, s, K, steps, viol_tol, disp, flights=True, par_true=None, D=None, Su=None, summary=True):
    xd, ud, p, pp = s["case"]
    dx0, gain, bias = disp
    D = dx0.shape[0] if D is None else D
    out, rec = np.full(au.W, 123.0), np.full((max(D, 1), au.W), 124.0)
    rc = pkg._lib.lib().scp_model_audit_tracking_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), au.vp(par_true), N,
                                                      au.vp(xd), au.vp(ud), au.vp(p) if p.size else None, au.vp(pp), au.vp(s["Sx"]),
                                                      au.vp(s["Su"] if Su is None else Su), au.vp(None if K is None else atu.to_lib(K)),
                                                      steps, float(viol_tol), D, au.vp(dx0), au.vp(gain), au.vp(bias),
                                                      au.vp(out) if summary else None, au.vp(rec) if flights else None)
    return rc, out, rec


@pytest.mark.parametrize("name,N", GAIN_CASES)
def test_gain_parity(pkg, orc, name, N):
    """scp_lqr_gains_host fed the oracle's A, B-, B+ against the numpy recursion (N = 2: the single step)"""
    s = atu.setup(orc, name, N)
    rc, K, info = _gains(pkg, *s["dyn"], *s["weights"])
    assert rc == 0
    tol = au.RTOL * max(1.0, np.abs(s["K"]).max())
    print(name, N, "max|K|", np.abs(s["K"]).max(), "err", np.abs(K - s["K"]).max(), "tol", tol, "info", info, s["info"])
    assert np.abs(K - s["K"]).max() <= tol
    assert info[0] == 0.0 and info[3] == 0.0
    for i in (1, 2):
        assert abs(info[i] - s["info"][i]) <= au.RTOL * abs(s["info"][i]), (i, info[i], s["info"][i])


def test_gain_failures_are_reported(pkg, orc):
    """a pivot <= 0 and non-finite data: info[0] = 1, K all NaN, no abort; and the problem next to it is not touched"""
    # two identical input columns and an R that is lost against Gam' P Gam = 4: the second pivot is exactly 0
    A = np.eye(6)[None].copy()
    Bm = np.zeros((1, 4, 6)); Bm[0, 0, 0] = Bm[0, 1, 0] = 1.0
    Bp = Bm.copy()
    rc, K, info = _gains(pkg, A, Bm, Bp, np.zeros(6), np.full(4, 1e-30), np.ones(6))
    assert rc == 0 and info[0] == 1.0 and np.isnan(K).all() and info[3] == 0.0
    rc, K, info = _gains(pkg, A, Bm, Bp, np.zeros(6), np.ones(4), np.ones(6))       # the same matrices with R = I are fine
    assert rc == 0 and info[0] == 0.0 and np.isfinite(K).all() and np.abs(K[0, :2, 0] - 2.0 / 9.0).max() < 1e-15
    s = atu.setup(orc, "rocket_landing", 5)
    for arr, val in ((1, np.nan), (0, np.inf)):
        dyn = [a.copy() for a in s["dyn"]]
        dyn[arr][2, 1, 3] = val                                                     # interval 3 of 4: K_4 is computed before it is met
        rc, K, info = _gains(pkg, *dyn, *s["weights"])
        assert rc == 0 and info[0] == 1.0 and np.isnan(K).all() and np.isnan(info[1:3]).all(), (arr, val, info)
    rc, K, info = _gains(pkg, *s["dyn"], *s["weights"])
    assert rc == 0 and info[0] == 0.0 and np.isfinite(K).all()


def test_gain_error_codes(pkg, orc):
    s = atu.setup(orc, "double_integrator", 5)
    A, Bm, Bp = s["dyn"]
    qx, ru, qf = s["weights"]
    assert _gains(pkg, A, Bm, Bp, qx, ru, qf)[0] == 0
    for bad in ((-qx, ru, qf), (qx, -ru, qf), (qx, 0.0 * ru, qf), (qx, ru, -qf), (qx * np.nan, ru, qf), (qx, ru * np.inf, qf),
                (None, ru, qf), (qx, None, qf), (qx, ru, None)):
        assert _gains(pkg, A, Bm, Bp, *bad)[0] == BAD
    assert _gains(pkg, A, Bm, Bp, 0.0 * qx, ru, 0.0 * qf)[0] == 0                  # zero state weights are allowed
    assert _gains(pkg, None, Bm, Bp, qx, ru, qf, dims=(2, 1), N=5)[0] == BAD
    assert _gains(pkg, A, Bm, Bp, qx, ru, qf, N=1)[0] == BAD
    big = np.zeros((4, 13 * 13))
    for dims in ((13, 6), (2, 2), (6, 3), (3, 1)):                                 # the free-flyer's and other pairs
        assert _gains(pkg, big, big, big, np.ones(13), np.ones(13), np.ones(13), dims=dims, N=5)[0] == UNSUPPORTED


@pytest.mark.parametrize("name,N,steps", FLIGHT_CASES)
def test_host_flights_match_reference_and_fold(pkg, orc, name, N, steps):
    """every flight record against the numpy sample-and-hold flight, the gains GIVEN (the reference's), and the summary bit for bit"""
    s = atu.setup(orc, name, N)
    refs = atu.references(orc, name, N, steps)
    tol = au.choose_viol_tol(refs)
    rc, out, rec = _fly(pkg, name, N, s, s["K"], steps, tol, s["disp"])
    assert rc == 0
    for d, ref in enumerate(refs):
        ref.check_tracking(rec[d], tol, "%s N=%d steps=%d d=%d" % (name, N, steps, d + 1))
    assert out.tobytes() == atu.fold(rec).tobytes(), (out, atu.fold(rec))
    assert out[13] == 3.0 and out[14] == 4.0 and out[11] == 0.0
    rc, only, _ = _fly(pkg, name, N, s, s["K"], steps, tol, s["disp"], flights=False)
    assert rc == 0 and only.tobytes() == out.tobytes()


@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_zero_gains_are_the_dispersed_flight(pkg, orc, name):
    N, steps = (atu.STARSHIP["N"], 2) if name == "starship" else (5, 4)
    s = atu.setup(orc, name, N)
    xd, ud, p, pp = s["case"]
    dx0, gain, bias = s["disp"]
    res = steps * (N - 1) + 1
    rc, out, rec = _fly(pkg, name, N, s, np.zeros_like(s["K"]), steps, 0.0, s["disp"])
    assert rc == 0
    dsum, drec = np.zeros(au.W), np.zeros((4, au.W))
    assert pkg._lib.lib().scp_model_audit_dispersed_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), None, N, au.vp(xd),
                                                         au.vp(ud), au.vp(p) if p.size else None, au.vp(pp), au.vp(s["Sx"]), res, 0.0, 4,
                                                         au.vp(dx0), au.vp(gain), au.vp(bias), au.vp(dsum), au.vp(drec)) == 0
    for d in range(4):
        fin = drec[d, :12][np.isfinite(drec[d, :12])]
        with np.errstate(invalid="ignore"):
            assert np.abs(rec[d, :12] - drec[d, :12])[np.isfinite(drec[d, :12])].max() <= au.RTOL * max(1.0, np.abs(fin).max()), d
        assert np.array_equal(rec[d, :12] == -np.inf, drec[d, :12] == -np.inf)
        assert np.array_equal(rec[d, [1, 3, 5, 10, 11]], drec[d, [1, 3, 5, 10, 11]])
        assert rec[d, 12] == 0.0 and rec[d, 13] == 1.0
        # [14]: the node tracking error of the open-loop flight, from the oracle's propagate of the same dispersed flight
        x0 = xd.copy(); x0[0] += dx0[d]
        _, xc = orc.propagate(name, orc.default_params(name), N, x0, ud * gain[d] + bias[d], p, res=res)
        err = np.abs((xc[::steps] - xd) / s["Sx"]).max(axis=1)
        assert abs(rec[d, 14] - err.max()) <= au.RTOL * max(1.0, err.max()), (d, rec[d, 14], err.max())
        assert abs(err[int(rec[d, 15]) - 1] - err.max()) <= au.RTOL * max(1.0, err.max())
    assert out[13] == 3.0 and dsum[13] == 2.0


@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_closing_the_loop_pays(pkg, orc, name):
    """the dx0-only flight: the reference's own closed-loop terminal drift is at most a third of its open-loop drift, and the host
    twin reproduces both flights"""
    N, steps = (atu.STARSHIP["N"], atu.STARSHIP["steps"]) if name == "starship" else (5, 4)
    s = atu.setup(orc, name, N)
    closed = atu.references(orc, name, N, steps, which=(3,))[0]
    K0 = np.zeros_like(s["K"])
    opened = atu.references(orc, name, N, steps, K=K0, which=(3,))[0]
    print(name, "open", opened.rec[8], "closed", closed.rec[8], "ratio", opened.rec[8] / closed.rec[8])
    assert closed.rec[8] <= opened.rec[8] / 3.0
    disp = tuple(a[3:4] for a in s["disp"])
    for ref, K in ((closed, s["K"]), (opened, K0)):
        tol = au.choose_viol_tol([ref])
        rc, out, rec = _fly(pkg, name, N, s, K, steps, tol, disp)
        assert rc == 0
        ref.check_tracking(rec[0], tol, name)
        assert out.tobytes() == atu.fold(rec).tobytes() and out[14] == 1.0


def test_a_nonfinite_flight_is_counted_and_left_out(pkg, orc):
    name, N, steps = "quadrotor", 5, 1
    s = atu.setup(orc, name, N)
    dx0, gain, bias = (a.copy() for a in s["disp"])
    dx0[1, 2] = np.nan
    rc, out, rec = _fly(pkg, name, N, s, s["K"], steps, 0.0, (dx0, gain, bias))
    assert rc == 0 and rec[1, 11] == 1.0 and out[11] == 1.0 and out[14] == 4.0 and out[13] == 3.0
    assert out.tobytes() == atu.fold(rec).tobytes()
    rc, _, rec0 = _fly(pkg, name, N, s, s["K"], steps, 0.0, s["disp"])
    assert rc == 0 and rec[[0, 2, 3]].tobytes() == rec0[[0, 2, 3]].tobytes()


def test_error_codes_without_a_device(pkg, orc):
    name, N = "quadrotor", 5
    s = atu.setup(orc, name, N)
    K, disp = s["K"], s["disp"]
    assert _fly(pkg, name, N, s, K, 1, 0.0, disp)[0] == 0
    assert _fly(pkg, name, N, s, K, 0, 0.0, disp)[0] == BAD                          # steps < 1
    assert _fly(pkg, name, N, s, K, -3, 0.0, disp)[0] == BAD
    assert _fly(pkg, name, N, s, K, 1, 0.0, disp, D=0)[0] == BAD
    assert _fly(pkg, name, N, s, None, 1, 0.0, disp)[0] == BAD                       # the host twin has no resident gains
    assert _fly(pkg, name, N, s, K, 1, 0.0, disp, summary=False)[0] == BAD
    xd, ud, p, pp = s["case"]
    for case in ((xd, ud, np.zeros(0), pp), ):
        assert _fly(pkg, name, N, dict(s, case=case), K, 1, 0.0, disp)[0] == BAD     # the model has a p
    L = pkg._lib.lib()
    out = np.zeros(au.W)
    args = (N, au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp), au.vp(s["Sx"]), au.vp(s["Su"]), au.vp(atu.to_lib(K)), 1, 0.0, 4,
            au.vp(disp[0]), au.vp(disp[1]), au.vp(disp[2]), au.vp(out), None)
    par = au.model_blob(pkg, name, N)
    assert L.scp_model_audit_tracking_host(pkg.models.MODEL_IDS[name], au.vp(par), None, *args) == 0
    assert L.scp_model_audit_tracking_host(42, au.vp(par), None, *args) == UNKNOWN
    ff = np.ones(16 * 16 * N)
    for other in ("freeflyer", "oscillator"):
        assert L.scp_model_audit_tracking_host(pkg.models.MODEL_IDS[other], au.vp(np.ones(64)), None, N, au.vp(ff), au.vp(ff), au.vp(ff),
                                               au.vp(ff), au.vp(np.ones(16)), au.vp(np.ones(16)), au.vp(ff), 1, 0.0, 1, None, None, None,
                                               au.vp(out), None) == UNSUPPORTED


def test_python_names_are_exported(pkg):
    for nm in ("lqr_gains", "lqr_gains_resident", "audit_tracking", "audit_tracking_resident"):
        assert callable(getattr(pkg, nm))
    for nm in ("scp_lqr_gains_batch_host", "scp_lqr_gains_resident", "scp_lqr_gains_host", "scp_audit_tracking_batch_host",
               "scp_audit_tracking_resident", "scp_model_audit_tracking_host"):
        assert nm in pkg._lib.EXPORTS and hasattr(pkg._lib.lib(), nm)
    raw = np.arange(2 * 3 * 6 * 4, dtype=float).reshape(2, 3, 6, 4)                 # the library's layout [B, N-1, nx, nu]
    info = np.array([[0.0, 5.0, 6.0, 0.0], [1.0, np.nan, np.nan, 0.0]])
    g = pkg.GainBatch(raw, info, np.ones(6), np.ones(4), np.ones(6))
    assert len(g) == 2 and g.K.shape == (2, 3, 4, 6) and g.K[1, 2, 3, 5] == raw[1, 2, 5, 3]
    assert list(g.failed) == [False, True] and g.k_max[0] == 5.0 and g.trace_p[0] == 6.0 and not g.skipped.any()
    s = np.arange(32.0).reshape(2, 16)
    fl = np.arange(2 * 3 * 16.0).reshape(2, 3, 16)
    a = pkg.TrackingAuditBatch(s, steps=4, res=17, viol_tol=0.5, D=3, flights=fl)
    assert isinstance(a, pkg.DispersedAuditBatch) and len(a) == 2 and a.steps == 4 and a.res == 17 and a.D == 3
    assert a.effort.shape == (2, 3) and a.effort[1, 2] == fl[1, 2, 12] and a.effort_node[0, 1] == fl[0, 1, 13]
    assert a.track_err[1, 0] == fl[1, 0, 14] and a.track_node[1, 1] == fl[1, 1, 15] and a.drift[0] == 8.0 and a.cost_max[1] == 31.0
    b = pkg.TrackingAuditBatch(s, 4, 17, 0.0, 3)
    assert b.flights is None and b.effort is None and b.effort_node is None and b.track_err is None and b.track_node is None
