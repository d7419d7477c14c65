"""The interval-parallel audit on the host (scp_model_audit_intervals_host: the bodies the device kernels run,
csrc/audit_kernel.hpp) against the CPU reference of tests/audit_intervals_util.py for the four models under FOH and the two
impulsive ones under IMPULSE; a pin on trajectories that ARE flown (defect 0 by construction); the ordered fold; the reach of a
NaN; the error codes that need no device."""
import numpy as np
import pytest

import audit_intervals_util as aiu
import audit_util as au

SEEDS = {"double_integrator": 21, "quadrotor": 22, "rocket_landing": 23, "starship": 24}
OK, BAD, UNKNOWN, UNSUPPORTED = 0, 1, 2, 7


def _call(pkg, name, method, N, xd, ud, p, pp, Sx, res, viol_tol, intervals=True):
    L = pkg._lib.lib()
    out, rec = np.full(aiu.W, 123.0), np.full((N - 1, aiu.WI), 321.0)
    rc = L.scp_model_audit_intervals_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, method, au.vp(xd), au.vp(ud),
                                          au.vp(p) if p is not None and p.size else None, au.vp(pp), au.vp(Sx), res, float(viol_tol),
                                          au.vp(out), au.vp(rec) if intervals else None)
    return rc, out, rec


@pytest.mark.parametrize("N", [3, 8])
@pytest.mark.parametrize("name,method", aiu.CASES)
def test_host_interval_audit_matches_reference(pkg, orc, name, method, N):
    Sx = au.state_scale(au.oracle_model(name, N))
    for res in aiu.res_values(N):
        (xd, ud, p, pp), ref = aiu.reference(orc, name, method, N, SEEDS[name] + N, res)
        assert ref.sub == {2: 2, 3 * (N - 1): 3, 6 * (N - 1) + 1: 7}[res]
        tol = au.choose_viol_tol([ref])
        rc, out, rec = _call(pkg, name, method, N, xd, ud, p, pp, Sx, res, tol)
        assert rc == OK
        ref.check(out, rec, tol, "%s %s N=%d res=%d" % (name, "FOH" if method == aiu.FOH else "IMPULSE", N, res))
        # the ordered fold: the summary is the fold of the returned records, bit for bit
        assert out.tobytes() == aiu.fold(rec, out[6], np.isfinite(ref.summary[6]), ref.sub).tobytes()
        rc, out2, _ = _call(pkg, name, method, N, xd, ud, p, pp, Sx, res, tol, intervals=False)
        assert rc == OK and out2.tobytes() == out.tobytes()


@pytest.mark.parametrize("name", ["double_integrator", "quadrotor", "rocket_landing"])
def test_flown_trajectory_has_no_defect(pkg, orc, name):
    """xd = every m-th sample of the oracle's single-shooting propagation at res = m (N - 1) + 1: the interval audit at that res
    takes the same m steps per interval from the same states, so every defect vanishes (the reference gives 1e-16), and the
    maxima and the cost agree with the single-shooting audit of the same build"""
    N, m = 8, 4
    res = m * (N - 1) + 1
    xg, ud, p, pp = au.make_case(name, N, SEEDS[name] + 100)
    _, xc = orc.propagate(name, orc.default_params(name), N, xg, ud, p, res=res)
    xd = np.ascontiguousarray(xc[::m])
    assert xd.shape == xg.shape
    Sx = au.state_scale(au.oracle_model(name, N))
    ref = aiu.IntervalReference(orc, name, N, aiu.FOH, xd, ud, p, pp, Sx, res)
    assert ref.sub == m + 1
    tol = au.choose_viol_tol([ref])
    rc, out, rec = _call(pkg, name, aiu.FOH, N, xd, ud, p, pp, Sx, res, tol)
    assert rc == OK
    ref.check(out, rec, tol, name)
    print("defects", rec[:, 6], "reference", ref.rec[:, 6])
    assert (rec[:, 6] <= 1e-9).all() and out[8] <= 1e-9
    single = np.zeros(au.W)
    assert pkg._lib.lib().scp_model_audit_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, au.vp(xd), au.vp(ud),
                                               au.vp(p) if p.size else None, au.vp(pp), au.vp(Sx), res, float(tol), au.vp(single)) == OK
    for f in range(3):
        if not np.isfinite(ref.summary[2 * f]):
            assert single[2 * f] == out[2 * f] == -np.inf
            continue
        kr = int(np.argmax(ref.rec[:, 2 * f])); jr = int(np.argmax(ref.fam[kr, :, f]))
        assert abs(single[2 * f] - out[2 * f]) <= aiu.RTOL * ref.scale[kr, jr, f], (f, single[2 * f], out[2 * f])
    assert abs(single[9] - out[9]) <= aiu.RTOL * max(1.0, abs(ref.summary[9])), (single[9], out[9])


def test_a_nan_node_flags_the_two_intervals_that_read_it(pkg, orc):
    N, res, k = 8, 3 * 7, 4                                       # node k (1-based): read by the intervals k-1 and k
    for name, method in (("quadrotor", aiu.FOH), ("quadrotor", aiu.IMPULSE), ("rocket_landing", aiu.FOH)):
        xd, ud, p, pp = au.make_case(name, N, 77)
        xd = xd.copy(); xd[k - 1, 1] = np.nan
        rc, out, rec = _call(pkg, name, method, N, xd, ud, p, pp, au.state_scale(au.oracle_model(name, N)), res, 0.0)
        assert rc == OK
        assert np.array_equal(np.nonzero(rec[:, 9])[0] + 1, [k - 1, k]), (name, method, rec[:, 9])
        assert out[11] == 1.0 and np.isfinite(rec[[i for i in range(N - 1) if i + 1 not in (k - 1, k)]]).all()


def test_error_codes_without_a_device(pkg, orc):
    N = 5
    xd, ud, p, pp = au.make_case("quadrotor", N, 96)
    Sx = np.ones(6)
    assert _call(pkg, "quadrotor", aiu.FOH, N, xd, ud, p, pp, Sx, 1, 0.0)[0] == BAD                 # res < 2
    assert _call(pkg, "quadrotor", aiu.FOH, N, xd, ud, None, pp, Sx, 4, 0.0)[0] == BAD              # the model has a p
    assert _call(pkg, "quadrotor", aiu.IMPULSE, N, xd, ud, p, None, Sx, 4, 0.0)[0] == BAD           # ... and a pp
    assert _call(pkg, "quadrotor", 2, N, xd, ud, p, pp, Sx, 4, 0.0)[0] == BAD                       # no such method
    L = pkg._lib.lib()
    par = au.model_blob(pkg, "quadrotor", N)
    args = (au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp), au.vp(Sx), 4, 0.0)
    rec = np.zeros((N - 1, aiu.WI))
    assert L.scp_model_audit_intervals_host(1, au.vp(par), N, aiu.FOH, *args, None, au.vp(rec)) == BAD    # NULL audit
    out = np.zeros(aiu.W)
    assert L.scp_model_audit_intervals_host(42, au.vp(par), N, aiu.FOH, *args, au.vp(out), au.vp(rec)) == UNKNOWN
    # IMPULSE with a model that has no impulsive-input form
    for name in ("rocket_landing", "starship"):
        c = au.make_case(name, N, 95)
        assert _call(pkg, name, aiu.IMPULSE, N, *c, au.state_scale(au.oracle_model(name, N)), 4, 0.0)[0] == UNSUPPORTED
    # the free-flyer (node parameters): refused whatever the arrays hold
    ff = np.zeros(13 * N)
    for method in (aiu.FOH, aiu.IMPULSE):
        assert L.scp_model_audit_intervals_host(pkg.models.MODEL_IDS["freeflyer"], au.vp(np.ones(64)), N, method, au.vp(ff), au.vp(ff),
                                                au.vp(ff), au.vp(ff), au.vp(np.ones(13)), 4, 0.0, au.vp(out), au.vp(rec)) == UNSUPPORTED
    assert _call(pkg, "quadrotor", aiu.IMPULSE, N, xd, ud, p, pp, Sx, 4, 0.0)[0] == OK


def test_python_names_are_exported(pkg):
    assert callable(pkg.audit_intervals) and callable(pkg.audit_intervals_resident)
    raw = np.arange(32.0).reshape(2, 16); raw[1] = np.nan
    a = pkg.IntervalAuditBatch(raw, res=8, viol_tol=0.0, sub=3, intervals=np.zeros((2, 4, 16)))
    assert isinstance(a, pkg.AuditBatch) and a.sub == 3 and a.intervals.shape == (2, 4, 16)
    assert a.defect[0] == 8.0 and a.s_max[0] == 0.0 and list(a.worst_interval) == [12, -1] and a.worst_interval.dtype.kind == "i"
    assert a.skipped[1] and a.summary(1e-6, 1e-3)["skipped"] == 1
    assert pkg.IntervalAuditBatch(raw, 8, 0.0, 3).intervals is None
