"""The dispersed-flight audit on the host (scp_model_audit_dispersed_host: the bodies the device kernels run, csrc/audit_kernel.hpp)
against the CPU reference of tests/audit_dispersed_util.py for the four supported models, the ordered fold bit for bit, the
non-finite flight, the truth model, and the error codes that need no device."""
import numpy as np
import pytest

import audit_dispersed_util as adu
import audit_util as au

BAD, UNKNOWN, UNSUPPORTED = 1, 2, 7


def _call(pkg, name, N, case, Sx, res, viol_tol, disp, par_true=None, flights=True, par=None, D=None):
    xd, ud, p, pp = case
    dx0, gain, bias = disp
    D = (dx0 if dx0 is not None else gain if gain is not None else bias).shape[0] if D is None else D
    out, rec = np.full(au.W, 123.0), np.full((max(D, 1), au.W), 124.0)
    par = au.model_blob(pkg, name, N) if par is None else par
    rc = pkg._lib.lib().scp_model_audit_dispersed_host(pkg.models.MODEL_IDS[name], au.vp(par), au.vp(par_true), N, au.vp(xd), au.vp(ud),
                                                       au.vp(p) if p is not None and p.size else None, au.vp(pp), au.vp(Sx), res,
                                                       float(viol_tol), D, au.vp(dx0), au.vp(gain), au.vp(bias), au.vp(out),
                                                       au.vp(rec) if flights else None)
    return rc, out, rec


@pytest.mark.parametrize("N", [5, 8])
@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_host_flights_match_reference_and_fold(pkg, orc, name, N):
    Sx = au.state_scale(au.oracle_model(name, N))
    for res in au.res_values(N):
        case, disp, refs = adu.reference(orc, name, N, adu.SEEDS[name] + N, res)
        tol = au.choose_viol_tol(refs)
        rc, out, rec = _call(pkg, name, N, case, Sx, res, tol, disp)
        assert rc == 0
        for d in range(adu.D3):
            refs[d].check(rec[d], tol, "%s N=%d res=%d d=%d" % (name, N, res, d + 1))
        assert out.tobytes() == adu.fold(rec).tobytes(), (out, adu.fold(rec))
        assert out[13] == 2.0 and out[14] == 3.0 and out[11] == 0.0
        rc, only, _ = _call(pkg, name, N, case, Sx, res, tol, disp, flights=False)
        assert rc == 0 and only.tobytes() == out.tobytes()


def test_null_dispersions_are_the_nominal_flight(pkg, orc):
    """NULL dx0 / ugain / ubias mean 0 / 1 / 0: the flight is the single-shooting audit's own, the same numbers"""
    name, N, res = "rocket_landing", 5, 17
    Sx = au.state_scale(au.oracle_model(name, N))
    case, ref = au.reference(orc, name, N, adu.SEEDS[name] + N, res)
    tol = au.choose_viol_tol([ref])
    rc, out, rec = _call(pkg, name, N, case, Sx, res, tol, (None, None, None), D=2)
    assert rc == 0 and rec[0].tobytes() == rec[1].tobytes()
    ref.check(rec[0], tol, "all NULL")
    single = np.zeros(au.W)
    xd, ud, p, pp = case
    assert pkg._lib.lib().scp_model_audit_host(pkg.models.MODEL_IDS[name], au.vp(au.model_blob(pkg, name, N)), N, au.vp(xd), au.vp(ud),
                                               au.vp(p), au.vp(pp), au.vp(Sx), res, float(tol), au.vp(single)) == 0
    assert np.abs(rec[0] - single).max() <= au.RTOL * max(1.0, np.abs(single[np.isfinite(single)]).max())
    assert np.array_equal(rec[0, [1, 3, 5, 10, 11]], single[[1, 3, 5, 10, 11]])


def test_a_nonfinite_flight_is_counted_and_left_out(pkg, orc):
    name, N, res = "quadrotor", 5, 9
    Sx = au.state_scale(au.oracle_model(name, N))
    case, (dx0, gain, bias), refs = adu.reference(orc, name, N, adu.SEEDS[name] + N, res)
    tol = au.choose_viol_tol(refs)
    bad = dx0.copy(); bad[1, 2] = np.nan
    rc, out, rec = _call(pkg, name, N, case, Sx, res, tol, (bad, gain, bias))
    assert rc == 0 and rec[1, 11] == 1.0 and out[11] == 1.0 and out[14] == 3.0
    for d in (0, 2):
        refs[d].check(rec[d], tol, "d=%d" % (d + 1))
    assert out.tobytes() == adu.fold(rec).tobytes()
    assert out.tobytes() != adu.fold(rec[[0, 2]]).tobytes()          # [11], [14] and the flight numbers differ ...
    two = adu.fold(rec[[0, 2]])
    assert np.array_equal(out[[0, 2, 4, 6, 7, 8, 9, 10, 15]], two[[0, 2, 4, 6, 7, 8, 9, 10, 15]])      # ... and nothing else
    assert set(out[[1, 3, 5, 12]]) <= {0.0, 1.0, 3.0}
    # that flight alone
    rc, out, rec = _call(pkg, name, N, case, Sx, res, tol, (bad[1:2], gain[1:2], bias[1:2]))
    assert rc == 0 and rec[0, 11] == 1.0 and out[11] == 1.0 and out[14] == 1.0 and out[10] == 0.0 and out[12] == 0.0
    assert np.isnan(out[[7, 8, 9, 15]]).all()
    assert (out[[0, 2, 4]] == -np.inf).all() and not out[[1, 3, 5]].any()
    assert out.tobytes() == adu.fold(rec).tobytes()


@pytest.mark.parametrize("name", ["quadrotor", "rocket_landing"])
def test_truth_model(pkg, orc, name):
    """the flight follows par_true: dynamics (gravity, and the rocket's alpha), the s rows (the rocket's rho_max) and the cost (the
    quadrotor's 1 / g^2).  The quadrotor's gravity moves the vertical channel only, which none of its row families reads, so its
    drift is measured in a scaling that weighs that channel"""
    N, res = 8, au.res_values(8)[2]
    Sx = au.state_scale(au.oracle_model(name, N))
    if name == "quadrotor":
        Sx = np.array([100.0, 100.0, 1.0, 100.0, 100.0, 1.0])
    case, disp, _ = adu.reference(orc, name, N, adu.SEEDS[name] + N, res)
    nominal = adu.flight_references(orc, name, N, case, Sx, res, *disp)
    blob, tr = adu.truth(pkg, orc, name, N)
    refs = adu.flight_references(orc, name, N, case, Sx, res, *disp, truth=tr)
    tol = au.choose_viol_tol(refs)
    rc, out, rec = _call(pkg, name, N, case, Sx, res, tol, disp, par_true=blob)
    assert rc == 0
    for d in range(adu.D3):
        refs[d].check(rec[d], tol, "%s truth d=%d" % (name, d + 1))
    assert out.tobytes() == adu.fold(rec).tobytes()
    # not the nominal flight: the drift (dynamics) and the cost moved by far more than the tolerance, in the reference and in the
    # code under test, and so did the rocket's s maximum, whose rows changed
    rc, out0, rec0 = _call(pkg, name, N, case, Sx, res, tol, disp)
    assert rc == 0
    far = 1e3 * au.RTOL
    for d in range(adu.D3):
        for i in (8, 9):
            assert abs(refs[d].rec[i] - nominal[d].rec[i]) > far * max(1.0, abs(nominal[d].rec[i])), (d, i, refs[d].rec[i], nominal[d].rec[i])
            assert abs(rec[d, i] - rec0[d, i]) > far * max(1.0, abs(rec0[d, i])), (d, i, rec[d, i], rec0[d, i])
        if name == "rocket_landing":
            assert abs(rec[d, 0] - rec0[d, 0]) > far * nominal[d].scale[:, 0].max(), (d, rec[d, 0], rec0[d, 0])
    # par_true = the handle's own blob: nothing changes
    rc, same, rsame = _call(pkg, name, N, case, Sx, res, tol, disp, par_true=au.model_blob(pkg, name, N))
    assert rc == 0 and same.tobytes() == out0.tobytes() and rsame.tobytes() == rec0.tobytes()
    # and model_par is not read where par_true is given
    rc, other, rother = _call(pkg, name, N, case, Sx, res, tol, disp, par_true=blob, par=au.model_blob(pkg, name, N) * 0.5)
    assert rc == 0 and other.tobytes() == out.tobytes() and rother.tobytes() == rec.tobytes()


def test_error_codes_without_a_device(pkg, orc):
    name, N = "quadrotor", 5
    case, disp, _ = adu.reference(orc, name, N, adu.SEEDS[name] + N, 2)
    xd, ud, p, pp = case
    Sx = np.ones(6)
    assert _call(pkg, name, N, case, Sx, 4, 0.0, disp, D=0)[0] == BAD
    assert _call(pkg, name, N, case, Sx, 4, 0.0, disp, D=-1)[0] == BAD
    assert _call(pkg, name, N, case, Sx, 1, 0.0, disp)[0] == BAD                                  # res < 2
    assert _call(pkg, name, N, (xd, ud, None, pp), Sx, 4, 0.0, disp)[0] == BAD                    # the model has a p
    assert _call(pkg, name, N, (xd, ud, p, None), Sx, 4, 0.0, disp)[0] == BAD                     # ... and a pp
    L = pkg._lib.lib()
    par = au.model_blob(pkg, name, N)
    rec = np.zeros((3, au.W))
    args = (N, au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp), au.vp(Sx), 4, 0.0, 3, au.vp(disp[0]), au.vp(disp[1]), au.vp(disp[2]))
    assert L.scp_model_audit_dispersed_host(1, au.vp(par), None, *args, None, au.vp(rec)) == BAD  # NULL summary
    out = np.zeros(au.W)
    assert L.scp_model_audit_dispersed_host(42, au.vp(par), None, *args, au.vp(out), au.vp(rec)) == UNKNOWN
    # node parameters (free-flyer, oscillator): refused whatever the arrays hold
    ff = np.ones(16 * N)
    for other in ("freeflyer", "oscillator"):
        assert L.scp_model_audit_dispersed_host(pkg.models.MODEL_IDS[other], au.vp(np.ones(64)), None, N, au.vp(ff), au.vp(ff), au.vp(ff),
                                                au.vp(ff), au.vp(np.ones(16)), 4, 0.0, 1, None, None, None, au.vp(out), None) == UNSUPPORTED
    assert _call(pkg, name, N, case, Sx, 4, 0.0, disp)[0] == 0


def test_python_names_are_exported(pkg):
    assert callable(pkg.audit_dispersed) and callable(pkg.audit_dispersed_resident)
    raw = np.arange(32.0).reshape(2, 16)
    fl = np.arange(2 * 3 * 16.0).reshape(2, 3, 16)
    a = pkg.DispersedAuditBatch(raw, res=8, viol_tol=0.5, D=3, flights=fl)
    assert len(a) == 2 and a.D == 3 and a.res == 8 and a.viol_tol == 0.5 and a.raw.shape == (2, 16) and not a.skipped.any()
    assert a.s_max[1] == 16.0 and a.flight_s[1] == 17.0 and a.lin_max[0] == 2.0 and a.flight_lin[0] == 3.0 and a.soc_max[0] == 4.0
    assert a.flight_soc[0] == 5.0 and a.par_max[0] == 6.0 and a.bc_tc[0] == 7.0 and a.drift[0] == 8.0 and a.cost_mean[1] == 25.0
    assert a.n_violating[0] == 10.0 and a.n_nonfinite[1] == 27.0 and a.flight_bc[0] == 12.0 and a.cost_max[1] == 31.0
    fb = a.flight_batch(1)
    assert isinstance(fb, pkg.AuditBatch) and len(fb) == 3 and fb.res == 8 and fb.s_max[2] == 80.0 and fb.cost[0] == 57.0
    raw[1] = np.nan
    b = pkg.DispersedAuditBatch(raw, 8, 0.0, 3)
    assert b.flights is None and list(b.skipped) == [False, True]
    with pytest.raises(ValueError):
        b.flight_batch(0)
