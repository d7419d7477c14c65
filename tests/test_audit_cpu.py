"""The continuous-time audit on the host (scp_model_audit_host: the body the device kernel runs, csrc/audit_kernel.hpp) against
the CPU reference of tests/audit_util.py -- the oracle's `propagate` and the closures of oracle/models.py -- for the four
supported models, and the error codes that need no device."""
import numpy as np
import pytest

import audit_util as au

SEEDS = {"double_integrator": 11, "quadrotor": 12, "rocket_landing": 13, "starship": 14}


def _call(pkg, name, N, xd, ud, p, pp, Sx, res, viol_tol, par=None):
    L = pkg._lib.lib()
    out = np.full(au.W, 123.0)
    par = au.model_blob(pkg, name, N) if par is None else par
    rc = L.scp_model_audit_host(pkg.models.MODEL_IDS[name], au.vp(par), N, au.vp(xd), au.vp(ud), au.vp(p) if p is not None and p.size else None,
                                au.vp(pp), au.vp(Sx), res, float(viol_tol), au.vp(out))
    return rc, out


@pytest.mark.parametrize("N", [5, 8])
@pytest.mark.parametrize("name", au.AUDIT_MODELS)
def test_host_audit_matches_reference(pkg, orc, name, N):
    Sx = au.state_scale(au.oracle_model(name, N))
    for res in au.res_values(N):
        (xd, ud, p, pp), ref = au.reference(orc, name, N, SEEDS[name] + N, res)
        tol = au.choose_viol_tol([ref])
        rc, out = _call(pkg, name, N, xd, ud, p, pp, Sx, res, tol)
        assert rc == 0
        ref.check(out, tol, "%s N=%d res=%d" % (name, N, res))


def test_node_index_follows_the_samples(pkg, orc):
    """the model functions see t = tc_j and the node of that sample: the rocket's glide-slope rows are switched off at t = 1 only
    (with res = 2 the two samples are t = 0 and t = 1), and a family without rows reports -Inf at time 0"""
    N = 5
    (xd, ud, p, pp), ref = au.reference(orc, "rocket_landing", N, 99, 2)
    xd = xd.copy(); xd[0, 0:3] = [0.0, 0.0, -50.0]       # below the ground at t = 0: glide-slope rows positive there
    Sx = au.state_scale(au.oracle_model("rocket_landing", N))
    r = au.Reference(orc, "rocket_landing", N, xd, ud, p, pp, Sx, 2)
    tol = au.choose_viol_tol([r])
    rc, out = _call(pkg, "rocket_landing", N, xd, ud, p, pp, Sx, 2, tol)
    assert rc == 0
    r.check(out, tol, "rocket below ground")
    assert out[2] > 0 and out[3] == 0.0
    (xd, ud, p, pp), ref = au.reference(orc, "double_integrator", N, 98, 7)
    rc, out = _call(pkg, "double_integrator", N, xd, ud, p, pp, au.state_scale(au.oracle_model("double_integrator", N)), 7, 0.0)
    assert rc == 0 and out[4] == -np.inf and out[5] == 0.0 and out[6] == -np.inf


def test_nonfinite_flag_on_the_host(pkg, orc):
    N = 5
    (xd, ud, p, pp), ref = au.reference(orc, "quadrotor", N, 97, 9)
    xd = xd.copy(); xd[0, 1] = np.nan
    rc, out = _call(pkg, "quadrotor", N, xd, ud, p, pp, np.ones(6), 9, 0.0)
    assert rc == 0 and out[11] == 1.0


def test_error_codes_without_a_device(pkg, orc):
    N = 5
    (xd, ud, p, pp), _ = au.reference(orc, "quadrotor", N, 96, 4)
    Sx = np.ones(6)
    BAD, UNKNOWN, UNSUPPORTED = 1, 2, 7
    assert _call(pkg, "quadrotor", N, xd, ud, p, pp, Sx, 1, 0.0)[0] == BAD                  # res < 2
    assert _call(pkg, "quadrotor", N, xd, ud, None, pp, Sx, 4, 0.0)[0] == BAD               # the model has a p
    assert _call(pkg, "quadrotor", N, xd, ud, p, None, Sx, 4, 0.0)[0] == BAD                # ... and a pp
    L = pkg._lib.lib()
    par = au.model_blob(pkg, "quadrotor", N)
    args = (au.vp(par), N, au.vp(xd), au.vp(ud), au.vp(p), au.vp(pp), au.vp(Sx), 4, 0.0)
    assert L.scp_model_audit_host(1, *args, None) == BAD                                    # NULL audit
    out = np.zeros(au.W)
    assert L.scp_model_audit_host(42, *args, au.vp(out)) == UNKNOWN
    # the free-flyer (node parameters): refused whatever the arrays hold
    ff = np.zeros(13 * N)
    assert L.scp_model_audit_host(pkg.models.MODEL_IDS["freeflyer"], au.vp(np.ones(64)), N, au.vp(ff), au.vp(ff), au.vp(ff), au.vp(ff),
                                  au.vp(np.ones(13)), 4, 0.0, au.vp(out)) == UNSUPPORTED
    assert _call(pkg, "quadrotor", N, xd, ud, p, pp, Sx, 4, 0.0)[0] == 0


def test_python_names_are_exported(pkg):
    assert callable(pkg.audit) and callable(pkg.audit_resident)
    a = pkg.AuditBatch(np.arange(32.0).reshape(2, 16), res=8, viol_tol=0.0)
    assert a.s_max[1] == 16.0 and a.t_soc[0] == 5.0 and a.nonfinite[1] == 27.0 and len(a) == 2
    raw = np.zeros((3, 16)); raw[:, [0, 2, 4, 6]] = -1.0; raw[1, 2] = 0.5; raw[2] = np.nan; raw[0, 7] = 1e-3
    s = pkg.AuditBatch(raw, 8, 0.0).summary(tol_con=1e-6, tol_bc=1e-2)
    assert (s["total"], s["skipped"], s["constraints_pass"], s["constraints_fail"], s["arrival_pass"], s["all_pass"]) == (3, 1, 1, 1, 2, 1)


def test_timing_tools_numpy_record_is_the_same_record(pkg, orc):
    """tools/audit_timing.py prices the audit against `propagate` + a numpy evaluation of the same record: that numpy twin
    (rocket landing, vectorised over the batch) agrees with scp_model_audit_host on the samples of the oracle's propagate"""
    import os
    import sys
    from types import SimpleNamespace as NS
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import audit_timing
    name, N, res, B = "rocket_landing", 8, 42, 3
    traj = pkg.TrajectoryProblem(name)
    scale = pkg.SCPScaling(*traj.mdl.scale_advice())
    pbm = NS(traj=traj, pars=NS(N=N), t_grid=pkg.models.linrange(0.0, 1.0, N), scale=scale)
    cases = [au.make_case(name, N, 50 + b) for b in range(B)]
    xd, ud, p, pp = (np.stack([c[i] for c in cases]) for i in range(4))
    prop = [orc.propagate(name, orc.default_params(name), N, xd[b], ud[b], p[b], res=res) for b in range(B)]
    rec = audit_timing.numpy_record(pkg, pbm, NS(xd=xd, ud=ud, p=p), pp, prop[0][0], np.stack([x for _, x in prop]))
    for b in range(B):
        rc, out = _call(pkg, name, N, xd[b], ud[b], p[b], pp[b], scale.Sx, res, 0.0)
        assert rc == 0
        assert np.abs(out - rec[b]).max() <= 1e-9 * max(1.0, np.abs(out[np.isfinite(out)]).max()), (b, out, rec[b])
        assert np.array_equal(out[[1, 3, 5, 10, 11]], rec[b][[1, 3, 5, 10, 11]])
