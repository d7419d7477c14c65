"""Where the audit families meet on ONE handle (-m gpu): gains, tracking, Monte-Carlo, covariance, dispersed, nominal and interval
audits in a row, the flight and Monte-Carlo buffers regrown on the way and the caller's gains staged beside the resident ones.
Every result equals, byte for byte, that of the same call on a fresh handle that has seen only the calls it depends on."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAME, N, NSUB, CAP, B, STEPS, SEED = "double_integrator", 5, 5, 3, 2, 5, 2026


def _same(got, want, fields):
    for f in fields:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f


def test_one_handle_through_every_family(pkg):
    traj = pkg.TrajectoryProblem(NAME)
    pp = np.ascontiguousarray(np.tile(traj.mdl.nominal_pp()[None], (B, 1)))
    g = [traj.guess(N, pp[i]) for i in range(B)]
    xd, ud, p = (np.ascontiguousarray(np.stack([gi[j] for gi in g])) for j in range(3))
    ud[1] = 0.5 * ud[1] + 0.125       # a second problem that is not the first
    sol = SimpleNamespace(xd=xd, ud=ud, p=p)

    def handle():
        return pkg.PTR.create(pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=1), traj, batch_capacity=CAP)

    rng = np.random.default_rng(SEED)
    A = handle()
    Sx, Su = A.scale.Sx, A.scale.Su
    sig = (0.01 * Sx, 0.01 * Su, 0.002 * Sx)

    def disp(D):
        return dict(dx0=0.01 * Sx * rng.standard_normal((B, D, Sx.size)), ugain=1.0 + 0.01 * rng.standard_normal((B, D, Su.size)),
                    ubias=0.01 * Su * rng.standard_normal((B, D, Su.size)))

    d2, d70, d2b = disp(2), disp(70), disp(2)
    TRACK, MC, COV = ("raw", "flights"), ("raw", "stat", "moments", "flights"), ("raw", "sig", "nodes")
    # (the call on a handle, the fields compared, does it read the gains resident in the handle?); gains[0] = those handle A made
    gains = []
    calls = [
        (lambda h: pkg.lqr_gains(sol, h), ("raw", "info"), False),
        (lambda h: pkg.audit_tracking(sol, h, None, STEPS, **d2, pp=pp, flights=True), TRACK, True),
        (lambda h: pkg.audit_montecarlo(sol, h, None, STEPS, *sig, 2, SEED, flights=True, pp=pp), MC, True),
        (lambda h: pkg.audit_covariance(sol, h, None, *sig, per_node=True, pp=pp), COV, True),
        (lambda h: pkg.audit_montecarlo(sol, h, None, STEPS, *sig, 65, SEED, flights=True, pp=pp), MC, True),      # flights regrow, W 1 -> 2
        (lambda h: pkg.audit_dispersed(sol, h, **d70, pp=pp, flights=True), TRACK, False),                         # flights regrow again
        (lambda h: pkg.audit_tracking(sol, h, gains[0], STEPS, **d2b, pp=pp, flights=True), TRACK, False),         # the caller's gains
        (lambda h: pkg.audit(sol, h, pp=pp), ("raw",), False),
        (lambda h: pkg.audit_intervals(sol, h, pp=pp), ("raw", "intervals"), False),
    ]
    got = []
    for call, _, _ in calls:
        got.append(call(A))
        if not gains:
            gains.append(got[0])
    A.close()
    assert np.isfinite(got[0].raw).all()
    for r, (call, fields, resident) in zip(got, calls):
        h = handle()
        if resident:
            pkg.lqr_gains(sol, h)
        _same(call(h), r, fields)
        h.close()
