"""CPU reference of the LQR gains and of the closed-loop tracking audit (include/scp_mi355x.h, scp_lqr_gains_* and
scp_audit_tracking_*), shared by tests/test_audit_tracking_cpu.py and tests/test_audit_tracking_gpu.py.  It takes nothing from
the code under test:

  gains    numpy Riccati, operation by operation as the header states it, over the oracle's `discretize!` (oracle.discretize)
  flights  numpy sample-and-hold RK4 flight over the oracle's dynamics (oracle.model_eval), every sample evaluated by the closures
           of oracle/models.py through audit_util._sample

Cases ("flown" trajectories).  audit_util.make_case(name, N, 7 + N) with its nodes re-sampled from the oracle's `propagate` at
res = 4 (N - 1) + 1, every 4th sample, so that the nodes are dynamically consistent; discretize! at Nsub = 5.  The Starship's RK4
inside discretize! is unstable at Nsub = 5 and its perturbed guesses explode: it is flown on the model's own unperturbed guess
re-sampled the same way at N = 9, Nsub = 51 and 50 flight steps per interval, and in no other configuration.
Weights: Bryson's rule qx = 1 / Sx^2, ru = 1 / Su^2, qf = 10 qx with Sx = audit_util.state_scale and Su = the input box widths
(widths below 1e-8 set to 1).
Flights: the three of audit_dispersed_util.dispersions drawn from default_rng(1000 + N), and a fourth with
dx0 = 0.01 Sx N(0,1) from default_rng(100 + N) only (the benefit test's).

Tolerances: audit_util's for records [0..11] (Reference.check, choose_viol_tol over all flights of a call, equal counts);
[12] and [14] with RTOL * max(1, |ref|); [13] and [15] must be nodes at which the reference's own value is within that tolerance
of its maximum."""
import numpy as np

import audit_dispersed_util as adu
import audit_util as au
from oracle.models import linrange

W = au.W
STARSHIP = dict(N=9, Nsub=51, steps=50)
NSUB = 5
FEAS_TOL = 1e-3


def input_scale(mdl):
    w = np.asarray(mdl.bbox()[1], float)
    w = w[:, 1] - w[:, 0]
    return np.where(w < 1e-8, 1.0, w)


def weights(Sx, Su):
    return 1.0 / Sx ** 2, 1.0 / Su ** 2, 10.0 / Sx ** 2


def flown_case(orc, name, N, seed=None):
    """(xd[N,nx], ud[N,nu], p, pp) with xd re-sampled from the oracle's propagate; seed = that of make_case (7 + N when None)"""
    if name == "starship":
        assert N == STARSHIP["N"]
        mdl = au.oracle_model(name, N)
        pp = mdl.nominal_pp()
        x, u, p = mdl.guess(N, pp)
        sub = STARSHIP["steps"]
    else:
        x, u, p, pp = au.make_case(name, N, 7 + N if seed is None else seed)
        sub = 4
    x, u, p, pp = (np.ascontiguousarray(a, float) for a in (x, u, p, pp))
    _, xc = orc.propagate(name, orc.default_params(name), N, x, u, p, res=sub * (N - 1) + 1)
    return np.ascontiguousarray(xc[::sub]), u, p, pp


def oracle_dynamics(orc, name, N, Nsub, xd, ud, p, Sx):
    """(A[N-1,nx,nx], Bm[N-1,nu,nx], Bp[N-1,nu,nx]) of ONE problem in the library's memory order: block k transposed is the matrix"""
    o = orc.discretize(name, orc.default_params(name), N, Nsub, xd[None], ud[None], p[None], 1.0 / Sx, FEAS_TOL)
    return o["A"][0].copy(), o["Bm"][0].copy(), o["Bp"][0].copy()


def riccati(A, Bm, Bp, qx, ru, qf):
    """the recursion of the header over memory-order blocks -> (K[N-1,nu,nx] math layout, info[4])"""
    M, nx, nu = A.shape[0], A.shape[1], Bm.shape[1]
    Q, R, P = np.diag(qx), np.diag(ru), np.diag(np.asarray(qf, float))
    K = np.zeros((M, nu, nx))
    with np.errstate(all="ignore"):
        for k in range(M - 1, -1, -1):
            Phi, Gam = A[k].T, (Bm[k] + Bp[k]).T
            H = R + Gam.T @ P @ Gam
            K[k] = np.linalg.solve(H, Gam.T @ P @ Phi)
            P = Q + Phi.T @ P @ (Phi - Gam @ K[k])
            P = 0.5 * (P + P.T)
    return K, np.array([0.0, np.abs(K).max(), np.trace(P), 0.0])


def to_lib(K):
    """K[..., nu, nx] math layout -> the library's memory order [..., nx, nu]"""
    return np.ascontiguousarray(np.swapaxes(K, -1, -2))


class TrackingReference(au.Reference):
    """ONE closed-loop flight on the CPU, in the form audit_util.Reference.check reads, and the per-node efforts and errors.
    par = the C oracle's parameter vector, mdl = the oracle model instance (a truth model: both with the constants overridden)"""

    def __init__(self, orc, name, N, xd, ud, p, pp, Sx, Su, K, steps, dx0, gain, bias, par=None, mdl=None):
        par = orc.default_params(name) if par is None else par
        mdl = au.oracle_model(name, N) if mdl is None else mdl
        res = steps * (N - 1) + 1
        self.name, self.res = name, res
        tgrid = linrange(0.0, 1.0, N)
        tc = np.array([(1 - j / (res - 1)) * 0.0 + (j / (res - 1)) * 1.0 for j in range(res)])
        self.tc = tc
        ct = mdl.cost_terms()
        nu = ud.shape[1]
        x, du = xd[0] + dx0, np.zeros(nu)
        self.effort, self.track = np.zeros(N - 1), np.zeros(N)

        def flown(t):
            return gain * (au._input(tgrid, ud, t) + du) + bias

        def f(t, xs):
            return orc.model_eval(name, par, t, N, xs, flown(t), p)[0]

        fam, scale, gam, par_max = np.full((res, 3), -np.inf), np.ones((res, 3)), np.zeros(res), -np.inf

        def sample(j):
            nonlocal par_max
            t = tc[j]
            k = max(int(np.sum(tgrid <= t)), 1)
            fam[j], scale[j], pm, gam[j] = au._sample(name, mdl, ct, t, k, x, flown(t), p)
            par_max = max(par_max, pm)

        def node(k):
            nonlocal du
            e = x - xd[k - 1]
            self.track[k - 1] = np.abs(e / Sx).max()
            if k < N:
                du = -(K[k - 1] @ e)
                self.effort[k - 1] = np.abs(du / Su).max()

        node(1)
        sample(0)
        for j in range(res - 1):
            if j > 0 and j % steps == 0:
                node(j // steps + 1)
            t, h = tc[j], tc[j + 1] - tc[j]
            k1 = f(t, x)
            k2 = f(t + h / 2, x + h / 2 * k1)
            k3 = f(t + h / 2, x + h / 2 * k2)
            k4 = f(t + h, x + h * k3)
            x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
            sample(j + 1)
        node(N)
        self.fam, self.scale = fam, scale
        rec = np.zeros(W)
        for i in range(3):
            if np.isfinite(fam[:, i]).any():
                j = int(np.argmax(fam[:, i]))
                rec[2 * i], rec[2 * i + 1] = fam[j, i], tc[j]
            else:
                rec[2 * i], rec[2 * i + 1] = -np.inf, 0.0
        rec[6] = par_max
        rec[7] = np.abs(mdl.gtc(x, p, pp)).max()
        rec[8] = np.abs((x - xd[-1]) / Sx).max()
        phi = ct["tx"] @ x + (ct["tp"] @ p + ct["Qp"] @ (p * p) if p.size else 0.0)
        rec[9] = phi + sum(0.5 * (tc[j + 1] - tc[j]) * (gam[j + 1] + gam[j]) for j in range(res - 1))
        rec[12], rec[13] = self.effort.max(), float(np.argmax(self.effort) + 1)
        rec[14], rec[15] = self.track.max(), float(np.argmax(self.track) + 1)
        self.worst = fam.max(axis=1)
        self.rec = rec
        assert np.isfinite(rec[[7, 8, 9, 12, 14]]).all() and np.isfinite(self.worst).all(), (name, N, steps, "the reference is not finite")

    def check_tracking(self, got, viol_tol, tag=""):
        got = np.asarray(got, float)
        head = got.copy()
        head[12:] = 0.0
        self.check(head, viol_tol, tag)
        print("%s ref[12:] %s got[12:] %s" % (tag, self.rec[12:], got[12:]))
        for i, per_node in ((12, self.effort), (14, self.track)):
            tol = au.RTOL * max(1.0, abs(self.rec[i]))
            assert abs(got[i] - self.rec[i]) <= tol, (tag, i, got[i], self.rec[i], tol)
            k = got[i + 1]
            assert k == int(k) and 1 <= k <= per_node.size, (tag, i + 1, k)
            assert abs(per_node[int(k) - 1] - self.rec[i]) <= tol, (tag, i + 1, k, per_node[int(k) - 1], self.rec[i])


def fold(R):
    """the dispersed fold over [0..11] of the flight records, marked 3.0"""
    S = adu.fold(R)
    S[13] = 3.0
    return S


def flights4(name, N):
    """(dx0[4,nx], ugain[4,nu], ubias[4,nu]): the three of audit_dispersed_util.dispersions and the benefit test's dx0-only flight"""
    dx0, gain, bias = adu.dispersions(name, N, np.random.default_rng(1000 + N))
    Sx = au.state_scale(au.oracle_model(name, N))
    extra = 0.01 * Sx * np.random.default_rng(100 + N).standard_normal(Sx.size)
    one, zero = np.ones((1, gain.shape[1])), np.zeros((1, gain.shape[1]))
    return np.vstack([dx0, extra[None]]), np.vstack([gain, one]), np.vstack([bias, zero])


_cache = {}


def setup(orc, name, N):
    """everything about one flown case that needs no flight, computed once per session: a dict with case = (xd, ud, p, pp), Sx, Su,
    Nsub, steps_default, weights (qx, ru, qf), dyn = (A, Bm, Bp) in memory order, K [N-1,nu,nx], info, disp = the four flights"""
    key = (name, N)
    if key not in _cache:
        mdl = au.oracle_model(name, N)
        Sx, Su = au.state_scale(mdl), input_scale(mdl)
        case = flown_case(orc, name, N)
        Nsub = STARSHIP["Nsub"] if name == "starship" else NSUB
        dyn = oracle_dynamics(orc, name, N, Nsub, *case[:3], Sx)
        w = weights(Sx, Su)
        K, info = riccati(*dyn, *w)
        assert np.isfinite(K).all(), (name, N, "the reference gains are not finite")
        _cache[key] = dict(case=case, Sx=Sx, Su=Su, Nsub=Nsub, weights=w, dyn=dyn, K=K, info=info, disp=flights4(name, N))
    return _cache[key]


def batch(orc, name, N, B):
    """B flown cases stacked for a device call: setup(name, N)'s first, then seeds 3000 + i (the Starship: B copies of its one
    configuration) -> (cases, xd[B,N,nx], ud, p, pp)"""
    first = setup(orc, name, N)["case"]
    key = ("batch", name, N, B)
    if key not in _cache:
        _cache[key] = [first] + [first if name == "starship" else flown_case(orc, name, N, 3000 + i) for i in range(1, B)]
    cases = _cache[key]
    return (cases,) + tuple(np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4))


_flights = {}


def references(orc, name, N, steps, K=None, which=(0, 1, 2, 3), Sx=None, Su=None, truth=None, case=None, disp=None, key=None):
    """[TrackingReference per flight in `which`] of setup(name, N) (or of `case` / `disp` given, cached under `key`) with the
    reference gains (or K given: K = 0 is the open-loop flight)"""
    s = setup(orc, name, N)
    ck = (name, N, steps, key, None if K is None else K.tobytes(), None if Sx is None else Sx.tobytes(), None if Su is None else Su.tobytes(),
          truth is not None)
    case = s["case"] if case is None else case
    disp = s["disp"] if disp is None else disp
    out = []
    for d in which:
        if ck + (d,) not in _flights:
            extra = {} if truth is None else dict(par=truth[0], mdl=truth[1])
            _flights[ck + (d,)] = TrackingReference(orc, name, N, *case, s["Sx"] if Sx is None else Sx, s["Su"] if Su is None else Su,
                                                    s["K"] if K is None else K, steps, disp[0][d], disp[1][d], disp[2][d], **extra)
        out.append(_flights[ck + (d,)])
    return out
