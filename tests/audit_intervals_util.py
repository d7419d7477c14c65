"""CPU reference of the interval-parallel audit (include/scp_mi355x.h, scp_audit_intervals_*), shared by
tests/test_audit_intervals_cpu.py and tests/test_audit_intervals_gpu.py.  It takes nothing from the code under test.

Flight.  FOH: a numpy RK4 per interval over the oracle's C model evaluation (oracle.model_eval), the input being the first-order
hold of the interval's own two nodes.  IMPULSE: oracle.propagate_impulse, whose samples are exactly these sub-grids (called with
res = sub (N - 1) so that its ceil(res / (N - 1)) is the `sub` under test, the floor of 2 included).  Families, Gamma, gtc and
cost_terms come from the closures of oracle/models.py as in audit_util.Reference; under IMPULSE they see z = [x; ud[k]].

Tolerances: audit_util's.  A family maximum is compared with 1e-9 * max(1, largest absolute term entering
the row at the reference's arg-max sample); a reported time must be a sample time of the interval (to 4 ulp: the device may
contract (1 - s) a + s b into one fused multiply-add, which moves a time by at most one rounding) at which the reference's own
value is within that tolerance of the reference maximum; fields 7, 10, 11 and the summary's 7, 9 with 1e-9 * max(1, |ref|); the
defect with 1e-9 * max(1, |ref|, largest |Sx^-1 x| over that interval's reference samples); the counts are equal for a
viol_tol chosen by audit_util.choose_viol_tol over the per-sample worst values (duplicated node samples included)."""
import numpy as np

import audit_util as au
from oracle.discretize_ref import _rk4
from oracle.models import linrange

W, WI = 16, 16      # SCP_AUDIT_WIDTH, SCP_AUDIT_INTERVAL_WIDTH
FOH, IMPULSE = 0, 1
RTOL = au.RTOL
IMPULSE_MODELS = ("double_integrator", "quadrotor")
CASES = [(n, FOH) for n in au.AUDIT_MODELS] + [(n, IMPULSE) for n in IMPULSE_MODELS]
TIME_ULPS = 4


def sub_of(N, res):
    return max(2, -(-int(res) // (N - 1)))


def res_values(N):
    """sub = 2 (one step), sub = 3, and sub = 7 through the ceiling"""
    return (2, 3 * (N - 1), 6 * (N - 1) + 1)


class IntervalReference:
    """the interval audit of ONE problem on the CPU: per-sample family values [N-1, sub, 3], the records and the summary"""

    def __init__(self, orc, name, N, method, xd, ud, p, pp, Sx, res):
        mdl = au.oracle_model(name, N)
        par = orc.default_params(name)
        sub = sub_of(N, res)
        td = linrange(0.0, 1.0, N)
        self.name, self.N, self.sub, self.res = name, N, sub, res
        self.tg = np.array([linrange(td[k], td[k + 1], sub) for k in range(N - 1)])
        xc = np.zeros((N - 1, sub, xd.shape[1]))
        if method == IMPULSE:
            _, xi = orc.propagate_impulse(name, par, N, xd, ud, p, res=sub * (N - 1))
            xc[:] = xi[1:].reshape(N - 1, sub, -1)
        else:
            for k in range(N - 1):
                t0, t1 = td[k], td[k + 1]

                def f(t, x):
                    c = (t1 - min(max(t, t0), t1)) / (t1 - t0)
                    return orc.model_eval(name, par, t, N, x, c * ud[k] + (1.0 - c) * ud[k + 1], p)[0]
                xc[k, 0] = xd[k]

                def keep(j, x):
                    xc[k, j] = x
                _rk4(f, xd[k].copy(), self.tg[k], on_step=keep)
        self.xc = xc
        ct = mdl.cost_terms()
        fam, scale = np.full((N - 1, sub, 3), -np.inf), np.ones((N - 1, sub, 3))
        gam, par_max = np.zeros((N - 1, sub)), -np.inf
        for k in range(N - 1):
            for j in range(sub):
                t = self.tg[k, j]
                if method == IMPULSE:
                    u = ud[k]
                else:
                    c = (td[k + 1] - t) / (td[k + 1] - td[k])
                    u = c * ud[k] + (1.0 - c) * ud[k + 1]
                node = k + 2 if j == sub - 1 else k + 1          # 1-based node index handed to the model functions
                fam[k, j], scale[k, j], pm, gam[k, j] = au._sample(name, mdl, ct, t, node, xc[k, j], u, p)
                par_max = max(par_max, pm)
        self.fam, self.scale = fam, scale
        self.worst = fam.max(axis=2).ravel()
        self.worst_k = fam.max(axis=2)
        rec = np.zeros((N - 1, WI))
        self.defect_scale = np.ones(N - 1)
        for k in range(N - 1):
            for f in range(3):
                if np.isfinite(fam[k, :, f]).any():
                    j = int(np.argmax(fam[k, :, f]))
                    rec[k, 2 * f], rec[k, 2 * f + 1] = fam[k, j, f], self.tg[k, j]
                else:
                    rec[k, 2 * f], rec[k, 2 * f + 1] = -np.inf, 0.0
            rec[k, 6] = np.abs((xc[k, -1] - xd[k + 1]) / Sx).max()
            self.defect_scale[k] = max(1.0, rec[k, 6], np.abs(xc[k] / Sx[None, :]).max())
            rec[k, 7] = sum(0.5 * (self.tg[k, j + 1] - self.tg[k, j]) * (gam[k, j + 1] + gam[k, j]) for j in range(sub - 1))
        xf = xc[-1, -1]
        rec[-1, 10] = np.abs(mdl.gtc(xf, p, pp)).max()
        rec[-1, 11] = ct["tx"] @ xf + (ct["tp"] @ p + ct["Qp"] @ (p * p) if p.size else 0.0)
        self.rec = rec
        s = np.zeros(W)
        for f in range(3):
            k = int(np.argmax(rec[:, 2 * f]))
            s[2 * f], s[2 * f + 1] = rec[k, 2 * f], rec[k, 2 * f + 1]
        s[6], s[7], s[8], s[9] = par_max, rec[-1, 10], rec[:, 6].max(), rec[-1, 11] + rec[:, 7].sum()
        s[12], s[13], s[14] = int(np.argmax(rec[:, 6])) + 1, 1.0, sub
        self.summary = s

    def _family(self, tag, f, v, t, ks, vref, tol):
        """value v reported at time t for family f, the maximum over the intervals `ks` whose reference maximum is vref"""
        if not np.isfinite(vref):
            assert v == -np.inf and t == 0.0, (tag, f, v, t)
            return
        assert abs(v - vref) <= tol, (tag, "family", f, v, vref, tol)
        hit = [(k, j) for k in ks for j in range(self.sub) if abs(self.tg[k, j] - t) <= TIME_ULPS * np.finfo(float).eps * max(1.0, abs(t))]
        assert hit, (tag, "family", f, "reported time is not a sample time", t)
        assert any(abs(self.fam[k, j, f] - vref) <= tol for k, j in hit), (tag, "family", f, "time", t, vref, tol)

    def check(self, got_summary, got_intervals, viol_tol, tag=""):
        """assert that both outputs of the code under test, computed with `viol_tol`, agree with this reference"""
        S, R = np.asarray(got_summary, float), np.asarray(got_intervals, float)
        N = self.N
        assert S.shape == (W,) and R.shape == (N - 1, WI), (tag, S.shape, R.shape)
        print("%s ref %s\n%s got %s" % (tag, np.array2string(self.summary, precision=15), tag, np.array2string(S, precision=15)))
        assert (np.abs(self.worst - viol_tol) > 1e-6 * max(1.0, abs(viol_tol))).all(), (tag, "viol_tol too close to a sample", viol_tol)
        for k in range(N - 1):
            tk = "%s k=%d" % (tag, k + 1)
            for f in range(3):
                jr = int(np.argmax(self.fam[k, :, f]))
                self._family(tk, f, R[k, 2 * f], R[k, 2 * f + 1], [k], self.rec[k, 2 * f], RTOL * self.scale[k, jr, f])
            assert abs(R[k, 6] - self.rec[k, 6]) <= RTOL * self.defect_scale[k], (tk, "defect", R[k, 6], self.rec[k, 6], self.defect_scale[k])
            for i in (7, 10, 11):
                assert abs(R[k, i] - self.rec[k, i]) <= RTOL * max(1.0, abs(self.rec[k, i])), (tk, i, R[k, i], self.rec[k, i])
            if k < N - 2:
                assert R[k, 10] == 0.0 and R[k, 11] == 0.0, (tk, R[k, 10:12])
            assert R[k, 8] == float((self.worst_k[k] > viol_tol).sum()), (tk, "n_viol", R[k, 8], self.worst_k[k], viol_tol)
            assert R[k, 9] == 0.0 and not R[k, 12:].any(), (tk, R[k, 9:])
        for f in range(3):
            kr = int(np.argmax(self.rec[:, 2 * f]))
            jr = int(np.argmax(self.fam[kr, :, f]))
            self._family(tag, f, S[2 * f], S[2 * f + 1], range(N - 1), self.summary[2 * f], RTOL * self.scale[kr, jr, f])
        if np.isfinite(self.summary[6]):
            assert abs(S[6] - self.summary[6]) <= RTOL * max(1.0, abs(self.summary[6])), (tag, 6, S[6], self.summary[6])
        else:
            assert S[6] == -np.inf, (tag, 6, S[6])
        for i in (7, 9):
            assert abs(S[i] - self.summary[i]) <= RTOL * max(1.0, abs(self.summary[i])), (tag, i, S[i], self.summary[i])
        kd = int(np.argmax(self.rec[:, 6]))
        assert abs(S[8] - self.summary[8]) <= RTOL * self.defect_scale[kd], (tag, "largest defect", S[8], self.summary[8])
        ki = int(S[12])
        assert S[12] == ki and 1 <= ki <= N - 1, (tag, 12, S[12])
        assert abs(self.rec[ki - 1, 6] - self.summary[8]) <= RTOL * self.defect_scale[kd], (tag, "worst interval", ki, self.rec[ki - 1, 6], self.summary[8])
        assert S[10] == float((self.worst > viol_tol).sum()), (tag, "n_viol", S[10])
        assert S[11] == 0.0 and S[13] == 1.0 and S[14] == self.sub and S[15] == 0.0, (tag, S[11:])


def fold(R, par_max, has_par_rows, sub):
    """the ordered fold of the interval records R[N-1, 16] of one problem, operation by operation as the header states it"""
    S = np.zeros(W)
    v, t = [-np.inf] * 3, [0.0] * 3
    dmax, kmax, integral, n_viol = -np.inf, 0.0, 0.0, 0.0
    bad = has_par_rows and not np.isfinite(par_max)
    for k in range(R.shape[0]):
        for f in range(3):
            if R[k, 2 * f] > v[f]:
                v[f], t[f] = R[k, 2 * f], R[k, 2 * f + 1]
        if R[k, 6] > dmax:
            dmax, kmax = R[k, 6], float(k + 1)
        integral = integral + R[k, 7]
        n_viol = n_viol + R[k, 8]
        bad = bad or R[k, 9] != 0.0
    cost = R[-1, 11] + integral
    bad = bad or not np.isfinite(cost)
    S[0:6] = [v[0], t[0], v[1], t[1], v[2], t[2]]
    S[6:16] = [par_max, R[-1, 10], dmax, cost, n_viol, 1.0 if bad else 0.0, kmax, 1.0, float(sub), 0.0]
    return S


_cache = {}


def reference(orc, name, method, N, seed, res, Sx=None):
    """(case, IntervalReference) for audit_util.make_case(name, N, seed) at `res`: computed once per session and shared"""
    key = (name, method, N, seed, sub_of(N, res))
    if key not in _cache:
        case = au.make_case(name, N, seed)
        sx = au.state_scale(au.oracle_model(name, N)) if Sx is None else np.asarray(Sx, float)
        _cache[key] = (case, IntervalReference(orc, name, N, method, *case, sx, res), sx)
    case, ref, sx = _cache[key]
    assert Sx is None or np.array_equal(sx, Sx)
    return case, ref
