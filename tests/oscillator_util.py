"""TEST INFRASTRUCTURE shared by the oscillator tests: the reference of the compiled oscillator model
(scptoolbox.jl_amd/csrc/models/oscillator.hpp).  The C oracle (oracle/scp_oracle.c) selects its models by name and knows no
oscillator, so everything the oracle's PTR restatement (oracle/ptr_ref.py, used UNCHANGED) needs is restated here in numpy:

  * `Oscillator`: the closures of test/examples/oscillator/definition.jl in the oracle's model interface (oracle/models.py):
    X / U as cone rows (the L1 cones of a scalar argument as the two NONPOS rows +-y - t <= 0), s / C / D / G with the smooth OR
    of src/utils/helper.jl:623-807, boundary conditions, cost_terms, guess, bbox;
  * `discretize`: `discretize!` of src/solvers/discretization.jl:160-217 with derivs_foh (:235-286), derivs_impulse (:304-340)
    and set_update_matrices (:354-406), for any model given as f / A / B / F closures -- checked against the C oracle on the
    double integrator by tests/test_oscillator_cpu.py;
  * `ptr_solve` / `homotopy`: the loop of src/solvers/ptr.jl:448-532 around ptr_ref.solve_subproblem and
    ptr_ref.solution_deviation with that discretisation, and the warm-started homotopy of oscillator/tests.jl:60-77.
"""
import math

import numpy as np

from oracle import ipm, ptr_ref
from oracle.models import linrange

# the five Monte-Carlo instances pp = (r0, v0) of the fixture tests/golden/oscillator_outcomes_n12.npz
INSTANCES = np.array([[0.15, 0.0], [0.4, 0.0], [1.0, 0.0], [0.7, 0.2], [-0.5, -0.1]])
LOG99 = math.log(1.0 / 1e-2 - 1.0)
KAPPA3 = [LOG99, LOG99 * 1e4, LOG99 * 1e8]            # Homotopy(1e-8) at x = 0, 1/2, 1 (src/utils/homotopy.jl:66-73)
KAPPA10 = [LOG99 / (1e-8 ** x) for x in linrange(0.0, 1.0, 10)]     # oscillator/tests.jl:60-62


def smooth_or(pred, grad, kappa, match, normalize):
    """or(predicates, gradient; kappa, match, normalize) -> (OR, dOR), helper.jl:775-807, through indicator (:724-749), sigmoid
    (:672-701) and logsumexp (:623-651), in the reference's order of operations."""
    f = np.asarray(pred, float) / normalize
    g = np.asarray(grad, float) / normalize
    mt = np.atleast_1d(np.asarray(match, float) / normalize)

    def logsumexp(v, dv):
        a = np.max(kappa * v)
        e = np.exp(kappa * v - a)
        E = e.sum()
        return (a + math.log(E)) / kappa, None if dv is None else float((dv * (e / E)).sum())

    def sigmoid(v, dv):
        with np.errstate(over="ignore", divide="ignore"):
            L, dL = logsumexp(v, dv)
            sig = 1.0 - 1.0 / (1.0 + np.exp(kappa * L))
            if dv is None:
                return sig, None
            c = np.exp(kappa * L + 2.0 * np.log(1.0 - sig))
            return sig, kappa * c * dL
    offset, _ = sigmoid(mt, None)
    sig, dsig = sigmoid(f, g)
    return float(sig + (1.0 - offset)), float(dsig)


class Oscillator:
    """test/examples/oscillator/{parameters,definition}.jl in the interface of oracle/models.py; N fixes np = N."""
    name = "oscillator"
    nx, nu, ns, nic, ntc = 2, 4, 2, 2, 0
    np_dyn = 0
    zeta, w0, a_db, a_max = 0.5, 1.0, 0.05, 0.3                        # parameters.jl:81-85
    tf, alpha, gamma, r_nrml = 10.0, 0.06, 1e-1, 1.0                   # :102-108 (r_nrml = traj.r0)

    def __init__(self, N, kappa1=1.0):
        self.N, self.np, self.kappa1 = int(N), int(N), float(kappa1)

    def par(self):
        return np.array([self.zeta, self.w0, self.a_db, self.a_max, self.tf, self.kappa1, self.alpha, self.gamma, self.r_nrml])

    def nominal_pp(self):
        return np.array([1.0, 0.0])

    def bbox(self):      # set_scale!, definition.jl:47-69, from the nominal r0 and v0 = 0
        a = self.a_max
        return (np.array([[-self.r_nrml, self.r_nrml], [0.0, 0.0]]), np.array([[-a, a], [-a, a], [0.0, a], [0.0, 2 * a]]),
                np.tile([[0.0, self.r_nrml]], (self.np, 1)))

    # -- dynamics (definition.jl:161-236); k < 0: the impulse response
    def Amat(self):
        return self.tf * np.array([[0.0, 1.0], [-self.w0 ** 2, -2.0 * self.zeta * self.w0]])

    def f(self, t, k, x, u, p):
        if k < 0:
            return np.array([0.0, u[0]])
        return self.tf * np.array([x[1], u[0] - self.w0 ** 2 * x[0] - 2.0 * self.zeta * self.w0 * x[1]])

    def A(self, t, k, x, u, p):
        return self.Amat()

    def B(self, t, k, x, u, p):
        B = np.zeros((2, 4)); B[1, 0] = 1.0
        return B if k < 0 else self.tf * B

    def F(self, t, k, x, u, p):
        return np.zeros((2, 0))

    def guess(self, N, pp):      # definition.jl:71-114
        A = self.Amat()
        tg = linrange(0.0, 1.0, 1000)
        X = np.zeros((1000, 2)); X[0] = np.asarray(pp, float)[:2]
        for i in range(999):     # rk4_core_step, helper.jl:411-424
            h, x = tg[i + 1] - tg[i], X[i]
            k1 = A @ x; k2 = A @ (x + h / 2 * k1); k3 = A @ (x + h / 2 * k2); k4 = A @ (x + h * k3)
            X[i + 1] = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        x = np.zeros((N, 2))
        for k, tau in enumerate(linrange(0.0, 1.0, N)):      # linterp with get_interval, helper.jl:84-118
            i = max(int((tau > tg).sum()), 1) - 1
            c = (tg[i + 1] - tau) / (tg[i + 1] - tg[i])
            x[k] = c * X[i] + (1.0 - c) * X[i + 1]
        return x, np.zeros((N, 4)), np.abs(x[:, 0]).copy()

    # -- cost (definition.jl:116-142): Gamma = l1r_k / r_nrml + alpha l1aa / a_max + gamma l1adiff / a_max.  The oracle's cost
    # form has no per-node running term; tp of length N with the trapezoid weights expresses the same sum
    def cost_terms(self):
        w = ptr_ref._trapz_weights(linrange(0.0, 1.0, self.N))
        return dict(Qu=np.zeros(4), lu=np.array([0.0, 0.0, self.alpha / self.a_max, self.gamma / self.a_max]), lx=np.zeros(2),
                    tx=np.zeros(2), tp=w / self.r_nrml, Qp=np.zeros(self.np))

    # -- convex sets (definition.jl:238-368)
    def X(self, t, k):
        rows = []
        for sg in (1.0, -1.0):
            Mp = np.zeros((1, self.np)); Mp[0, k - 1] = -1.0
            rows.append(("NONPOS", np.array([[sg, 0.0]]), Mp, np.zeros(1)))
        return rows

    def U(self, t, k):
        a, Z = self.a_max, np.zeros((1, self.np))
        rows = [("NONPOS", np.array([[1.0, 0, 0, 0]]), Z, np.array([-a])), ("NONPOS", np.array([[-1.0, 0, 0, 0]]), Z, np.array([-a])),
                ("NONPOS", np.array([[0, 1.0, 0, 0]]), Z, np.array([-a])), ("NONPOS", np.array([[0, -1.0, 0, 0]]), Z, np.array([-a]))]
        for sg in (1.0, -1.0):
            rows.append(("NONPOS", np.array([[sg, 0, -1.0, 0]]), Z, np.zeros(1)))
        for sg in (1.0, -1.0):
            rows.append(("NONPOS", np.array([[sg, -sg, 0, -1.0]]), Z, np.zeros(1)))
        return rows

    # -- non-convex deadband (definition.jl:370-444)
    def _or(self, ar):
        n = self.a_max - self.a_db
        return smooth_or([ar - self.a_db, -self.a_db - ar], [1.0, -1.0], self.kappa1, n, n)

    def s(self, t, k, x, u, p):
        OR, _ = self._or(u[1])
        return np.array([u[0] - OR * u[1], OR * u[1] - u[0]])

    def C(self, t, k, x, u, p):
        return np.zeros((2, 2))

    def D(self, t, k, x, u, p):
        OR, dOR = self._or(u[1])
        d = dOR * u[1] + OR
        return np.array([[1.0, -d, 0, 0], [-1.0, d, 0, 0]])

    def G(self, t, k, x, u, p):
        return np.zeros((2, self.np))

    # -- boundary conditions (definition.jl:446-473): initial condition only
    def gic(self, x, p, pp):
        return x - np.asarray(pp, float)[:2]

    def H0(self, x, p, pp):
        return np.eye(2)

    def K0(self, x, p, pp):
        return np.zeros((2, self.np))

    def gtc(self, x, p, pp):
        return np.zeros(0)

    def Hf(self, x, p, pp):
        return np.zeros((0, 2))

    def Kf(self, x, p, pp):
        return np.zeros((0, self.np))


def _rk4(f, V, tgrid):      # rk4 over a grid by rk4_core_step, helper.jl:379-424
    for j in range(len(tgrid) - 1):
        t, h = tgrid[j], tgrid[j + 1] - tgrid[j]
        k1 = f(t, V); k2 = f(t + h / 2, V + h / 2 * k1); k3 = f(t + h / 2, V + h / 2 * k2); k4 = f(t + h, V + h * k3)
        V = V + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return V


def discretize_arrays(mdl, N, Nsub, x, u, p, iSx, feas_tol, method="foh"):
    """discretize! (discretization.jl:160-217) for one trajectory of any model with f / A / B / F closures; math-layout
    outputs A[N-1,nx,nx], Bm, Bp[N-1,nx,nu], F[N-1,nx,npF], r[N-1,nx], E[N-1,nx,nx], defect[N-1,nx], feas.  IMPULSE: Bm holds the
    single input matrix A_k B(t_k, -k) (:384-390), Bp is zero."""
    nx, nu = mdl.nx, mdl.nu
    npF = mdl.F(0.0, 1, x[0], u[0], p).shape[1]
    t = linrange(0.0, 1.0, N)
    imp = method == "impulse"
    o = np.cumsum([0, nx, nx * nx, nx * nu, nx * nu, nx * npF, nx, nx * nx])      # x, Phi, B-, B+, F, r, E (column-major blocks)
    col = lambda M: np.asarray(M).reshape(-1, order="F")
    out = dict(A=np.zeros((N - 1, nx, nx)), Bm=np.zeros((N - 1, nx, nu)), Bp=np.zeros((N - 1, nx, nu)), F=np.zeros((N - 1, nx, npF)),
               r=np.zeros((N - 1, nx)), E=np.zeros((N - 1, nx, nx)), defect=np.zeros((N - 1, nx)))
    feas = True
    for k in range(N - 1):
        tspan = t[k:k + 2]

        def derivs(tt, V):      # derivs_foh :235-286 / derivs_impulse :304-340
            xs = V[o[0]:o[1]]
            Phi = V[o[1]:o[2]].reshape(nx, nx, order="F")
            if imp:
                us = np.zeros(nu)
                sm = sp = 0.0
            else:
                tc = max(tspan[0], min(tspan[1], tt))      # linterp, helper.jl:107-118
                c = (tspan[1] - tc) / (tspan[1] - tspan[0])
                us = c * u[k] + (1 - c) * u[k + 1]
                sm = (tspan[1] - tt) / (tspan[1] - tspan[0]); sp = (tt - tspan[0]) / (tspan[1] - tspan[0])
            f = mdl.f(tt, k + 1, xs, us, p); A = mdl.A(tt, k + 1, xs, us, p); B = mdl.B(tt, k + 1, xs, us, p)
            F = mdl.F(tt, k + 1, xs, us, p)
            r = f - A @ xs - (0.0 if imp else B @ us) - (F @ p[:npF] if npF else 0.0)
            iPhi = np.linalg.solve(Phi, np.eye(nx))
            return np.concatenate([f, col(A @ Phi), col(iPhi @ (sm * B)), col(iPhi @ (sp * B)), col(iPhi @ F), iPhi @ r, col(iPhi)])
        V0 = np.zeros(o[-1])
        V0[o[1]:o[2]] = col(np.eye(nx))
        V0[o[0]:o[1]] = x[k] + mdl.f(t[k], -(k + 1), x[k], u[k], p) if imp else x[k]      # :184-193
        V = _rk4(derivs, V0, linrange(t[k], t[k + 1], Nsub))
        Ak = V[o[1]:o[2]].reshape(nx, nx, order="F")      # set_update_matrices :354-406
        out["A"][k] = Ak
        if imp:
            out["Bm"][k] = Ak @ mdl.B(t[k], -(k + 1), x[k], u[k], p)
        else:
            out["Bm"][k] = Ak @ V[o[2]:o[3]].reshape(nx, nu, order="F")
            out["Bp"][k] = Ak @ V[o[3]:o[4]].reshape(nx, nu, order="F")
        out["F"][k] = Ak @ V[o[4]:o[5]].reshape(nx, npF, order="F")
        out["r"][k] = Ak @ V[o[5]:o[6]]
        out["E"][k] = Ak @ V[o[6]:o[7]].reshape(nx, nx, order="F")
        out["defect"][k] = x[k + 1] - V[o[0]:o[1]]
        if np.abs(iSx * out["defect"][k]).max() > feas_tol:
            feas = False
    out["feas"] = feas
    return out


def discretize_variational(mdl, N, Nsub, x, u, p):
    """The variational form of discretize! the library's K1v kernel integrates for constant Jacobians (Psi' = A Psi + rhs(t),
    Psi(t_k) = 0; csrc/discretize_kernel.hpp) -- A, Bm, Bp, r, E in math layout: what the oscillator's var_form_max_step was
    measured with (against `discretize_arrays`)."""
    nx, nu = mdl.nx, mdl.nu
    t = linrange(0.0, 1.0, N)
    out = dict(A=np.zeros((N - 1, nx, nx)), Bm=np.zeros((N - 1, nx, nu)), Bp=np.zeros((N - 1, nx, nu)), r=np.zeros((N - 1, nx)),
               E=np.zeros((N - 1, nx, nx)))
    for k in range(N - 1):
        t0, t1 = t[k], t[k + 1]
        A = mdl.A(t0, k + 1, x[k], u[k], p); B = mdl.B(t0, k + 1, x[k], u[k], p)
        W = nx + 2 * nu + nx + 1

        def derivs(tt, V):
            M = V[nx:].reshape(nx, W, order="F")
            xs = V[:nx]
            tc = max(t0, min(t1, tt)); c = (t1 - tc) / (t1 - t0)
            us = c * u[k] + (1 - c) * u[k + 1]
            sm, sp = (t1 - tt) / (t1 - t0), (tt - t0) / (t1 - t0)
            f = mdl.f(tt, k + 1, xs, us, p)
            rhs = np.hstack([np.zeros((nx, nx)), sm * B, sp * B, np.eye(nx), (f - A @ xs - B @ us)[:, None]])
            return np.concatenate([f, (A @ M + rhs).reshape(-1, order="F")])
        M0 = np.hstack([np.eye(nx), np.zeros((nx, W - nx))])
        V = _rk4(derivs, np.concatenate([x[k], M0.reshape(-1, order="F")]), linrange(t0, t1, Nsub))
        M = V[nx:].reshape(nx, W, order="F")
        out["A"][k] = M[:, :nx]; out["Bm"][k] = M[:, nx:nx + nu]; out["Bp"][k] = M[:, nx + nu:nx + 2 * nu]
        out["E"][k] = M[:, nx + 2 * nu:2 * nx + 2 * nu]; out["r"][k] = M[:, -1]
    return out


def variational_vs_reference(N, Nsub, seed=0):
    """largest relative difference (per block, scaled by max(1, |block|_max)) between the two forms on a perturbed trajectory"""
    mdl = Oscillator(N)
    rng = np.random.default_rng(seed)
    x, u, p = mdl.guess(N, mdl.nominal_pp())
    x = x + 0.1 * rng.standard_normal(x.shape); u = 0.3 * rng.uniform(-1, 1, u.shape)
    a = discretize_arrays(mdl, N, Nsub, x, u, p, np.ones(2), 1.0)
    b = discretize_variational(mdl, N, Nsub, x, u, p)
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(a[k]).max()) for k in ("A", "Bm", "Bp", "r", "E"))


def discretize(mdl, pars, scale, x, u, p, method="foh"):
    """the SubproblemSolution of oracle/ptr_ref.py::discretize from the numpy discretisation"""
    o = discretize_arrays(mdl, pars.N, pars.Nsub, x, u, p, 1.0 / scale.Sx, pars.feas_tol, method)
    s = ptr_ref.Sol()
    s.xd, s.ud, s.p = x, u, p
    s.A, s.Bm, s.Bp, s.r, s.E = o["A"], o["Bm"], o["Bp"], o["r"], o["E"]
    s.F = np.zeros((pars.N - 1, mdl.nx, mdl.np))
    s.F[:, :, :o["F"].shape[2]] = o["F"]
    s.defect, s.feas = o["defect"], bool(o["feas"])
    s.J_aug = np.nan      # ptr.jl:350
    return s


def reference_pars(N, Nsub=10, iter_max=10):
    """PTR.Parameters of oscillator/tests.jl:24-57"""
    return ptr_ref.PTRParameters(N, Nsub, iter_max, 1e2, 1e-3, -np.inf, 1e-3 / 100, 5e-3)


def ptr_solve(mdl, pars, pp, guess=None, ipm_opts=None):
    """PTR.solve(pbm, warm) for one problem (src/solvers/ptr.jl:448-532; the loop of oracle/ptr_ref.py::ptr_solve with the
    discretisation above).  Returns (status, history); history[i] = dict(sub, sol, ref, stop)."""
    scale = ptr_ref.Scaling(*mdl.bbox())
    x, u, p = mdl.guess(pars.N, pp) if guess is None else guess
    ref = discretize(mdl, pars, scale, x, u, p)
    hist, k, status = [], 1, "SCP_SOLVED"
    while True:
        sub = ptr_ref.solve_subproblem(mdl, pars, scale, ref, pp, ipm_opts)
        sol = discretize(mdl, pars, scale, sub["x"], sub["u"], sub["p"])
        sol.J_aug = sub["J_aug"]
        if sub["status"] not in (ipm.OPTIMAL, ipm.ALMOST_OPTIMAL):
            status = "SCP_FAILED (%s)" % sub["status"]
            hist.append(dict(sub=sub, sol=sol, ref=ref, stop=False)); break
        dev = ptr_ref.solution_deviation(scale, pars, ref, sol)
        improv = (ref.J_aug - sol.J_aug) / abs(ref.J_aug) if not np.isnan(ref.J_aug) else np.nan
        stop = k > 1 and (sol.feas and (abs(improv) <= pars.eps_rel or dev <= pars.eps_abs))
        hist.append(dict(sub=sub, sol=sol, ref=ref, stop=stop))
        if stop:
            break
        ref = sol
        k += 1
        if k > pars.iter_max:
            break
    return status, hist


def homotopy(N, Nsub, kappas, pp, iter_max=10):
    """oscillator/tests.jl:60-77: one solve per kappa1, each warm-started with the previous SOLUTION.  Returns a list of
    (status, history) per stage."""
    mdl = Oscillator(N)
    pars = reference_pars(N, Nsub, iter_max)
    out, warm = [], None
    for kap in kappas:
        mdl.kappa1 = float(kap)
        st, hist = ptr_solve(mdl, pars, np.asarray(pp, float), guess=warm)
        last = hist[-1]["sol"]
        warm = (last.xd, last.ud, last.p)
        out.append((st, hist))
    return out
