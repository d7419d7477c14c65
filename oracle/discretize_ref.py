"""CPU ORACLE (test infrastructure, NOT product code): numpy restatement of `discretize!` for a numpy-dynamics model
(oracle/models.py), i.e. any model given as f / A / B / F(t, k, x, u, p) closures.

Follows, line by line:
  discretize!            src/solvers/discretization.jl:160-217
  derivs_foh             discretization.jl:235-286
  derivs_impulse         discretization.jl:304-340
  set_update_matrices    discretization.jl:354-406
plus the variational form that the library's K1v kernel integrates.  Checked against the C oracle on the double integrator,
which both know, by tests/test_oscillator_cpu.py.  oracle/ptr_ref.py::discretize is the caller inside the SCP loops.
"""
import numpy as np

from .models import Oscillator, linrange


def _rk4(f, V, tgrid, on_step=None):      # rk4 over a grid by rk4_core_step, helper.jl:379-424; on_step(j, V) at tgrid[j], j >= 1
    for j in range(len(tgrid) - 1):
        t, h = tgrid[j], tgrid[j + 1] - tgrid[j]
        k1 = f(t, V); k2 = f(t + h / 2, V + h / 2 * k1); k3 = f(t + h / 2, V + h / 2 * k2); k4 = f(t + h, V + h * k3)
        V = V + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        if on_step is not None:
            on_step(j + 1, V)
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
