"""SCvx on the MI355X behind the reference's solver contract (src/solvers/scvx.jl).

    pars = SCvx.Parameters(N=30, Nsub=15, iter_max=15, lam=30, rho_0=0, rho_1=0.1, rho_2=0.7, beta_sh=2, beta_gr=2,
                           eta_init=1, eta_lb=1e-3, eta_ub=10, eps_abs=0, eps_rel=0, feas_tol=1e-3)
    pbm = SCvx.create(pars, traj, batch_capacity=B)        # scvx.jl:160-206
    sol, history = SCvx.solve(pbm, pp)                     # scvx.jl:459-540

The subproblem (hard trust region ||dx||_q + ||du||_q + ||dp||_q <= eta, scvx.jl:578-678; cost L + lambda (trapz P +
sum Pf), :804-901) and the guess projection `correct_convex!` (scp.jl:275-361) are formulated once as conic templates
(subproblem.py); the whole loop -- discretize!, formulate, solve, check_stopping_criterion! (:711-734),
update_trust_region! (:753-769, 1000-1045) -- runs on the device (csrc/scp_generic.hip)."""
import numpy as np

from . import _lib
from .conic import default_options
from .generic import GenericSubproblem, LoopProblem, SCPSolutionBatch, solve_projected  # noqa: F401
from .scp import FOH
from .subproblem import ModelRows, build_correct_convex, build_scvx

H_NAMES = ("L", "L_pen", "L_aug", "J_ref", "J_sol", "pre_improv", "act_improv", "rho", "eta", "eta_next", "accepted", "stop",
           "deviation", "feas", "solver_status", "solver_iters")


class Parameters:
    """SCvx.Parameters, src/solvers/scvx.jl:60-81 (lam = λ, rho_i = ρ_i, beta_* = β_*, eta_* = η_*)."""

    def __init__(self, N, Nsub, iter_max, lam, rho_0, rho_1, rho_2, beta_sh, beta_gr, eta_init, eta_lb, eta_ub, eps_abs=0.0,
                 eps_rel=0.0, feas_tol=1e-3, q_tr=np.inf, q_exit=np.inf, disc_method=FOH, solver_opts=None):
        if not q_exit >= 1:
            raise ValueError("q_exit must be >= 1 or Inf (norm of solution_deviation, scp.jl:909-931)")
        self.N, self.Nsub, self.iter_max, self.lam = N, Nsub, iter_max, lam
        self.rho_0, self.rho_1, self.rho_2, self.beta_sh, self.beta_gr = rho_0, rho_1, rho_2, beta_sh, beta_gr
        self.eta_init, self.eta_lb, self.eta_ub = eta_init, eta_lb, eta_ub
        self.eps_abs, self.eps_rel, self.feas_tol, self.q_tr, self.q_exit = eps_abs, eps_rel, feas_tol, q_tr, q_exit
        self.disc_method = disc_method
        self.solver_opts = dict(solver_opts or {})

    def c_struct(self):
        c = _lib.ScpScvxParams()
        for k in ("iter_max", "lam", "rho_0", "rho_1", "rho_2", "beta_sh", "beta_gr", "eta_init", "eta_lb", "eta_ub",
                  "eps_abs", "eps_rel", "q_exit"):
            setattr(c, k, getattr(self, k))
        c.solver = default_options(**self.solver_opts)
        return c


class SCvxProblem(LoopProblem):
    def __init__(self, pars, traj, batch_capacity=1, device=0):
        super().__init__(pars, traj, batch_capacity, device)
        mr = ModelRows(traj.mdl)
        self.template = build_scvx(mr, pars.N, self.scale, pars.lam, pars.q_tr)
        self.sub = GenericSubproblem(self, self.template)
        self.proj = GenericSubproblem(self, build_correct_convex(mr, pars.N, self.scale))


def create(pars, traj, batch_capacity=1, device=0):
    return SCvxProblem(pars, traj, batch_capacity, device)


def solve(pbm, pp=None, guess=None, project_guess=True, all_reduce=None):
    """`SCvx.solve(pbm[, warm])` for a Monte-Carlo batch (pp[B,npp]); guess = (xd, ud, p) arrays or None (traj.guess).
    The guess is projected onto the convex sets first (correct_convex!, scvx.jl:555-565) unless project_guess=False."""
    L = _lib.lib()
    return solve_projected(pbm, (L.scp_scvx_init_host, L.scp_scvx_iterate, L.scp_scvx_get_host), pbm.pars.c_struct(), pp, guess,
                           project_guess, all_reduce, H_NAMES)
