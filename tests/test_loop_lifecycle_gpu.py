"""Life cycle of the three device-resident outer loops of the generic conic path (csrc/scp_generic.hip: SCvx, GuSTO, PTR)
through the C ABI (-m gpu): what get_host answers before any iteration, an iterate past iter_max, a second init on the same
handle, and calls of another loop's entry points on a handle.  Quadrotor, N = 12, Nsub = 8, iter_max = 3; a batch of 3 on a
handle of capacity 4, i.e. smaller than the interleave stride.  No projection handle: the reference is the uploaded guess."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NSUB, ITER_MAX, B, CAP = 12, 8, 3, 3, 4
SCP_OK, SCP_ERR_BAD_ARGUMENT = 0, 1
LOOPS = ("scvx", "gusto", "ptr")


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Loop:
    """One problem handle with the template of `kind` and the raw entry points of every loop."""

    def __init__(self, pkg, kind):
        self.pkg, self.kind, self.L = pkg, kind, pkg._lib.lib()
        traj = pkg.TrajectoryProblem("quadrotor")
        if kind == "scvx":
            pars = pkg.SCvx.Parameters(N=N, Nsub=NSUB, iter_max=ITER_MAX, lam=30.0, rho_0=0.0, rho_1=0.1, rho_2=0.7, beta_sh=2.0,
                                       beta_gr=2.0, eta_init=1.0, eta_lb=1e-3, eta_ub=10.0, eps_abs=1e-4, eps_rel=1e-3)
            self.pbm = pkg.SCvx.create(pars, traj, batch_capacity=CAP)
            self.sub, self.cp = self.pbm.sub, pars.c_struct()
        elif kind == "gusto":       # the reference's quadrotor parameters (test/examples/quadrotor/tests.jl:86-130)
            pars = pkg.GuSTO.Parameters(N=N, Nsub=NSUB, iter_max=ITER_MAX, lam_init=1e4, lam_max=1e9, rho_0=0.1, rho_1=0.9,
                                        beta_sh=2.0, beta_gr=2.0, gamma_fail=5.0, eta_init=10.0, eta_lb=1e-3, eta_ub=10.0, mu=0.8,
                                        iter_mu=6, eps_abs=1e-4, eps_rel=1e-3)
            self.pbm = pkg.GuSTO.create(pars, traj, batch_capacity=CAP)
            self.sub, self.cp = self.pbm.sub, pars.c_struct(self.pbm.template.nst)
        else:
            pars = pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=ITER_MAX, wvc=1e3, wtr=0.1, q_tr=1.0, q_exit=2.0)
            self.pbm = pkg.PTR.create(pars, traj, batch_capacity=CAP)
            self.sub = pkg.PTR._generic_sub(self.pbm)
            self.cp = pkg._lib.ScpPtrGenericParams()
            self.cp.iter_max, self.cp.wvc, self.cp.wtr, self.cp.eps_abs, self.cp.eps_rel = ITER_MAX, 1e3, 0.1, 1e-5, 1e-4
            self.cp.q_exit, self.cp.cost_const = 2.0, self.sub.T.cost_const
            self.cp.solver = pkg.conic.default_options()
        rng = np.random.default_rng(11)
        self.pp = np.stack([traj.mdl.nominal_pp() * (1 + 0.03 * rng.uniform(-1, 1, 12)) for _ in range(B)])
        g = [traj.guess(N, self.pp[b]) for b in range(B)]
        self.guess = [np.ascontiguousarray(np.stack([gi[j] for gi in g]), np.float64) for j in range(3)]

    def fn(self, what, kind=None):
        return getattr(self.L, "scp_%s_%s" % ({"scvx": "scvx", "gusto": "gusto", "ptr": "ptr_generic"}[kind or self.kind], what))

    def init(self):
        xd, ud, p = self.guess
        head = (self.sub._h, B, ctypes.byref(self.cp)) if self.kind == "ptr" else (self.sub._h, None, B, ctypes.byref(self.cp))
        return self.fn("init_host")(*head, _vp(xd), _vp(ud), _vp(p) if self.pbm.np else None, _vp(self.pp))

    def iterate(self, kind=None):
        na = ctypes.c_int(-1)
        return self.fn("iterate", kind)(self.sub._h, ctypes.byref(na)), na.value

    def get(self, kind=None):
        pbm = self.pbm
        out = dict(xd=np.zeros((B, N, pbm.nx)), ud=np.zeros((B, N, pbm.nu)), p=np.zeros((B, pbm.np)),
                   status=np.full(B, -1, np.int32), iterations=np.full(B, -1, np.int32),
                   cost=np.zeros((B, 4) if (kind or self.kind) == "ptr" else (2, B)), feas=np.zeros(B, np.uint8),
                   defect=np.zeros((B, N - 1, pbm.nx)), hist=np.full((ITER_MAX, B, self.pkg._lib.SCVX_HIST_WIDTH), -1.0))
        rc = self.fn("get_host", kind)(self.sub._h, _vp(out["xd"]), _vp(out["ud"]), _vp(out["p"]) if pbm.np else None,
                                       _vp(out["status"]), _vp(out["iterations"]), _vp(out["cost"]), _vp(out["feas"]),
                                       _vp(out["defect"]), _vp(out["hist"]))
        return rc, out

    def run(self):
        assert self.init() == SCP_OK
        for _ in range(ITER_MAX):
            rc, _na = self.iterate()
            assert rc == SCP_OK
        rc, out = self.get()
        assert rc == SCP_OK
        return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


@pytest.mark.parametrize("kind", LOOPS)
def test_loop_lifecycle(pkg, kind):
    assert pkg._lib.HIST_WIDTH == pkg._lib.SCVX_HIST_WIDTH      # one history buffer serves the three loops
    lp = Loop(pkg, kind)
    # ---- before any iteration: the reference, i.e. the uploaded guess; nothing done, nothing recorded ----
    assert lp.init() == SCP_OK
    rc, o0 = lp.get()
    assert rc == SCP_OK
    for k, g in zip(("xd", "ud", "p"), lp.guess):
        assert np.array_equal(o0[k], g.reshape(o0[k].shape)), k
    assert (o0["iterations"] == 0).all() and (o0["status"] == 0).all() and (o0["hist"] == 0.0).all()
    print(kind, "cost before the first iteration:", o0["cost"].tolist())
    if kind == "gusto":
        assert np.isnan(o0["cost"][0]).all()        # ref.J_aug = NaN before the first solve (cost[0] = J of the reference)
    if kind == "ptr":
        # J_aug of the guess is NaN too (ptr.jl:350), but scp_ptr_generic_get_host has no output for the reference's cost:
        # cost[B, 4] is the cost split of the LAST SUBPROBLEM, and none has been solved
        assert (o0["cost"] == 0.0).all()
    # ---- a full run, then one iterate too many: SCP_OK, nothing active, nothing changes ----
    for _ in range(ITER_MAX):
        rc, _na = lp.iterate()
        assert rc == SCP_OK
    rc, o1 = lp.get()
    assert rc == SCP_OK and (o1["iterations"] > 0).all()
    assert lp.iterate() == (SCP_OK, 0)
    rc, o2 = lp.get()
    assert rc == SCP_OK and _same(o1, o2)
    # ---- another loop's iterate / get_host refuse the handle and leave the run alone ----
    for other in LOOPS:
        if other != kind:
            assert lp.iterate(other)[0] == SCP_ERR_BAD_ARGUMENT, other
            assert lp.get(other)[0] == SCP_ERR_BAD_ARGUMENT, other
    rc, o3 = lp.get()
    assert rc == SCP_OK and _same(o1, o3)
    # ---- a second init on the same handle starts over: the same run again (1e-9: test_scvx_stopping_and_batch_independence) ----
    o4 = lp.run()
    assert np.array_equal(o4["status"], o1["status"]) and np.array_equal(o4["iterations"], o1["iterations"])
    for k in ("xd", "ud", "p", "cost", "hist"):
        assert np.allclose(o4[k], o1[k], rtol=0.0, atol=1e-9, equal_nan=True), (k, np.nanmax(np.abs(o4[k] - o1[k])))
    lp.pbm.close()
