"""Life cycle of the structured PTR run of a problem handle through the C ABI (-m gpu), in the style of
test_loop_lifecycle_gpu.py: what get_host answers before any iteration, an iterate past iter_max, restart, a second init with a
longer history, the stand-alone subproblem solve that ends a run, and who owns the handle's trajectory buffers when a generic
loop of a subproblem handle shares them.  double_integrator (no parameter vector) at N = 9 and quadrotor (one parameter) at
N = 8, Nsub = 4, iter_max = 2, eps_abs = eps_rel = 0; a batch of 3 on a handle of capacity 4."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSUB, ITER_MAX, B, CAP = 4, 2, 3, 4
SCP_OK, SCP_ERR_BAD_ARGUMENT = 0, 1
MODELS = [("double_integrator", 9), ("quadrotor", 8)]


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Run:
    """One problem handle and the raw entry points of the structured PTR run."""

    def __init__(self, pkg, model, N, iter_max=ITER_MAX, q_tr=float("inf")):
        self.pkg, self.L, self.N = pkg, pkg._lib.lib(), N
        self.traj = pkg.TrajectoryProblem(model)
        pars = pkg.PTR.Parameters(N=N, Nsub=NSUB, iter_max=iter_max, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0, q_tr=q_tr)
        self.pbm = pkg.PTR.create(pars, self.traj, batch_capacity=CAP)
        self.h = self.pbm.handle
        rng = np.random.default_rng(11)
        nom = self.traj.mdl.nominal_pp()
        self.pp = np.ascontiguousarray(np.stack([nom * (1 + 0.03 * rng.uniform(-1, 1, nom.size)) for _ in range(B)]))
        g = [self.traj.guess(N, self.pp[b]) for b in range(B)]
        self.guess = [np.ascontiguousarray(np.stack([gi[j] for gi in g]), np.float64) for j in range(3)]

    def cp(self, iter_max=ITER_MAX):
        """scp_ptr_params of the structured path (q_tr = Inf whatever the handle's own template uses)"""
        return self.pkg.PTR.Parameters(N=self.N, Nsub=NSUB, iter_max=iter_max, wvc=1e3, wtr=0.1, eps_abs=0.0, eps_rel=0.0).c_struct()

    def init(self, iter_max=ITER_MAX):
        xd, ud, p = self.guess
        cp = self.cp(iter_max)
        return self.L.scp_ptr_init_host(self.h, B, ctypes.byref(cp), _vp(xd), _vp(ud), _vp(p) if self.pbm.np else None, _vp(self.pp))

    def iterate(self):
        na = ctypes.c_int(-1)
        return self.L.scp_ptr_iterate(self.h, ctypes.byref(na)), na.value

    def restart(self):
        return self.L.scp_ptr_restart(self.h)

    def get(self, iter_max=ITER_MAX):
        pbm, N = self.pbm, self.N
        out = dict(xd=np.full((B, N, pbm.nx), -1.0), ud=np.full((B, N, pbm.nu), -1.0), p=np.full((B, pbm.np), -1.0),
                   status=np.full(B, -1, np.int32), iterations=np.full(B, -1, np.int32), cost=np.zeros((B, 4)),
                   feas=np.zeros(B, np.uint8), defect=np.zeros((B, N - 1, pbm.nx)),
                   hist=np.full((iter_max, B, self.pkg._lib.HIST_WIDTH), -1.0))
        rc = self.L.scp_ptr_get_host(self.h, _vp(out["xd"]), _vp(out["ud"]), _vp(out["p"]) if pbm.np else None, _vp(out["status"]),
                                     _vp(out["iterations"]), _vp(out["cost"]), _vp(out["feas"]), _vp(out["defect"]), _vp(out["hist"]))
        return rc, out

    def run(self, iter_max=ITER_MAX, init=True):
        """(init,) iter_max iterations, get_host: every call SCP_OK"""
        if init:
            assert self.init(iter_max) == SCP_OK
        for _ in range(iter_max):
            assert self.iterate()[0] == SCP_OK
        rc, out = self.get(iter_max)
        assert rc == SCP_OK
        return out

    def solve_subproblem(self):
        xd, ud, p = self.guess
        cp = self.cp()
        return self.L.scp_ptr_solve_subproblem_batch_host(self.h, B, ctypes.byref(cp), _vp(xd), _vp(ud), _vp(p) if self.pbm.np else None,
                                                          _vp(self.pp), *([None] * 11))

    def virtual_controls(self):
        return self.L.scp_ptr_get_virtual_controls_host(self.h, *([None] * 6))

    def refused(self):
        """iterate, restart and get_host all answer SCP_ERR_BAD_ARGUMENT"""
        return (self.iterate()[0], self.restart(), self.get()[0]) == (SCP_ERR_BAD_ARGUMENT,) * 3


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in (keys or a))


@pytest.mark.parametrize("model,N", MODELS)
def test_guess_returned_after_init(pkg, model, N):
    """the host-upload variant; the guess rule on the device: test_device_side_guess_equals_host_guess"""
    r = Run(pkg, model, N)
    assert r.init() == SCP_OK
    rc, o = r.get()
    assert rc == SCP_OK
    for k, g in zip(("xd", "ud", "p"), r.guess):
        assert np.array_equal(o[k], g.reshape(o[k].shape)), k
    assert (o["iterations"] == 0).all() and (o["status"] == 0).all() and (o["hist"] == 0.0).all()
    r.pbm.close()


@pytest.mark.parametrize("model,N", MODELS)
def test_iterate_past_iter_max_and_restart(pkg, model, N):
    r = Run(pkg, model, N)
    o1 = r.run()
    assert (o1["iterations"] > 0).all()
    # ---- one iterate too many: SCP_OK, nothing active, nothing changes ----
    assert r.iterate() == (SCP_OK, 0)
    rc, o2 = r.get()
    assert rc == SCP_OK and _same(o1, o2)
    # ---- restart: the same run again, bit for bit ----
    assert r.restart() == SCP_OK
    o3 = r.run(init=False)
    assert _same(o1, o3, ("xd", "ud", "p", "cost", "hist"))
    r.pbm.close()


@pytest.mark.parametrize("model,N", MODELS)
def test_longer_history_on_reinit(pkg, model, N):
    r = Run(pkg, model, N)
    r.run()
    o5 = r.run(iter_max=5)                     # the history buffer grows from 2 to 5 records
    assert o5["hist"].shape[0] == 5 and (o5["iterations"] > 0).all()
    fresh = Run(pkg, model, N, iter_max=5)
    f5 = fresh.run(iter_max=5)
    assert np.array_equal(o5["hist"][:2], f5["hist"][:2], equal_nan=True)
    r.pbm.close(); fresh.pbm.close()


@pytest.mark.parametrize("model,N", MODELS)
def test_standalone_subproblem_solve_ends_the_run(pkg, model, N):
    r = Run(pkg, model, N)
    assert r.virtual_controls() == SCP_ERR_BAD_ARGUMENT        # no subproblem solved yet
    assert r.init() == SCP_OK
    assert r.virtual_controls() == SCP_ERR_BAD_ARGUMENT
    assert r.iterate()[0] == SCP_OK
    assert r.virtual_controls() == SCP_OK
    assert r.solve_subproblem() == SCP_OK
    assert r.refused()
    assert r.virtual_controls() == SCP_OK                      # those of the stand-alone solve
    r.run()                                                    # a new init makes the handle usable again
    r.pbm.close()


def test_ownership_of_the_trajectory_buffers(pkg):
    """The structured run of the parent handle and the generic PTR loop of a child (q_tr = 1 template) write into the same
    trajectory buffers: whoever initialised last owns them, the other side is refused until its own init."""
    model, N = MODELS[1]
    r = Run(pkg, model, N, q_tr=1.0)
    L, sub = r.L, pkg.PTR._generic_sub(r.pbm)
    gp = pkg._lib.ScpPtrGenericParams()
    gp.iter_max, gp.wvc, gp.wtr, gp.eps_abs, gp.eps_rel, gp.q_exit = ITER_MAX, 1e3, 0.1, 0.0, 0.0, float("inf")
    gp.cost_const, gp.solver = sub.T.cost_const, pkg.conic.default_options()
    xd, ud, p = r.guess

    def child_init():
        return L.scp_ptr_generic_init_host(sub._h, B, ctypes.byref(gp), _vp(xd), _vp(ud), _vp(p), _vp(r.pp))

    def child_iterate():
        na = ctypes.c_int(-1)
        return L.scp_ptr_generic_iterate(sub._h, ctypes.byref(na))

    def child_get():
        st = np.zeros(B, np.int32)
        return L.scp_ptr_generic_get_host(sub._h, None, None, None, _vp(st), *([None] * 5))

    def child_run():
        assert child_init() == SCP_OK
        for _ in range(ITER_MAX):
            assert child_iterate() == SCP_OK
        assert child_get() == SCP_OK

    # ---- a structured init on the parent takes the buffers from the child's running loop ----
    assert child_init() == SCP_OK and child_iterate() == SCP_OK
    assert r.init() == SCP_OK
    assert child_iterate() == SCP_ERR_BAD_ARGUMENT and child_get() == SCP_ERR_BAD_ARGUMENT
    assert L.scp_sub_last_error(sub._h) != b""
    child_run()
    # ---- ... and the child's init takes them from the parent's run ----
    assert r.init() == SCP_OK and r.iterate()[0] == SCP_OK
    assert child_init() == SCP_OK
    assert r.refused()
    assert L.scp_last_error(r.h) != b""
    r.run()
    # ---- a stand-alone solve on the child ends its own loop ----
    assert child_init() == SCP_OK and child_iterate() == SCP_OK
    opts = pkg.conic.default_options()
    scal = np.zeros((B, max(sub.nscal, 1)))
    assert L.scp_sub_solve_batch_host(sub._h, B, _vp(xd), _vp(ud), _vp(p), _vp(r.pp), _vp(scal), ctypes.byref(opts),
                                      *([None] * 11)) == SCP_OK
    assert child_iterate() == SCP_ERR_BAD_ARGUMENT
    child_run()
    r.pbm.close()
