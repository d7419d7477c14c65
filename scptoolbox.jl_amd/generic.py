"""Generic `solve_subproblem!` on the device for any conic template (scptoolbox.jl_amd/subproblem.py).

`GenericSubproblem` binds a template to an `SCPProblem` handle (scp_sub_create): the pattern is analysed once, the
affine value maps and read-out indices are uploaded, and every `solve` is discretize! -> linearise -> gather ->
conic_ipm_kernel -> read-out -> discretize! on the MI355X (scp_sub_solve_batch_host).  The reference does the same work
per iteration and per problem in Julia/JuMP + ECOS (src/solvers/scp.jl:942-950 and the add_*! functions)."""
import ctypes
from types import SimpleNamespace

import numpy as np

from . import _lib
from .conic import default_options
from .scp import SCPProblem
from .subproblem import trapz_weights


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _amap(m, keep):
    am = _lib.ScpAffineMap()
    arrs = [np.ascontiguousarray(m.const, np.float64), np.ascontiguousarray(m.ptr, np.int32),
            np.ascontiguousarray(m.src, np.int32), np.ascontiguousarray(m.coef, np.float64)]
    keep.extend(arrs)
    am.len = int(m.size)
    am.val0, am.ptr, am.sidx, am.coef = (a.ctypes.data for a in arrs)
    return am


class LinearFunctionals:
    """fun[j] = const[j] + sum coef * x[idx]: rows over the conic solution."""

    def __init__(self, n):
        self.n = n
        self.rows = []

    def add(self, idx, coef, const=0.0):
        self.rows.append((np.atleast_1d(idx).astype(np.int64), np.atleast_1d(np.asarray(coef, float)), float(const)))
        return len(self.rows) - 1

    def as_map(self):
        from .affine import AffineMap
        const = np.array([r[2] for r in self.rows])
        slot = np.concatenate([np.full(r[0].size, j) for j, r in enumerate(self.rows)]) if self.rows else np.zeros(0, np.int64)
        src = np.concatenate([r[0] for r in self.rows]) if self.rows else np.zeros(0, np.int64)
        coef = np.concatenate([r[1] for r in self.rows]) if self.rows else np.zeros(0)
        return AffineMap.from_terms(const, slot, src, coef)


def standard_functionals(T):
    """Cost pieces the outer loops read from the solved subproblem (ptr.jl:773-789,889-892; scvx.jl:895-898):
    fun[0] = trapz(P) + sum(Pf);  PTR additionally fun[1] = trapz(eta_x) + trapz(eta_u) + eta_p."""
    F = LinearFunctionals(T.n)
    w = trapz_weights(T.N)
    v = T.variables
    if "P" in v:
        F.add(np.concatenate([v["P"], v["Pf"]]), np.concatenate([w, np.ones(2)]))
    if getattr(T, "algo", "") == "gusto":      # the penalty variables themselves: v_tr[k], then v_st[k][i] (gusto.jl:534-550)
        for k in range(T.N):
            F.add(v["v_tr"][k], 1.0)
        for k in range(T.N):
            for i in range(T.nst):
                F.add(T.v_st_nodes[k, i], 1.0)
    if "etax" in v:
        F.add(np.concatenate([v["etax"], v["etau"], v["etap"]]), np.concatenate([w, w, np.ones(1)]))
    return F


class GenericSubproblem:
    def __init__(self, pbm, T, functionals=None):
        self.pbm, self.T = pbm, T
        L = _lib.lib()
        nscal = T.sources.segs["scal"][1][0]
        offs = np.zeros(21, np.int32)
        nsrc = ctypes.c_int(0)
        _lib.check(L.scp_sub_source_layout(pbm.handle, nscal, _ptr(offs), ctypes.byref(nsrc)), pbm.handle)
        mine = [T.sources.segs[k][0] for k in ("xref", "uref", "pref", "A", "Bm", "Bp", "F", "r", "E", "C", "D", "Gs", "rs",
                                               "H0", "K0", "l0", "Hf", "Kf", "lf", "scal")] + [T.sources.n]
        if list(offs) != mine or nsrc.value != T.nsrc:
            raise RuntimeError("source layout of the template does not match the library's (scp_sub_source_layout)")
        self.F = functionals if functionals is not None else standard_functionals(T)
        keep = []
        st = _lib.ScpSubTemplate()
        st.n, st.p, st.m, st.l, st.ncones = T.n, T.p, T.m, T.l, len(T.q)
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        arrs = dict(q=i32(T.q), Pp=i32(T.P.indptr), Pi=i32(T.P.indices), Ap=i32(T.A.indptr), Ai=i32(T.A.indices),
                    Gp=i32(T.G.indptr), Gi=i32(T.G.indices))
        N = T.N
        arrs["ix"] = i32(T.variables["xh"])     # xh blocks were created node by node: [N, nx] row-major == (nx, N) col-major
        arrs["iu"] = i32(T.variables["uh"])
        arrs["ip"] = i32(T.variables.get("ph", np.zeros(0, np.int64)))
        for k, a in arrs.items():
            setattr(st, k, a.ctypes.data)
        keep.extend(arrs.values())
        for k in ("c", "b", "h", "Gx", "Ax", "Px"):
            setattr(st, k, _amap(T.maps[k], keep))
        st.nsrc, st.nscal = T.nsrc, nscal
        fm = self.F.as_map()
        st.nfun = fm.size
        st.fun = _amap(fm, keep)
        self.nfun, self.nscal = fm.size, nscal
        self._keep = keep
        self._h = ctypes.c_void_p()
        rc = L.scp_sub_create(pbm.handle, ctypes.byref(st), ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            _lib.check(rc, pbm.handle)
        if not hasattr(pbm, "_children"):
            pbm._children = []
        pbm._children.append(self)       # the problem handle must outlive this one (SCPProblem.close closes us first)

    def close(self):
        if self._h:
            _lib.lib().scp_sub_destroy(self._h)
            self._h = ctypes.c_void_p()
        if self in getattr(self.pbm, "_children", []):
            self.pbm._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise _lib.ScpError(rc, _lib.lib().scp_sub_last_error(self._h).decode(errors="replace"))

    def stats(self):
        """symbolic / run statistics of this subproblem's conic engine (scp_sub_stats: the fields of ConicProgramBatch.stats)"""
        st = np.zeros(16, np.int64)
        self._check(_lib.lib().scp_sub_stats(self._h, _ptr(st)))
        return dict(nnzL=int(st[0]), factor_madds=int(st[1]), kkt_dim=int(st[2]), nnzGt=int(st[3]), bytes_per_problem=int(st[4]),
                    levels=int(st[5]), back_levels=int(st[6]), waves=int(st[7]), nd_depth=int(st[8]), fallback_solves=int(st[9]),
                    solves=int(st[10]), fallback_levels=int(st[11]), fallback_rescued=int(st[12]))

    def solve(self, xd, ud, p, pp=None, scal=None, want_conic=False, **opts):
        """`solve_subproblem!` about the reference trajectories xd[B,N,nx], ud[B,N,nu], p[B,np]."""
        pbm = self.pbm
        xd = np.ascontiguousarray(xd, np.float64); ud = np.ascontiguousarray(ud, np.float64)
        p = np.ascontiguousarray(p, np.float64)
        B, N = xd.shape[0], pbm.pars.N
        npp = pbm.info.npp
        pp = np.ascontiguousarray(np.tile(pbm.traj.mdl.nominal_pp(), (B, 1)) if pp is None else pp, np.float64)
        assert pp.shape == (B, npp)
        scal = np.zeros((B, self.nscal)) if scal is None else np.ascontiguousarray(scal, np.float64).reshape(B, self.nscal)
        x = np.zeros((B, N, pbm.nx)); u = np.zeros((B, N, pbm.nu)); po = np.zeros((B, pbm.np))
        fun = np.zeros((B, self.nfun)); xc = np.zeros((B, self.T.n)) if want_conic else None
        status = np.zeros(B, np.int32); iters = np.zeros(B, np.int32); info = np.zeros((B, 8))
        defect = np.zeros((B, N - 1, pbm.nx)); feas = np.zeros(B, np.uint8)
        sec = ctypes.c_double(0.0)
        o = default_options(**opts)
        self._check(_lib.lib().scp_sub_solve_batch_host(
            self._h, B, _ptr(xd), _ptr(ud), _ptr(p) if pbm.np else None, _ptr(pp) if npp else None, _ptr(scal),
            ctypes.byref(o), _ptr(x), _ptr(u), _ptr(po) if pbm.np else None, _ptr(fun), _ptr(xc), _ptr(status), _ptr(iters),
            _ptr(info), _ptr(defect), _ptr(feas), ctypes.byref(sec)))
        out = dict(x=x, u=u, p=po, fun=fun, status=status, iters=iters, pcost=info[:, 0] + self.T.cost_const, gap=info[:, 2],
                   pres=info[:, 3], dres=info[:, 4], defect=defect, feas=feas.astype(bool), seconds=sec.value)
        if want_conic:
            out["xconic"] = xc
            for name in ("vd", "vs", "vic", "vtc", "P", "Pf", "etax", "etau", "etap", "dx_lq", "du_lq", "dp_lq"):
                if name in self.T.variables:
                    out[name] = xc[:, self.T.variables[name]]
        return out


# ---- what the device-resident outer loops (SCvx, GuSTO, PTR on the generic path; csrc/scp_generic.hip) share on the host ----
class LoopProblem(SCPProblem):
    """An SCPProblem that owns its subproblem template `sub` and its guess projection `proj` (SCvx, GuSTO)."""

    def close(self):
        for s in ("sub", "proj"):
            if getattr(self, s, None) is not None:
                getattr(self, s).close()
                setattr(self, s, None)
        super().close()


def stack_guesses(pbm, pp, guess=None):
    """The initial guess of every instance as contiguous arrays xd[B,N,nx], ud[B,N,nu], p[B,np]: `guess` = (xd, ud, p) of the
    caller, or traj.guess per instance."""
    if guess is None:
        g = [pbm.traj.guess(pbm.pars.N, pp[b]) for b in range(pp.shape[0])]
        guess = [np.stack([gi[j] for gi in g]) for j in range(3)]
    return tuple(np.ascontiguousarray(a, np.float64) for a in guess)


def run_loop(pbm, sub, fns, head, guess, pp, cost_shape, hist_width, all_reduce=None, summary_only=False):
    """One run of a device-resident loop on `sub`: fns = its (init, iterate, get_host) of the C ABI; `head` = the arguments of
    init between the handle and the guess (projection handle, B, parameter struct).  all_reduce: n -> global n (the
    per-iteration convergence all-reduce of a batch sharded over GPUs, dist.py; identity on one GPU).  Returns every output of
    get_host: xd, ud, p, status, iterations, cost[cost_shape], feas, defect, hist[iter_max, B, hist_width]."""
    init, iterate, get_host = fns
    xd, ud, p = guess
    B = pp.shape[0]
    sub._check(init(sub._h, *head, _ptr(xd), _ptr(ud), _ptr(p) if pbm.np else None, _ptr(pp) if pbm.info.npp else None))
    pbm.resident_B = B      # size of the batch the run on this handle holds (audit_resident)
    return iterate_and_read(pbm, sub, iterate, get_host, B, cost_shape, hist_width, all_reduce, summary_only)


def iterate_and_read(pbm, sub, iterate, get_host, B, cost_shape, hist_width, all_reduce=None, summary_only=False):
    """The iterations of a run that has been started (by its init, or by scp_ptr_generic_continue) and its get_host.
    summary_only: get_host copies status, iterations and cost only (every other pointer NULL); the other fields are None."""
    iter_max = pbm.pars.iter_max
    na = ctypes.c_int(1)
    k, n = 0, 1
    while k < iter_max and n > 0:
        sub._check(iterate(sub._h, ctypes.byref(na)))
        n = na.value if all_reduce is None else all_reduce(na.value)
        k += 1
    if summary_only:
        r = SimpleNamespace(xd=None, ud=None, p=None, status=np.zeros(B, np.int32), iterations=np.zeros(B, np.int32),
                            cost=np.zeros(cost_shape), feas=None, defect=None, hist=None)
        sub._check(get_host(sub._h, None, None, None, _ptr(r.status), _ptr(r.iterations), _ptr(r.cost), None, None, None))
        return r
    rc, r = read_result(pbm, B, get_host, sub._h, cost_shape, hist_width)
    sub._check(rc)
    return r


def read_result(pbm, B, get_host, handle, cost_shape, hist_width):
    """(status, outputs) of one of the get_host entry points of the C ABI, which share one signature (structured PTR run: `handle`
    = the problem handle; the loops: the subproblem handle)"""
    N, iter_max = pbm.pars.N, pbm.pars.iter_max
    r = SimpleNamespace(xd=np.zeros((B, N, pbm.nx)), ud=np.zeros((B, N, pbm.nu)), p=np.zeros((B, pbm.np)),
                        status=np.zeros(B, np.int32), iterations=np.zeros(B, np.int32), cost=np.zeros(cost_shape),
                        feas=np.zeros(B, np.uint8), defect=np.zeros((B, N - 1, pbm.nx)), hist=np.zeros((iter_max, B, hist_width)))
    rc = get_host(handle, _ptr(r.xd), _ptr(r.ud), _ptr(r.p) if pbm.np else None, _ptr(r.status), _ptr(r.iterations),
                  _ptr(r.cost), _ptr(r.feas), _ptr(r.defect), _ptr(r.hist))
    r.feas = r.feas.astype(bool)
    return rc, r


class SCPSolutionBatch:
    """Batched `SCPSolution` of SCvx and GuSTO from the outputs of run_loop (cost[2, B] = J of the reference, J of the last
    solution: the nonlinear augmented cost, sol.J_aug)."""
    STATUS = {0: "SCP_SOLVED", 1: "SCP_FAILED", 2: "SCP_GUESS_PROJECTION_FAILED"}

    def __init__(self, r):
        self.xd, self.ud, self.p, self.defect = r.xd, r.ud, r.p, r.defect
        self.status = [self.STATUS[int(v)] for v in r.status]
        self.iterations, self.feas = r.iterations, r.feas
        self.J_ref, self.cost = r.cost[0], r.cost[1]


def solve_projected(pbm, fns, cp, pp, guess, project_guess, all_reduce, h_names):
    """`solve` of SCvx and GuSTO: the guess is projected onto the convex sets first (pbm.proj) unless project_guess=False.
    Returns (SCPSolutionBatch, history by column name)."""
    pp = np.ascontiguousarray(np.atleast_2d(pbm.traj.mdl.nominal_pp() if pp is None else pp), np.float64)
    B = pp.shape[0]
    r = run_loop(pbm, pbm.sub, fns, (pbm.proj._h if project_guess else None, B, ctypes.byref(cp)), stack_guesses(pbm, pp, guess),
                 pp, (2, B), _lib.SCVX_HIST_WIDTH, all_reduce)
    return SCPSolutionBatch(r), {nm: r.hist[:, :, j] for j, nm in enumerate(h_names)}
