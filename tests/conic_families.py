"""Three families of conic programs for the launch-geometry tests of the generic batched conic solver (a plain helper module like
audit_util.py): one sparsity pattern per family, per-problem values, and what is known about every member.

  mixed()     70 small SOCPs (n = 15, cones R+^11 x Q^4 x Q^3 x Q^5 x Q^1 x Q^2) whose members finish at different iterations and
              of which every seventh is infeasible and every seventh unbounded;
  chain()     20 time-staged programs (n = 241, KKT dimension 1011) with one global variable: long KKT rows, chunked factor rows;
  softplus()  70 two-cone softplus programs (exponential cones) with a closed-form optimum.

`certify` recomputes, in extended precision and from the returned x, y, z, s alone, what the solver claims with a status: the KKT
residuals of run() (csrc/conic_ipm.hpp) for OPTIMAL, the Farkas vector for INFEASIBLE, the ray for DUAL_INFEASIBLE, and membership
of s and z in their cones.  tests/test_conic_families_cpu.py pins all of it on the host build and the oracle;
tests/test_conic_geometry_gpu.py holds the device kernel to the same facts in every launch geometry."""
import functools
import os

import numpy as np
import scipy.sparse as sp

from oracle import conic_host, ipm
from test_conic_cpu import _random_chain, random_socp
from test_oracle_exp_cone import exp_rows

OPTIMAL, ALMOST_OPTIMAL, ITERATION_LIMIT, NUMERICAL_ERROR, INFEASIBLE, DUAL_INFEASIBLE = range(6)
LD = np.longdouble
TOL = 1.01e-8       # the solver tested the same quantities against 1e-8 in fp64; their evaluation error here is below 1e-12
RESULT_KEYS = ("x", "y", "z", "s", "status", "iters", "pcost", "dcost", "gap", "pres", "dres", "relgap", "dyn_regs", "refinements")


class Family:
    """B programs  min 1/2 x'Px + c'x  s.t.  Ax = b, Gx + s = h, s in K  with the values of G, A, P shared and c, h, b per problem"""

    def __init__(self, name, c, G, h, l, q, A, b, P, kind):
        self.name = name
        self.c, self.h, self.b = np.ascontiguousarray(c), np.ascontiguousarray(h), np.ascontiguousarray(b)
        self.l, self.q, self.kind = int(l), [int(v) for v in q], np.asarray(kind, int)
        canon = lambda M: None if M is None else _canonical(M)
        self.G, self.A, self.P = canon(G), canon(A), canon(P)
        self.B, self.n = self.c.shape
        self.m, self.p = self.h.shape[1], self.b.shape[1]
        assert self.m == self.l + sum(abs(v) for v in self.q) and self.G.shape == (self.m, self.n)

    def cones(self):
        """(offset, dimension, is_exponential) of every cone after the R+ rows"""
        o = self.l
        for d in self.q:
            yield o, abs(d), d < 0
            o += abs(d)


def _canonical(M):
    M = sp.csc_matrix(M)
    M.sum_duplicates(); M.sort_indices()
    return M


def mixed_data(seed=34, B=70, q=(4, 3, 5, 1, 2), n=14, pe=2, l=8):
    rng = np.random.default_rng(seed)
    c, G, h, l, q, A, b = random_socp(rng, n=n, pe=pe, l=l, q=q)
    m = G.shape[0]
    Gn = np.zeros((m + 3, n + 1))
    Gn[0, n] = -1.0; Gn[1, 0] = 1.0; Gn[2, 0] = -1.0      # -v <= 0 ; x0 <= h1 ; -x0 <= h2
    Gn[3:, :n] = G.toarray()
    hn = np.concatenate([[0.0, 50.0, 50.0], h])
    An = sp.csc_matrix(np.hstack([A.toarray(), np.zeros((pe, 1))]))
    cn = np.concatenate([c, [1.0]])
    cs = np.tile(cn, (B, 1)); hs = np.tile(hn, (B, 1)); kind = np.zeros(B, int)
    for t in range(B):
        cs[t, :n] *= 10.0 ** rng.uniform(-2, 2)
        hs[t, 3:3 + l] += rng.uniform(0, 1.0, l)
        if t % 7 == 3: hs[t, 1] = hs[t, 2] = -1.0; kind[t] = 4     # x0 <= -1 and x0 >= 1: infeasible
        if t % 7 == 5: cs[t, n] = -1.0; kind[t] = 5                # min -v, v >= 0: unbounded
    return cs, sp.csc_matrix(Gn), hs, l + 3, list(q), An, b, kind   # kind: intended scp_conic_status


def mixed(seed=34):
    cs, G, hs, l, q, A, b, kind = mixed_data(seed)
    return Family("mixed", cs, G, hs, l, q, A, np.tile(b, (cs.shape[0], 1)), None, kind)


def chain(B=20):
    rng = np.random.default_rng(48)
    c, G, h, l, q, A, b, P = _random_chain(rng, 48, 3, 2, True)
    cs = c[None] * 10.0 ** rng.uniform(-1, 1, B)[:, None]          # (both drawn from the generator that made the program, after it)
    bs = b[None] + 0.05 * rng.standard_normal((B, b.size))
    return Family("chain", cs, G, np.tile(h, (B, 1)), l, q, A, bs, P, np.zeros(B, int))


def softplus(B=70):
    """min t f + w over (f, w, u, v) with (-w, 1, u), (f - w, 1, v) in K_exp, u + v <= 1 (tests/test_oracle_exp_cone.py)"""
    G1, h1 = exp_rows(4, ([0, -1, 0, 0], 0.0), ([0, 0, 0, 0], 1.0), ([0, 0, 1, 0], 0.0))
    G2, h2 = exp_rows(4, ([1, -1, 0, 0], 0.0), ([0, 0, 0, 0], 1.0), ([0, 0, 0, 1], 0.0))
    G = np.vstack([np.array([[0.0, 0.0, 1.0, 1.0]]), G1, G2])
    h = np.concatenate([[1.0], h1, h2])
    ts = -np.linspace(0.02, 0.98, B)
    cs = np.stack([np.array([t, 1.0, 0.0, 0.0]) for t in ts])
    fam = Family("softplus", cs, G, np.tile(h, (B, 1)), 1, [-3, -3], None, np.zeros((B, 0)), None, np.zeros(B, int))
    fam.t = ts
    fam.f_star = np.log(-ts / (1 + ts))
    fam.value = ts * fam.f_star + np.log1p(np.exp(fam.f_star))
    return fam


FAMILIES = {"mixed": mixed, "chain": chain, "softplus": softplus}


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


# ---- references (computed once per process, never modified) ---------------------------------------------------------------------
def _solve_host(fam, order, **opts):
    old = os.environ.get("CONIC_HOST_ORDER")
    os.environ["CONIC_HOST_ORDER"] = order
    try:
        r = conic_host.solve(fam.c[0], fam.G, fam.h[0], fam.l, fam.q, fam.A, fam.b[0] if fam.p else None, P=fam.P, B=fam.B,
                             values=dict(c=fam.c, h=fam.h, b=fam.b), **opts)
    finally:
        if old is None:
            del os.environ["CONIC_HOST_ORDER"]
        else:
            os.environ["CONIC_HOST_ORDER"] = old
    r["relgap"], r["dyn_regs"], r["refinements"] = r["info"][:, 5], r["info"][:, 6], r["info"][:, 7]
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def host(name, order="seq", max_iter=100, reg=-1.0):
    """the family through the host build of the product's solver body (single worker), elimination order seq | nd"""
    return _solve_host(family(name), order, max_iter=max_iter, reg=reg)


@functools.lru_cache(maxsize=None)
def oracle_costs(name):
    """(status, pcost) of oracle/ipm.py on every member the family intends to be feasible (NaN cost elsewhere)"""
    fam = family(name)
    assert not any(d < 0 for d in fam.q)
    st, pc = [], np.full(fam.B, np.nan)
    for t in range(fam.B):
        if fam.kind[t] != OPTIMAL:
            st.append(None)
            continue
        r = ipm.solve(fam.c[t], fam.G, fam.h[t], fam.l, fam.q, fam.A, fam.b[t], P=fam.P)
        st.append(r["status"]); pc[t] = r["pcost"]
    pc.setflags(write=False)
    return tuple(st), pc


# ---- the product on the device ---------------------------------------------------------------------------------------------------
def device_batch(pkg, fam, capacity=None):
    return pkg.conic.ConicProgramBatch(fam.n, fam.G, fam.l, fam.q, A=fam.A, P=fam.P, batch_capacity=capacity or fam.B)


def device_solve(prog, fam, members=None, **opts):
    """solve the members `members` (default: all, in order) of the family on an existing batch object"""
    idx = np.arange(fam.B) if members is None else np.asarray(members)
    return prog.solve(fam.c[idx], fam.h[idx], b=fam.b[idx] if fam.p else None, **opts)


def same_bits(r0, i0, r1, i1):
    """names of the result arrays in which member i0 of r0 and member i1 of r1 differ in any bit"""
    return [k for k in RESULT_KEYS if not np.array_equal(np.asarray(r0[k])[i0], np.asarray(r1[k])[i1], equal_nan=True)]


# ---- extended-precision certificates ---------------------------------------------------------------------------------------------
def _norm(v):
    v = np.asarray(v, LD)
    return np.sqrt(np.sum(v * v)) if v.size else LD(0)


def cone_violations(fam, v, dual=False):
    """list of (cone, amount) where the m-vector v is outside K (dual: K*); second-order cones may miss by round-off of their own norm"""
    v = np.asarray(v, LD)
    bad = [("R+ row %d" % i, v[i]) for i in range(fam.l) if not v[i] >= 0]
    for o, d, is_exp in fam.cones():
        w = v[o:o + d]
        if not is_exp:
            slack = w[0] - _norm(w[1:])
            if not slack >= -8 * np.finfo(float).eps * _norm(w):
                bad.append(("Q^%d at %d" % (d, o), slack))
        elif dual:       # K*_exp = closure{(u, v, w): u < 0, w > 0, v - u + u log(-u / w) >= 0}
            u_, v_, w_ = w
            if not (u_ < 0 and w_ > 0 and v_ - u_ + u_ * np.log(-u_ / w_) >= 0):
                bad.append(("K*_exp at %d" % o, v_ - u_ + u_ * np.log(-u_ / w_) if u_ < 0 and w_ > 0 else LD(-1)))
        else:            # K_exp = closure{(x, y, w): y > 0, y exp(x / y) <= w}
            x_, y_, w_ = w
            if not (y_ > 0 and w_ > 0 and y_ * np.log(w_ / y_) - x_ >= 0):
                bad.append(("K_exp at %d" % o, y_ * np.log(w_ / y_) - x_ if y_ > 0 and w_ > 0 else LD(-1)))
    return bad


def kkt(fam, t, x, y, z, s):
    """pcost, pres, dres, gap, relgap of run() (csrc/conic_ipm.hpp) for member t at (x, y, z, s), in np.longdouble"""
    x, y, z, s = (np.asarray(a, LD) for a in (x, y, z, s))
    c, h, b = fam.c[t].astype(LD), fam.h[t].astype(LD), fam.b[t].astype(LD)
    G = fam.G.toarray().astype(LD)
    A = fam.A.toarray().astype(LD) if fam.p else np.zeros((0, fam.n), LD)
    Pu = fam.P.toarray().astype(LD) if fam.P is not None else np.zeros((fam.n, fam.n), LD)
    P = np.triu(Pu) + np.triu(Pu, 1).T
    mc = max(np.abs(fam.c[t]).max(), np.abs(fam.P.data).max() if fam.P is not None and fam.P.nnz else 0.0)
    osc = LD(1e4 / mc) if mc > 1e4 else LD(1)                 # objective scale of run(): the dual residual is measured on osc * objective
    Px = P @ x
    rx, ry, rz = osc * (Px + A.T @ y + G.T @ z + c), A @ x - b, G @ x + s - h
    pcost = (0.5 * x @ Px + c @ x)
    gap = s @ z
    dcost = pcost + y @ ry + z @ rz - gap
    pres = max(_norm(ry) / max(LD(1), _norm(b)), _norm(rz) / max(LD(1), _norm(h)))
    dres = _norm(rx) / max(LD(1), _norm(osc * c))
    relgap = gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else LD(np.inf))
    return dict(pcost=pcost, pres=pres, dres=dres, gap=gap, relgap=relgap)


def certify(fam, r, t, k=None):
    """Problems with the claim that status r['status'][k] makes about member t of the family, as a list of strings (empty: certified).
    k: position of the member in r (default t)."""
    k = t if k is None else k
    st = int(r["status"][k])
    x, y, z, s = (np.asarray(r[key][k], LD) for key in ("x", "y", "z", "s"))
    out = []
    c, h, b = fam.c[t].astype(LD), fam.h[t].astype(LD), fam.b[t].astype(LD)
    G = fam.G.toarray().astype(LD)
    A = fam.A.toarray().astype(LD) if fam.p else np.zeros((0, fam.n), LD)
    if st == OPTIMAL:
        q = kkt(fam, t, x, y, z, s)
        if not q["pres"] <= TOL: out.append("pres %.3e" % q["pres"])
        if not q["dres"] <= TOL: out.append("dres %.3e" % q["dres"])
        if not (q["gap"] <= TOL or q["relgap"] <= TOL): out.append("gap %.3e relgap %.3e" % (q["gap"], q["relgap"]))
        out += ["s outside K: %s %.3e" % v for v in cone_violations(fam, s)]
        out += ["z outside K*: %s %.3e" % v for v in cone_violations(fam, z, dual=True)]
        # what the solver reports is what its solution has: to 1e-12 on the normalised quantities -- pres and dres are normalised
        # by max(1, |b|), max(1, |h|), max(1, |c|) already, the cost by max(1, |pcost|) as in every cost bound of these tests (one
        # ulp of the largest cost of the mixed family, 2.8e3, is 4.5e-13: an absolute 1e-12 would be a bound on the last two bits)
        for key in ("pres", "dres", "pcost"):
            if not abs(LD(r[key][k]) - q[key]) <= 1e-12 * (max(LD(1), abs(q[key])) if key == "pcost" else 1):
                out.append("reported %s %.17g, recomputed %.17g" % (key, r[key][k], q[key]))
    elif st == INFEASIBLE:          # Farkas: b'y + h'z < 0, A'y + G'z = 0, z in K*
        bh = b @ y + h @ z
        if not bh < 0: out.append("b'y + h'z = %.3e" % bh)
        elif not _norm(A.T @ y + G.T @ z) <= TOL * -bh: out.append("|A'y + G'z| / -(b'y + h'z) = %.3e" % (_norm(A.T @ y + G.T @ z) / -bh))
        out += ["z outside K*: %s %.3e" % v for v in cone_violations(fam, z, dual=True)]
    elif st == DUAL_INFEASIBLE:     # ray: c'x < 0, Ax = 0, Gx + s = 0, s in K
        cx = c @ x
        res = max(_norm(A @ x), _norm(G @ x + s))
        if not cx < 0: out.append("c'x = %.3e" % cx)
        elif not res <= TOL * -cx: out.append("max(|Ax|, |Gx + s|) / -c'x = %.3e" % (res / -cx))
        out += ["s outside K: %s %.3e" % v for v in cone_violations(fam, s)]
    else:
        out.append("status %d makes no claim" % st)
    return out
