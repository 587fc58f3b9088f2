"""An extended-precision reference for the derivatives with respect to the mesh motion ``uhat`` (numpy only; no GPU).

The oracle evaluates F = I + grad(uhat), gradx and J in the primal only: it has no shape derivative.  ``rowscaled_cases.extended``
evaluates the same formulas in numpy.longdouble, and every scalar the shape kernels differentiate is a sum of local terms Phi_t(uhat_t),
each a function of the uhat of ONE cell (or of one penalty facet's cell):

  * the elastic term   lam_e . Ke(uhat) w_e            and the load term   - lam_e . F_e(uhat)      (dRdT:uhat),
  * each penalty facet lam_f . P_f(uhat) (w_f - g_f)                                                (dRdT:uhat),
  * the cell shares of int u.u J dx (compliance: its regularisation does not see uhat), int rho h J dx (mass), 1/2 w_e . Ke w_e
    (elastic_energy: matrix-free, cell by cell) and of the inner sum int (m vm)^rho J dx of pnorm_stress, which is divided by the
    reference area of the selection afterwards, in longdouble (the aggregate has no outer power: oracle pnorm_stress).

Each term is differenced by itself with respect to every (vertex, component) of its own cell: Romberg-extrapolated central differences
in longdouble, first step FRACTION * hK of that cell, halved LEVELS - 1 times.  (Differencing the global sum instead puts the 1e15 penalty
of order 1e12 beside elastic terms of order 1: what is left of them is 1e-10 of their scale.)  The term derivatives are summed per vertex.

  unc_i   = sum over the terms at vertex i of |last Romberg diagonal - the one before|
  scale_i = sum over the terms touching vertex i of A_t / hK_t, A_t the term with its factors replaced by their absolute values
            (|lam_e|^T |Ke| |w_e|, |lam_e|^T |F_e|, |lam_f|^T |P_f| |w_f - g_f|; the functional shares are sums of non-negative
            terms up to the interpolation of the state, which enters as |N||u_e|): the derivative with respect to a node position of a
            quantity of size A on a cell of size h has size A / h, and summing the same terms in another order moves an entry by a
            multiple of u scale_i whatever cancels
  shape_scaled(g, g_ref, scale) = max_i |g - g_ref|_i / scale_i      (a zero scale demands an exact match)

Forward mode: (dR/duhat) v is the same difference of the local residual vectors Ke(uhat) w_e - F_e(uhat) and P_f(uhat) (w_f - g_f) along
v restricted to the cell, with the row scale  sum over t touching row r of (|Ke| |w_e| + |F_e|)_r max|v_t| / hK_t  (penalty blocks alike);
rows of strong Dirichlet DOFs are zero, as femo_residual_jvp returns them.

This is a differenced extended-precision oracle, not an analytic derivative: ``unc`` is what it knows about its own error, and
tests/test_shape_ref_cpu.py holds it below a tenth of every bound it is used with."""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_metrics as pm          # noqa: E402
import rowscaled_cases as rc         # noqa: E402

LD = np.longdouble
# first step / cell diameter, and the number of central differences at FRACTION hK / 2^l.  A vertex component moves F = I + grad(uhat) along
# a rank-one direction, so F^-1 has one pole, at a distance of about the cell's altitude over that vertex: hK / 16 is within a factor
# two of it on the slender triangles of the delaunay mesh (eight levels from there leave 4e-9 of the scale there, 3e-16 on the
# quadrilaterals), while below hK / 8192 the rounding of the longdouble terms (1e-19 A / step) passes a tenth of the tightest bound.
FRACTION = 1.0 / 256.0
LEVELS = 6
STRESS_M, STRESS_RHO, STRESS_REG = 1e-6, 6.0, 0.5e3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_sens.npz")

CASES = ("warped-uhat-penalty", "tri-ewm-uhat-strong", "tee-uhat-penalty", "delaunay-uhat-penalty", "cg1-uhat-strong",
         "cr1-uhat-penalty", "laminate")
REGULARIZED = "warped-uhat-penalty"          # the case that also checks pnorm_stress with the thickness regularisation
SUBDOMAIN = "delaunay-uhat-penalty"          # ... and the one that also checks it on a selected sub-domain
REVERSE = ("dRdT:uhat", "dJ:compliance:uhat", "dJ:mass:uhat", "dJ:elastic_energy:uhat", "dJ:pnorm_stress:uhat")
FORWARD = ("jvp:uhat:dense", "jvp:uhat:clamp")


def quantities(name):
    q = list(REVERSE)
    if name == REGULARIZED:
        q.append("dJ:pnorm_stress:uhat@reg")
    if name == SUBDOMAIN:
        q.append("dJ:pnorm_stress:uhat@sub")
    return q + list(FORWARD)


def shape_scaled(g, g_ref, scale):
    """max_i |g - g_ref|_i / scale_i; an entry whose scale is zero must match exactly."""
    scale = np.asarray(scale, dtype=np.float64)
    return pm._ratio(pm._diff(np.asarray(g).reshape(np.shape(g_ref)), g_ref), scale.reshape(np.shape(g_ref)))


def subdomain_cells(k):
    """The selected sub-domain of the SUBDOMAIN case: a seeded third of the cells."""
    return np.sort(np.random.default_rng(7).permutation(k.m.nel)[: k.m.nel // 3])


def clamped_vertices(k):
    c = set(k.clamped.tolist())
    return np.array([v for v in range(k.m.nn) if 3 * v in c], dtype=np.int64)


def directions(k):
    """The two directions of the forward products: a seeded dense one, and a single vertex on the clamp."""
    dense = np.random.default_rng(11).uniform(-1, 1, (k.m.nn, 3))
    single = np.zeros((k.m.nn, 3))
    single[clamped_vertices(k)[0]] = (1.0, -0.5, 0.25)
    return {"jvp:uhat:dense": dense, "jvp:uhat:clamp": single}


def sample_vertices(k):
    """A clamped (or penalty) vertex and the vertices of lowest and highest valence."""
    val = np.bincount(k.m.cells.ravel(), minlength=k.m.nn)
    return np.unique([int(clamped_vertices(k)[0]), int(np.argmin(val)), int(np.argmax(val))])


# ------------------------------------------------------------------ the oracle on cells taken apart
def stress_oracle(k):
    """The oracle of the case on the rule of the stress measure (degree 4), with the case's fields."""
    from oracle.rm_shell_oracle import ShellOracle, degree4_rule
    o = k.o
    o3 = ShellOracle(k.m, element_wise_material=o.ewm, elementwise_pressure=o.ewp, nquad=degree4_rule(k.m))
    o3.set_fields(h=o.h, E=o.E, nu=o.nu, rho=o.rho, f=o.f, uhat=o.uhat)
    return o3


def broken(o, idx, ld=True):
    """``o`` restricted to the cells ``idx`` (repeats allowed), each with vertices, nodal fields and uhat of its own: cell j of the
    result is cell idx[j], its vertices are nvc j .. nvc j + nvc - 1.  With ``ld`` everything is cast as rowscaled_cases.extended does."""
    idx = np.asarray(idx, dtype=np.int64)
    b = rc.extended(o) if ld else copy.copy(o)
    if not ld:
        b.mesh = copy.copy(o.mesh)
    cells = o.mesh.cells[idx]
    n, nvc = cells.shape
    b.mesh.nodes = b.mesh.nodes[cells].reshape(-1, 3)
    b.mesh.cells = np.arange(n * nvc).reshape(n, nvc)
    b.mesh.nel, b.mesh.nn = n, n * nvc
    b.mesh.cell_p2, b.mesh.cell_edges = o.mesh.cell_p2[idx], o.mesh.cell_edges[idx]      # (the penalty blocks look their DOFs up here)
    b.hK, b.dofs = o.hK[idx], o.dofs[idx]
    b.uhat = b.uhat[cells].reshape(-1, 3)
    for name in ("h", "E", "nu", "rho"):
        v = getattr(b, name)
        setattr(b, name, v[idx] if o.ewm else v[cells].ravel())
    b.f = b.f[idx] if o.ewp else b.f[cells].reshape(-1, 3)
    if getattr(b, "clt", None) is not None:
        b.clt = b.clt[idx]
    b.penalty_facets = np.zeros((0, 2), np.int32)
    b.strong_dofs = np.zeros(0, np.int32)
    return b


class Terms:
    """The local terms of one case on the cells ``idx`` (default: all) and on the penalty facets whose cell is among them."""

    def __init__(self, k, idx=None, ld=True):
        o = k.o
        self.k, self.ld = k, ld
        self.idx = np.arange(k.m.nel) if idx is None else np.asarray(idx, dtype=np.int64)
        t = (lambda a: a.astype(LD)) if ld else (lambda a: np.asarray(a, dtype=np.float64))
        self.cell = broken(o, self.idx, ld)
        self.stress = broken(stress_oracle(k), self.idx, ld)
        self.we, self.le = t(k.w)[o.dofs[self.idx]], t(k.lam)[o.dofs[self.idx]]
        # penalty facets: one cell of its own per facet, in the order of o._penalty_blocks()
        pf = o.penalty_facets
        keep = np.nonzero(np.isin(pf[:, 0], self.idx))[0] if pf.shape[0] else np.zeros(0, dtype=np.int64)
        self.facets = keep
        self.fcell = pf[keep, 0].astype(np.int64)
        if keep.size:
            self.pen = broken(o, self.fcell, ld)
            self.pen.penalty_facets = np.stack([np.arange(keep.size), pf[keep, 1]], axis=1).astype(np.int32)
            blocks = o._penalty_blocks()
            per = len(blocks) // pf.shape[0]
            self.per = per
            self.pdofs = [[blocks[per * f + j][0] for j in range(per)] for f in keep]
            g = getattr(o, "g_dirichlet", None)
            wg = t(k.w if g is None else k.w - g)
            self.pw = [[wg[d] for d in ds] for ds in self.pdofs]
            self.pl = [[t(k.lam)[d] for d in ds] for ds in self.pdofs]
        self.stress_m, self.stress_rho = STRESS_M, STRESS_RHO

    # -- the scalars: name -> (n_terms,) values; every name of ``want``
    def scalars(self, want, absolute=False):
        out = {}
        b = self.cell
        a = np.abs if absolute else (lambda v: v)
        if {"elastic", "energy"} & set(want):
            B, g = b._B(slice(None))
            C = b._C(slice(None), g)
            if absolute:
                Ke = np.abs(np.einsum("eqik,eqij,eqjl->ekl", B, C, B, optimize=True))
                out["elastic"] = np.einsum("ek,ekl,el->e", np.abs(self.le), Ke, np.abs(self.we))
                out["energy"] = 0.5 * np.einsum("ek,ekl,el->e", np.abs(self.we), Ke, np.abs(self.we))
            else:
                sw = np.einsum("eqij,ej->eqi", B, self.we)
                sl = np.einsum("eqij,ej->eqi", B, self.le)
                out["elastic"] = np.einsum("eqi,eqij,eqj->e", sl, C, sw)
                out["energy"] = 0.5 * np.einsum("eqi,eqij,eqj->e", sw, C, sw)
        if {"load", "compliance", "mass"} & set(want):
            g = b._geometry(slice(None), b.N1, b.dN1)
            wj = a(b.wts[None, :] * g["det"] * g["Ju"])
            nu = 3 * b.npc
            Fe = self._load(b, wj, a)
            out["load"] = (1 if absolute else -1) * np.einsum("ek,ek->e", a(self.le[:, :nu]), Fe)
            u = np.einsum("qa,eac->eqc", a(b.N2), a(self.we[:, :nu].reshape(-1, b.npc, 3)))
            out["compliance"] = np.sum(wj * np.einsum("eqc,eqc->eq", u, u), axis=1)
            out["mass"] = np.sum(wj * a(b._at_qp(b.rho, slice(None))) * a(b._at_qp(b.h, slice(None))), axis=1)
        for name, reg in (("pnorm", False), ("pnorm@reg", True)):
            if name in want:
                s = self.stress
                vm, g = s.von_mises_top(self.we_full(s), slice(None))
                wj = s.wts[None, :] * g["det"] * g["Ju"]
                val = np.sum(wj * (self.stress_m * vm) ** self.stress_rho, axis=1)
                if reg:
                    val = val + np.sum(wj * STRESS_REG * s._at_qp(s.h, slice(None)) ** self.stress_rho, axis=1)
                out[name] = a(val)
        if "penalty" in want and self.facets.size:
            blocks = self.pen._penalty_blocks()
            vals = []
            for f in range(self.facets.size):
                vals.append(sum(a(self.pl[f][j]) @ (a(blocks[self.per * f + j][1]) @ a(self.pw[f][j])) for j in range(self.per)))
            out["penalty"] = np.array(vals, dtype=LD if self.ld else np.float64)
        return {n: out[n] for n in want if n in out}

    def we_full(self, s):
        """A state vector in which ``s.dofs`` (the global numbers of the cells taken apart) finds the local values."""
        w = np.zeros(self.k.m.ndof, dtype=self.we.dtype)
        w[s.dofs] = self.we
        return w

    @staticmethod
    def _load(b, wj, a):
        if b.ewp:
            fq = np.repeat(a(b.f)[:, None, :], b.nq, axis=1)
        else:
            fq = np.einsum("qb,ebc->eqc", a(b.N1), a(b.f[b.mesh.cells]))
        return np.einsum("eq,qa,eqc->eac", wj, a(b.N2), fq).reshape(fq.shape[0], -1)

    # -- the local residual vectors (forward mode): cells (n, ldof) and penalty blocks (list of lists)
    def vectors(self, absolute=False, penalty=True):
        b = self.cell
        a = np.abs if absolute else (lambda v: v)
        B, g = b._B(slice(None))
        C = b._C(slice(None), g)
        wj = a(b.wts[None, :] * g["det"] * g["Ju"])
        Fe = self._load(b, wj, a)
        if absolute:
            y = np.einsum("ekl,el->ek", np.abs(np.einsum("eqik,eqij,eqjl->ekl", B, C, B, optimize=True)), np.abs(self.we))
            y[:, : Fe.shape[1]] += Fe
        else:
            y = np.einsum("eqik,eqij,eqj->ek", B, C, np.einsum("eqij,ej->eqi", B, self.we))
            y[:, : Fe.shape[1]] -= Fe
        yp = []
        if penalty and self.facets.size:
            blocks = self.pen._penalty_blocks()
            yp = [[a(blocks[self.per * f + j][1]) @ a(self.pw[f][j]) for j in range(self.per)] for f in range(self.facets.size)]
        return y, yp


def _romberg(D):
    """D[l]: central differences at steps h0 / 2^l.  Returns (last diagonal, |last - the one before|)."""
    prev_diag, row = D[0], [D[0]]
    for l in range(1, len(D)):
        new = [D[l]]
        for j in range(1, l + 1):
            new.append(new[j - 1] + (new[j - 1] - row[j - 1]) / (LD(4) ** j - 1))
        prev_diag, row = row[-1], new
    return row[-1], np.abs(row[-1] - prev_diag)


_CELL_TERMS = ("elastic", "load", "energy", "compliance", "mass", "pnorm", "pnorm@reg")
_QUANTITY_TERMS = {"dRdT:uhat": ("elastic", "load", "penalty"), "dJ:compliance:uhat": ("compliance",), "dJ:mass:uhat": ("mass",),
                   "dJ:elastic_energy:uhat": ("energy",), "dJ:pnorm_stress:uhat": ("pnorm",), "dJ:pnorm_stress:uhat@reg": ("pnorm@reg",),
                   "dJ:pnorm_stress:uhat@sub": ("pnorm",)}


def _pnorm_factor(k, q, cells):
    """Per cell of ``cells``: 1 / alpha (alpha the reference area of the selection, longdouble) inside the selection, zero outside."""
    s = rc.extended(stress_oracle(k))
    g = s._geometry(slice(None), s.N1, s.dN1)
    area = np.sum(s.wts[None, :] * g["det"], axis=1)
    sel = np.ones(k.m.nel, dtype=bool)
    if q.endswith("@sub"):
        sel = np.isin(np.arange(k.m.nel), subdomain_cells(k))
    return np.where(sel[cells], LD(1) / np.sum(area[sel]), LD(0))


def reverse(k, names, idx=None, fraction=FRACTION, levels=LEVELS):
    """quantity -> (reference (nn, 3) longdouble, unc, scale), float64 the last two -- complete at the vertices all of whose cells are
    in ``idx`` (default: every cell)."""
    T = Terms(k, idx)
    m = k.m
    nvc = m.cells.shape[1]
    terms = sorted({t for q in names for t in _QUANTITY_TERMS[q]})
    cterms = [t for t in terms if t != "penalty"]
    pen = "penalty" in terms and T.facets.size > 0
    deriv = {t: np.zeros((T.idx.size, nvc, 3), dtype=LD) for t in cterms}
    unc = {t: np.zeros((T.idx.size, nvc, 3)) for t in cterms}
    if pen:
        deriv["penalty"], unc["penalty"] = np.zeros((T.facets.size, nvc, 3), dtype=LD), np.zeros((T.facets.size, nvc, 3))
    holders = [(T.cell, T.cell.uhat.copy(), T.cell.hK), (T.stress, T.stress.uhat.copy(), T.stress.hK)]
    if pen:
        holders.append((T.pen, T.pen.uhat.copy(), T.pen.hK))
    for bv in range(nvc):
        for comp in range(3):
            D = {t: [] for t in deriv}
            for l in range(levels):
                vals = []
                for sgn in (1, -1):
                    for b, base, hK in holders:
                        step = (hK * fraction / 2 ** l).astype(LD)
                        d = np.zeros_like(base)
                        d[bv::nvc, comp] = sgn * step
                        b.uhat = base + d
                    v = T.scalars(cterms)
                    if pen:
                        v.update(T.scalars(["penalty"]))
                    vals.append(v)
                for t in deriv:
                    hK = T.pen.hK if t == "penalty" else T.cell.hK
                    D[t].append((vals[0][t] - vals[1][t]) / (2 * (hK * fraction / 2 ** l).astype(LD)))
            for t in deriv:
                deriv[t][:, bv, comp], unc[t][:, bv, comp] = _romberg(D[t])
    for b, base, _ in holders:
        b.uhat = base
    A = T.scalars(cterms, absolute=True)
    if pen:
        A.update(T.scalars(["penalty"], absolute=True))
    out = {}
    for q in names:
        ref, u, s = np.zeros((m.nn, 3), dtype=LD), np.zeros((m.nn, 3)), np.zeros((m.nn, 3))
        for t in _QUANTITY_TERMS[q]:
            if t not in deriv:
                continue
            cells = T.fcell if t == "penalty" else T.idx
            hK = k.o.hK[cells]
            fac = _pnorm_factor(k, q, cells) if t.startswith("pnorm") else np.ones(cells.size, dtype=LD)
            vid = m.cells[cells]
            np.add.at(ref, vid, fac[:, None, None] * deriv[t])
            np.add.at(u, vid, (fac[:, None, None] * unc[t]).astype(np.float64))
            np.add.at(s, vid, np.broadcast_to((fac * A[t] / hK).astype(np.float64)[:, None, None], vid.shape + (3,)))
        out[q] = (ref, u, s)
    return out


def forward(k, V, idx=None, fraction=FRACTION, levels=LEVELS):
    """(dR/duhat) V for one direction V (nn, 3): (reference (ndof,) longdouble, unc, scale) -- complete at the rows all of whose cells
    are in ``idx``."""
    T = Terms(k, idx)
    m, o = k.m, k.o
    nvc = m.cells.shape[1]
    V = np.asarray(V, dtype=np.float64)
    sets = [(T.cell, T.idx)] + ([(T.pen, T.fcell)] if T.facets.size else [])
    base = [b.uhat.copy() for b, _ in sets]
    vloc = [V[m.cells[cells]].reshape(-1, 3) for _, cells in sets]
    vmax = [np.abs(V[m.cells[cells]]).reshape(cells.size, -1).max(axis=1) for _, cells in sets]
    # per cell: uhat + s v, s = fraction hK / max|v| / 2^l (a cell the direction does not touch contributes zero: s = 0 there)
    s0 = [np.where(vm > 0, fraction * b.hK / np.where(vm > 0, vm, 1.0), 0.0).astype(LD) for (b, _), vm in zip(sets, vmax)]
    Dc, Dp = [], []
    for l in range(levels):
        vals = []
        for sgn in (1, -1):
            for (b, _), u0, vl, s in zip(sets, base, vloc, s0):
                b.uhat = u0 + sgn * np.repeat(s / 2 ** l, nvc)[:, None] * vl.astype(LD)
            vals.append(T.vectors())
        sc = 2 * s0[0] / 2 ** l
        Dc.append(np.where(sc[:, None] > 0, (vals[0][0] - vals[1][0]) / np.where(sc > 0, sc, 1)[:, None], 0))
        if T.facets.size:
            sp_ = 2 * s0[1] / 2 ** l
            Dp.append([[(a - b_) / sp_[f] if sp_[f] > 0 else 0 * a for a, b_ in zip(vals[0][1][f], vals[1][1][f])]
                       for f in range(T.facets.size)])
    for (b, _), u0 in zip(sets, base):
        b.uhat = u0
    ref, u, s = np.zeros(m.ndof, dtype=LD), np.zeros(m.ndof), np.zeros(m.ndof)
    yc, ucell = _romberg(Dc)
    Ay, Ap = T.vectors(absolute=True)
    np.add.at(ref, o.dofs[T.idx], yc)
    np.add.at(u, o.dofs[T.idx], ucell.astype(np.float64))
    np.add.at(s, o.dofs[T.idx], (Ay * (vmax[0] / o.hK[T.idx])[:, None]).astype(np.float64))
    for f in range(T.facets.size):
        for j in range(T.per):
            y, du = _romberg([Dp[l][f][j] for l in range(levels)])
            d = T.pdofs[f][j]
            ref[d] += y
            u[d] += du.astype(np.float64)
            s[d] += (Ap[f][j] * vmax[1][f] / o.hK[T.fcell[f]]).astype(np.float64)
    ref[o.strong_dofs] = 0
    u[o.strong_dofs] = 0
    s[o.strong_dofs] = 0
    return ref, u, s


def reference(k, idx=None, fraction=FRACTION, levels=LEVELS):
    """Every quantity of the case: name -> (reference, unc, scale)."""
    qs = quantities(k.name)
    out = reverse(k, [q for q in qs if q in _QUANTITY_TERMS], idx, fraction, levels)
    for q, V in directions(k).items():
        out[q] = forward(k, V, idx, fraction, levels)
    return out


def cells_of(k, vertices):
    """The cells that touch any of ``vertices``."""
    return np.nonzero(np.isin(k.m.cells, vertices).any(axis=1))[0]


# ------------------------------------------------------------------ floors: float64 local scalars against the extended ones
def measure_floors(k):
    """quantity -> max over its terms of |Phi_t (float64 oracle) - Phi_t (extended)| / A_t."""
    T64, TLD = Terms(k, ld=False), Terms(k, ld=True)
    names = list(_CELL_TERMS) + ["penalty"]
    v64, vld, A = T64.scalars(names), TLD.scalars(names), TLD.scalars(names, absolute=True)
    err = {t: pm._ratio(pm._diff(v64[t], vld[t]), A[t].astype(np.float64)) for t in v64}
    out = {q: max(err[t] for t in ts if t in err) for q, ts in _QUANTITY_TERMS.items() if q in quantities(k.name)}
    # forward mode: the local residual vectors, each row against its own |Ke| |w_e| + |F_e| (penalty blocks: |P_f| |w_f - g_f|)
    y64, p64 = T64.vectors()
    yld, pld = TLD.vectors()
    Ay, Ap = TLD.vectors(absolute=True)
    e = pm._ratio(pm._diff(y64, yld), Ay.astype(np.float64))
    for f in range(len(pld)):
        for j in range(len(pld[f])):
            e = max(e, pm._ratio(pm._diff(p64[f][j], pld[f][j]), Ap[f][j].astype(np.float64)))
    out["jvp:uhat:dense"] = out["jvp:uhat:clamp"] = e
    return out


# ------------------------------------------------------------------ the golden file
def load_golden():
    """(case, quantity) -> (reference as longdouble hi + lo, unc, scale)."""
    g = np.load(GOLDEN)
    out = {}
    for name in CASES:
        for q in quantities(name):
            key = f"{name}|{q}|"
            out[(name, q)] = (g[key + "hi"].astype(LD) + g[key + "lo"].astype(LD), g[key + "unc"], g[key + "scale"])
    return out


def split(ref):
    """A longdouble array as a pair of float64 (hi + lo == ref where longdouble has 64 mantissa bits)."""
    hi = ref.astype(np.float64)
    return hi, (ref - hi.astype(LD)).astype(np.float64)


# SHAPE_FLOOR[(quantity, case)]: twice the value measure_floors gave when the table was made; tests/test_shape_ref_cpu.py measures it again
# and holds every constant between that and four times that.
SHAPE_FLOOR = {
    ("dRdT:uhat", "warped-uhat-penalty"): 1.42e-15,
    ("dJ:compliance:uhat", "warped-uhat-penalty"): 8.11e-16,
    ("dJ:mass:uhat", "warped-uhat-penalty"): 2.15e-15,
    ("dJ:elastic_energy:uhat", "warped-uhat-penalty"): 1.79e-15,
    ("dJ:pnorm_stress:uhat", "warped-uhat-penalty"): 1.48e-14,
    ("dJ:pnorm_stress:uhat@reg", "warped-uhat-penalty"): 1.48e-14,
    ("jvp:uhat:dense", "warped-uhat-penalty"): 5.15e-15,
    ("jvp:uhat:clamp", "warped-uhat-penalty"): 5.15e-15,
    ("dRdT:uhat", "tri-ewm-uhat-strong"): 2.24e-14,
    ("dJ:compliance:uhat", "tri-ewm-uhat-strong"): 2.77e-15,
    ("dJ:mass:uhat", "tri-ewm-uhat-strong"): 8.96e-15,
    ("dJ:elastic_energy:uhat", "tri-ewm-uhat-strong"): 3.27e-14,
    ("dJ:pnorm_stress:uhat", "tri-ewm-uhat-strong"): 2.26e-13,
    ("jvp:uhat:dense", "tri-ewm-uhat-strong"): 6.53e-14,
    ("jvp:uhat:clamp", "tri-ewm-uhat-strong"): 6.53e-14,
    ("dRdT:uhat", "tee-uhat-penalty"): 1.31e-15,
    ("dJ:compliance:uhat", "tee-uhat-penalty"): 2.46e-16,
    ("dJ:mass:uhat", "tee-uhat-penalty"): 5.11e-16,
    ("dJ:elastic_energy:uhat", "tee-uhat-penalty"): 1.58e-15,
    ("dJ:pnorm_stress:uhat", "tee-uhat-penalty"): 1.13e-14,
    ("jvp:uhat:dense", "tee-uhat-penalty"): 2.37e-15,
    ("jvp:uhat:clamp", "tee-uhat-penalty"): 2.37e-15,
    ("dRdT:uhat", "delaunay-uhat-penalty"): 1.42e-14,
    ("dJ:compliance:uhat", "delaunay-uhat-penalty"): 5.84e-15,
    ("dJ:mass:uhat", "delaunay-uhat-penalty"): 1.21e-14,
    ("dJ:elastic_energy:uhat", "delaunay-uhat-penalty"): 2.82e-14,
    ("dJ:pnorm_stress:uhat", "delaunay-uhat-penalty"): 1.75e-13,
    ("dJ:pnorm_stress:uhat@sub", "delaunay-uhat-penalty"): 1.75e-13,
    ("jvp:uhat:dense", "delaunay-uhat-penalty"): 5.39e-14,
    ("jvp:uhat:clamp", "delaunay-uhat-penalty"): 5.39e-14,
    ("dRdT:uhat", "cg1-uhat-strong"): 1.27e-15,
    ("dJ:compliance:uhat", "cg1-uhat-strong"): 1.12e-15,
    ("dJ:mass:uhat", "cg1-uhat-strong"): 2.15e-15,
    ("dJ:elastic_energy:uhat", "cg1-uhat-strong"): 2.99e-15,
    ("dJ:pnorm_stress:uhat", "cg1-uhat-strong"): 1.6e-14,
    ("jvp:uhat:dense", "cg1-uhat-strong"): 3.68e-15,
    ("jvp:uhat:clamp", "cg1-uhat-strong"): 3.68e-15,
    ("dRdT:uhat", "cr1-uhat-penalty"): 1.55e-14,
    ("dJ:compliance:uhat", "cr1-uhat-penalty"): 7.68e-15,
    ("dJ:mass:uhat", "cr1-uhat-penalty"): 1.62e-14,
    ("dJ:elastic_energy:uhat", "cr1-uhat-penalty"): 3.78e-14,
    ("dJ:pnorm_stress:uhat", "cr1-uhat-penalty"): 3.25e-13,
    ("jvp:uhat:dense", "cr1-uhat-penalty"): 7.01e-14,
    ("jvp:uhat:clamp", "cr1-uhat-penalty"): 7.01e-14,
    ("dRdT:uhat", "laminate"): 1.43e-15,
    ("dJ:compliance:uhat", "laminate"): 8.11e-16,
    ("dJ:mass:uhat", "laminate"): 2.15e-15,
    ("dJ:elastic_energy:uhat", "laminate"): 3.89e-15,
    ("dJ:pnorm_stress:uhat", "laminate"): 1.48e-14,
    ("jvp:uhat:dense", "laminate"): 1.41e-14,
    ("jvp:uhat:clamp", "laminate"): 1.41e-14,
}
# widened single constants: (quantity, case) -> (bound, the argument); none may reach 1e-12
WIDENED = {}


def bound(quantity, case):
    """What a shape kernel may differ from the reference by: parity_metrics.BOUND_FACTOR floors, or the widened constant."""
    if (quantity, case) in WIDENED:
        b = WIDENED[(quantity, case)][0]
        assert b < 1e-12
        return b
    return pm.BOUND_FACTOR * SHAPE_FLOOR[(quantity, case)]
