"""Cases and quantities of the row-scaled operator parity (tests/test_gpu_operator_rowscaled.py on the device, tests/test_parity_metrics_cpu.py
for the oracle's own floors): which problems, which inputs, what the oracle says in float64, what a higher-precision evaluation of the
same thing says, and the scale each error is relative to.  No GPU is needed to import this; ``build(name, device=True)`` makes the context."""
import copy
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_metrics as pm          # noqa: E402
import test_gpu_parity as par        # noqa: E402

LD = np.longdouble
OPERATOR = (0.5, 2.0 / 1e-3 ** 2)    # the step operator of the transient path at dt = 1e-3: aK K + aM M


def _name(kind, ewm, ewp, uhat, bc):
    return kind + ("-ewm" if ewm else "") + ("-ewp" if ewp else "") + ("-uhat" if uhat else "") + "-" + bc


# the nine cases of test_gpu_parity.test_operator_level_parity, then the variants they leave out
CASES = {_name(*t): dict(kind=t[0], ewm=t[1], ewp=t[2], uhat=t[3], bc=t[4]) for t in par.CASES}
CASES.update({
    "cg1-penalty": dict(kind="warped", element="CG1CG1", bc="penalty"),
    "cg1-uhat-strong": dict(kind="warped", element="CG1CG1", bc="strong", uhat=True),
    "cr1-uhat-penalty": dict(kind="tri", element="CG2CR1", bc="penalty", uhat=True),
    "cr1-strong": dict(kind="tri", element="CG2CR1", bc="strong"),
    "laminate": dict(kind="warped", bc="penalty", uhat=True, laminate=True),
    "nred2": dict(kind="warped", bc="penalty", nred=2),
    "transient": dict(kind="warped", bc="strong", operator=OPERATOR),       # op_apply_vec2 applies it unmasked and without the penalty
    "prescribed": dict(kind="warped", bc="penalty", uhat=True, prescribed=True),
    "fan70": dict(kind="fan70", bc="penalty"),                                # a vertex of valence 70; 1896 DOF
})
PROBES = ("uniform", "element", "free")
ISOTROPIC = ("thickness", "E", "nu")
ORACLE_FIELD = {"thickness": "h", "E": "E", "nu": "nu"}


class Case:
    pass


def build(name, device=True):
    """The case ``name``: mesh, float64 oracle, context (None without ``device``) and the inputs every check of the case uses."""
    spec = CASES[name]
    k = Case()
    k.name, k.spec = name, spec
    k.m, o, k.c, rng = par._pair(spec["kind"], spec.get("ewm", False), spec.get("ewp", False), spec.get("uhat", False), spec["bc"],
                                 element=spec.get("element"), device=device)
    k.laminate, k.operator, k.prescribed = bool(spec.get("laminate")), spec.get("operator"), bool(spec.get("prescribed"))
    m, c = k.m, k.c
    if k.laminate or spec.get("nred"):
        from laminate_ref import LaminateOracle
        from oracle.rm_shell_oracle import ShellOracle
        o2 = (LaminateOracle if k.laminate else ShellOracle)(m, penalty_facets=o.penalty_facets, beta=o.beta, nred=spec.get("nred", 0))
        o2.set_fields(h=o.h, E=o.E, nu=o.nu, rho=o.rho, f=o.f, uhat=o.uhat)
        o = o2
        if spec.get("nred") and c is not None:
            c.set_strain_quadrature(spec["nred"])
    if k.laminate:
        from test_gpu_laminate import random_laminate
        k.clt = random_laminate(m.nel, np.random.default_rng(4))
        o.set_laminate(k.clt)
        if c is not None:
            c.set_laminate(k.clt)
    k.o = o
    if k.operator is not None and c is not None:
        c.set_operator(*k.operator)
    blocks = o._penalty_blocks()
    k.clamped = np.unique(np.concatenate([d for d, _ in blocks])) if blocks else np.asarray(o.strong_dofs, dtype=np.int64)
    assert k.clamped.size > 0
    if k.prescribed:
        touched = np.unique(o.dofs[np.unique(o.penalty_facets[:, 0])])
        g = np.zeros(m.ndof)
        g[touched] = 1e-3 * rng.uniform(-1, 1, touched.size)
        o.set_dirichlet_values(g)
        if c is not None:
            c.set_field("dirichlet", g)
    # an interior element (none of its DOFs clamped), the one nearest to the middle of the mesh, and its first vertex
    is_clamped = np.zeros(m.ndof, dtype=bool)
    is_clamped[k.clamped] = True
    inner = np.nonzero(~is_clamped[o.dofs].any(axis=1))[0]
    centre = m.nodes[m.cells].mean(axis=1)
    k.element = int(inner[np.argmin(np.linalg.norm(centre[inner] - m.nodes.mean(axis=0), axis=1))])
    k.node = int(m.cells[k.element, 0])
    # inputs
    x = rng.uniform(-1, 1, m.ndof)
    xe = np.zeros(m.ndof)
    xe[o.dofs[k.element]] = rng.uniform(-1, 1, o.ldof)
    xf = rng.uniform(-1, 1, m.ndof)
    xf[k.clamped] = 0.0
    k.x = dict(uniform=x, element=xe, free=xf)
    k.w = 1e-3 * rng.uniform(-1, 1, m.ndof)
    k.w[o.strong_dofs] = 0.0
    k.lam = rng.uniform(-1, 1, m.ndof)
    # the operators of the oracle
    k.Kel = sp.csr_matrix(o.assemble_K(with_penalty=False, with_strong=False))
    k.Kel.sort_indices()
    if k.operator is None:
        k.K = sp.csr_matrix(o.assemble_K())
        k.Kvec = sp.csr_matrix(o.assemble_K(with_strong=False)) if o.strong_dofs.size else k.K
    else:
        k.K = k.Kvec = sp.csr_matrix(k.operator[0] * k.Kel + k.operator[1] * o.assemble_M())
    return k


def quantities(k):
    """The names of what is checked on the case, as test and floor table spell them."""
    kx = [f"Kx:{p}" for p in PROBES]
    if k.operator is not None:
        return kx
    if k.prescribed:
        return ["load", "residual"]
    q = ["Ke"] + kx + ["Kxvec:uniform", "diag", "residual", "load", "csr"]
    q += ["dRdT:laminate"] if k.laminate else [f"dRdT:{a}" for a in ISOTROPIC]
    q += ["dRdT:F_solid", "dJ:compliance:thickness", "dJ:compliance:disp_solid", "dJ:elastic_energy:disp_solid"]
    q += ["dJ:elastic_energy:laminate" if k.laminate else "dJ:elastic_energy:thickness"]
    return q


THICKNESS_DEPENDENT = ["Ke", "Kx:uniform", "Kx:element", "Kx:free", "Kxvec:uniform", "diag", "residual", "csr", "dRdT:thickness", "dRdT:E",
                       "dRdT:nu", "dJ:compliance:thickness", "dJ:elastic_energy:disp_solid", "dJ:elastic_energy:thickness"]


# ------------------------------------------------------------------ what the oracle says
def apply_M(o, x):
    """M x element by element in the accumulator type of ``o`` (the sums of ShellOracle.assemble_M without the matrix)."""
    y = np.zeros(o.mesh.ndof, dtype=o.acc)
    nu = 3 * o.npc
    for sl in o._chunks():
        g = o._geometry(sl, o.N1, o.dN1)
        c = o.wts[None, :] * g["det"] * g["Ju"] * o._at_qp(o.rho, sl) * o._at_qp(o.h, sl)
        d = o.dofs[sl]
        yu = np.einsum("eq,qa,qb,ebc->eac", c, o.N2, o.N2, x[d[:, :nu]].reshape(-1, o.npc, 3))
        yt = np.einsum("eq,qa,qb,ebc->eac", c * (o.hK[sl] ** 2)[:, None], o.NR, o.NR, x[d[:, nu:]].reshape(-1, o.nvc, 3))
        np.add.at(y, d[:, :nu].ravel(), yu.ravel())
        np.add.at(y, d[:, nu:].ravel(), yt.ravel())
    return y


def _matrix_free(k, o, x, strong=True):
    """The operator of the case applied element by element in the accumulator type of ``o``."""
    if k.operator is not None:
        return k.operator[0] * o.apply_K(x, with_penalty=False) + k.operator[1] * apply_M(o, x)
    if not (strong and o.strong_dofs.size):
        return o.apply_K(x)
    xm = x.copy()
    xm[o.strong_dofs] = 0
    y = o.apply_K(xm)
    y[o.strong_dofs] = x[o.strong_dofs]
    return y


def oracle_values(k, o=None, only=None):
    """quantity -> value.  With the float64 oracle of the case: through its assembled matrices, as the operator-level tests always
    compared.  With ``extended(k.o)``: the same sums element by element in numpy.longdouble."""
    f64 = o is None
    o = k.o if f64 else o
    t = (lambda a: a) if f64 else (lambda a: a.astype(LD))
    w, lam = t(k.w), t(k.lam)
    want = [q for q in quantities(k) if only is None or q in only]
    v = {}
    Ke = o.element_matrices() if not f64 and {"Ke", "diag", "csr"} & set(want) else None
    for q in want:
        if q == "Ke":
            v[q] = o.element_matrices() if f64 else Ke
        elif q.startswith("Kx:"):
            x = k.x[q[3:]]
            v[q] = k.K @ x if f64 else _matrix_free(k, o, t(x))
        elif q == "Kxvec:uniform":
            v[q] = k.Kvec @ k.x["uniform"] if f64 else _matrix_free(k, o, t(k.x["uniform"]), strong=False)
        elif q == "diag":
            if f64:
                v[q] = k.K.diagonal()
            else:
                d = np.zeros(k.m.ndof, dtype=LD)
                np.add.at(d, o.dofs.ravel(), np.einsum("eii->ei", Ke).ravel())
                for dofs, blk in o._penalty_blocks():
                    d[dofs] += np.diag(blk)
                d[o.strong_dofs] = 1
                v[q] = d
        elif q == "csr":
            if f64:
                v[q] = k.Kel
            else:
                n = k.m.ndof
                keys = (np.repeat(o.dofs, o.ldof, axis=1).astype(np.int64) * n + np.tile(o.dofs, (1, o.ldof))).ravel()
                uniq, inv = np.unique(keys, return_inverse=True)
                assert uniq.size == k.Kel.nnz
                vals = np.zeros(uniq.size, dtype=LD)
                np.add.at(vals, inv.ravel(), Ke.ravel())
                v[q] = vals
        elif q == "load":
            v[q] = o.load_vector()
        elif q == "residual":
            v[q] = (k.K @ k.w if f64 else _matrix_free(k, o, w)) - o.load_vector()
        elif q == "dRdT:laminate":
            v[q] = o.dRdlam_T(w, lam).ravel()
        elif q == "dRdT:F_solid":
            v[q] = o.dRdf_T(lam)
        elif q.startswith("dRdT:"):
            v[q] = o.dRdfield_T(ORACLE_FIELD[q[5:]], w, lam)
        elif q == "dJ:compliance:thickness":
            v[q] = o.dcompliance_dh(w)
        elif q == "dJ:compliance:disp_solid":
            v[q] = o.dcompliance_du(w)
        elif q == "dJ:elastic_energy:disp_solid":
            v[q] = o.apply_K(w, with_penalty=False)
        elif q == "dJ:elastic_energy:thickness":
            v[q] = 0.5 * o.dRdfield_T("h", w, w)
        elif q == "dJ:elastic_energy:laminate":
            v[q] = 0.5 * o.dRdlam_T(w, w).ravel()
        else:
            raise KeyError(q)
    return v


def extended(o):
    """The oracle with its operands cast to numpy.longdouble -- node coordinates, fields, laminate and prescribed values (the
    quadrature tables and the cell diameters are data of the discrete problem and stay as they are) -- and ``acc`` raised to longdouble:
    the same methods then form the geometry, B, C, every einsum and every scatter-add in extended precision."""
    e = copy.copy(o)
    e.acc = LD
    e.mesh = copy.copy(o.mesh)
    e.mesh.nodes = o.mesh.nodes.astype(LD)
    for name in ("h", "E", "nu", "rho", "f", "uhat", "clt", "g_dirichlet"):
        if getattr(o, name, None) is not None:
            setattr(e, name, getattr(o, name).astype(LD))
    return e


def supports_dd(k):
    """CpuShell.assemble_K_dd: the isotropic law with the rotation on the vertices, no strong DOFs, the stiffness alone."""
    return not (k.laminate or k.o.strong_dofs.size or k.o.cr or k.operator is not None or k.prescribed)


def dd_values(k):
    """K x, the diagonal and the CSR values from the double-double assembly (hi + lo, applied in numpy.longdouble)."""
    from oracle.cpu_baseline import CpuShell
    rowptr, colidx, val = CpuShell(k.o).assemble_K_dd()
    hi, lo = val[:, 0].astype(LD), val[:, 1].astype(LD)
    assert np.all(np.diff(rowptr) > 0)
    heads = rowptr[:-1].astype(np.int64)

    def mv(x):
        xl = x.astype(LD)[colidx]
        return np.add.reduceat(hi * xl + lo * xl, heads)
    v = {f"Kx:{p}": mv(k.x[p]) for p in PROBES}
    v["Kxvec:uniform"] = v["Kx:uniform"]
    rows = np.repeat(np.arange(k.m.ndof), np.diff(rowptr))
    on = rows == colidx
    assert on.sum() == k.m.ndof
    v["diag"] = (hi + lo)[on]
    el = copy.copy(k.o)
    el.penalty_facets = np.zeros((0, 2), np.int32)
    rp, ci, ve = CpuShell(el).assemble_K_dd()
    assert np.array_equal(rp, k.Kel.indptr) and np.array_equal(ci, k.Kel.indices)
    v["csr"] = ve[:, 0].astype(LD) + ve[:, 1].astype(LD)
    return v


# ------------------------------------------------------------------ the error of a value under the metric of its quantity
class Reference:
    """The float64 oracle's values of a case with their scales, computed once and left unchanged."""

    def __init__(self, k):
        self.k = k
        self.values = oracle_values(k)
        self._scale = {}

    def scale(self, q):
        if q not in self._scale:
            k, o = self.k, self.k.o
            if q == "load":
                s = o.load_vector(absolute=True)
            elif q == "dRdT:laminate":
                s = o.dRdlam_T(k.w, k.lam, absolute=True).ravel()
            elif q == "dRdT:F_solid":
                s = o.dRdf_T(k.lam, absolute=True)
            elif q.startswith("dRdT:"):
                s = o.dRdfield_T(ORACLE_FIELD[q[5:]], k.w, k.lam, absolute=True)
            elif q == "dJ:compliance:thickness":
                s = o.dcompliance_dh(k.w, absolute=True)
            elif q == "dJ:compliance:disp_solid":
                s = o.dcompliance_du(k.w, absolute=True)
            elif q == "dJ:elastic_energy:thickness":
                s = 0.5 * o.dRdfield_T("h", k.w, k.w, absolute=True)
            elif q == "dJ:elastic_energy:laminate":
                s = 0.5 * o.dRdlam_T(k.w, k.w, absolute=True).ravel()
            else:
                raise KeyError(q)
            self._scale[q] = s
        return self._scale[q]

    def error(self, q, value):
        """``q`` may carry a route after '@' (``Kx:uniform@lanes5``, ``csr@host``): the same quantity, the same reference."""
        k = self.k
        q = q.split("@")[0]
        ref = self.values[q]
        if q == "Ke":
            return pm.entry_scaled(value, ref)
        if q == "csr":
            return pm.entry_scaled(value, ref)
        if q.startswith("Kx:"):
            return pm.row_scaled(value, ref, k.K, k.x[q[3:]])
        if q == "Kxvec:uniform":
            return pm.row_scaled(value, ref, k.Kvec, k.x["uniform"])
        if q == "diag":
            return pm.entrywise(value, ref)
        if q == "residual":
            return pm.row_scaled(value, ref, k.K, k.w, extra=np.abs(k.o.load_vector()))
        if q == "dJ:elastic_energy:disp_solid":
            return pm.row_scaled(value, ref, k.Kel, k.w)
        return pm.term_scaled(value, ref, self.scale(q))


def measure_floors(k, ref=None):
    """quantity -> (metric of the float64 oracle against the higher-precision evaluation, its source "dd" | "ld")."""
    ref = Reference(k) if ref is None else ref
    out = {}
    dd = dd_values(k) if supports_dd(k) else {}
    ld = oracle_values(k, extended(k.o), only=[q for q in quantities(k) if q not in dd])
    for q in quantities(k):
        hp, src = (dd[q], "dd") if q in dd else (ld[q], "ld")
        # the metric is symmetric in its first two arguments up to the scale, which comes from the float64 reference either way
        out[q] = (ref.error(q, hp), src)
    return out
