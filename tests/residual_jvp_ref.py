"""CPU reference of the forward products (dR/d arg) v of the static shell residual, for arg in thickness / E / nu (nodal or element-wise),
F_solid and laminate: numpy restatements on the oracle's ``_B``, ``_C(deriv=...)`` and ``_geometry`` -- the same building blocks as its
transposed products ``dRdfield_T`` / ``dRdf_T``, contracted the other way.  No complex steps, no finite differences.

R is the residual the library returns (femo_residual): rows of strong Dirichlet DOFs hold w - g, which no input moves, and the operator
sees the state with those rows zeroed -- so the products zero the strong rows of the result and the strong entries of the state."""
import numpy as np

from oracle.rm_shell_oracle import ShellOracle       # noqa: F401  (the oracle is imported as the other *_ref helpers import it)


def _state(o, w):
    w = np.array(w, dtype=np.float64)
    w[o.strong_dofs] = 0.0
    return w


def _scatter(o, sl, ye, out):
    np.add.at(out, o.dofs[sl].ravel(), ye.ravel())


def jvp_field(o, name, w, v):
    """(dR/d field) v, field 'h', 'E' or 'nu': y_e = sum_q B^T (dC/d field . v(q)) B w, v interpolated to the point as the field is."""
    w = _state(o, w)
    out = np.zeros(o.mesh.ndof)
    for sl in o._chunks():
        B, g = o._B(sl)
        dC = o._C(sl, g, deriv=name) * o._at_qp(np.asarray(v, dtype=np.float64), sl)[..., None, None]
        sw = np.einsum("eqij,ej->eqi", B, w[o.dofs[sl]])
        _scatter(o, sl, np.einsum("eqik,eqij,eqj->ek", B, dC, sw), out)
    out[o.strong_dofs] = 0.0
    return out


def jvp_load(o, v):
    """(dR/d F_solid) v = - int N_a v J dx (the load vector of the direction, with the residual's sign)."""
    keep = o.f
    o.f = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    g_keep = getattr(o, "g_dirichlet", None)
    o.g_dirichlet = None                              # the penalty's P g does not depend on the load
    try:
        out = -o.load_vector()
    finally:
        o.f = keep
        o.g_dirichlet = g_keep
    return out


def jvp_laminate(o, w, v):
    """(dR/d laminate) v for a ``LaminateOracle``: R is linear in the per-cell values, so the product is the elastic operator with the
    direction as the law (it acts through the symmetric parts of its blocks, as the law itself does)."""
    w = _state(o, w)
    keep = o.clt
    o.clt = np.asarray(v, dtype=np.float64).reshape(o.mesh.nel, 32)
    try:
        out = o.apply_K(w, with_penalty=False)
    finally:
        o.clt = keep
    out[o.strong_dofs] = 0.0
    return out
