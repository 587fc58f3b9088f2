"""The forward-product reference (tests/residual_jvp_ref.py) against the oracle's existing transposed products by dense probing: row i
of J = dR/d arg is ``dRdfield_T(name, w, e_i)`` / ``dRdf_T(e_i)`` / ``dRdlam_T(w, e_i)`` over all unit vectors e_i, and the reference's
J v must equal J @ v to 1e-12 of the largest entry (restatement against restatement, same formulas
contracted in another order).  Meshes of a few hundred DOFs keep the probing to seconds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import residual_jvp_ref as ref                                                    # noqa: E402
from femo_alpha_amd.mesh import plate_mesh, quads_to_triangles, wing_skin_mesh    # noqa: E402
from laminate_ref import LaminateOracle                                           # noqa: E402
from oracle.rm_shell_oracle import ShellOracle                                    # noqa: E402

TOL = 1e-12


def _mesh(kind):
    if kind == "quad":
        return wing_skin_mesh(2, 3, shuffle=True)
    if kind == "tri":
        return quads_to_triangles(wing_skin_mesh(2, 2, shuffle=True))
    return plate_mesh(2.0, 10.0, 2, 3)


def _oracle(kind, ewm, ewp=False, strong=False, cls=ShellOracle, seed=0):
    m = _mesh(kind)
    rng = np.random.default_rng(seed)
    nT = m.nel if ewm else m.nn
    nF = m.nel if ewp else m.nn
    sd = m.locate_dofs_geometrical(lambda x: np.less(x[1], 1e-12)) if strong else None
    o = cls(m, element_wise_material=ewm, elementwise_pressure=ewp, strong_dofs=sd)
    o.set_fields(h=0.05 * (1 + 0.3 * rng.uniform(-1, 1, nT)), E=3e7 * (1 + 0.2 * rng.uniform(-1, 1, nT)),
                 nu=0.3 + 0.05 * rng.uniform(-1, 1, nT), rho=np.ones(nT), f=rng.uniform(-1, 1, (nF, 3)),
                 uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3)))
    w = rng.uniform(-1, 1, m.ndof) * 1e-3
    w[o.strong_dofs] = 0.0
    assert m.ndof < 400
    return m, o, w, rng


def _probe(m, o, column):
    """J with row i = column(e_i); strong rows zeroed (R = w - g there)."""
    rows = []
    for i in range(m.ndof):
        e = np.zeros(m.ndof); e[i] = 1.0
        rows.append(np.asarray(column(e)).ravel())
    J = np.array(rows)
    J[o.strong_dofs] = 0.0
    return J


def _close(got, want):
    assert np.abs(got - want).max() <= TOL * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("kind,ewm,strong", [("quad", False, False), ("quad", True, True), ("tri", False, True), ("tri", True, False)])
def test_field_products_equal_the_probed_transposes(kind, ewm, strong):
    m, o, w, rng = _oracle(kind, ewm, strong=strong)
    for name in ("h", "E", "nu"):
        J = _probe(m, o, lambda e: o.dRdfield_T(name, w, e))
        assert np.abs(J).max() > 0
        for _ in range(2):
            v = rng.uniform(-1, 1, o.h.size)
            got = ref.jvp_field(o, name, w, v)
            _close(got, J @ v)
            assert np.all(got[o.strong_dofs] == 0.0)


@pytest.mark.parametrize("kind,ewp,strong", [("quad", False, True), ("quad", True, False), ("tri", False, False)])
def test_load_product_equals_the_probed_transpose(kind, ewp, strong):
    m, o, w, rng = _oracle(kind, False, ewp=ewp, strong=strong)
    J = _probe(m, o, o.dRdf_T)
    v = rng.uniform(-1, 1, o.f.shape)
    got = ref.jvp_load(o, v)
    _close(got, J @ v.ravel())
    assert np.all(got[o.strong_dofs] == 0.0)
    assert np.array_equal(o.f, _oracle(kind, False, ewp=ewp, strong=strong)[1].f)          # the oracle's own load is put back


@pytest.mark.parametrize("kind,strong", [("quad", False), ("tri", True)])
def test_laminate_product_equals_the_probed_transpose(kind, strong):
    m, o, w, rng = _oracle(kind, False, strong=strong, cls=LaminateOracle)
    o.set_laminate(rng.uniform(0.5, 1.5, (m.nel, 32)))                # the products never read the laminate itself
    J = _probe(m, o, lambda e: o.dRdlam_T(w, e))
    v = rng.uniform(-1, 1, (m.nel, 32))                               # not symmetric: the law acts through the symmetric parts
    _close(ref.jvp_laminate(o, w, v), J @ v.ravel())
    vs = v.copy()
    for lo, n in ((0, 3), (9, 3), (18, 3), (27, 2)):
        b = v[:, lo: lo + n * n].reshape(-1, n, n)
        vs[:, lo: lo + n * n] = (0.5 * (b + b.transpose(0, 2, 1))).reshape(-1, n * n)
    assert not np.array_equal(vs, v)
    _close(ref.jvp_laminate(o, w, vs), J @ v.ravel())
