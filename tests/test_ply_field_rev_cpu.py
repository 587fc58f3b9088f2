"""The numpy reference of the reverse mode of the ply failure field (tests/ply_field_rev_ref.py) without a GPU: its two Jacobians
against the forward reference tests/field_jvp_ref.py, and against central differences of the oracle's own field."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_jvp_ref import fi_gap, ply_field_tangent                               # noqa: E402
from oracle.rm_shell_oracle import degree4_rule                                  # noqa: E402
from ply_failure_ref import PlyFailureOracle                                     # noqa: E402
from ply_field_rev_ref import ply_field_jacobians                                # noqa: E402
from test_gpu_laminate import _mesh, random_laminate                             # noqa: E402
from test_gpu_ply_failure import random_table                                    # noqa: E402

PLY_KINDS = ["warped", "tri", "quad CG1CG1", "tri CG2CR1"]


def _oracle(kind, seed=0, nply=2):
    """The oracle half of test_gpu_ply_failure.py::_pair, with the same draws in the same order."""
    m = _mesh(kind)
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (m.nn, 3))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    random_laminate(m.nel, rng)
    tab = random_table(m.nel, rng, nply)
    o = PlyFailureOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f, uhat=uh)
    o.set_ply_table(tab, 2 * nply)
    return m, o, rng, tab


@pytest.mark.parametrize("kind", PLY_KINDS)
def test_jacobians_against_the_forward_reference(kind):
    """J_w dw and J_t dt equal ply_field_tangent (both take the first maximiser) to 1e-13 of the largest entry; the shapes, and every
    row of J_t inside its own recovery point's 16 columns."""
    m, o, rng, tab = _oracle(kind)
    npt = tab.shape[1]
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    Jw, Jt = ply_field_jacobians(o, w, tab)
    assert Jw.shape == (m.nel * npt, m.ndof) and Jt.shape == (m.nel * npt, tab.size)
    assert np.array_equal(Jt.indices.reshape(-1, 16), np.arange(tab.size).reshape(-1, 16))
    for _ in range(3):
        dw = 2e-3 * rng.uniform(-1, 1, m.ndof)
        dt = tab * rng.uniform(-1, 1, tab.shape)
        for got, want in ((Jw @ dw, ply_field_tangent(o, w, tab, dw=dw)[0]), (Jt @ dt.ravel(), ply_field_tangent(o, w, tab, dtable=dt)[0])):
            err = np.abs(got - want.ravel()).max() / np.abs(want).max()
            print(f"{kind}: {err:.1e}")
            assert np.abs(want).max() > 0 and err <= 1e-13


@pytest.mark.parametrize("kind", PLY_KINDS)
def test_state_jacobian_against_central_differences_of_the_field(kind):
    """Central differences of o.field along a state direction, step 1e-6 relative, bar 1e-6 of the largest entry, on the entries whose
    two largest FI differ by 1e-6 max|FI| (FI is quadratic in the state: the difference is exact up to rounding where the maximiser
    stays)."""
    m, o, rng, tab = _oracle(kind)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    dw = 2e-3 * rng.uniform(-1, 1, m.ndof)
    Jw, _ = ply_field_jacobians(o, w, tab)
    fi = o.failure_index(w)[0]
    keep = fi_gap(fi) >= 1e-6 * np.abs(fi).max()
    eps = 1e-6
    fd = (o.field(w + eps * dw) - o.field(w - eps * dw)) / (2 * eps)
    got = (Jw @ dw).reshape(fd.shape)
    err = np.abs(got - fd)[keep].max() / np.abs(fd).max()
    print(f"{kind}: {err:.1e}, kept {100 * keep.mean():.1f} %")
    assert keep.mean() >= 0.99 and err <= 1e-6
