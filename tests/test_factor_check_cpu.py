"""tests/factor_check.py pinned on the CPU: the scaled backward error omega of an exact (LAPACK) Cholesky factor of the oracle's K sits at
rounding level on a penalised plate (penalty 1e15, cond ~1e13) and on a wing skin with strong conditions, one factor entry off by a
relative 1e-10 raises it a hundredfold and more, and the metric the factor was checked with before (rel(K M^-1 v, v) < 1e-7) does not
notice that same perturbation."""
import numpy as np
import pytest
import scipy.linalg as la

from factor_check import omega, omega_fit, rel
from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh
from oracle.rm_shell_oracle import ShellOracle


def _case(name):
    r = np.random.default_rng(1)
    if name == "plate":
        m = plate_mesh(2.0, 5.0, 12, 12)
        o = ShellOracle(m, penalty_facets=m.penalty_facets(lambda x: np.less(x[0], 3e-16)))
        o.set_fields(h=0.02 * (1 + 0.3 * r.uniform(-1, 1, m.nn)), E=7e10, nu=0.3, rho=2700.0)
    else:
        m = wing_skin_mesh(8, 20, shuffle=True).renumbered()[0]
        o = ShellOracle(m, strong_dofs=m.locate_dofs_geometrical(lambda x: np.less(x[1], 1e-9)))
        o.set_fields(h=0.05 * (1 + 0.3 * r.uniform(-1, 1, m.nn)), E=3e7, nu=0.3, rho=10.0)
    return m, o.assemble_K().tocsr()


# (mesh, pivot): a diagonal entry of L whose relative change of 1e-10 moves omega above 1e-11 while rel(K z, v) stays below the old
# bound -- found by a first-order scan over all pivots of these two (deterministic) problems; most pivots move omega less, the metric
# is a maximum over rows and right-hand sides and a single entry is the smallest error a kernel can make
@pytest.mark.parametrize("name,pivot", [("plate", 2381), ("wing", 2210)])
def test_backward_error_sees_one_wrong_factor_entry(name, pivot):
    m, K = _case(name)
    assert m.ndof in (2382, 2658)
    L = la.cholesky(K.toarray(), lower=True)
    V = np.random.default_rng(5).uniform(-1, 1, (m.ndof, 4))
    Z = la.cho_solve((L, True), V)
    w0 = omega(K, V, Z)
    assert w0 < 1e-13
    assert max(omega(K, V[:, j], Z[:, j]) for j in range(4)) == w0          # one column at a time: the same maximum
    assert rel(K @ Z, V) > 1e-9                                                # the conditioning floor of the old metric
    Lp = L.copy()
    Lp[pivot, pivot] *= 1 + 1e-10
    Zp = la.cho_solve((Lp, True), V)
    wp = omega(K, V, Zp)
    assert wp > 1e-11 and wp > 100 * w0
    assert rel(K @ Zp, V) < 1e-7                                               # ... which the old bound lets through
    # omega_fit: blind to the scale of x, not to its direction
    assert omega_fit(K, V[:, 0], 3.7 * Z[:, 0]) < 1e-13
    assert omega(K, V[:, 0], 3.7 * Z[:, 0]) > 0.5
    assert max(omega_fit(K, V[:, j], -2.0 * Zp[:, j]) for j in range(4)) > 1e-11


def test_omega_shapes_and_zero_rows():
    import scipy.sparse as sp
    K = sp.diags([2.0, 3.0, 4.0]).tocsr()
    v = np.array([2.0, 0.0, 4.0])
    assert omega(K, v, np.array([1.0, 0.0, 1.0])) == 0.0                      # 0 / 0 rows count as exact
    assert omega(K, v, np.array([1.0, 1e-3, 1.0])) == 1.0                     # a row with only the error: omega = 1
    with pytest.raises(ValueError):
        omega(K, v, np.ones((3, 2)))
    with pytest.raises(ValueError):
        omega(sp.diags([1.0, 0.0, 1.0]).tocsr(), v, v)
