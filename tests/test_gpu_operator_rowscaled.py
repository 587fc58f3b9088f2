"""Operator-level kernels against the oracle under metrics that see every row (tests/parity_metrics.py): element matrices, the
matrix-free operator on three probes, under both lane layouts and through the vector-id route, the diagonal, the residual, the load
vector, the CSR values with either map, the transposed derivative products and the partial gradients of the functionals -- each within
50 reference floors of the oracle (REFERENCE_FLOOR: what the float64 oracle itself reaches against a higher-precision evaluation;
tests/test_parity_metrics_cpu.py).  The kernels sum the same terms in another order (9-25 quadrature points, up to 39 columns, float
atomics on some paths): a random walk over n ~ 1e4 terms grows to sqrt(n) u ~ 1e-14 where the oracle's floor is ~1.5e-15, and 50 floors
stay five decades below what one thickness off by 1e-7 produces (3.8e-8).  The rel checks of test_gpu_parity.py stay beside these: they
are blind below the penalty rows (parity_metrics.py has the numbers), these are not.

Every value is printed as ``rowscaled <case> <quantity> <value>`` before anything is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_metrics as pm          # noqa: E402
import rowscaled_cases as rc         # noqa: E402
from test_gpu_building_blocks import _get, _put          # noqa: E402

pytestmark = pytest.mark.gpu

_cases = {}


def _case(name):
    """(case with its context, the oracle's reference) -- built once, shared by the tests of this module, left unchanged."""
    if name not in _cases:
        k = rc.build(name)
        _cases[name] = (k, rc.Reference(k))
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k, _ in _cases.values():
        k.c.close()
    _cases.clear()


def _apply(k, c, x, vec=False):
    """The operator of the case on the device: femo_apply_K; through vector ids (femo_op_apply_vec: no strong rows); or, for the
    transient case, femo_op_apply_vec2 with the coefficients of the step operator (unmasked, without the penalty)."""
    if k.operator is None and not vec:
        return c.apply_K(x)
    _put(c, "p", x)
    if k.operator is None:
        c.op_apply_vec("p", "Ap")
    else:
        c.op_apply_vec2("p", "Ap", k.operator[0], k.operator[1], with_penalty=False)
    return _get(c, "Ap").copy()


def device_values(k, c, only=None, routes=True):
    """quantity[@route] -> what the device computes, for the quantities of the case (``only``: a subset; ``routes``: also the lane
    layouts of the operator and the host-built CSR map)."""
    want = [q for q in rc.quantities(k) if only is None or q in only]
    v = {}
    if any(q.startswith(("dRdT:", "dJ:")) for q in want):
        c.set_state(k.w)
    for q in want:
        if q == "Ke":
            v[q] = c.element_matrices()
        elif q.startswith("Kx:"):
            x = k.x[q[3:]]
            v[q] = _apply(k, c, x)
            if routes:
                for lanes in ((4,) if k.laminate else (4, 5)):          # (the laminate operator exists for four lanes only)
                    c.set_option("apply_lanes", lanes)
                    v[f"{q}@lanes{lanes}"] = _apply(k, c, x)
                c.set_option("apply_lanes", 0)
        elif q == "Kxvec:uniform":
            v[q] = _apply(k, c, k.x["uniform"], vec=True)
        elif q == "diag":
            v[q] = c.diagonal()
        elif q == "residual":
            v[q] = c.residual(k.w)
        elif q == "load":
            v[q] = c.load_vector()
        elif q == "csr":
            info = c.enable_csr()
            assert np.array_equal(info["rowptr"], k.Kel.indptr) and np.array_equal(info["colidx"], k.Kel.indices)
            v[q] = c.assemble_csr()
            if routes:
                c.enable_csr(host_map=True)
                v[q + "@host"] = c.assemble_csr()
        elif q.startswith("dRdT:"):
            v[q] = c.dRdarg_T(q[5:], k.lam)
        elif q.startswith("dJ:"):
            _, fn, wrt = q.split(":")
            v[q] = c.dfunctional(fn, wrt)
        else:
            raise KeyError(q)
    return v


@pytest.mark.parametrize("name", list(rc.CASES))
def test_every_row_within_fifty_reference_floors(name):
    k, ref = _case(name)
    c = k.c
    values = device_values(k, c)
    assert {q.split("@")[0] for q in values} == set(rc.quantities(k))
    over = []
    for q, value in values.items():
        e, b = ref.error(q, value), pm.bound(q.split("@")[0], name)
        print(f"rowscaled {name} {q} {e:.3e}   (bound {b:.2e}, floor {pm.REFERENCE_FLOOR[(q.split('@')[0], name)]:.2e})")
        if not e <= b:
            over.append((q, e, b))
    if k.laminate:
        # the laminate replaces thickness, E and nu inside the elastic energy: no dependence, exact zeros
        for arg in rc.ISOTROPIC:
            assert np.all(c.dRdarg_T(arg, k.lam) == 0.0) and np.all(c.dfunctional("elastic_energy", arg) == 0.0)
    assert not over, over


@pytest.mark.parametrize("name", ["plate-penalty", "warped-uhat-penalty", "tri-penalty", "cg1-penalty", "cr1-uhat-penalty", "laminate",
                                  "fan70"])
def test_the_penalty_does_not_leak_into_other_rows(name):
    """Rows of apply_K(x) and entries of diagonal() that belong to no penalty facet's DOFs, with the facets at beta = 1e15 and at
    beta = 1: equal to 4 u (|K| |x|)_i, |K| from the device's own CSR values; for the diagonal, which has no x, the all-ones vector (the
    absolute row sum: the element pass adds the diagonal with float atomics, so two runs may differ by the order of a node's few
    contributions, and the entry comes back through two reciprocals).  No oracle."""
    k, _ = _case(name)
    c, pf = k.c, k.o.penalty_facets
    free = np.ones(k.m.ndof, dtype=bool)
    free[k.clamped] = False
    x = k.x["uniform"]
    c.enable_csr()
    Ka = abs(c.assemble_csr())
    scale, rowsum = Ka @ np.abs(x), Ka @ np.ones(k.m.ndof)
    got = {}
    try:
        for beta in (1e15, 1.0):
            c.set_penalty_facets(pf, beta)
            got[beta] = (c.apply_K(x), c.diagonal())
    finally:
        c.set_penalty_facets(pf, k.o.beta)
    ey = np.abs(got[1e15][0] - got[1.0][0])[free] / scale[free]
    ed = np.abs(got[1e15][1] - got[1.0][1])[free] / rowsum[free]
    print(f"rowscaled {name} penalty-leak:Kx {ey.max():.3e}")
    print(f"rowscaled {name} penalty-leak:diag {ed.max():.3e}")
    assert np.all(scale[free] > 0)
    assert ey.max() <= 4 * pm.U and ed.max() <= 4 * pm.U
    # and the clamped rows did change: the two runs are not one run
    assert np.all(np.abs(got[1e15][1][k.clamped]) > 1e6 * np.abs(got[1.0][1][k.clamped]))


@pytest.mark.parametrize("name", ["plate-penalty", "warped-penalty"])
def test_negative_control_one_thickness_off_by_1e_7(name):
    """The context with the thickness of one interior node scaled by 1 + 1e-7, the oracle with the unperturbed field: the old metric
    passes, every new one that depends on the thickness is at least 1000 bounds."""
    k, ref = _case(name)
    k2 = rc.build(name)
    c = k2.c
    try:
        h = c.get_field("thickness")
        h[k.node] *= 1.0 + 1e-7
        c.set_field("thickness", h)
        values = device_values(k2, c, only=rc.THICKNESS_DEPENDENT, routes=False)
    finally:
        c.close()
    assert set(values) == set(rc.THICKNESS_DEPENDENT)
    r_kx, r_d = pm.rel(values["Kx:uniform"], ref.values["Kx:uniform"]), pm.rel(values["diag"], ref.values["diag"])
    print(f"rowscaled {name} control:rel(Kx) {r_kx:.3e}")
    print(f"rowscaled {name} control:rel(diag) {r_d:.3e}")
    seen = {}
    for q, value in values.items():
        seen[q] = ref.error(q, value) / pm.bound(q, name)
        print(f"rowscaled {name} control:{q} {ref.error(q, value):.3e}   ({seen[q]:.1e} bounds)")
    assert r_kx < 1e-11 and r_d < 1e-11
    assert all(s >= 1000.0 for s in seen.values()), {q: s for q, s in seen.items() if s < 1000.0}
