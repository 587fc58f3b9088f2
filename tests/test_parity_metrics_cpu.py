"""The metrics of tests/parity_metrics.py on the CPU: the floors of the float64 oracle against a higher-precision evaluation of the same
quantities (the constants the GPU bounds are multiples of), what the old and the new metrics make of a known perturbation, and the
edges of the metric functions."""
import copy
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity_metrics as pm          # noqa: E402
import rowscaled_cases as rc         # noqa: E402

_cases = {}


def _case(name):
    if name not in _cases:
        k = rc.build(name, device=False)
        _cases[name] = (k, rc.Reference(k))
    return _cases[name]


# ------------------------------------------------------------------ floors of the reference alone
@pytest.mark.parametrize("name", list(rc.CASES))
def test_recorded_floors_are_the_measured_ones(name):
    """Every REFERENCE_FLOOR constant of the case lies between the value measured now and four times that, and comes from the source
    the table names: the double-double assembly where it takes the case, the oracle's own sums in numpy.longdouble elsewhere."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.fail("numpy.longdouble is not wider than float64 here: the floors cannot be measured")
    k, ref = _case(name)
    measured = rc.measure_floors(k, ref)
    assert {q for q, c in pm.REFERENCE_FLOOR if c == name} == set(rc.quantities(k))
    bad = []
    for q, (value, source) in measured.items():
        recorded = pm.REFERENCE_FLOOR[(q, name)]
        print(f"floor {name} {q} {value:.3e} ({source}; recorded {recorded:.3e})")
        assert source == ("dd" if q in pm.REFERENCE_SOURCE[name] else "ld")
        if not value <= recorded <= 4.0 * value:
            bad.append((q, value, recorded))
    assert not bad, bad


def test_double_double_assembly_is_the_same_operator():
    """The double-double values are a better evaluation of the oracle's matrix, not another matrix: they agree to float64 rounding."""
    k, ref = _case("warped-uhat-penalty")
    dd = rc.dd_values(k)
    assert pm.entry_scaled(dd["csr"], k.Kel) < 1e-13
    assert pm.entrywise(dd["diag"], k.K.diagonal()) < 1e-13


# ------------------------------------------------------------------ sensitivity, pinned
def _perturbed(k, factor):
    """The case with the thickness of its interior node scaled by ``factor`` (inputs unchanged)."""
    k2 = copy.copy(k)
    o = k2.o = copy.copy(k.o)
    o.h = k.o.h.copy()
    o.h[k.node] *= factor
    k2.Kel = sp.csr_matrix(o.assemble_K(with_penalty=False, with_strong=False))
    k2.Kel.sort_indices()
    k2.K = k2.Kvec = sp.csr_matrix(o.assemble_K())
    return k2


@pytest.mark.parametrize("name", ["plate-penalty", "warped-penalty"])
def test_one_thickness_off_by_1e_7_passes_rel_and_fails_every_new_metric(name):
    k, ref = _case(name)
    off = rc.oracle_values(_perturbed(k, 1.0 + 1e-7))
    r_kx, r_d = pm.rel(off["Kx:uniform"], ref.values["Kx:uniform"]), pm.rel(off["diag"], ref.values["diag"])
    print(f"sensitivity {name} rel(K x) {r_kx:.2e} rel(diag) {r_d:.2e}")
    assert r_kx < 1e-11 and r_d < 1e-11              # the blindness of the old metric, on record
    assert r_kx < 1e-14 and r_d < 1e-14              # (it does not even come close)
    for q in rc.THICKNESS_DEPENDENT:
        e, b = ref.error(q, off[q]), pm.bound(q, name)
        print(f"sensitivity {name} {q} {e:.2e} = {e / b:.1e} bounds")
        assert e > 1000.0 * b, q


@pytest.mark.parametrize("name", ["plate-penalty", "warped-penalty"])
def test_interior_rows_off_by_1e_8_pass_rel_and_fail_row_scaled(name):
    k, ref = _case(name)
    free = np.ones(k.m.ndof, dtype=bool)
    free[k.clamped] = False
    for q in ("Kx:uniform", "residual"):             # (a probe that is zero on the penalty DOFs has no penalty row to hide behind)
        y = ref.values[q].copy()
        y[free] *= 1.0 + 1e-8
        r, e, b = pm.rel(y, ref.values[q]), ref.error(q, y), pm.bound(q, name)
        print(f"sensitivity {name} {q} rows x (1 + 1e-8): rel {r:.2e}, row_scaled {e:.2e} = {e / b:.1e} bounds")
        assert r < 1e-11
        assert e > 1000.0 * b
    # the measurements parity_metrics.py quotes: three decades further off the old metric still passes (at 1e-4: 4e-12 on the plate,
    # 1.7e-11 on the warped mesh), and most rows lie far below the largest one
    y = ref.values["Kx:uniform"].copy()
    y[free] *= 1.0 + 1e-5
    assert pm.rel(y, ref.values["Kx:uniform"]) < 1e-11
    small = np.mean(np.abs(ref.values["Kx:uniform"]) < 1e-6 * np.abs(ref.values["Kx:uniform"]).max())
    print(f"sensitivity {name} rows of K x below 1e-6 of the largest: {100 * small:.1f} %")
    assert small > 0.9


def test_absolute_sums_bound_the_signed_ones():
    """absolute=True: every entry is at least the size of the signed sum and never negative; absolute=False is the plain call."""
    k, ref = _case("warped-uhat-penalty")
    o = k.o
    assert np.array_equal(o.load_vector(), o.load_vector(absolute=False))
    assert np.array_equal(o.dRdfield_T("h", k.w, k.lam), o.dRdfield_T("h", k.w, k.lam, absolute=False))
    for q in ("load", "dRdT:thickness", "dRdT:E", "dRdT:nu", "dRdT:F_solid", "dJ:compliance:thickness", "dJ:compliance:disp_solid",
              "dJ:elastic_energy:thickness"):
        s, v = ref.scale(q), ref.values[q]
        assert s.shape == v.shape and np.all(s >= 0)
        assert np.all(np.abs(v) <= s * (1 + 1e-12)), q
        assert np.any(np.abs(v) < 0.5 * s), q          # terms do cancel: the scale is not the value


# ------------------------------------------------------------------ edges of the metric functions
def test_rows_without_a_scale_must_match_exactly():
    K = sp.csr_matrix(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]))
    x = np.array([1.0, 1.0, 5.0])
    y = K @ x
    assert pm.row_scaled(y, y, K, x) == 0.0
    assert pm.row_scaled(y + [0.0, 3e-16, 0.0], y, K, x) == pytest.approx(1e-16)
    assert pm.row_scaled(y + [0.0, 0.0, 1e-300], y, K, x) == float("inf")          # row 2 adds nothing: any value but 0 is wrong
    assert pm.row_scaled(y + [0.0, 0.0, 1e-300], y, K, x, extra=[0.0, 0.0, 1.0]) == pytest.approx(1e-300)
    assert pm.row_scaled([np.nan, 1.0, 0.0], y, K, x) == float("inf")
    assert pm.term_scaled([1.0, 0.0], [1.0, 0.0], [2.0, 0.0]) == 0.0
    assert pm.term_scaled([1.0, 1e-30], [1.0, 0.0], [2.0, 0.0]) == float("inf")
    assert pm.entrywise([1.0, 0.0], [1.0, 0.0]) == 0.0
    assert pm.entrywise([1.0 + 2.0 ** -40, -2.0], [1.0, -2.0]) == pytest.approx(2.0 ** -40)
    assert pm.entrywise([1.0, 1e-30], [1.0, 0.0]) == float("inf")


def test_a_penalty_row_does_not_hide_the_others():
    K = sp.csr_matrix(np.array([[1e15, 0.0], [0.0, 3.0]]))
    x = np.array([1.0, 1.0])
    y = K @ x
    off = y * [1.0, 1.0 + 1e-4]
    assert pm.rel(off, y) < 1e-18
    assert pm.row_scaled(off, y, K, x) == pytest.approx(1e-4, rel=1e-6)
    assert pm.row_scaled(2.0 * off, 2.0 * y, 2.0 * K, x) == pytest.approx(1e-4, rel=1e-6)       # invariant to a scaling of the rows
    D = sp.diags([1e-6, 1.0])
    assert pm.row_scaled(D @ off, D @ y, D @ K, x) == pytest.approx(1e-4, rel=1e-6)


def test_entry_scaled_is_invariant_to_the_units_and_needs_a_diagonal():
    A = np.array([[[4.0, 1.0], [1.0, 9.0]]])
    E = np.array([[[0.0, 6e-12], [6e-12, 0.0]]])
    assert pm.entry_scaled(A + E, A) == pytest.approx(1e-12)
    D = np.diag([1e3, 1e-3])
    assert pm.entry_scaled((D @ (A + E)[0] @ D)[None], (D @ A[0] @ D)[None]) == pytest.approx(1e-12, rel=1e-3)
    S = sp.csr_matrix(A[0])
    assert pm.entry_scaled(sp.csr_matrix((A + E)[0]), S) == pytest.approx(1e-12)
    assert pm.entry_scaled(S.data.astype(np.longdouble) + np.longdouble(6e-12) * np.array([0, 1, 1, 0]), S) == pytest.approx(1e-12)
    with pytest.raises(ValueError):
        pm.entry_scaled(A, np.array([[[4.0, 1.0], [1.0, 0.0]]]))
    with pytest.raises(ValueError):
        pm.entry_scaled(S, sp.csr_matrix(np.array([[4.0, 1.0], [1.0, 0.0]])))
    with pytest.raises(ValueError):
        pm.entry_scaled(S, sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 2.0]])))


def test_shape_errors_are_raised():
    K = sp.identity(3, format="csr")
    with pytest.raises(ValueError):
        pm.row_scaled(np.zeros(2), np.zeros(3), K, np.zeros(3))
    with pytest.raises(ValueError):
        pm.row_scaled(np.zeros(3), np.zeros(3), K, np.zeros(4))
    with pytest.raises(ValueError):
        pm.row_scaled(np.zeros(3), np.zeros(3), sp.csr_matrix(np.ones((3, 2))), np.zeros(3))
    with pytest.raises(ValueError):
        pm.row_scaled(np.zeros(3), np.zeros(3), K, np.zeros(3), extra=-np.ones(3))
    with pytest.raises(ValueError):
        pm.entry_scaled(np.ones((2, 3, 3)), np.ones((2, 3, 4)))
    with pytest.raises(ValueError):
        pm.entry_scaled(np.ones((1, 3, 3)), np.stack([np.eye(3), np.eye(3)]))
    with pytest.raises(ValueError):
        pm.entry_scaled(sp.identity(4, format="csr"), K)
    with pytest.raises(ValueError):
        pm.entrywise(np.zeros(3), np.ones(4))
    with pytest.raises(ValueError):
        pm.term_scaled(np.zeros(3), np.zeros(3), np.ones(4))
    with pytest.raises(ValueError):
        pm.term_scaled(np.zeros(3), np.zeros(3), -np.ones(3))


def test_widened_bounds_stay_below_the_worst_case():
    """A widened constant carries its argument and stays below 1e-12, about the worst-case n u of these sums."""
    for key, (b, why) in pm.WIDENED.items():
        assert key in pm.REFERENCE_FLOOR and pm.BOUND_FACTOR * pm.REFERENCE_FLOOR[key] < b < 1e-12 and len(why) > 40
