"""The reference of the not-positive-definite verdict (tests/indefinite_ref.py) checked against itself, and the coverage the GPU
test (tests/test_gpu_indefinite.py) draws from it stated where no GPU is needed: which tree levels, panels and sub-blocks the first
non-positive pivot of the cases falls into.  If a condition fails, the choice of sigma or of the cell changes, not the condition."""
import numpy as np
import pytest

import indefinite_ref as ref

NAMES = ["plate", "plate_small", "wing_small"]


def _cases(name):
    return ref.shifted_cases(name, scan=name != "plate")


@pytest.mark.parametrize("name", NAMES)
def test_negative_pivots_count_the_eigenvalues_below_the_shift(name):
    """Sylvester: the elimination of K - sigma M in the plan's order has as many negative pivots as the pencil (K, M) has
    eigenvalues below sigma; the near miss has none.  Prints the table of the cases."""
    lam, cases = _cases(name)
    print("\n" + ref.table(name, cases))
    print("  lowest eigenvalues " + " ".join(f"{x:.4e}" for x in lam[:8]))
    assert cases[0]["label"] == "near miss" and cases[0]["count"] == 0 and cases[0]["level"] is None
    assert cases[0]["min_ratio_before"] >= ref.MARGIN
    for r in cases:
        assert lam[-1] > r["sigma"], "more eigenvalues than were computed may lie below the shift"
        assert r["count"] == int(np.sum(lam < r["sigma"])), (name, r["label"], r["count"], int(np.sum(lam < r["sigma"])))
        assert ref.has_margin(r), r
    assert [r["count"] for r in cases[:3]] == [0, 1, 3]


def test_plate_one_negative_pivot_late_in_the_root():
    """The one-negative case of the 64 x 64 plate: in the root front, beyond the first 256-column super-panel, and not in the first
    sub-block of its 128-column panel."""
    plan = ref.plan_of("plate")
    r = _cases("plate")[1][1]
    assert r["count"] == 1 and r["level"] == plan.nlevels - 1
    assert r["column"] >= 256 and r["column"] % ref.NBO >= ref.NB, r
    assert r["npiv_front"] > 512


@pytest.mark.parametrize("name", ["plate_small", "wing_small"])
def test_cases_reach_the_root_the_leaves_and_levels_between(name):
    plan = ref.plan_of(name)
    levels = {r["level"] for r in _cases(name)[1][1:]}
    assert plan.nlevels - 1 in levels and 0 in levels, levels
    assert len(levels - {0, plan.nlevels - 1}) >= 2, levels
    # the first negative position never moves up the tree as sigma grows
    by_sigma = sorted(_cases(name)[1][1:], key=lambda r: r["sigma"])
    assert all(a["level"] >= b["level"] for a, b in zip(by_sigma, by_sigma[1:]))


def test_a_first_negative_pivot_outside_the_first_sub_block():
    subs = [(n, r["label"], r["sub"]) for n in NAMES for r in _cases(n)[1][1:] if r["sub"] > 0]
    assert subs
    # and one in a later 128-column panel
    assert any(r["panel"] > 0 for n in NAMES for r in _cases(n)[1][1:])


def test_negative_cells_fail_in_their_leaf_front():
    cases = ref.negative_cell_cases("wing_small")
    print("\n" + ref.table("wing_small", cases))
    assert {r["factor"] for r in cases} == set(ref.CELL_FACTORS)
    for r in cases:
        assert r["count"] >= 1 and r["level"] == 0 and r["column"] > 0 and ref.has_margin(r), r
        # Sylvester again, on the matrix itself (2 658 DOFs: dense)
        assert r["count"] == int(np.sum(np.linalg.eigvalsh(r["K"].toarray()) < 0))


def test_elimination_order_is_a_permutation_that_follows_the_tree():
    for name in NAMES[1:]:
        plan = ref.plan_of(name)
        o = ref.elimination_order(plan)
        n = ref._mesh(name).ndof
        assert np.array_equal(np.sort(o["dofs"]), np.arange(n))
        assert np.all(np.diff(o["level"]) >= 0)
        assert np.all(o["panel"] * ref.NBO + o["sub"] * ref.NB <= o["column"]) and np.all(o["sub"] < ref.NBO // ref.NB)
        npiv = np.asarray(plan.npiv)
        assert np.all(o["column"] < npiv[o["front"]])
