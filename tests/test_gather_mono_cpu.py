"""The "increasing" flag of the extend-add gathers (option "gather_mono"): per front, whether the boundary rows of its left / right
child land in strictly increasing rows.  The rule in host C++ (femo_child_maps_increasing, csrc/child_maps.h -- what
femo_set_frontal_plan uploads) against its numpy statement (solver.symbolic.child_maps_increasing), and what the two node orders of
the plan give: every front increasing with node_order 1 (also behind the tail-delay pass), both kinds with node_order 0, so that
both paths of the gathering kernels can be tested at small size."""
import numpy as np
import pytest

from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh
from femo_alpha_amd.solver import symbolic

CASES = {
    "plate8": (lambda: plate_mesh(2.0, 5.0, 8, 8), 4),
    "plate16": (lambda: plate_mesh(2.0, 5.0, 16, 16), 4),
    "wing": (lambda: wing_skin_mesh(32, 96, shuffle=True).renumbered()[0], 8),
}


def _by_hand(plan):
    """bit 0 / 1 of front p: cleared when the left / right child's rows in p do not rise (written out entry by entry)."""
    flags = [3] * plan.ntree
    for t in range(plan.ntree):
        p = int(plan.parent[t])
        if p < 0:
            continue
        rows = [int(x) for x in plan.up_map[plan.dof_off[t] + plan.npiv[t]:plan.dof_off[t + 1]]]
        if any(b <= a for a, b in zip(rows, rows[1:])):
            flags[p] &= ~(1 if int(plan.left[p]) == t else 2)
    return np.array(flags, dtype=np.int32)


@pytest.mark.parametrize("tail_max", [0, 32])
@pytest.mark.parametrize("node_order", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_native_flags_equal_the_numpy_flags(name, node_order, tail_max):
    make, leaf = CASES[name]
    plan = symbolic.build_plan(make(), leaf, node_order=node_order, tail_max=tail_max)
    a = symbolic.child_maps_increasing(plan)
    b = symbolic.child_maps_increasing(plan, impl="python")
    assert a.dtype == np.int32 and a.shape == (plan.ntree,)
    assert np.array_equal(a, b) and np.array_equal(a, _by_hand(plan))
    assert np.all(a[plan.left < 0] == 3)                             # leaves: no children, nothing to order
    if node_order == 1:
        assert np.all(a == 3)                                        # every front takes the per-column gather
    else:
        inner = a[plan.left >= 0]
        bits = np.concatenate([inner & 1, (inner >> 1) & 1])         # one per (front, child)
        assert bits.min() == 0 and bits.max() == 1                   # both values occur in one plan


def test_one_child_out_of_order_clears_only_its_own_bit():
    plan = symbolic.build_plan(plate_mesh(2.0, 5.0, 8, 8), 4, node_order=1)
    p = int(np.nonzero(plan.left >= 0)[0][-1])
    for side, child in ((1, int(plan.left[p])), (2, int(plan.right[p]))):
        lo, hi = int(plan.dof_off[child] + plan.npiv[child]), int(plan.dof_off[child + 1])
        assert hi - lo >= 2
        up = plan.up_map.copy()
        up[lo], up[lo + 1] = up[lo + 1], up[lo]
        broken = symbolic.FrontalPlan()
        broken.__dict__.update(plan.__dict__)
        broken.up_map = up
        for impl in ("native", "python"):
            f = symbolic.child_maps_increasing(broken, impl=impl)
            assert f[p] == 3 & ~side and np.all(np.delete(f, p) == 3), (side, impl)
