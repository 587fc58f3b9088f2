"""Option "gather_mono": on fronts whose two children land in increasing rows the gathering kernels (k_extend_gather,
k_trailing_mfma<true>, k_trailing_fine<true>) address the children per column instead of ordering every pair of child rows.  The operands
and the order of the sums are the same, so the factor is the same BIT FOR BIT: after a factorisation the Schur block of every front with
boundary rows is compared between gather_mono 1 and 0 -- under the default schedule, with every level forced onto the right-looking
super-panel schedule (a gathering first update, then plain ones) and with the narrow updates forced onto the fine kernel; with a
node_order 0 plan, whose fronts are not increasing and fall back to the general gather; and the solution and gradient agree with the
plainest schedule as in tests/test_gpu_schedules.py.

Meshes: the 16 x 16 plate at leaf 4 (4134 DOF, 7 levels, fronts of up to 222 rows: tiles on and off the diagonal, fronts of more than
one outer panel: a gathering first update and later panels) and the 32 x 96 wing skin with strong DOFs (the masked unit diagonal)."""
import numpy as np
import pytest

from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh

pytestmark = pytest.mark.gpu

SCHEDULES = {
    "default": {},
    "right_super": dict(trailing=2, super_panel=512, super_panel_cnt=100000),
    "fine": dict(narrow_fine_wg=100000),
}
PLAIN = dict(super_panel=0, fused_schur=0, lookahead=0)


def _problem(case):
    if case == "plate":
        return plate_mesh(2.0, 5.0, 16, 16), (lambda x: np.less(x[0], 3e-16)), False, 4
    return wing_skin_mesh(32, 96, shuffle=True).renumbered()[0], (lambda x: np.less(x[1], 1e-9)), True, 8


_plans = {}


def _plan(case, node_order):
    from femo_alpha_amd.solver.symbolic import TAIL_MAX, build_plan
    if (case, node_order) not in _plans:
        m, _, _, leaf = _problem(case)
        _plans[case, node_order] = build_plan(m, leaf, node_order=node_order, tail_max=TAIL_MAX)
    return _plans[case, node_order]


def _context(case, node_order, options):
    from femo_alpha_amd.backend import ShellContext
    m, marker, strong, _ = _problem(case)
    c = ShellContext(m)
    r = np.random.default_rng(1)
    c.set_field("thickness", 0.02 * (1 + 0.3 * r.uniform(-1, 1, m.nn)))
    for k, v in (("E", [7e10]), ("nu", [0.3]), ("density", [2700.0])):
        c.set_field(k, v)
    c.set_field("F_solid", r.uniform(-1, 1, (m.nn, 3)))
    if strong:
        c.set_strong_dofs(m.locate_dofs_geometrical(marker))
    else:
        c.set_penalty_facets(m.penalty_facets(marker))
    for k, v in options.items():
        c.set_option(k, v)
    c.enable_frontal(plan=_plan(case, node_order))
    c.set_solver(preconditioner=2, rtol=1e-12, maxit=30, check_every=1)
    return c


def _schur_blocks(c, plan):
    """The packed Schur blocks of all fronts with boundary rows after one factorisation, in one tensor, and where each starts."""
    import torch
    nb = (plan.nf - plan.npiv).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(nb * (nb + 1) // 2)])
    buf = torch.zeros(int(off[-1]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    c.factorize()
    for t in np.nonzero(nb)[0]:
        c.front_schur_pack(int(t), buf[int(off[t]):int(off[t + 1])])
    c.sync()
    return buf, off


def _assert_same_blocks(case, node_order, schedule):
    import torch
    plan = _plan(case, node_order)
    out = {}
    for gm in (1, 0):
        # assemble_fc 2: every leaf front filled by one workgroup in a fixed order.  The element-wise assembly (the default below 20
        # points per cell) adds with float atomics, and two factorisations of one context already differ in the last place
        c = _context(case, node_order, dict(SCHEDULES[schedule], gather_mono=gm, assemble_fc=2))
        try:
            out[gm] = _schur_blocks(c, plan)
        finally:
            c.close()
    (a, off), (b, _) = out[1], out[0]
    assert int(off[-1]) > 0 and bool(torch.isfinite(a).all()) and int(torch.count_nonzero(a)) > int(off[-1]) // 2
    if not torch.equal(a, b):
        bad = [int(t) for t in range(plan.ntree) if not torch.equal(a[int(off[t]):int(off[t + 1])], b[int(off[t]):int(off[t + 1])])]
        raise AssertionError(f"{case} node_order {node_order} {schedule}: Schur blocks of fronts {bad[:20]} differ ({len(bad)} of {plan.ntree})")


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("case", ["plate", "wing_strong"])
def test_factor_is_bit_identical_with_and_without_the_per_column_gather(case, schedule):
    from femo_alpha_amd.solver.symbolic import child_maps_increasing
    plan = _plan(case, 1)
    assert np.all(child_maps_increasing(plan) == 3)                     # every front takes the new path
    if case == "plate":
        assert plan.nlevels == 7 and int(plan.nf.max()) > 128 and int(plan.npiv.max()) > 128
    _assert_same_blocks(case, 1, schedule)


@pytest.mark.parametrize("case", ["plate", "wing_strong"])
def test_fronts_that_are_not_increasing_fall_back_to_the_general_gather(case):
    from femo_alpha_amd.solver.symbolic import child_maps_increasing
    flags = child_maps_increasing(_plan(case, 0))
    assert np.any(flags != 3)
    _assert_same_blocks(case, 0, "default")


_plain = {}


def _solve(case, node_order, options):
    c = _context(case, node_order, options)
    try:
        c.factorize(); c.factorize()
        c.set_field("thickness", c.get_field("thickness"))            # the solve factorises once more, from cold
        it, _ = c.solve_state(True)
        w = c.get_state()
        g, _, _ = c.total_gradient("compliance", "thickness")
    finally:
        c.close()
    return it, w, g


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("case", ["plate", "wing_strong"])
def test_solution_and_gradient_agree_with_the_plain_schedule(case, schedule):
    if case not in _plain:
        _plain[case] = _solve(case, 1, dict(PLAIN, gather_mono=0))
    it0, w0, g0 = _plain[case]
    it, w, g = _solve(case, 1, dict(SCHEDULES[schedule], gather_mono=1))
    assert it <= it0 + 1
    assert np.abs(w - w0).max() < 1e-9 * np.abs(w0).max()
    assert np.abs(g - g0).max() < 1e-8 * np.abs(g0).max()
