"""Load-proportional ply strength index on the GPU ("ply_strength_index", femo_ply_strength_index_field,
"ply_strength_index_field") against the numpy reference tests/ply_strength_ref.py, the existing ply failure kernels, central
differences with re-solves, and the refusals.  The bars are the project's: 1e-11 of the largest entry against the reference,
1e-6 |fd| + 1e-9 max|G| against central differences, 1e-10 between grouped and separate routes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh                       # noqa: E402
from oracle.rm_shell_oracle import degree4_rule                                  # noqa: E402
from test_gpu_laminate import BETA, CLAMP, ROOT_EDGE, _mesh, block_scale, random_laminate, tight   # noqa: E402
from test_gpu_ply_failure import random_table                                    # noqa: E402
from test_layup_cpu import _plies                                                # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0])
SI, SIF = "ply_strength_index", "ply_strength_index_field"
bar = lambda g, fd, G: abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()


def _pair(m, bc=None, uhat=True, seed=0, npt=4):
    from femo_alpha_amd.backend import ShellContext
    from ply_strength_ref import PlyStrengthOracle
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (m.nn, 3))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3)) if uhat else None
    clt = random_laminate(m.nel, rng)
    tab = random_table(m.nel, rng, (npt + 1) // 2)[:, :npt]
    o = PlyStrengthOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f, uhat=uh)
    o.set_ply_table(tab, npt)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=f).items():
        c.set_field(k, v)
    if uh is not None:
        c.set_field("uhat", uh)
    if bc == "penalty":
        c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_table(np.ascontiguousarray(tab))
    return o, c, rng, clt, np.ascontiguousarray(tab)


def _close(a, r, what, per_kind=False):
    """1e-11 of the largest entry of the reference; the table gradients per entry kind, each against its own largest."""
    if per_kind:
        for k in range(16):
            assert np.abs(a[..., k] - r[..., k]).max() <= 1e-11 * np.abs(r[..., k]).max(), (what, k)
    else:
        assert a.shape == r.shape and np.abs(a - r).max() <= 1e-11 * np.abs(r).max(), what


def _check(o, c, w, rho, cells=None, alpha=None, tag=""):
    fr = o.field(w)
    fg = c.ply_strength_index_field()
    _close(fg, fr, "field")
    Kr = o.value(w, rho, alpha=alpha, cells=cells)
    K = c.functional(SI)
    print(f"{tag}: max r {fr.max():.3e}  K {K:.15e} reference {Kr:.15e}")
    assert abs(K - Kr) <= 1e-11 * np.abs(fr).max()
    gwr, gtr = o.gradients(w, rho, cells=cells)
    gw = c.dfunctional(SI, "disp_solid")
    gt = c.dfunctional(SI, "ply_table").reshape(gtr.shape)
    print(f"  dK/dw {np.abs(gw - gwr).max() / np.abs(gwr).max():.2e}  dK/dtable (per entry kind) "
          f"{max(np.abs(gt[..., k] - gtr[..., k]).max() / np.abs(gtr[..., k]).max() for k in range(16)):.2e}")
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gt))
    _close(gw, gwr, "dK/dw")
    _close(gt, gtr, "dK/dtable", per_kind=True)
    if cells is not None:
        assert not np.any(gt[np.setdiff1d(np.arange(gt.shape[0]), cells)])


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("kind", ["warped", "tri", "quad CG1CG1", "tri CG2CR1"])
def test_field_value_and_partials_against_the_reference(kind, sub):
    """uhat != 0, a random state, two plies with four recovery points; the whole mesh with the reference area, or a tagged
    sub-domain with a given alpha; 32 and 36 cells: one partial wave."""
    m = _mesh(kind)
    o, c, rng, _, tab = _pair(m)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    rho = 5.0 / o.field(w).max()
    c.set_ply_failure_params(rho)
    cells, alpha = None, None
    if sub:
        tags = (np.arange(m.nel) % 3).astype(np.int32)
        c.set_cell_tags(tags, 3)
        c.select_subdomain(1)
        alpha = 2.5
        c.set_stress_alpha(alpha, 1)
        cells = np.where(tags == 1)[0]
    _check(o, c, w, rho, cells, alpha, f"{kind} sub={sub}")
    for name in ("laminate", "thickness", "E", "nu", "density", "F_solid"):
        assert not np.any(c.dfunctional(SI, name))
    c.close()


@pytest.mark.parametrize("npt", [1, 32])
def test_two_blocks_and_a_selection_inside_the_second(npt):
    """80 cells: one full wave and a partial one.  The selection lies entirely in the second block, so the combine merges an empty
    block slot with a filled one."""
    m = plate_mesh(2.0, 10.0, 4, 20)
    assert m.nel == 80
    o, c, rng, _, tab = _pair(m, npt=npt, seed=3)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    rho = 5.0 / o.field(w).max()
    c.set_ply_failure_params(rho)
    _check(o, c, w, rho, tag=f"80 cells npt={npt}")
    tags = np.where(np.arange(m.nel) >= 66, 1, 0).astype(np.int32)
    c.set_cell_tags(tags, 2)
    c.select_subdomain(1)
    _check(o, c, w, rho, cells=np.arange(66, 80), tag=f"80 cells npt={npt}, cells 66..79")
    c.close()


def test_field_reverse_products_against_the_reference():
    for kind in ("warped", "tri"):
        m = _mesh(kind)
        o, c, rng, clt, tab = _pair(m, seed=2)
        w = 2e-3 * rng.uniform(-1, 1, m.ndof)
        c.set_state(w)
        cbar = rng.uniform(-1, 1, (3, m.nel * 4))
        gw = c.field_output_vjp(SIF, "disp_solid", cbar)
        gt = c.field_output_vjp(SIF, "ply_table", cbar).reshape(3, m.nel, 4, 16)
        for k in range(3):
            gwr, gtr = o.field_vjp(w, cbar[k])
            _close(gw[k], gwr, "field vjp, state")
            _close(gt[k], gtr, "field vjp, table", per_kind=True)
        assert np.array_equal(c.field_output_vjp(SIF, "disp_solid", cbar[1]), gw[1])
        for name in ("laminate", "thickness", "E", "nu", "density", "F_solid"):
            assert not np.any(c.field_output_vjp(SIF, name, cbar[0]))
        c.close()


def test_isotropic_ply_with_equal_strengths_gives_the_von_mises_ratio():
    """F1 = F2 = 0 and FI = (vm / X)^2: the field is vm / X at the bottom and the top of the ply."""
    from femo_alpha_amd.backend import ShellContext
    from ply_failure_ref import PlyFailureOracle
    m = wing_skin_mesh(4, 8)
    rng = np.random.default_rng(0)
    h = 0.05 * (1 + 0.3 * rng.uniform(-1, 1, m.nel))
    E, nu, X = 1e8, 0.3, 3e5
    col = lambda v: np.full((m.nel, 1), v)
    tab = lm.ply_table(col(E), col(E), col(E / 2 / (1 + nu)), col(nu), h[:, None], col(0.0), lm.tsai_wu(X, X, X, X, X / np.sqrt(3.0)))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    o = PlyFailureOracle(m, element_wise_material=True, nquad=degree4_rule(m))
    o.set_fields(h=h, E=np.full(m.nel, E), nu=np.full(m.nel, nu), rho=np.ones(m.nel), f=np.zeros((m.nn, 3)), uhat=uh)
    c = ShellContext(m, element_wise_material=True)
    for k, v in dict(thickness=h, E=[E], nu=[nu], density=[1.0], F_solid=[0.0], uhat=uh).items():
        c.set_field(k, v)
    c.set_laminate(lm.isotropic(h, E, nu))
    c.set_ply_table(tab)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    fg = c.ply_strength_index_field()
    for p, zf in ((0, -0.5), (1, 0.5)):
        ref = (o.von_mises_top(w, zf=zf)[0] / X).max(axis=1)
        assert np.abs(fg[:, p] - ref).max() <= 1e-11 * ref.max()
    c.close()


def test_the_index_predicts_the_load_at_which_the_failure_index_reaches_one():
    m = _mesh("warped")
    o, c, rng, _, tab = _pair(m)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    r = c.ply_strength_index_field()
    c.set_state(w / r.max())
    fi = c.ply_failure_field()
    print(f"max r {r.max():.6e}; at w / max r the largest failure index is 1 {fi.max() - 1.0:+.2e}")
    assert abs(fi.max() - 1.0) <= 1e-12
    assert np.unravel_index(fi.argmax(), fi.shape) == np.unravel_index(r.argmax(), r.shape)
    c.close()


def test_half_of_the_mesh_unloaded_and_the_zero_state():
    """The state vanishes on every degree of freedom of the cells 16..31: there r = 0 and D = 0, the apex of the cone, where the
    derivative is defined as zero.  Every gradient is finite and matches the reference.  w = 0: K = 0 with the reference area, and the
    gradients are exactly zero (uhat = 0: the weights add up to the reference area)."""
    m = _mesh("warped")
    o, c, rng, _, tab = _pair(m, uhat=False, seed=5)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    off = np.arange(m.nel // 2, m.nel)
    w[np.unique(o.dofs[off])] = 0.0
    c.set_state(w)
    fr = o.field(w)
    assert np.all(fr[off] == 0.0) and fr.max() > 0
    assert np.all(c.ply_strength_index_field()[off] == 0.0)
    rho = 5.0 / fr.max()
    c.set_ply_failure_params(rho)
    _check(o, c, w, rho, tag="half unloaded")
    gt = c.dfunctional(SI, "ply_table").reshape(tab.shape)
    assert not np.any(gt[off])
    cbar = rng.uniform(-1, 1, m.nel * 4)
    gw, gtab = c.field_output_vjp(SIF, "disp_solid", cbar), c.field_output_vjp(SIF, "ply_table", cbar).reshape(tab.shape)
    gwr, gtr = o.field_vjp(w, cbar)
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gtab)) and not np.any(gtab[off])
    _close(gw, gwr, "field vjp, state")
    _close(gtab, gtr, "field vjp, table", per_kind=True)
    c.set_state(np.zeros(m.ndof))
    assert abs(c.functional(SI)) <= 1e-15
    assert not np.any(c.ply_strength_index_field())
    for call in (lambda: c.dfunctional(SI, "disp_solid"), lambda: c.dfunctional(SI, "ply_table"),
                 lambda: c.field_output_vjp(SIF, "disp_solid", cbar), lambda: c.field_output_vjp(SIF, "ply_table", cbar)):
        g = call()
        assert np.all(g == 0.0)
    c.close()


def test_large_exponent_stays_finite_within_the_bounds_and_repeats_bit_for_bit():
    m = _mesh("warped")
    o, c, rng, _, tab = _pair(m, uhat=False)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    w *= 1e3 / o.field(w).max()                                           # indices of order 1e3: r is proportional to the state
    c.set_state(w)
    rho = 1e4
    c.set_ply_failure_params(rho)
    K = c.functional(SI)
    lo, hi = o.bounds(w, rho)
    print(f"rho = 1e4: max r {o.field(w).max():.3e}, K {K:.6e} in [{lo:.6e}, {hi:.6e}]")
    assert np.isfinite(K) and lo <= K <= hi
    assert abs(K - o.value(w, rho)) <= 1e-11 * abs(hi)
    cbar = rng.uniform(-1, 1, (2, m.nel * 4))
    calls = [lambda: np.array([c.functional(SI)]), lambda: c.dfunctional(SI, "disp_solid"), lambda: c.dfunctional(SI, "ply_table"),
             lambda: c.ply_strength_index_field(), lambda: c.field_output_vjp(SIF, "disp_solid", cbar),
             lambda: c.field_output_vjp(SIF, "ply_table", cbar)]
    for call in calls:
        a, b = call(), call()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    c.close()


def test_ply_failure_is_bit_identical_after_calls_of_the_new_outputs():
    m = _mesh("warped")
    o, c, rng, _, tab = _pair(m, bc="penalty")
    c.use_direct_solver()
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    old = lambda: [np.array([c.functional("ply_failure")]), c.ply_failure_field(), c.dfunctional("ply_failure", "disp_solid"),
                   c.dfunctional("ply_failure", "ply_table")]
    before = old()
    cbar = np.ones(m.nel * 4)
    K = c.functional(SI)
    c.ply_strength_index_field()
    c.dfunctional(SI, "disp_solid"); c.dfunctional(SI, "ply_table")
    c.field_output_vjp(SIF, "disp_solid", cbar)
    # the value pass of the new aggregate between the value pass and the gradient of the old one: each reads its own shift
    v0 = c.functional("ply_failure")
    assert c.functional(SI) == K
    g = c.dfunctional("ply_failure", "disp_solid")
    assert v0 == before[0][0] and np.array_equal(g, before[2])
    for a, b in zip(before, old()):
        assert np.array_equal(a, b)
    c.close()


TABLE_OF = {"ply_failure": "ply_table", "ply_shear_failure": "ply_shear_table", "ply_strength_index": "ply_table",
            "ply_hashin_fibre": "ply_table", "ply_hashin_matrix": "ply_table"}


@pytest.fixture(scope="module")
def five_criteria_context():
    """80 quadrilaterals (two blocks of 64 cells), four recovery points in every table, a random state, and a selected
    sub-domain that lies inside the second block: the first block's slot of every value pass is the empty pair."""
    from test_gpu_ply_hashin import _context
    from test_ply_hashin_cpu import case_inputs
    from test_gpu_laminate import PLY
    m = plate_mesh(2.0, 10.0, 4, 20)
    assert m.nel == 80
    inp = case_inputs(m, 11, 4)
    c = _context(m, inp)
    mat = [np.full((m.nel, 4), PLY[k]) for k in ("G13", "G23")]
    c.set_ply_shear_table(lm.ply_shear_table(*mat, inp["rng"].uniform(-90, 90, (m.nel, 4)), lm.shear_strength(3e4, 2e4)))
    c.set_state(inp["w"])
    c.set_ply_failure_params(5.0 / max(np.abs(c.ply_failure_field()).max(), c.ply_strength_index_field().max(),
                                       *(f.max() for f in c.ply_hashin_field())))
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    tags = (np.arange(m.nel) >= 68).astype(np.int32)
    c.set_cell_tags(tags, 2)
    c.select_subdomain(1)
    c.set_stress_alpha(2.5, 1)
    yield c
    c.close()


@pytest.mark.parametrize("first", list(TABLE_OF))
def test_every_criterion_is_bit_identical_after_calls_of_the_other_four(five_criteria_context, first):
    """The criteria share tables, kernels' plumbing and one table of descriptors, but each has block slots and a shift of its
    own: the value and the state gradient of one are the same bits after the value, the state gradient and the table gradient
    of every other one."""
    c = five_criteria_context
    take = lambda: (c.functional(first), c.dfunctional(first, "disp_solid"))
    v0, g0 = take()
    assert np.isfinite(v0) and np.all(np.isfinite(g0)) and np.any(g0)
    for other, table in TABLE_OF.items():
        if other != first:
            assert np.isfinite(c.functional(other))
            assert np.any(c.dfunctional(other, "disp_solid")) and np.any(c.dfunctional(other, table))
    v1, g1 = take()
    assert v1 == v0 and np.array_equal(g1, g0)
    # a value pass of every other criterion between the value pass and the gradient of this one: each reads its own shift
    v2 = c.functional(first)
    for other in TABLE_OF:
        if other != first:
            c.functional(other)
    assert v2 == v0 and np.array_equal(c.dfunctional(first, "disp_solid"), g0)


def _table_ctx(m, rng):
    """Laminate and recovery points of the same two plies, clamped, refined to the rounding floor."""
    from femo_alpha_amd.backend import ShellContext
    from test_gpu_ply_failure import _pipeline
    nply = 2
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (m.nel, nply)))
    ang = rng.uniform(-90, 90, (m.nel, nply))
    clt, tab, _, _ = _pipeline(m, t, ang, 50.0)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=rng.uniform(-1, 1, (m.nn, 3)), uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_table(tab)
    tight(c)
    return c, clt, tab


def test_total_gradients_against_central_differences_with_re_solves():
    m = _mesh("warped")
    rng = np.random.default_rng(6)
    c, clt, tab = _table_ctx(m, rng)

    def solved():
        c.solve_state(True)
        return c.functional(SI)
    solved()
    c.set_ply_failure_params(5.0 / c.ply_strength_index_field().max())        # rho r of order 5: every point contributes
    solved()
    gl = c.total_gradient(SI, "laminate")[0].reshape(m.nel, 32)
    for e, k in [(0, 0), (5, 10), (7, 13), (2, 18), (3, 22), (4, 27), (1, 31)]:
        d = clt.copy()
        s = 1e-5 * block_scale(clt, e, k)
        d[e, k] += s; c.set_laminate(d); jp = solved()
        d[e, k] -= 2 * s; c.set_laminate(d); jm = solved()
        c.set_laminate(clt)
        print(f"laminate [{e}, {k}]: {gl[e, k]:.8e} against {(jp - jm) / (2 * s):.8e}")
        assert bar(gl[e, k], (jp - jm) / (2 * s), gl), ("laminate", e, k)
    solved()
    gt = c.total_gradient(SI, "ply_table")[0].reshape(tab.shape)
    assert np.array_equal(gt, c.dfunctional(SI, "ply_table").reshape(tab.shape))      # the explicit partial alone
    # at the three recovery points with the largest index: elsewhere the aggregate moves by less than its own rounding under a
    # step small enough for a central difference (the reasoning of test_gpu_ply_failure.py)
    fld = c.ply_strength_index_field()
    top = [np.unravel_index(i, fld.shape) for i in np.argsort(fld.ravel())[::-1][:3]]
    for (e, p), k in zip(top * 4, [0, 4, 8, 9, 10, 11, 12, 13, 14, 15, 2, 6]):
        d = tab.copy()
        s = 1e-4 * np.abs(tab[:, :, k]).max()
        d[e, p, k] += s; c.set_field("ply_table", d); jp = c.functional(SI)
        d[e, p, k] -= 2 * s; c.set_field("ply_table", d); jm = c.functional(SI)
        c.set_field("ply_table", tab)
        print(f"ply_table [{e}, {p}, {k}]: {gt[e, p, k]:.8e} against {(jp - jm) / (2 * s):.8e}")
        assert bar(gt[e, p, k], (jp - jm) / (2 * s), gt[:, :, k]), ("ply_table", e, p, k)
    gf = c.total_gradient(SI, "F_solid")[0]
    f0 = c.get_field("F_solid")
    for i in (4, 31, 77):
        s = 1e-5
        x = f0.copy(); x[i] += s; c.set_field("F_solid", x); jp = solved()
        x[i] -= 2 * s; c.set_field("F_solid", x); jm = solved()
        c.set_field("F_solid", f0)
        assert bar(gf[i], (jp - jm) / (2 * s), gf), ("F_solid", i)
    for name in ("thickness", "E", "nu", "density"):
        assert not np.any(c.total_gradient(SI, name)[0])
    c.close()


def _layup_ctx(m, nply, seed=0, bc=ROOT_EDGE):
    from femo_alpha_amd.backend import ShellContext
    rng = np.random.default_rng(seed)
    pc = _plies(nply, rng)
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (m.nel, nply)))
    theta = rng.uniform(-180, 180, (m.nel, nply))
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=rng.uniform(-1, 1, (m.nn, 3)), uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(bc), BETA)
    c.set_layup(pc, t, theta, ("bot", "top"))
    return c, rng, pc, t, theta


def test_layup_totals_against_central_differences_with_re_solves():
    m = _mesh("warped")
    c, rng, pc, t, theta = _layup_ctx(m, 2, seed=3)
    tight(c)

    def solved():
        c.solve_state(True)
        return c.functional(SI)
    solved()
    c.set_ply_failure_params(5.0 / c.ply_strength_index_field().max())
    solved()
    Ga = c.total_gradient(SI, "ply_angle")[0].reshape(m.nel, 2)
    Gt = c.total_gradient(SI, "ply_thickness")[0].reshape(m.nel, 2)
    for e, j in [(5, 0), (3, 1), (8, 0), (11, 1)]:
        s = 1e-2                                                                  # degrees
        vals = []
        for sg in (1, -1):
            th = theta.copy(); th[e, j] += sg * s
            c.set_field("ply_angle", th)
            vals.append(solved())
        c.set_field("ply_angle", theta)
        print(f"angle totals [cell {e}, ply {j}]: {Ga[e, j]:.8e} against {(vals[0] - vals[1]) / (2 * s):.8e}")
        assert bar(Ga[e, j], (vals[0] - vals[1]) / (2 * s), Ga), ("ply_angle", e, j)
    for e, j in [(1, 0), (9, 1), (14, 0), (20, 1)]:
        s = 1e-4 * t[e, j]
        vals = []
        for sg in (1, -1):
            tt = t.copy(); tt[e, j] += sg * s
            c.set_field("ply_thickness", tt)
            vals.append(solved())
        c.set_field("ply_thickness", t)
        print(f"thickness totals [cell {e}, ply {j}]: {Gt[e, j]:.8e} against {(vals[0] - vals[1]) / (2 * s):.8e}")
        assert bar(Gt[e, j], (vals[0] - vals[1]) / (2 * s), Gt), ("ply_thickness", e, j)
    c.close()


def test_grouped_totals_and_the_forward_chain_agree_with_the_separate_totals():
    m = _mesh("warped")
    o, c, rng, clt, tab = _pair(m, bc="penalty")
    c.use_direct_solver()
    tags = (np.arange(m.nel) % 3).astype(np.int32)
    c.set_cell_tags(tags, 3)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / max(np.abs(c.ply_failure_field()).max(), c.ply_strength_index_field().max()))
    names, subs = ["compliance", SI, "ply_failure", SI], [-1, -1, -1, 1]
    for arg in ("laminate", "F_solid", "ply_table"):
        G = c.total_gradients(names, arg, subdomains=subs)[0]
        for i, (n, s) in enumerate(zip(names, subs)):
            c.select_subdomain(s)
            g = c.total_gradient(n, arg)[0]
            assert np.abs(G[i] - g).max() <= 1e-10 * max(np.abs(g).max(), 1e-300), (n, s, arg)
        c.select_subdomain(-1)
        assert np.abs(G[1]).max() > 0 and np.abs(G[3]).max() > 0
        scale = np.abs(clt).ravel() if arg == "laminate" else np.abs(tab).ravel() if arg == "ply_table" else 1.0
        V = rng.uniform(-1, 1, G.shape[1]) * scale
        dJ = c.total_jvp(arg, V, names, subdomains=subs, want_states=False)[1]
        for i in range(len(names)):
            assert abs(dJ[i] - G[i] @ V) <= 1e-10 * np.abs(G[i] * V).sum(), (names[i], arg)
    c.close()


def test_field_totals_with_two_cotangents_against_single_calls_and_central_differences():
    """One-signed cotangents on the largest indices and directions that move every entry the same way (every cell's laminate
    stiffer, the whole load larger), as tests/test_gpu_ply_shear.py: a mixed-sign cotangent over every entry would amplify the
    rounding of the re-solved states by the cancellation of its own sum."""
    m = _mesh("tri")
    o, c, rng, clt, tab = _pair(m, bc="penalty", seed=2)
    tight(c)

    def solved():
        c.solve_state(True)
        return c.ply_strength_index_field().ravel()
    f0 = solved()
    top = np.argsort(f0)[::-1]
    cb = np.zeros((2, f0.size))
    cb[0, top[:8]] = rng.uniform(0.5, 1.0, 8) / f0.max()
    cb[1, top[:40]] = rng.uniform(0.5, 1.0, 40) / f0.max()
    G, its, _ = c.field_total_gradients(SIF, cb, "laminate")
    assert np.all(its > 0)
    for k in range(2):
        g1 = c.field_total_gradients(SIF, cb[k], "laminate")[0][0]
        assert np.abs(G[k] - g1).max() <= 1e-10 * np.abs(g1).max()
    d = clt * rng.uniform(0.5, 1.5, (m.nel, 1))
    s = 1e-4
    c.set_laminate(clt + s * d); fp = solved()
    c.set_laminate(clt - s * d); fm = solved()
    c.set_laminate(clt)
    solved()
    for k in range(2):
        fd, g = cb[k] @ (fp - fm) / (2 * s), G[k] @ d.ravel()
        print(f"field totals, laminate direction, cotangent {k}: {g:.10e} against {fd:.10e}: {abs(g - fd) / abs(fd):.1e} of it")
        assert bar(g, fd, G[k] * d.ravel())
    Gf = c.field_total_gradients(SIF, cb, "F_solid")[0]
    F0 = c.get_field("F_solid")
    df = F0 * rng.uniform(0.5, 1.5, F0.size)
    c.set_field("F_solid", F0 + s * df); fp = solved()
    c.set_field("F_solid", F0 - s * df); fm = solved()
    c.set_field("F_solid", F0)
    solved()
    for k in range(2):
        fd, g = cb[k] @ (fp - fm) / (2 * s), Gf[k] @ df
        print(f"field totals, load direction, cotangent {k}: {g:.10e} against {fd:.10e}: {abs(g - fd) / abs(fd):.1e} of it")
        assert bar(g, fd, Gf[k] * df)
    Gs, its, rr = c.field_total_gradients(SIF, cb, "ply_table")
    assert not np.any(its) and np.array_equal(Gs, c.field_output_vjp(SIF, "ply_table", cb))
    c.close()


def test_field_totals_reach_the_layup_and_group_four_to_a_solve():
    m = _mesh("warped")
    c, rng, pc, t, theta = _layup_ctx(m, 2, seed=4)
    c.use_direct_solver()
    c.solve_state(True)
    f0 = c.ply_strength_index_field().ravel()
    cb = rng.uniform(0.0, 1.0, (5, f0.size)) / f0.max()
    for arg in ("ply_thickness", "ply_angle"):
        G = c.field_total_gradients(SIF, cb, arg)[0]
        for k in (0, 4):
            g1 = c.field_total_gradients(SIF, cb[k], arg)[0][0]
            assert np.abs(g1).max() > 0 and np.abs(G[k] - g1).max() <= 1e-10 * np.abs(g1).max(), (arg, k)
    c.close()


def test_refusals_and_the_check_of_the_table():
    from femo_alpha_amd._lib import FemoHipError, dptr
    from femo_alpha_amd.backend import ShellContext
    m = plate_mesh(2.0, 10.0, 4, 20)
    rng = np.random.default_rng(4)
    clt, tab = random_laminate(m.nel, rng), random_table(m.nel, rng)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.use_direct_solver()
    c.set_laminate(clt)
    cb = np.ones(m.nel * 4)
    for call in (lambda: c.functional(SI), lambda: c.dfunctional(SI, "disp_solid"), lambda: c.ply_strength_index_field(),
                 lambda: c.total_gradient(SI, "laminate"), lambda: c.total_gradients(["compliance", SI], "laminate"),
                 lambda: c.total_jvp("laminate", clt.ravel(), [SI]), lambda: c.field_output_vjp(SIF, "disp_solid", cb),
                 lambda: c.field_total_gradients(SIF, cb, "laminate")):
        with pytest.raises(FemoHipError, match="femo_set_ply_table"):
            call()
    c.solve_state(True)
    c.set_ply_table(tab)
    assert c.field_size_of(SIF) == m.nel * 4
    K, fld = c.functional(SI), c.ply_strength_index_field()
    assert np.isfinite(K) and fld.shape == (m.nel, 4)
    for call in (lambda: c.dfunctional(SI, "uhat"), lambda: c.total_gradient(SI, "uhat"),
                 lambda: c.total_gradients(["compliance", SI], "uhat"), lambda: c.total_jvp("uhat", np.ones(3 * m.nn), [SI]),
                 lambda: c.field_output_vjp(SIF, "uhat", cb), lambda: c.field_total_gradients(SIF, cb, "uhat"),
                 lambda: c.field_output_jvp(SIF, "disp_solid", np.ones(m.ndof)),
                 lambda: c.field_total_jvp([SIF], "laminate", clt.ravel()),
                 lambda: c.field_output_jacobian(SIF, "disp_solid")):
        with pytest.raises(FemoHipError, match="not provided"):
            call()
    out5 = np.empty(5)
    assert c.lib.femo_ply_strength_index_field(c._h, dptr(out5), 5) != 0 and b"nel * npt entries" in c.lib.femo_last_error(c._h)
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_dfunctional(c._h, SI.encode(), b"ply_table", dptr(out5), 5))
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_field_output_vjp(c._h, SIF.encode(), b"ply_table", dptr(cb), 1, dptr(out5), 5))
    with pytest.raises(ValueError, match="wrong length"):
        c.field_output_vjp(SIF, "disp_solid", cb[:-1])
    assert c.functional(SI) == K and np.array_equal(c.ply_strength_index_field(), fld)
    # f12 = +-1 makes the quadratic form singular: F12^2 = F11 F22 up to the rounding the slack covers
    for f12 in (1.0, -1.0):
        t2 = tab.copy()
        t2[:, :, 15] = f12 * np.sqrt(t2[:, :, 12] * t2[:, :, 13])
        c.set_ply_table(t2)
        assert np.isfinite(c.functional(SI))
    # an indefinite form: refused with the cell and the point, by every entry point; ply_failure still answers
    bad = tab.copy()
    bad[7, 2, 15] = -1.001 * np.sqrt(bad[7, 2, 12] * bad[7, 2, 13])
    bad[9, 1, 14] = -bad[9, 1, 14]
    c.set_ply_table(bad)
    for call in (lambda: c.functional(SI), lambda: c.ply_strength_index_field(), lambda: c.dfunctional(SI, "ply_table"),
                 lambda: c.total_gradient(SI, "laminate"), lambda: c.field_output_vjp(SIF, "disp_solid", cb)):
        with pytest.raises(FemoHipError, match="recovery point 2 of cell 7"):
            call()
    assert np.isfinite(c.functional("ply_failure")) and np.all(np.isfinite(c.ply_failure_field()))
    assert np.all(np.isfinite(c.dfunctional("ply_failure", "disp_solid")))
    c.set_ply_table(tab)
    assert c.functional(SI) == K
    c.close()


@pytest.mark.parametrize("renumber", [False, True])
def test_through_the_model_with_a_layup_matches_the_backend_totals(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.fea.fea_hip import computeMatVecProductBwd, computePartials
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel, nply = mesh.nn, mesh.nel, 2
    rng = np.random.default_rng(8)
    pc = _plies(nply, rng)
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    theta = rng.uniform(-180, 180, (nel, nply))
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    pressure = csdl.Variable(value=np.tile([0.5, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=0.05 * np.ones(nn), name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=np.ones(nn), name="density")
    node_disp = csdl.Variable(value=np.zeros((nn, 3)), name="node_disp")
    ply_t = csdl.Variable(value=t, name="ply_thickness")
    ply_a = csdl.Variable(value=theta, name="ply_angle")
    layup = dict(plies=pc, t=t[0], theta=theta[0], surfaces=("bot", "top"))
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, rho=20, layup=layup,
                         ply_strength=True)
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    ctx = model.shell_pde.ctx
    npt = 2 * nply
    print(f"model: max index {ctx.ply_strength_index_field().max():.3e}, K {ctx.functional(SI):.6e}")      # of order one under this load
    assert model.fea.outputs_dict[SI]["arguments"] == model.fea.outputs_dict["ply_failure"]["arguments"]
    for var, arg in ((ply_t, "ply_thickness"), (ply_a, "ply_angle")):
        got = np.asarray(recorder.compute_totals(out.ply_strength_index, var)).reshape(nel, nply)
        ref = np.empty((nel, nply))
        ref[model.cell_of_new] = ctx.total_gradient(SI, arg)[0].reshape(nel, nply)        # solver order -> caller order
        assert np.abs(ref).max() > 0 and np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), arg
    fea = model.fea
    cb = rng.uniform(0.0, 1.0, (2, nel * npt))                                       # caller order
    cbs = cb.reshape(2, nel, npt)[:, model.cell_of_new].reshape(2, -1)               # the backend's own order
    for arg in ("ply_angle", "ply_thickness"):
        got = fea.field_gradients(SIF, cb, arg)
        g = ctx.field_total_gradients(SIF, cbs, arg)[0].reshape(2, nel, nply)
        want = np.empty_like(g)
        want[:, model.cell_of_new] = g
        assert got.shape == (2, nel * nply) and np.abs(got - want.reshape(2, -1)).max() <= 1e-10 * np.abs(want).max(), arg
    form = model.ply_strength_index_field_form
    for role in ("disp_solid", "ply_angle"):
        func = fea.states_dict[role]["function"] if role == "disp_solid" else fea.inputs_dict[role]["function"]
        assert np.array_equal(computeMatVecProductBwd(computePartials(form, func), cbs[0]), ctx.field_output_vjp(SIF, role, cbs[0]))
    # opt-in: a model built without the option is unchanged, and the option needs a ply table
    model2 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, layup=layup)
    assert SI not in model2.fea.outputs_dict and not hasattr(model2, "ply_strength_index_field_form")
    with pytest.raises(ValueError, match="ply_strength"):
        RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, ply_strength=True)
    model3 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, ply_failure=4, ply_strength=True)
    assert model3.fea.outputs_dict[SI]["arguments"] == ["disp_solid", "ply_table"]
