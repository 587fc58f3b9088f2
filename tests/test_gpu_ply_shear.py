"""Interlaminar shear failure aggregate and field on the GPU (femo_set_ply_shear_table, "ply_shear_failure",
femo_ply_shear_failure_field, "ply_shear_failure_field", femo_set_layup_shear_strength) against the numpy reference
tests/ply_shear_ref.py, the closed form of the clamped strip, central differences with re-solves, the host step of
femo_alpha_amd/laminate.py, and the handling of the table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh                                       # noqa: E402
from oracle.rm_shell_oracle import degree4_rule                                  # noqa: E402
from test_gpu_laminate import BETA, CLAMP, PLY, ROOT_EDGE, _mesh, block_scale, random_laminate, tight   # noqa: E402
from test_layup_cpu import _plies                                                # noqa: E402
from test_ply_shear_cpu import random_shear_table, strip                         # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0])
bar = lambda g, fd, G: abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()


def _pair(m, bc=None, uhat=True, seed=0, npt=3):
    from femo_alpha_amd.backend import ShellContext
    from ply_shear_ref import PlyShearOracle
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (m.nn, 3))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3)) if uhat else None
    clt = random_laminate(m.nel, rng)
    tab = random_shear_table(m.nel, npt, rng)
    o = PlyShearOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f, uhat=uh)
    o.set_ply_shear_table(tab, npt)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=f).items():
        c.set_field(k, v)
    if uh is not None:
        c.set_field("uhat", uh)
    if bc == "penalty":
        c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_shear_table(tab)
    return o, c, rng, clt, tab


def _check(o, c, w, rho, cells=None, alpha=None, tag=""):
    """Field, value, state and table gradients of the context against the reference: 1e-11 of the largest entry, each of the six
    entry kinds of the table against its own largest, K against the largest index."""
    fr = o.field(w)
    fg = c.ply_shear_failure_field()
    assert fg.shape == fr.shape and np.abs(fg - fr).max() <= 1e-11 * np.abs(fr).max()
    Kr = o.value(w, rho, alpha=alpha, cells=cells)
    K = c.functional("ply_shear_failure")
    print(f"{tag}: max FI {fr.max():.3e}  K {K:.15e} reference {Kr:.15e}")
    assert abs(K - Kr) <= 1e-11 * np.abs(fr).max()
    gwr, gtr = o.gradients(w, rho, cells=cells)
    gw = c.dfunctional("ply_shear_failure", "disp_solid")
    gt = c.dfunctional("ply_shear_failure", "ply_shear_table").reshape(gtr.shape)
    print(f"  dK/dw {np.abs(gw - gwr).max() / np.abs(gwr).max():.2e}  dK/dtable (per entry kind) "
          f"{max(np.abs(gt[..., k] - gtr[..., k]).max() / np.abs(gtr[..., k]).max() for k in range(6)):.2e}")
    assert np.abs(gw - gwr).max() <= 1e-11 * np.abs(gwr).max()
    for k in range(6):
        assert np.abs(gt[..., k] - gtr[..., k]).max() <= 1e-11 * np.abs(gtr[..., k]).max(), k
    if cells is not None:
        assert not np.any(gt[np.setdiff1d(np.arange(gt.shape[0]), cells)])


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("kind", ["warped", "tri", "quad CG1CG1", "tri CG2CR1"])
def test_field_value_and_partials_against_the_reference(kind, sub):
    """uhat != 0, a random state, general 2 x 2 Gs, npt_s = 3; whole mesh with the reference area, or a tagged sub-domain with a given
    alpha; 32 and 36 cells: one partial wave."""
    m = _mesh(kind)
    o, c, rng, _, tab = _pair(m)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    rho = 5.0 / o.field(w).max()
    c.set_ply_shear_params(rho)
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
        assert not np.any(c.dfunctional("ply_shear_failure", name))
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
    c.set_ply_shear_params(rho)
    _check(o, c, w, rho, tag=f"80 cells npt={npt}")
    tags = np.where(np.arange(m.nel) >= 66, 1, 0).astype(np.int32)
    c.set_cell_tags(tags, 2)
    c.select_subdomain(1)
    _check(o, c, w, rho, cells=np.arange(66, 80), tag=f"80 cells npt={npt}, cells 66..79")
    c.close()


def test_large_exponent_stays_finite_within_the_bounds_and_repeats_bit_for_bit():
    m = _mesh("warped")
    o, c, rng, _, tab = _pair(m, uhat=False)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    tab = tab.copy(); tab[:, :, 4:6] *= 1e3 / o.field(w).max()          # failure indices of order 1e3
    c.set_field("ply_shear_table", tab)
    o.set_ply_shear_table(tab, 3)
    rho = 1e4
    c.set_ply_shear_params(rho)
    K = c.functional("ply_shear_failure")
    lo, hi = o.bounds(w, rho)
    print(f"rho = 1e4: max FI {o.field(w).max():.3e}, K {K:.6e} in [{lo:.6e}, {hi:.6e}]")
    assert np.isfinite(K) and lo <= K <= hi
    assert abs(K - o.value(w, rho)) <= 1e-11 * abs(hi)
    cbar = rng.uniform(-1, 1, (2, m.nel * 3))
    calls = [lambda: np.array([c.functional("ply_shear_failure")]), lambda: c.dfunctional("ply_shear_failure", "disp_solid"),
             lambda: c.dfunctional("ply_shear_failure", "ply_shear_table"), lambda: c.ply_shear_failure_field(),
             lambda: c.field_output_vjp("ply_shear_failure_field", "disp_solid", cbar),
             lambda: c.field_output_vjp("ply_shear_failure_field", "ply_shear_table", cbar)]
    for call in calls:
        a, b = call(), call()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    c.set_state(np.zeros(m.ndof))                                         # w = 0: K = 0
    assert abs(c.functional("ply_shear_failure")) <= 1e-15
    c.close()


def _layup_ctx(m, nply, seed=0, equal=False, bc=ROOT_EDGE):
    """A context in layup mode with shear strengths; ``equal``: G13 = G23 and S13 = S23 in every ply."""
    from femo_alpha_amd.backend import ShellContext
    rng = np.random.default_rng(seed)
    pc = _plies(nply, rng)
    S = 5e4 * (1 + 0.3 * rng.uniform(0, 1, (nply, 2)))
    if equal:
        pc[:, 5] = pc[:, 4]
        S[:, 1] = S[:, 0]
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (m.nel, nply)))
    theta = rng.uniform(-180, 180, (m.nel, nply))
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=rng.uniform(-1, 1, (m.nn, 3)), uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(bc), BETA)
    c.set_layup(pc, t, theta, ("bot", "top"), shear_strength=S)
    return c, rng, pc, S, t, theta


def test_equal_moduli_and_strengths_make_the_field_independent_of_the_ply_angles():
    m = _mesh("warped")
    c, rng, pc, S, t, theta = _layup_ctx(m, 3, equal=True)
    c.set_state(2e-3 * rng.uniform(-1, 1, m.ndof))
    f1 = c.ply_shear_failure_field()
    c.set_field("ply_angle", rng.uniform(-180, 180, theta.shape))
    f2 = c.ply_shear_failure_field()
    assert f1.shape == (m.nel, 3) and f1.max() > 0
    assert np.abs(f2 - f1).max() <= 1e-13 * f1.max()
    c.close()


def test_strip_field_against_the_closed_form():
    """The strip of tests/test_ply_shear_cpu.py solved on the device, refined to the rounding floor: the CPU reference sits at 5e-12 of
    the closed form, the bar here is the project's 1e-8."""
    from femo_alpha_amd.backend import ShellContext
    m, clt, tab, closed, far = strip(2, 20)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=np.tile([0.0, 0.0, 1.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.set_laminate(clt)
    c.set_ply_shear_table(tab)
    tight(c)
    c.solve_state(True)
    fld = c.ply_shear_failure_field()
    err = np.abs(fld[far] - closed[far]).max() / np.abs(closed[far]).max()
    print(f"strip 2 x 20, ply t = 0.1: device field against the closed form over 3 <= x <= 7: {err:.2e}")
    assert err <= 1e-8
    c.close()


def test_total_gradients_against_central_differences_with_re_solves():
    from femo_alpha_amd.backend import ShellContext
    m = _mesh("warped")
    rng = np.random.default_rng(6)
    nply = 3
    clt = random_laminate(m.nel, rng)
    tab = lm.ply_shear_table(PLY["G13"], PLY["G23"], rng.uniform(-90, 90, (m.nel, nply)), lm.shear_strength(6e4, 4e4))
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=rng.uniform(-1, 1, (m.nn, 3)), uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_shear_table(tab)
    tight(c)

    def solved():
        c.solve_state(True)
        return c.functional("ply_shear_failure")
    solved()
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())            # rho FI of order 5: every point contributes
    solved()
    gl = c.total_gradient("ply_shear_failure", "laminate")[0].reshape(m.nel, 32)
    for e, k in [(0, 0), (5, 10), (2, 18), (4, 27), (6, 28), (9, 29), (12, 30), (1, 31)]:
        d = clt.copy()
        s = 1e-5 * block_scale(clt, e, k)
        d[e, k] += s; c.set_laminate(d); jp = solved()
        d[e, k] -= 2 * s; c.set_laminate(d); jm = solved()
        c.set_laminate(clt)
        print(f"laminate [{e}, {k}]: {gl[e, k]:.8e} against {(jp - jm) / (2 * s):.8e}")
        assert bar(gl[e, k], (jp - jm) / (2 * s), gl), ("laminate", e, k)
    solved()
    gt = c.total_gradient("ply_shear_failure", "ply_shear_table")[0].reshape(tab.shape)
    assert np.array_equal(gt, c.dfunctional("ply_shear_failure", "ply_shear_table").reshape(tab.shape))      # the explicit partial alone
    fld = c.ply_shear_failure_field()
    top = [np.unravel_index(i, fld.shape) for i in np.argsort(fld.ravel())[::-1][:3]]
    for (e, p), k in zip(top * 2, range(6)):
        d = tab.copy()
        s = 1e-4 * np.abs(tab[:, :, k]).max()
        d[e, p, k] += s; c.set_field("ply_shear_table", d); jp = c.functional("ply_shear_failure")
        d[e, p, k] -= 2 * s; c.set_field("ply_shear_table", d); jm = c.functional("ply_shear_failure")
        c.set_field("ply_shear_table", tab)
        assert bar(gt[e, p, k], (jp - jm) / (2 * s), gt[:, :, k]), ("ply_shear_table", e, p, k)
    gf = c.total_gradient("ply_shear_failure", "F_solid")[0]
    f0 = c.get_field("F_solid")
    for i in (4, 31, 77):
        s = 1e-5
        x = f0.copy(); x[i] += s; c.set_field("F_solid", x); jp = solved()
        x[i] -= 2 * s; c.set_field("F_solid", x); jm = solved()
        c.set_field("F_solid", f0)
        assert bar(gf[i], (jp - jm) / (2 * s), gf), ("F_solid", i)
    for name in ("thickness", "E", "nu", "density"):
        assert not np.any(c.total_gradient("ply_shear_failure", name)[0])
    c.close()


def test_layup_totals_against_central_differences_with_re_solves():
    m = _mesh("warped")
    c, rng, pc, S, t, theta = _layup_ctx(m, 2, seed=3)
    tight(c)

    def solved():
        c.solve_state(True)
        return c.functional("ply_shear_failure")
    solved()
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    solved()
    Ga = c.total_gradient("ply_shear_failure", "ply_angle")[0].reshape(m.nel, 2)
    Gt = c.total_gradient("ply_shear_failure", "ply_thickness")[0].reshape(m.nel, 2)
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
    from test_gpu_ply_failure import random_table
    m = _mesh("warped")
    o, c, rng, clt, tab = _pair(m, bc="penalty")
    c.set_ply_table(random_table(m.nel, rng))
    c.use_direct_solver()
    tags = (np.arange(m.nel) % 3).astype(np.int32)
    c.set_cell_tags(tags, 3)
    c.solve_state(True)
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    # with a ply table set: the in-plane table is an argument of the shear output with exact zeros, partial and total
    assert not np.any(c.dfunctional("ply_shear_failure", "ply_table")) and not np.any(c.total_gradient("ply_shear_failure", "ply_table")[0])
    names, subs = ["compliance", "ply_shear_failure", "ply_failure", "ply_shear_failure"], [-1, -1, -1, 1]
    for arg in ("laminate", "F_solid", "ply_shear_table"):
        G = c.total_gradients(names, arg, subdomains=subs)[0]
        for i, (n, s) in enumerate(zip(names, subs)):
            c.select_subdomain(s)
            g = c.total_gradient(n, arg)[0]
            assert np.abs(G[i] - g).max() <= 1e-10 * max(np.abs(g).max(), 1e-300), (n, s, arg)
        c.select_subdomain(-1)
        if arg == "ply_shear_table":                       # every other output: exact zeros
            assert not np.any(G[0]) and not np.any(G[2])
        V = rng.uniform(-1, 1, G.shape[1]) * (np.abs(clt).ravel() if arg == "laminate" else 1.0)
        dJ = c.total_jvp(arg, V, names, subdomains=subs, want_states=False)[1]
        for i in range(len(names)):
            assert abs(dJ[i] - G[i] @ V) <= 1e-10 * np.abs(G[i] * V).sum(), (names[i], arg)
    c.close()


def test_field_reverse_mode_against_the_reference_and_central_differences():
    m = _mesh("tri")
    o, c, rng, clt, tab = _pair(m, bc="penalty", seed=2)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    cbar = rng.uniform(-1, 1, (3, m.nel * 3))
    gw = c.field_output_vjp("ply_shear_failure_field", "disp_solid", cbar)
    gt = c.field_output_vjp("ply_shear_failure_field", "ply_shear_table", cbar).reshape(3, m.nel, 3, 6)
    for k in range(3):
        gwr, gtr = o.field_vjp(w, cbar[k])
        assert np.abs(gw[k] - gwr).max() <= 1e-11 * np.abs(gwr).max()
        for j in range(6):
            assert np.abs(gt[k, ..., j] - gtr[..., j]).max() <= 1e-11 * np.abs(gtr[..., j]).max(), (k, j)
    assert np.array_equal(c.field_output_vjp("ply_shear_failure_field", "disp_solid", cbar[1]), gw[1])
    for name in ("laminate", "thickness", "E", "nu", "density", "F_solid"):
        assert not np.any(c.field_output_vjp("ply_shear_failure_field", name, cbar[0]))
    # totals: cbar . (field(x + eps d) - field(x - eps d)) / 2 eps with re-solves against field_total_gradients . d.  The check is
    # kept well conditioned: a re-solved state carries ~1e-7 of rounding noise in a difference quotient of the field (penalty 1e10,
    # cancellation inside the shear strains), which a mixed-sign cotangent over every entry amplifies by the cancellation of its own
    # sum (22 x here: the bar would sit inside the noise).  So the cotangents are one-signed weights on the largest indices, as the
    # scalar totals use, and the directions move every entry the same way: every cell's laminate stiffer (the indices fall like
    # (1 + s d)^-2: 2 (s d)^2 < 5e-8 of truncation) and the whole load larger (the indices are quadratic in it: no truncation).
    tight(c)

    def solved():
        c.solve_state(True)
        return c.ply_shear_failure_field().ravel()
    f0 = solved()
    top = np.argsort(f0)[::-1]
    cb = np.zeros((2, f0.size))
    cb[0, top[:8]] = rng.uniform(0.5, 1.0, 8) / f0.max()
    cb[1, top[:40]] = rng.uniform(0.5, 1.0, 40) / f0.max()
    G, its, _ = c.field_total_gradients("ply_shear_failure_field", cb, "laminate")
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
    Gf = c.field_total_gradients("ply_shear_failure_field", cb, "F_solid")[0]
    F0 = c.get_field("F_solid")
    df = F0 * rng.uniform(0.5, 1.5, F0.size)
    c.set_field("F_solid", F0 + s * df); fp = solved()
    c.set_field("F_solid", F0 - s * df); fm = solved()
    c.set_field("F_solid", F0)
    for k in range(2):
        fd, g = cb[k] @ (fp - fm) / (2 * s), Gf[k] @ df
        print(f"field totals, load direction, cotangent {k}: {g:.10e} against {fd:.10e}: {abs(g - fd) / abs(fd):.1e} of it")
        assert bar(g, fd, Gf[k] * df)
    Gs, its, rr = c.field_total_gradients("ply_shear_failure_field", cb, "ply_shear_table")
    assert not np.any(its) and np.array_equal(Gs, c.field_output_vjp("ply_shear_failure_field", "ply_shear_table", cb))
    c.close()


def test_what_repeats_bit_for_bit_on_a_clamped_layup_and_what_repeats_to_the_solver_tolerance():
    """Clamped, solved, in layup mode.  The kernels of these outputs use no float atomics: the value, the field, every partial (the
    layup names included) and the field's reverse products return the same bits when called twice.  The totals go through the adjoint
    solve, whose dot products add block sums with a float atomic (k_dot), and total_jvp contracts with the same k_dot: they are
    compared at 1e-10 of the largest entry, the bar of the derivative routes, and whether they happened to repeat is printed."""
    m = _mesh("warped")
    c, rng, pc, S, t, theta = _layup_ctx(m, 3, seed=7)
    c.use_direct_solver()
    c.solve_state(True)
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    SF, SFF = "ply_shear_failure", "ply_shear_failure_field"
    cbar = rng.uniform(-1, 1, (2, m.nel * 3))
    exact = [lambda: np.array([c.functional(SF)]), lambda: c.ply_shear_failure_field()]
    exact += [lambda a=a: c.dfunctional(SF, a) for a in ("disp_solid", "ply_shear_table", "ply_angle", "ply_thickness")]
    exact += [lambda a=a: c.field_output_vjp(SFF, a, cbar) for a in ("disp_solid", "ply_shear_table", "ply_angle", "ply_thickness")]
    for call in exact:
        a, b = call(), call()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    V = rng.uniform(-1, 1, m.nel * 3)
    solved = {f"total_gradient {a}": (lambda a=a: c.total_gradient(SF, a)[0]) for a in ("ply_angle", "ply_thickness", "laminate", "F_solid")}
    solved["total_gradients"] = lambda: c.total_gradients(["compliance", SF, "ply_failure"], "ply_angle")[0]
    solved["total_jvp"] = lambda: np.asarray(c.total_jvp("ply_angle", V, [SF, "compliance"], want_states=False)[1])
    solved.update({f"field_total_gradients {a}": (lambda a=a: c.field_total_gradients(SFF, cbar, a)[0])
                   for a in ("ply_angle", "ply_thickness", "laminate")})
    for name, call in solved.items():
        a, b = call(), call()
        print(f"{name}: two calls differ by {np.abs(a - b).max() / np.abs(a).max():.1e} of the largest entry")
        assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 1e-10 * np.abs(a).max(), name
    c.close()


def test_layup_route_builds_the_table_and_pulls_its_cotangent_back_to_the_angles():
    m = plate_mesh(2.0, 10.0, 4, 20)
    nply = 5
    c, rng, pc, S, t, theta = _layup_ctx(m, nply, seed=5, bc=CLAMP)
    host = lambda th: lm.ply_shear_table(np.broadcast_to(pc[:, 4], th.shape), np.broadcast_to(pc[:, 5], th.shape), th,
                                         lm.shear_strength(S[:, 0], S[:, 1]))
    ref = host(theta)
    tab = c.get_field("ply_shear_table").reshape(ref.shape)
    for k in range(6):
        assert np.abs(tab[..., k] - ref[..., k]).max() <= 1e-13 * np.abs(ref[..., k]).max(), k
    th2 = rng.uniform(-180, 180, theta.shape)
    c.set_field("ply_angle", th2)                                                   # the angles rebuild it, the thicknesses do not enter
    assert np.abs(c.get_field("ply_shear_table").reshape(ref.shape) - host(th2)).max() <= 1e-13 * np.abs(ref).max()
    c.set_field("ply_thickness", 1.3 * t)
    assert np.abs(c.get_field("ply_shear_table").reshape(ref.shape) - host(th2)).max() <= 1e-13 * np.abs(ref).max()
    c.set_field("ply_thickness", t)
    c.set_state(2e-3 * rng.uniform(-1, 1, m.ndof))
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    dG = lm.ply_shear_table_dtheta(np.broadcast_to(pc[:, 4], th2.shape), np.broadcast_to(pc[:, 5], th2.shape), th2).reshape(m.nel, nply, 4)
    gt = c.dfunctional("ply_shear_failure", "ply_shear_table").reshape(ref.shape)
    ga = c.dfunctional("ply_shear_failure", "ply_angle").reshape(m.nel, nply)
    hc = np.einsum("epk,epk->ep", gt[..., :4], dG)
    assert np.abs(ga - hc).max() <= 1e-12 * np.abs(hc).max()
    assert not np.any(c.dfunctional("ply_shear_failure", "ply_thickness"))
    cbar = rng.uniform(-1, 1, m.nel * nply)
    va = c.field_output_vjp("ply_shear_failure_field", "ply_angle", cbar).reshape(m.nel, nply)
    vt = c.field_output_vjp("ply_shear_failure_field", "ply_shear_table", cbar).reshape(ref.shape)
    hv = np.einsum("epk,epk->ep", vt[..., :4], dG)
    assert np.abs(va - hv).max() <= 1e-12 * np.abs(hv).max()
    assert not np.any(c.field_output_vjp("ply_shear_failure_field", "ply_thickness", cbar))
    c.close()


def test_table_handling_and_refusals():
    from femo_alpha_amd._lib import FemoHipError, dptr
    from femo_alpha_amd.backend import ShellContext
    m = plate_mesh(2.0, 10.0, 4, 20)
    rng = np.random.default_rng(4)
    clt, tab = random_laminate(m.nel, rng), random_shear_table(m.nel, 4, rng)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.use_direct_solver()
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    with pytest.raises(FemoHipError, match="laminate mode"):
        c.set_ply_shear_table(tab)
    c.set_laminate(clt)
    cb = np.ones(m.nel * 4)
    for call in (lambda: c.functional("ply_shear_failure"), lambda: c.dfunctional("ply_shear_failure", "disp_solid"),
                 lambda: c.ply_shear_failure_field(), lambda: c.total_gradient("ply_shear_failure", "laminate"),
                 lambda: c.total_gradients(["compliance", "ply_shear_failure"], "laminate"),
                 lambda: c.total_jvp("laminate", clt.ravel(), ["ply_shear_failure"]),
                 lambda: c.field_output_vjp("ply_shear_failure_field", "disp_solid", cb),
                 lambda: c.field_total_gradients("ply_shear_failure_field", cb, "laminate"),
                 lambda: c.set_field("ply_shear_table", tab)):
        with pytest.raises(FemoHipError, match="femo_set_ply_shear_table"):
            call()
    with pytest.raises(FemoHipError, match="npt must be 1..32"):
        c.set_ply_shear_table(np.zeros((m.nel, 33, 6)))
    with pytest.raises(FemoHipError, match="npt must be 1..32"):
        c.set_ply_shear_table(np.zeros(0), npt=0)
    with pytest.raises(FemoHipError, match=r"x 4 points x 80 cells = 1920, got 1914"):
        c.set_ply_shear_table(tab.ravel()[:-6], npt=4)
    bad = tab.copy(); bad[7, 2, 5] = np.nan
    with pytest.raises(FemoHipError, match="value 5 of recovery point 2 of cell 7 is not finite"):
        c.set_ply_shear_table(bad)
    with pytest.raises(FemoHipError, match="rho must be finite and > 0"):
        c.set_ply_shear_params(np.inf)
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    # the context is still usable; setting a table does not trigger a re-factorisation
    c.solve_state(True)
    w, info = c.get_state(), c.frontal_info()
    c.set_ply_shear_table(tab)
    assert c.field_size("ply_shear_table") == tab.size and np.array_equal(c.get_field("ply_shear_table"), tab.ravel())
    assert c.field_size_of("ply_shear_failure_field") == m.nel * 4
    c.solve_state(True)
    assert c.frontal_info() == info
    assert np.abs(c.get_state() - w).max() <= 1e-12 * np.abs(w).max()
    K = c.functional("ply_shear_failure")
    fld = c.ply_shear_failure_field()
    assert np.isfinite(K)
    for call in (lambda: c.dfunctional("ply_shear_failure", "uhat"), lambda: c.total_gradient("ply_shear_failure", "uhat"),
                 lambda: c.total_gradients(["compliance", "ply_shear_failure"], "uhat"),
                 lambda: c.total_jvp("uhat", np.ones(3 * m.nn), ["ply_shear_failure"]),
                 lambda: c.field_output_vjp("ply_shear_failure_field", "uhat", cb),
                 lambda: c.field_total_gradients("ply_shear_failure_field", cb, "uhat"),
                 lambda: c.field_output_jvp("ply_shear_failure_field", "disp_solid", np.ones(m.ndof)),
                 lambda: c.field_total_jvp(["ply_shear_failure_field"], "laminate", clt.ravel()),
                 lambda: c.field_output_jacobian("ply_shear_failure_field", "disp_solid")):
        with pytest.raises(FemoHipError, match="not provided"):
            call()
    out5 = np.empty(5)
    assert c.lib.femo_ply_shear_failure_field(c._h, dptr(out5), 5) != 0 and b"nel * npt entries" in c.lib.femo_last_error(c._h)
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_dfunctional(c._h, b"ply_shear_failure", b"ply_shear_table", dptr(out5), 5))
    assert c.functional("ply_shear_failure") == K and np.array_equal(c.ply_shear_failure_field(), fld)
    assert np.array_equal(c.get_field("ply_shear_table"), tab.ravel())
    # for every other output the table is an argument with exact zeros
    assert not np.any(c.dfunctional("compliance", "ply_shear_table")) and not np.any(c.total_gradient("compliance", "ply_shear_table")[0])
    assert not np.any(c.dRdarg_T("ply_shear_table", rng.uniform(-1, 1, m.ndof)))
    # the table survives new laminate values and goes with the laminate
    c.set_field("laminate", clt * 1.01)
    assert c.field_size("ply_shear_table") == tab.size and np.array_equal(c.get_field("ply_shear_table"), tab.ravel())
    c.set_ply_shear_table(None)
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    c.set_ply_shear_table(tab)
    c.set_laminate(None)
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    with pytest.raises(FemoHipError, match="femo_set_ply_shear_table"):
        c.functional("ply_shear_failure")
    c.close()


def test_layup_strengths_own_the_table_and_live_with_the_layup():
    from femo_alpha_amd._lib import FemoHipError
    m = plate_mesh(2.0, 10.0, 3, 7)
    c, rng, pc, S, t, theta = _layup_ctx(m, 3, bc=CLAMP)
    tab = c.get_field("ply_shear_table")
    assert tab.size == 6 * 3 * m.nel
    for call in (lambda: c.set_ply_shear_table(tab.reshape(m.nel, 3, 6)), lambda: c.set_field("ply_shear_table", tab),
                 lambda: c.set_ply_shear_table(None)):
        with pytest.raises(FemoHipError, match="femo_set_layup_shear_strength"):
            call()
    bad = S.copy(); bad[1, 1] = 0.0
    with pytest.raises(FemoHipError, match="S23 of ply 1"):
        c.set_layup_shear_strength(bad)
    with pytest.raises(FemoHipError, match="the layup has 3 plies, got 2"):
        c.set_layup_shear_strength(S[:2])
    assert np.array_equal(c.get_field("ply_shear_table"), tab)
    c.set_layup(pc, t, theta, ("bot", "top"))                                       # the same ply count keeps the strengths
    assert np.array_equal(c.get_field("ply_shear_table"), tab)
    c.set_layup_shear_strength(None)
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    c.set_ply_shear_table(tab.reshape(m.nel, 3, 6))                                 # without strengths the table is the caller's again
    c.set_layup_shear_strength(S)
    c.set_layup(pc[:2], t[:, :2], theta[:, :2], ("bot", "top"))                     # another ply count drops them with their table
    assert c.lib.femo_field_size(c._h, b"ply_shear_table") == -1
    c.set_layup(None)
    with pytest.raises(FemoHipError, match="no layup is active"):
        c.set_layup_shear_strength(S[:2])
    c.close()


@pytest.mark.parametrize("renumber", [False, True])
def test_reverse_mode_through_the_model_matches_the_backend_totals(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel, nply = mesh.nn, mesh.nel, 3
    rng = np.random.default_rng(8)
    pc = _plies(nply, rng)
    pc[:, 6:8] *= 1e-3; pc[:, 8:12] *= 1e-6
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    theta = rng.uniform(-180, 180, (nel, nply))
    S = 1500.0 * (1 + 0.3 * rng.uniform(0, 1, (nply, 2)))                             # failure indices of order one under this load
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
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, rho=20,
                         layup=dict(plies=pc, t=t[0], theta=theta[0], surfaces=("bot", "top"), shear_strength=S))
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    ctx = model.shell_pde.ctx
    fld = ctx.ply_shear_failure_field()
    print(f"model: max shear index {fld.max():.3e}, K {ctx.functional('ply_shear_failure'):.6e}")
    assert model.fea.outputs_dict["ply_shear_failure"]["arguments"] == model.fea.outputs_dict["ply_failure"]["arguments"]
    for var, arg in ((ply_t, "ply_thickness"), (ply_a, "ply_angle")):
        got = np.asarray(recorder.compute_totals(out.ply_shear_failure, var)).reshape(nel, nply)
        ref = np.empty((nel, nply))
        ref[model.cell_of_new] = ctx.total_gradient("ply_shear_failure", arg)[0].reshape(nel, nply)     # solver order -> caller order
        assert np.abs(ref).max() > 0 and np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), arg
    # the field through the model: FEA.field_gradients takes cotangents and answers in caller order, and the partial of the field form
    # transposes through computeMatVecProductBwd
    from femo_alpha_amd.fea.fea_hip import computeMatVecProductBwd, computePartials
    fea, SFF = model.fea, "ply_shear_failure_field"
    cb = rng.uniform(0.0, 1.0, (2, nel * nply))                                      # caller order
    cbs = cb.reshape(2, nel, nply)[:, model.cell_of_new].reshape(2, -1)              # the backend's own order
    for arg in ("ply_angle", "ply_thickness"):
        got = fea.field_gradients(SFF, cb, arg)
        g = ctx.field_total_gradients(SFF, cbs, arg)[0].reshape(2, nel, nply)
        want = np.empty_like(g)
        want[:, model.cell_of_new] = g
        assert got.shape == (2, nel * nply) and np.abs(got - want.reshape(2, -1)).max() <= 1e-10 * np.abs(want).max(), arg
        one = fea.field_gradients(SFF, cb[0], arg)
        assert one.shape == (nel * nply,) and np.abs(one - got[0]).max() <= 1e-10 * np.abs(got[0]).max()
    form = model.ply_shear_failure_field_form
    for role in ("disp_solid", "ply_angle"):
        func = fea.states_dict[role]["function"] if role == "disp_solid" else fea.inputs_dict[role]["function"]
        assert np.array_equal(computeMatVecProductBwd(computePartials(form, func), cbs[0]), ctx.field_output_vjp(SFF, role, cbs[0]))
    model2 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, layup=dict(plies=pc, t=t[0], theta=theta[0]))
    assert "ply_shear_failure" not in model2.fea.outputs_dict
