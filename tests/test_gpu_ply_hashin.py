"""Hashin fibre and matrix failure outputs on the GPU ("ply_hashin_fibre", "ply_hashin_matrix", femo_ply_hashin_field and the field
names "ply_hashin_fibre_field", "ply_hashin_matrix_field") against the numpy reference tests/ply_hashin_ref.py, the existing ply
failure kernels, closed forms, central differences with re-solves, and the refusals.  The bars are the project's: 1e-11 of the largest
entry against the reference, 1e-6 |fd| + 1e-9 max|G| against central differences, 1e-10 between grouped and separate routes.  The
inputs and the entries of the central differences come from tests/test_ply_hashin_cpu.py, which asserts on the reference that every
branch is populated and that no point changes branch inside a difference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from test_gpu_laminate import BETA, CLAMP, PLY, ROOT_EDGE, block_scale, random_laminate, tight   # noqa: E402
from test_gpu_ply_failure import random_table                                    # noqa: E402
from test_layup_cpu import _plies                                                # noqa: E402
from test_ply_hashin_cpu import (FD_ANGLE, FD_FORCE, FD_LAMINATE, FD_THICKNESS, LAYUP_CDRILL, case_inputs, flat_plate_case,   # noqa: E402
                                 layup_inputs, mesh_of, oracle_of, random_strengths, tsai_wu_only)

pytestmark = pytest.mark.gpu

FIELDS = dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0])
MODES = ("fibre", "matrix")
FN = {m: "ply_hashin_" + m for m in MODES}
FLD = {m: "ply_hashin_" + m + "_field" for m in MODES}
ZERO_ARGS = ("laminate", "thickness", "E", "nu", "density", "F_solid")
bar = lambda g, fd, G: abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()


def _context(m, inp, bc=None):
    from femo_alpha_amd.backend import ShellContext
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=inp["f"]).items():
        c.set_field(k, v)
    if inp.get("uhat") is not None:
        c.set_field("uhat", inp["uhat"])
    if bc == "penalty":
        c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(inp["clt"])
    c.set_ply_table(inp["tab"])
    c.set_ply_hashin_table(inp["H"])
    return c


def _pair(kind, seed=0, npt=4, bc=None, uhat=True):
    m = mesh_of(kind)
    inp = case_inputs(m, seed, npt, uhat)
    return m, inp, oracle_of(m, inp), _context(m, inp, bc)


def _close(a, r, what, per_kind=False):
    """1e-11 of the largest entry of the reference; the table gradients per entry kind, each against its own largest (an entry kind
    the index does not depend on has to be exactly zero)."""
    if per_kind:
        for k in range(16):
            assert np.abs(a[..., k] - r[..., k]).max() <= 1e-11 * np.abs(r[..., k]).max(), (what, k)
    else:
        assert a.shape == r.shape and np.abs(a - r).max() <= 1e-11 * np.abs(r).max(), what


def _check(o, c, w, cells=None, alpha=None, tag=""):
    """Both fields, and per mode the value and the state and table partials, rho = 5 / max FI of the mode."""
    refs = o.field(w)
    got = c.ply_hashin_field()
    for mode, fr, fg in zip(MODES, refs, got):
        _close(fg, fr, mode + " field")
        rho = 5.0 / fr.max()
        c.set_ply_failure_params(rho)
        Kr = o.value(w, rho, mode, alpha=alpha, cells=cells)
        K = c.functional(FN[mode])
        gwr, gtr = o.gradients(w, rho, mode, cells=cells)
        gw = c.dfunctional(FN[mode], "disp_solid")
        gt = c.dfunctional(FN[mode], "ply_table").reshape(gtr.shape)
        kinds = [k for k in range(10) if np.abs(gtr[..., k]).max() > 0]
        print(f"{tag} {mode}: FI in [{fr.min():.3e}, {fr.max():.3e}]  K {K:.15e} reference {Kr:.15e}  dK/dw "
              f"{np.abs(gw - gwr).max() / np.abs(gwr).max():.2e}  dK/dtable (per entry kind) "
              f"{max(np.abs(gt[..., k] - gtr[..., k]).max() / np.abs(gtr[..., k]).max() for k in kinds):.2e}")
        assert abs(K - Kr) <= 1e-11 * np.abs(fr).max()
        assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gt))
        _close(gw, gwr, mode + " dK/dw")
        _close(gt, gtr, mode + " dK/dtable", per_kind=True)
        assert not np.any(gt[..., 10:16])
        assert len(kinds) == (4 if mode == "fibre" else 7)                      # the rows of G the index reads, and z
        if cells is not None:
            assert not np.any(gt[np.setdiff1d(np.arange(gt.shape[0]), cells)])


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("kind", ["warped", "tri", "quad CG1CG1", "tri CG2CR1"])
def test_fields_values_and_partials_against_the_reference(kind, sub):
    """uhat != 0, a random state, two plies with four recovery points, strengths drawn per (cell, point) with Yt < Yc and
    ST != Yc / 2; the whole mesh with the reference area, or a tagged sub-domain with a given alpha; 32 and 36 cells: one partial
    wave."""
    m, inp, o, c = _pair(kind)
    w = inp["w"]
    c.set_state(w)
    cells, alpha = None, None
    if sub:
        tags = (np.arange(m.nel) % 3).astype(np.int32)
        c.set_cell_tags(tags, 3)
        c.select_subdomain(1)
        alpha = 2.5
        c.set_stress_alpha(alpha, 1)
        cells = np.where(tags == 1)[0]
    else:
        nel = m.nel
        mat = [np.full((nel, 2), PLY[k]) for k in ("G13", "G23")]
        c.set_ply_shear_table(lm.ply_shear_table(*mat, inp["rng"].uniform(-90, 90, (nel, 2)), lm.shear_strength(3e4, 2e4)))
    _check(o, c, w, cells, alpha, f"{kind} sub={sub}")
    for mode in MODES:
        for name in ZERO_ARGS + (() if sub else ("ply_shear_table",)):
            assert not np.any(c.dfunctional(FN[mode], name)), (mode, name)
    c.close()


@pytest.mark.parametrize("npt", [1, 32])
def test_two_blocks_and_a_selection_inside_the_second(npt):
    """80 cells: one full wave and a partial one.  The selection lies entirely in the second block, so the combine merges an empty
    block slot with a filled one."""
    m, inp, o, c = _pair("plate80", seed=3, npt=npt)
    assert m.nel == 80
    w = inp["w"]
    c.set_state(w)
    _check(o, c, w, tag=f"80 cells npt={npt}")
    tags = np.where(np.arange(m.nel) >= 66, 1, 0).astype(np.int32)
    c.set_cell_tags(tags, 2)
    c.select_subdomain(1)
    _check(o, c, w, cells=np.arange(66, 80), tag=f"80 cells npt={npt}, cells 66..79")
    c.close()


def test_equal_strengths_reproduce_the_ply_failure_kernels():
    """Xt = Xc = X: the fibre outputs are those of "ply_failure" on the same G, z with only F11 = 1 / X^2.  Yt = Yc = Y and
    ST = Y / 2: the matrix outputs are those with only F22 = 1 / Y^2 and F66 = 1 / SL^2.  Fields, values and dK/dw, 1e-11."""
    m, inp, o, c = _pair("warped")
    H = inp["H"].copy()
    H[..., 1] = H[..., 0]
    H[..., 3] = H[..., 2]
    H[..., 5] = 0.5 * H[..., 3]
    c.set_ply_hashin_table(H)
    c.set_state(inp["w"])
    tabs = dict(fibre=tsai_wu_only(inp["tab"], F11=1 / H[..., 0] ** 2),
                matrix=tsai_wu_only(inp["tab"], F22=1 / H[..., 2] ** 2, F66=1 / H[..., 4] ** 2))
    for i, mode in enumerate(MODES):
        c.set_ply_table(tabs[mode])                                             # the Hashin kernels do not read the entries 10..15
        fr = c.ply_failure_field()
        c.set_ply_failure_params(5.0 / fr.max())
        fg = c.ply_hashin_field()[i]
        Kr, K = c.functional("ply_failure"), c.functional(FN[mode])
        gr, g = c.dfunctional("ply_failure", "disp_solid"), c.dfunctional(FN[mode], "disp_solid")
        tr, t = (c.dfunctional(n, "ply_table").reshape(inp["tab"].shape)[..., :10] for n in ("ply_failure", FN[mode]))
        print(f"{mode}: field {np.abs(fg - fr).max() / fr.max():.2e}  K {abs(K - Kr):.2e}  dK/dw {np.abs(g - gr).max() / np.abs(gr).max():.2e}")
        _close(fg, fr, mode + " field")
        assert abs(K - Kr) <= 1e-11 * fr.max()
        _close(g, gr, mode + " dK/dw")
        for k in range(10):
            assert np.abs(t[..., k] - tr[..., k]).max() <= 1e-11 * np.abs(tr[..., k]).max(), (mode, k)
    c.close()


def test_fibre_field_is_bit_identical_under_a_change_of_sign_with_swapped_strengths():
    """The branch is a select on the sign: at -w with Xt and Xc swapped every product sees the same operands."""
    m, inp, o, c = _pair("tri")
    c.set_state(inp["w"])
    f0, m0 = c.ply_hashin_field()
    ff, tf = o.indices(inp["w"])[0], o.indices(inp["w"])[2]
    assert tf.any() and (~tf).any()
    c.set_ply_hashin_table(inp["H"][..., [1, 0, 2, 3, 4, 5]])
    c.set_state(-inp["w"])
    f1, m1 = c.ply_hashin_field()
    assert np.array_equal(f1, f0)
    assert not np.array_equal(m1, m0)                                           # the matrix strengths were not swapped
    c.close()


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("eps", [1e-3, -1e-3])
def test_closed_form_of_a_uniformly_strained_flat_plate(eps, direction):
    """One 0-degree ply, u_x = eps x or u_y = eps y: FI_f = (s1 / X)^2 and the matrix formulas in tension and compression, the
    linear term c1 s2 included, with (s1, s2) = (Q11, Q12) eps or (Q12, Q22) eps as the cell frame has it."""
    from femo_alpha_amd.backend import ShellContext
    m, tab, H, w, Q = flat_plate_case(eps, direction)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=[0.0]).items():
        c.set_field(k, v)
    c.set_laminate(lm.isotropic(np.full(m.nel, 0.05), 1e8, 0.3))
    c.set_ply_table(tab)
    c.set_ply_hashin_table(H)
    c.set_state(w)
    gf, gm = c.ply_hashin_field()
    Xt, Xc, Yt, Yc, SL, ST = H
    ok = False
    for s1, s2 in ((Q[0, 0] * eps, Q[1, 0] * eps), (Q[0, 1] * eps, Q[1, 1] * eps)):      # the frame's first axis along x, or along y
        ff = (s1 / Xt) ** 2 if eps > 0 else (s1 / Xc) ** 2
        fm = (s2 / Yt) ** 2 if eps > 0 else (s2 / (2 * ST)) ** 2 + ((Yc / (2 * ST)) ** 2 - 1) * s2 / Yc
        ok = ok or (np.abs(gf - ff).max() <= 1e-11 * ff and np.abs(gm - fm).max() <= 1e-11 * abs(fm))
    print(f"eps {eps:+.0e} direction {direction}: fibre {gf[0, 0]:.12e} matrix {gm[0, 0]:.12e}")
    assert ok and gf.shape == (m.nel, 2)
    # the frame the reference sees decides which of the two it has to be
    o = oracle_of(m, dict(f=np.zeros((m.nn, 3)), uhat=None, tab=tab, H=H))
    rf, rm = o.field(w)
    _close(gf, rf, "fibre field")
    _close(gm, rm, "matrix field")
    c.close()


def _layup_ctx(m, inp):
    from femo_alpha_amd.backend import ShellContext
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=inp["f"], uhat=inp["uhat"]).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_layup(inp["pc"], inp["t"], inp["theta"], ("bot", "top"), c_drill=LAYUP_CDRILL, reference="bot", hashin=inp["Hp"])
    return c


@pytest.mark.parametrize("mode", MODES)
def test_layup_totals_against_central_differences_with_re_solves(mode):
    """set_layup(..., hashin=...) about the bottom surface, clamped root: totals in the ply angles and thicknesses; then the same
    laminate and table as ordinary values (the strengths stay): totals in laminate entries and load entries."""
    m = mesh_of("warped")
    inp = layup_inputs(m)
    t, theta = inp["t"], inp["theta"]
    c = _layup_ctx(m, inp)
    tight(c)
    fn, i = FN[mode], MODES.index(mode)

    def solved():
        c.solve_state(True)
        return c.functional(fn)
    solved()
    c.set_ply_failure_params(5.0 / c.ply_hashin_field()[i].max())
    solved()
    Ga = c.total_gradient(fn, "ply_angle")[0].reshape(m.nel, 2)
    Gt = c.total_gradient(fn, "ply_thickness")[0].reshape(m.nel, 2)
    for e, j, s in FD_ANGLE:
        vals = []
        for sg in (1, -1):
            th = theta.copy(); th[e, j] += sg * s
            c.set_field("ply_angle", th)
            vals.append(solved())
        c.set_field("ply_angle", theta)
        print(f"{mode} angle totals [cell {e}, ply {j}]: {Ga[e, j]:.8e} against {(vals[0] - vals[1]) / (2 * s):.8e}")
        assert bar(Ga[e, j], (vals[0] - vals[1]) / (2 * s), Ga), ("ply_angle", e, j)
    for e, j, rel in FD_THICKNESS:
        s = rel * t[e, j]
        vals = []
        for sg in (1, -1):
            tt = t.copy(); tt[e, j] += sg * s
            c.set_field("ply_thickness", tt)
            vals.append(solved())
        c.set_field("ply_thickness", t)
        print(f"{mode} thickness totals [cell {e}, ply {j}]: {Gt[e, j]:.8e} against {(vals[0] - vals[1]) / (2 * s):.8e}")
        assert bar(Gt[e, j], (vals[0] - vals[1]) / (2 * s), Gt), ("ply_thickness", e, j)
    K0 = solved()
    clt = c.get_field("laminate").reshape(m.nel, 32)
    c.set_layup(None)                                                             # the laminate and the table stay as ordinary values
    assert abs(solved() - K0) <= 1e-12 * abs(K0)
    gl = c.total_gradient(fn, "laminate")[0].reshape(m.nel, 32)
    for e, k, rel in FD_LAMINATE:
        d = clt.copy()
        s = rel * block_scale(clt, e, k)
        d[e, k] += s; c.set_laminate(d); jp = solved()
        d[e, k] -= 2 * s; c.set_laminate(d); jm = solved()
        c.set_laminate(clt)
        print(f"{mode} laminate [{e}, {k}]: {gl[e, k]:.8e} against {(jp - jm) / (2 * s):.8e}")
        assert bar(gl[e, k], (jp - jm) / (2 * s), gl), ("laminate", e, k)
    solved()
    gf = c.total_gradient(fn, "F_solid")[0]
    f0 = c.get_field("F_solid")
    for j, s in FD_FORCE:
        x = f0.copy(); x[j] += s; c.set_field("F_solid", x); jp = solved()
        x[j] -= 2 * s; c.set_field("F_solid", x); jm = solved()
        c.set_field("F_solid", f0)
        print(f"{mode} F_solid [{j}]: {gf[j]:.8e} against {(jp - jm) / (2 * s):.8e}")
        assert bar(gf[j], (jp - jm) / (2 * s), gf), ("F_solid", j)
    solved()
    gt = c.total_gradient(fn, "ply_table")[0]
    assert np.array_equal(gt, c.dfunctional(fn, "ply_table"))                     # the explicit partial alone
    for name in ("thickness", "E", "nu", "density"):
        assert not np.any(c.total_gradient(fn, name)[0])
    c.close()


def test_grouped_totals_and_the_forward_chain_agree_with_the_separate_totals():
    m, inp, o, c = _pair("warped", bc="penalty")
    c.use_direct_solver()
    tags = (np.arange(m.nel) % 3).astype(np.int32)
    c.set_cell_tags(tags, 3)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / max(np.abs(c.ply_failure_field()).max(), *(f.max() for f in c.ply_hashin_field())))
    names, subs = ["compliance", FN["fibre"], "ply_failure", FN["matrix"], FN["matrix"]], [-1, -1, -1, -1, 1]
    for arg in ("laminate", "F_solid", "ply_table"):
        G = c.total_gradients(names, arg, subdomains=subs)[0]
        for i, (n, s) in enumerate(zip(names, subs)):
            c.select_subdomain(s)
            g = c.total_gradient(n, arg)[0]
            assert np.abs(G[i] - g).max() <= 1e-10 * max(np.abs(g).max(), 1e-300), (n, s, arg)
        c.select_subdomain(-1)
        assert all(np.abs(G[i]).max() > 0 for i in (1, 3, 4))
        scale = np.abs(inp["clt"]).ravel() if arg == "laminate" else np.abs(inp["tab"]).ravel() if arg == "ply_table" else 1.0
        V = inp["rng"].uniform(-1, 1, G.shape[1]) * scale
        dJ = c.total_jvp(arg, V, names, subdomains=subs, want_states=False)[1]
        for i in range(len(names)):
            assert abs(dJ[i] - G[i] @ V) <= 1e-10 * np.abs(G[i] * V).sum(), (names[i], arg)
    c.close()
    # ... and under a layup, in the ply thicknesses
    m = mesh_of("warped")
    linp = layup_inputs(m)
    c = _layup_ctx(m, linp)
    c.use_direct_solver()
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / max(np.abs(c.ply_failure_field()).max(), *(f.max() for f in c.ply_hashin_field())))
    names = ["compliance", FN["fibre"], "ply_failure", FN["matrix"]]
    for arg in ("ply_thickness", "ply_angle"):
        G = c.total_gradients(names, arg)[0]
        for i, n in enumerate(names):
            g = c.total_gradient(n, arg)[0]
            assert np.abs(g).max() > 0 and np.abs(G[i] - g).max() <= 1e-10 * np.abs(g).max(), (n, arg)
        V = linp["rng"].uniform(-1, 1, G.shape[1]) * (linp["t"].ravel() if arg == "ply_thickness" else 1.0)
        dJ = c.total_jvp(arg, V, names, want_states=False)[1]
        for i in range(len(names)):
            assert abs(dJ[i] - G[i] @ V) <= 1e-10 * np.abs(G[i] * V).sum(), (names[i], arg)
    c.close()


@pytest.mark.parametrize("kind", ["warped", "tri"])
def test_field_reverse_products_against_the_reference(kind):
    m, inp, o, c = _pair(kind, seed=2)
    w, rng = inp["w"], inp["rng"]
    c.set_state(w)
    cbar = rng.uniform(-1, 1, (3, m.nel * 4))
    for mode in MODES:
        gw = c.field_output_vjp(FLD[mode], "disp_solid", cbar)
        gt = c.field_output_vjp(FLD[mode], "ply_table", cbar).reshape(3, m.nel, 4, 16)
        for k in range(3):
            gwr, gtr = o.field_vjp(w, cbar[k], mode)
            _close(gw[k], gwr, mode + " field vjp, state")
            _close(gt[k], gtr, mode + " field vjp, table", per_kind=True)
        assert not np.any(gt[..., 10:16])
        assert np.array_equal(c.field_output_vjp(FLD[mode], "disp_solid", cbar[1]), gw[1])
        for name in ZERO_ARGS:
            assert not np.any(c.field_output_vjp(FLD[mode], name, cbar[0]))
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_field_totals_against_single_calls_and_central_differences(mode):
    """One-signed cotangents on the largest entries and directions that move every entry the same way (every cell's laminate
    stiffer, the whole load larger), as tests/test_gpu_ply_strength.py.  The reference asserts at the re-solved states of both legs
    that no entry with a cotangent changes its maximiser or its branch there."""
    m, inp, o, c = _pair("tri", seed=2, bc="penalty")
    clt, rng, i = inp["clt"], inp["rng"], MODES.index(mode)
    tight(c)
    name = FLD[mode]

    def solved():
        c.solve_state(True)
        return c.ply_hashin_field()[i].ravel(), c.get_state()
    f0, w0 = solved()
    top = np.argsort(f0)[::-1]
    cb = np.zeros((2, f0.size))
    cb[0, top[:8]] = rng.uniform(0.5, 1.0, 8) / f0.max()
    cb[1, top[:40]] = rng.uniform(0.5, 1.0, 40) / f0.max()
    live = (cb != 0).any(axis=0).reshape(m.nel, 4)

    def same_branches(wp, wm):
        for w in (wp, wm):
            assert np.array_equal(o.maximisers(w, mode)[live], o.maximisers(w0, mode)[live])
            q = o.maximisers(w0, mode)
            for k in (2, 3):                                                     # the tension masks of s1 and s2 at the maximiser
                a, b = (np.take_along_axis(o.indices(x)[k], q[:, None, :], 1)[:, 0] for x in (w, w0))
                assert np.array_equal(a[live], b[live])

    G, its, _ = c.field_total_gradients(name, cb, "laminate")
    assert np.all(its > 0)
    for k in range(2):
        g1 = c.field_total_gradients(name, cb[k], "laminate")[0][0]
        assert np.abs(G[k] - g1).max() <= 1e-10 * np.abs(g1).max()
    d = clt * rng.uniform(0.5, 1.5, (m.nel, 1))
    s = 1e-4
    c.set_laminate(clt + s * d); fp, wp = solved()
    c.set_laminate(clt - s * d); fm, wm = solved()
    c.set_laminate(clt)
    solved()
    same_branches(wp, wm)
    for k in range(2):
        fd, g = cb[k] @ (fp - fm) / (2 * s), G[k] @ d.ravel()
        print(f"{mode} field totals, laminate direction, cotangent {k}: {g:.10e} against {fd:.10e}: {abs(g - fd) / abs(fd):.1e} of it")
        assert bar(g, fd, G[k] * d.ravel())
    Gf = c.field_total_gradients(name, cb, "F_solid")[0]
    F0 = c.get_field("F_solid")
    df = F0 * rng.uniform(0.5, 1.5, F0.size)
    c.set_field("F_solid", F0 + s * df); fp, wp = solved()
    c.set_field("F_solid", F0 - s * df); fm, wm = solved()
    c.set_field("F_solid", F0)
    solved()
    same_branches(wp, wm)
    for k in range(2):
        fd, g = cb[k] @ (fp - fm) / (2 * s), Gf[k] @ df
        print(f"{mode} field totals, load direction, cotangent {k}: {g:.10e} against {fd:.10e}: {abs(g - fd) / abs(fd):.1e} of it")
        assert bar(g, fd, Gf[k] * df)
    Gs, its, rr = c.field_total_gradients(name, cb, "ply_table")
    assert not np.any(its) and np.array_equal(Gs, c.field_output_vjp(name, "ply_table", cb))
    c.close()


def test_field_totals_reach_the_layup_and_group_four_to_a_solve():
    m = mesh_of("warped")
    inp = layup_inputs(m, seed=4)
    c = _layup_ctx(m, inp)
    c.use_direct_solver()
    c.solve_state(True)
    for i, mode in enumerate(MODES):
        f0 = c.ply_hashin_field()[i].ravel()
        cb = inp["rng"].uniform(0.0, 1.0, (5, f0.size)) / f0.max()
        for arg in ("ply_thickness", "ply_angle"):
            G = c.field_total_gradients(FLD[mode], cb, arg)[0]
            for k in (0, 4):
                g1 = c.field_total_gradients(FLD[mode], cb[k], arg)[0][0]
                assert np.abs(g1).max() > 0 and np.abs(G[k] - g1).max() <= 1e-10 * np.abs(g1).max(), (mode, arg, k)
    c.close()


def test_repeats_are_bit_identical_and_the_other_ply_outputs_are_not_disturbed():
    m, inp, o, c = _pair("warped", bc="penalty")
    nel = m.nel
    mat = [np.full((nel, 2), PLY[k]) for k in ("G13", "G23")]
    c.set_ply_shear_table(lm.ply_shear_table(*mat, inp["rng"].uniform(-90, 90, (nel, 2)), lm.shear_strength(3e4, 2e4)))
    c.use_direct_solver()
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / max(np.abs(c.ply_failure_field()).max(), *(f.max() for f in c.ply_hashin_field())))
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())
    others = ("ply_failure", "ply_strength_index", "ply_shear_failure")
    old = lambda: [np.array([c.functional(n) for n in others]), c.ply_failure_field(), c.ply_strength_index_field(),
                   c.ply_shear_failure_field(), c.dfunctional("ply_failure", "disp_solid"), c.dfunctional("ply_failure", "ply_table"),
                   c.dfunctional("ply_strength_index", "disp_solid"), c.dfunctional("ply_shear_failure", "disp_solid")]
    before = old()
    cbar = inp["rng"].uniform(-1, 1, (2, nel * 4))
    calls = [lambda: np.array([c.functional(FN[k]) for k in MODES]), lambda: np.stack(c.ply_hashin_field())]
    for mode in MODES:
        calls += [lambda mode=mode: c.dfunctional(FN[mode], "disp_solid"), lambda mode=mode: c.dfunctional(FN[mode], "ply_table"),
                  lambda mode=mode: c.field_output_vjp(FLD[mode], "disp_solid", cbar),
                  lambda mode=mode: c.field_output_vjp(FLD[mode], "ply_table", cbar)]
    for call in calls:
        a, b = call(), call()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    # a value pass of a new aggregate between the value pass and the gradient of an old one: each reads its own shift
    v0 = c.functional("ply_failure")
    K = [c.functional(FN[k]) for k in MODES]
    g = c.dfunctional("ply_failure", "disp_solid")
    assert v0 == before[0][0] and np.array_equal(g, before[4])
    kf = c.functional(FN["fibre"])
    c.functional(FN["matrix"])
    assert np.array_equal(c.dfunctional(FN["fibre"], "disp_solid"), calls[2]()) and kf == K[0]
    for a, b in zip(before, old()):
        assert np.array_equal(a, b)
    c.close()


def test_refusals_and_the_check_of_the_strengths():
    from femo_alpha_amd._lib import FemoHipError, dptr
    from femo_alpha_amd.backend import ShellContext
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    m = mesh_of("plate80")
    rng = np.random.default_rng(4)
    clt, tab, H = random_laminate(m.nel, rng), random_table(m.nel, rng), random_strengths((m.nel, 4), rng)
    c = ShellContext(m)
    for k, v in dict(FIELDS, F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.use_direct_solver()
    with pytest.raises(FemoHipError, match="laminate mode first"):
        c.set_ply_hashin_table(H)
    c.set_laminate(clt)
    cb = np.ones(m.nel * 4)
    F, FF = FN["matrix"], FLD["fibre"]
    every = (lambda: c.functional(F), lambda: c.dfunctional(F, "disp_solid"), lambda: c.ply_hashin_field(),
             lambda: c.total_gradient(F, "laminate"), lambda: c.total_gradients(["compliance", F], "laminate"),
             lambda: c.total_jvp("laminate", clt.ravel(), [F]), lambda: c.field_output_vjp(FF, "disp_solid", cb),
             lambda: c.field_total_gradients(FF, cb, "laminate"))
    c.set_ply_hashin_table(H)                                                    # strengths without a ply table
    for call in every:
        with pytest.raises(FemoHipError, match="femo_set_ply_table"):
            call()
    c.set_ply_hashin_table(None)
    c.solve_state(True)
    c.set_ply_table(tab)                                                          # a ply table without strengths
    for call in every:
        with pytest.raises(FemoHipError, match="femo_set_ply_hashin_table"):
            call()
    c.set_ply_hashin_table(H[:, :3])                                              # another number of recovery points
    for call in every:
        with pytest.raises(FemoHipError, match="3 recovery points per cell, the ply table 4"):
            call()
    with pytest.raises(FemoHipError, match="expected 6 values per recovery point"):
        c.set_ply_hashin_table(H.ravel()[:-6], npt=4)
    with pytest.raises(FemoHipError, match="npt must be 1..32"):
        c.set_ply_hashin_table(np.ones((m.nel, 33, 6)))
    c.set_ply_hashin_table(H)
    assert c.field_size_of(FF) == m.nel * 4
    K, fld = c.functional(F), c.ply_hashin_field()
    assert np.isfinite(K) and fld[0].shape == (m.nel, 4)
    # a strength that is not finite and > 0: the entry, the point and the cell; the table the context holds stays
    for val, (e, p, k, nm) in zip((0.0, -1.0, np.nan, np.inf), ((7, 2, 3, "Yc"), (9, 1, 0, "Xt"), (0, 0, 5, "ST"), (79, 3, 4, "SL"))):
        bad = H.copy()
        bad[e, p, k] = val
        bad[79, 3, 5] = val                                                      # a later one: the first is named
        with pytest.raises(FemoHipError, match=f"value {k} \\(the strength {nm}\\) of recovery point {p} of cell {e} is not finite and > 0"):
            c.set_ply_hashin_table(bad)
        assert c.functional(F) == K
    for call in (lambda: c.dfunctional(F, "uhat"), lambda: c.total_gradient(F, "uhat"),
                 lambda: c.total_gradients(["compliance", FN["fibre"]], "uhat"), lambda: c.total_jvp("uhat", np.ones(3 * m.nn), [F]),
                 lambda: c.field_output_vjp(FF, "uhat", cb), lambda: c.field_total_gradients(FLD["matrix"], cb, "uhat")):
        with pytest.raises(FemoHipError, match="shape derivative"):
            call()
    for name in FLD.values():
        for call in (lambda: c.field_output_jvp(name, "disp_solid", np.ones(m.ndof)), lambda: c.field_total_jvp([name], "laminate", clt.ravel()),
                     lambda: c.field_output_jacobian(name, "disp_solid")):
            with pytest.raises(FemoHipError, match=f"forward mode and the sparse Jacobian of '{name}' are not provided"):
                call()
    out5 = np.empty(5)
    assert c.lib.femo_ply_hashin_field(c._h, dptr(out5), None, 5) != 0 and b"nel * npt entries" in c.lib.femo_last_error(c._h)
    only_m = np.empty(m.nel * 4)
    c._chk(c.lib.femo_ply_hashin_field(c._h, None, dptr(only_m), only_m.size))    # either pointer may be null
    assert np.array_equal(only_m.reshape(m.nel, 4), fld[1])
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_dfunctional(c._h, F.encode(), b"ply_table", dptr(out5), 5))
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_field_output_vjp(c._h, FF.encode(), b"ply_table", dptr(cb), 1, dptr(out5), 5))
    with pytest.raises(ValueError, match="wrong length"):
        c.field_output_vjp(FF, "disp_solid", cb[:-1])
    assert c.functional(F) == K and all(np.array_equal(a, b) for a, b in zip(c.ply_hashin_field(), fld))
    # broadcasts on the host, and leaving laminate mode drops the strengths
    c.set_ply_hashin_table(H[0, 0])
    c.set_ply_hashin_table(H[0])
    f1 = c.ply_hashin_field()[0]
    c.set_ply_hashin_table(np.broadcast_to(H[0], H.shape))
    assert np.array_equal(c.ply_hashin_field()[0], f1)
    c.set_laminate(None)
    c.set_laminate(clt)
    c.set_ply_table(tab)
    with pytest.raises(FemoHipError, match="femo_set_ply_hashin_table"):
        c.functional(F)
    c.close()
    with pytest.raises(ValueError, match="hashin needs laminate=True"):
        RMShellModel(m, shell_bc_func=CLAMP, record=False, hashin=True)
    with pytest.raises(ValueError, match="hashin needs a ply table"):
        RMShellModel(m, shell_bc_func=CLAMP, record=False, laminate=True, hashin=True)


@pytest.mark.parametrize("renumber", [False, True])
def test_through_the_model_with_a_layup_matches_the_backend_totals(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.fea.fea_hip import computeMatVecProductBwd, computePartials
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = mesh_of("plate80")
    nn, nel, nply = mesh.nn, mesh.nel, 2
    rng = np.random.default_rng(8)
    pc = _plies(nply, rng)
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    theta = rng.uniform(-180, 180, (nel, nply))
    Hp = random_strengths((nply,), rng)
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
    layup = dict(plies=pc, t=t[0], theta=theta[0], surfaces=("bot", "top"), hashin=Hp)
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, rho=20, layup=layup, hashin=True)
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    ctx = model.shell_pde.ctx
    npt = 2 * nply
    ff, fm = ctx.ply_hashin_field()
    print(f"model: max indices {ff.max():.3e} {fm.max():.3e}, K {ctx.functional(FN['fibre']):.6e} {ctx.functional(FN['matrix']):.6e}")
    fea = model.fea
    cb = rng.uniform(0.0, 1.0, (2, nel * npt))                                       # caller order
    cbs = cb.reshape(2, nel, npt)[:, model.cell_of_new].reshape(2, -1)               # the backend's own order
    for mode in MODES:
        assert fea.outputs_dict[FN[mode]]["arguments"] == fea.outputs_dict["ply_failure"]["arguments"]
        for var, arg in ((ply_t, "ply_thickness"), (ply_a, "ply_angle")):
            got = np.asarray(recorder.compute_totals(getattr(out, FN[mode]), var)).reshape(nel, nply)
            ref = np.empty((nel, nply))
            ref[model.cell_of_new] = ctx.total_gradient(FN[mode], arg)[0].reshape(nel, nply)      # solver order -> caller order
            assert np.abs(ref).max() > 0 and np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (mode, arg)
        for arg in ("ply_angle", "ply_thickness"):
            got = fea.field_gradients(FLD[mode], cb, arg)
            g = ctx.field_total_gradients(FLD[mode], cbs, arg)[0].reshape(2, nel, nply)
            want = np.empty_like(g)
            want[:, model.cell_of_new] = g
            assert got.shape == (2, nel * nply) and np.abs(got - want.reshape(2, -1)).max() <= 1e-10 * np.abs(want).max(), (mode, arg)
        form = getattr(model, FLD[mode] + "_form")
        for role in ("disp_solid", "ply_angle"):
            func = fea.states_dict[role]["function"] if role == "disp_solid" else fea.inputs_dict[role]["function"]
            assert np.array_equal(computeMatVecProductBwd(computePartials(form, func), cbs[0]), ctx.field_output_vjp(FLD[mode], role, cbs[0]))
    # opt-in: a model built without the option is unchanged; the table route takes the strengths of its recovery points
    model2 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, layup=dict(layup, hashin=None))
    assert FN["fibre"] not in model2.fea.outputs_dict and not hasattr(model2, FLD["fibre"] + "_form")
    model3 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, laminate=True, ply_failure=4, hashin=Hp[0])
    assert model3.fea.outputs_dict[FN["matrix"]]["arguments"] == ["disp_solid", "ply_table"]
    # the strengths given to the model instead of the layup: the same table on the device
    model4 = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, layup=dict(layup, hashin=None), hashin=Hp)
    assert FN["fibre"] in model4.fea.outputs_dict
    ctx4 = model4.shell_pde.ctx
    for name in ("ply_thickness", "ply_angle"):
        ctx4.set_field(name, ctx.get_field(name))
    ctx4.set_state(ctx.get_state())
    assert all(np.array_equal(a, b) for a, b in zip(ctx4.ply_hashin_field(), (ff, fm)))
