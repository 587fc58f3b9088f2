"""Interlaminar shear outputs without a GPU: the numpy reference (tests/ply_shear_ref.py) -- its derivatives against complex steps of
its own value, the bounds of the aggregate and the zero state, the clamped strip against the closed form -- and the host helpers
``laminate.shear_strength`` / ``laminate.ply_shear_table`` / ``laminate.ply_shear_table_dtheta``."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh, quads_to_triangles, wing_skin_mesh   # noqa: E402
from laminate_ref import LaminateOracle                                          # noqa: E402
from oracle.rm_shell_oracle import degree4_rule                                  # noqa: E402
from ply_shear_ref import PlyShearOracle                                         # noqa: E402

PLY = dict(E1=1.35e8, E2=1.0e7, G12=5e6, nu12=0.3, G13=5e6, G23=3.5e6)          # the plies of test_gpu_laminate.py
CLAMP = lambda x: np.less(x[0], 3e-16)
BETA = 1e10


def random_shear_table(nel, npt, rng):
    """General 2 x 2 Gs (every entry exercised) and positive strengths."""
    tab = np.empty((nel, npt, 6))
    tab[:, :, 0:4] = 4e6 * rng.uniform(-1, 1, (nel, npt, 4))
    tab[:, :, 4:6] = 1.0 / (5e4 * (1 + 0.5 * rng.uniform(0, 1, (nel, npt, 2)))) ** 2
    return tab


def oracle_of(m, rng, uhat=True):
    o = PlyShearOracle(m, nquad=degree4_rule(m))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3)) if uhat else None
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=np.zeros((m.nn, 3)), uhat=uh)
    return o


def test_reference_gradients_against_complex_steps_of_its_value():
    """uhat != 0, the warped quadrilaterals and the triangles, the whole mesh and a selection: 1e-12 of the largest entry (the bar of
    test_ply_failure_cpu.py)."""
    for m in (wing_skin_mesh(3, 4), quads_to_triangles(wing_skin_mesh(3, 4))):
        rng = np.random.default_rng(1)
        o = oracle_of(m, rng)
        tab = random_shear_table(m.nel, 3, rng)
        o.set_ply_shear_table(tab, 3)
        w = 2e-3 * rng.uniform(-1, 1, m.ndof)
        rho = 5.0 / o.field(w).max()
        cells = np.arange(0, m.nel, 2)
        for sel in (None, cells):
            gw, gt = o.gradients(w, rho, cells=sel)
            K = o.value(w, rho, cells=sel)
            shift = rho * o.field(w)[o._cells(sel)].max()
            hstep = 1e-30
            for i in rng.choice(m.ndof, 12, replace=False):
                wc = w.astype(complex); wc[i] += 1j * hstep
                d = o.value(wc, rho, cells=sel, shift=shift).imag / hstep
                assert abs(gw[i] - d) <= 1e-12 * np.abs(gw).max(), i
            for _ in range(24):
                e, p, k = rng.integers(m.nel), rng.integers(3), rng.integers(6)
                tc = tab.astype(complex)
                step = hstep * abs(tab[e, p, k])
                tc[e, p, k] += 1j * step
                d = o.value(w, rho, cells=sel, table=tc, shift=shift).imag / step
                assert abs(gt[e, p, k] - d) <= 1e-12 * np.abs(gt[:, :, k]).max(), (e, p, k)
            assert abs(o.value(w.astype(complex), rho, cells=sel, shift=shift).real - K) <= 1e-13 * abs(K)
            if sel is not None:
                assert np.all(gt[np.setdiff1d(np.arange(m.nel), cells)] == 0.0)
        # the field's reverse product is the same routine with the cotangent in place of the KS weight
        cbar = rng.uniform(-1, 1, (m.nel, 3))
        gw, gt = o.field_vjp(w, cbar)
        for i in rng.choice(m.ndof, 6, replace=False):
            wc = w.astype(complex); wc[i] += 1j * 1e-30
            d = np.sum(cbar * o.field(wc).imag) / 1e-30
            assert abs(gw[i] - d) <= 1e-12 * np.abs(gw).max(), i


def test_shear_table_against_a_hand_written_loop_and_its_angle_derivative():
    G13, G23 = PLY["G13"], PLY["G23"]
    ang = np.array([20.0, -50.0, 75.0, 0.0])
    S = np.array([[6e4, 4e4], [5e4, 3e4], [6e4, 4e4], [7e4, 2e4]])
    F = lm.shear_strength(S[:, 0], S[:, 1])
    assert F.shape == (4, 2) and np.allclose(F, 1.0 / S ** 2, rtol=1e-15, atol=0)
    tab = lm.ply_shear_table(G13, G23, ang, F)
    assert tab.shape == (1, 4, 6)
    for k in range(4):
        c, s = np.cos(np.deg2rad(ang[k])), np.sin(np.deg2rad(ang[k]))
        Gs = np.diag([G13, G23]) @ np.array([[c, s], [-s, c]])
        assert np.allclose(tab[0, k, :4].reshape(2, 2), Gs, rtol=1e-15, atol=1e-9)
        assert np.array_equal(tab[0, k, 4:], [1 / S[k, 0] ** 2, 1 / S[k, 1] ** 2])
    # consistency with clt_from_plies: A_s = K_SHEAR sum_k t_k R^T Gs
    t = np.array([0.01, 0.02, 0.015, 0.01])
    As = lm.clt_from_plies(PLY["E1"], PLY["E2"], PLY["G12"], PLY["nu12"], G13, G23, t, ang)[3][0]
    R = lm._r_shear(ang)
    As2 = lm.K_SHEAR * sum(t[k] * R[k].T @ tab[0, k, :4].reshape(2, 2) for k in range(4))
    assert np.allclose(As, As2, rtol=1e-13)
    # per cell angles, and the derivative per degree against central differences
    rng = np.random.default_rng(0)
    a2 = rng.uniform(-90, 90, (5, 4))
    d = lm.ply_shear_table_dtheta(G13, G23, a2)
    assert d.shape == (5, 4, 2, 2)
    h = 1e-4
    fd = (lm.ply_shear_table(G13, G23, a2 + h, F) - lm.ply_shear_table(G13, G23, a2 - h, F)) / (2 * h)
    assert np.abs(fd[..., :4].reshape(5, 4, 2, 2) - d).max() <= 1e-9 * np.abs(d).max()
    assert np.abs(fd[..., 4:]).max() == 0.0


def test_bounds_of_the_aggregate_and_the_zero_state():
    m = wing_skin_mesh(3, 4)
    rng = np.random.default_rng(2)
    o = oracle_of(m, rng, uhat=False)
    o.set_ply_shear_table(random_shear_table(m.nel, 3, rng), 3)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    mx = o.field(w).max()
    for rho in (1.0 / mx, 100.0 / mx, 1e4 / mx):
        for sel in (None, np.arange(3, 9)):
            K = o.value(w, rho, cells=sel)
            lo, hi = o.bounds(w, rho, cells=sel)
            assert np.isfinite(K) and lo <= K <= hi
    # w = 0: every FI is zero and K = 1/rho log(sum a_e / alpha) = 0 with the reference area (uhat = 0: a_e is the cell's area)
    assert abs(o.value(np.zeros(m.ndof), 100.0)) <= 1e-15
    assert np.all(o.field(np.zeros(m.ndof)) == 0.0)


def strip(nw, nl, t=0.1, p=1.0):
    """Clamped 1 x 10 strip, [0/90/90/0], uniform transverse pressure p: the mesh, the layup's A_s, the shear table with F44 = 0 on
    the 0-degree plies and F55 = 0 on the 90-degree plies (only the gamma_x term counts), and the closed form of the field
    (G p (L - xbar_e) / (A_s00 S))^2 per (cell, ply) with xbar_e the cell's mean x."""
    m = plate_mesh(1.0, 10.0, nw, nl)
    ang = np.array([0.0, 90.0, 90.0, 0.0])
    mat = [np.full(4, PLY[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")]
    A, B, D, As = lm.clt_from_plies(*mat, np.full(4, t), ang)
    S13, S23 = 6e4, 4e4
    F = lm.shear_strength(S13, S23) * np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    tab = np.repeat(lm.ply_shear_table(PLY["G13"], PLY["G23"], ang, F), m.nel, 0)
    xbar = m.nodes[m.cells][:, :, 0].mean(axis=1)
    # 0-degree plies: t13 = G13 gamma_x; 90-degree plies: t23 = -G23 gamma_x
    GS = np.array([PLY["G13"] / S13, PLY["G23"] / S23, PLY["G23"] / S23, PLY["G13"] / S13])
    closed = (GS[None, :] * p * (10.0 - xbar[:, None]) / As[0, 0, 0]) ** 2
    clt = lm.pack(np.repeat(A, m.nel, 0), np.repeat(B, m.nel, 0), np.repeat(D, m.nel, 0), np.repeat(As, m.nel, 0), 12 * D.max())
    return m, clt, tab, closed, (xbar >= 3.0) & (xbar <= 7.0)


def test_strip_field_against_the_closed_form():
    """gamma_x = p (L - x) / A_s00 away from the clamp and the free end.  The reference reaches 5.4e-12 of the closed form on 2 x 20
    cells (1.1e-11 on 2 x 40): the bar is 1e-10."""
    m, clt, tab, closed, far = strip(2, 20)
    f = np.tile([0.0, 0.0, 1.0], (m.nn, 1))
    fields = dict(h=np.full(m.nn, 0.4), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f)
    s = LaminateOracle(m, penalty_facets=m.penalty_facets(CLAMP), beta=BETA)
    s.set_fields(**fields)
    s.set_laminate(clt)
    w = spla.spsolve(s.assemble_K().tocsc(), s.load_vector())
    o = PlyShearOracle(m, nquad=degree4_rule(m))
    o.set_fields(**fields)
    o.set_ply_shear_table(tab, 4)
    fld = o.field(w)
    err = np.abs(fld[far] - closed[far]).max() / np.abs(closed[far]).max()
    print(f"strip 2 x 20, ply t = 0.1: field against the closed form over 3 <= x <= 7: {err:.2e}")
    assert err <= 1e-10
