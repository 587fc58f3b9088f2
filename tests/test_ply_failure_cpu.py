"""Ply failure outputs without a GPU: the numpy reference (tests/ply_failure_ref.py) tied to the oracle's von Mises recovery, its
derivatives against complex steps of its own value, the bounds of the aggregate, and the host helpers ``laminate.tsai_wu`` /
``laminate.ply_table``."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import ShellMesh, plate_mesh, wing_skin_mesh            # noqa: E402
from oracle.rm_shell_oracle import ShellOracle, degree4_rule                     # noqa: E402
from ply_failure_ref import PlyFailureOracle                                     # noqa: E402

PLY = dict(E1=1.35e8, E2=1.0e7, G12=5e6, nu12=0.3)
STRENGTH = dict(Xt=1.5e6, Xc=1.2e6, Yt=5e4, Yc=2e5, S=7e4)


def random_plies(nel, nply, rng, h=0.05):
    t = h / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    ang = rng.uniform(-90, 90, (nel, nply))
    return t, ang


def table_of(t, ang, f12=-0.5):
    nel, nply = t.shape
    mat = [np.full((nel, nply), PLY[k]) for k in ("E1", "E2", "G12", "nu12")]
    return lm.ply_table(*mat, t, ang, lm.tsai_wu(f12=f12, **STRENGTH))


def oracle_of(m, rng, uhat=True):
    o = PlyFailureOracle(m, nquad=degree4_rule(m))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3)) if uhat else None
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=np.zeros((m.nn, 3)), uhat=uh)
    return o


def test_isotropic_ply_gives_the_squared_von_mises_ratio_of_the_oracle():
    """One isotropic ply, Xt = Xc = Yt = Yc = X, S = X / sqrt(3), f12 = -1/2: FI at z = -+h/2 is (vm / X)^2 with vm the oracle's
    von_mises_top(zf = -+1/2) on an element-wise-material oracle (no thickness-gradient term)."""
    m = wing_skin_mesh(4, 8)
    rng = np.random.default_rng(0)
    h = 0.05 * (1 + 0.3 * rng.uniform(-1, 1, m.nel))
    E, nu, X = 1e8, 0.3, 3e5
    F = lm.tsai_wu(X, X, X, X, X / np.sqrt(3.0))
    assert np.allclose(F, [0, 0, 1 / X ** 2, 1 / X ** 2, 3 / X ** 2, -0.5 / X ** 2], rtol=1e-14, atol=0)
    col = lambda v: np.full((m.nel, 1), v)
    tab = lm.ply_table(col(E), col(E), col(E / 2 / (1 + nu)), col(nu), h[:, None], col(0.0), F)
    assert tab.shape == (m.nel, 2, 16) and np.allclose(tab[:, 0, 9], -h / 2) and np.allclose(tab[:, 1, 9], h / 2)
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    fields = dict(h=h, E=np.full(m.nel, E), nu=np.full(m.nel, nu), rho=np.ones(m.nel), f=np.zeros((m.nn, 3)), uhat=uh)
    o = PlyFailureOracle(m, element_wise_material=True, nquad=degree4_rule(m))
    o.set_fields(**fields)
    o.set_ply_table(tab, 2)
    w = rng.uniform(-1, 1, m.ndof)
    fi = o.failure_index(w)[0]
    for p, zf in ((0, -0.5), (1, 0.5)):
        vm = o.von_mises_top(w, zf=zf)[0]
        ref = (vm / X) ** 2
        assert np.abs(fi[:, :, p] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_ply_table_against_a_hand_written_loop_and_its_thickness_jacobian():
    E1, E2, G12, nu12 = (PLY[k] for k in ("E1", "E2", "G12", "nu12"))
    t = np.array([0.010, 0.025, 0.015])
    ang = np.array([20.0, -50.0, 75.0])
    F = lm.tsai_wu(**STRENGTH)
    tab, dz = lm.ply_table(E1, E2, G12, nu12, t, ang, F, jacobian=True)
    assert tab.shape == (1, 6, 16) and dz.shape == (6, 3)
    nu21 = nu12 * E2 / E1
    den = 1 - nu12 * nu21
    Q = np.array([[E1 / den, nu12 * E2 / den, 0], [nu12 * E2 / den, E2 / den, 0], [0, 0, G12]])
    H = t.sum()
    zb = -H / 2
    for k in range(3):
        c, s = np.cos(np.deg2rad(ang[k])), np.sin(np.deg2rad(ang[k]))
        T = np.array([[c * c, s * s, c * s], [s * s, c * c, -c * s], [-2 * c * s, 2 * c * s, c * c - s * s]])
        for j, z in enumerate((zb, zb + t[k])):
            row = tab[0, 2 * k + j]
            assert np.allclose(row[:9].reshape(3, 3), Q @ T, rtol=1e-14, atol=0)
            assert abs(row[9] - z) <= 1e-16 and np.array_equal(row[10:], F)
        zb += t[k]
    # consistency with clt_from_plies: A = sum_k Qbar_k t_k with Qbar = T^T Q T = T^T G
    A = lm.clt_from_plies(E1, E2, G12, nu12, G12, G12, t, ang)[0][0]
    Tm = lm._t_eps(ang)
    A2 = sum(Tm[k].T @ tab[0, 2 * k, :9].reshape(3, 3) * t[k] for k in range(3))
    assert np.allclose(A, A2, rtol=1e-13)
    # thickness Jacobian: only z moves
    for j in range(3):
        d = 1e-6
        tp, tm_ = t.copy(), t.copy()
        tp[j] += d; tm_[j] -= d
        fd = (lm.ply_table(E1, E2, G12, nu12, tp, ang, F) - lm.ply_table(E1, E2, G12, nu12, tm_, ang, F)) / (2 * d)
        assert np.abs(fd[0, :, 9] - dz[:, j]).max() <= 1e-9
        assert np.abs(np.delete(fd[0], 9, axis=1)).max() == 0.0
    mid = lm.ply_table(E1, E2, G12, nu12, t, ang, F, surfaces=("mid",))
    assert np.allclose(mid[0, :, 9], 0.5 * (tab[0, 0::2, 9] + tab[0, 1::2, 9]))


def test_failure_index_follows_the_frame_on_a_flat_plate():
    """Every ply turned by -90 degrees together with a shift of every cell's vertex list by one (E0 turns by +90 degrees): the same
    structure, the same state, the same failure indices."""
    m1 = plate_mesh(2.0, 10.0, 3, 6)
    m2 = ShellMesh(m1.nodes, np.roll(m1.cells, -1, axis=1))
    rng = np.random.default_rng(3)
    t, ang = random_plies(m1.nel, 3, rng)
    w = rng.uniform(-1, 1, m1.ndof)
    # same nodal values on both meshes: vertices are shared, the P2 numbering is the mesh's own -- carry the state by coordinates
    def p2_xyz(m):
        X = np.zeros((m.nP2, 3))
        ref = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1], [0, -1], [1, 0], [0, 1], [-1, 0], [0, 0]], float)
        N = 0.25 * (1 + ref[:, :1] * np.array([-1, 1, 1, -1.0])[None]) * (1 + ref[:, 1:] * np.array([-1, -1, 1, 1.0])[None])
        for e in range(m.nel):
            X[m.cell_p2[e]] = N @ m.nodes[m.cells[e]]
        return X
    X1, X2 = p2_xyz(m1), p2_xyz(m2)
    key = lambda X: [tuple(np.round(r, 9)) for r in X]
    pos = {k: i for i, k in enumerate(key(X1))}
    perm = np.array([pos[k] for k in key(X2)])
    w2 = w.copy()
    w2[: m1.ndof_u] = w[: m1.ndof_u].reshape(-1, 3)[perm].ravel()
    out = []
    for m, a, ww in ((m1, ang, w), (m2, ang - 90.0, w2)):
        o = oracle_of(m, rng, uhat=False)
        o.set_ply_table(table_of(t, a), 6)
        out.append(o.field(ww))
    assert np.abs(out[1] - out[0]).max() <= 1e-10 * np.abs(out[0]).max()


def test_reference_gradients_against_complex_steps_of_its_value():
    m = wing_skin_mesh(3, 4)
    rng = np.random.default_rng(1)
    o = oracle_of(m, rng)
    t, ang = random_plies(m.nel, 2, rng)
    tab = table_of(t, ang)
    o.set_ply_table(tab, 4)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    rho = 30.0
    cells = np.arange(0, m.nel, 2)
    for sel in (None, cells):
        gw, gt = o.gradients(w, rho, cells=sel)
        K = o.value(w, rho, cells=sel)
        shift = rho * o.failure_index(w)[0][o._cells(sel)].max()
        hstep = 1e-30
        for i in rng.choice(m.ndof, 12, replace=False):
            wc = w.astype(complex); wc[i] += 1j * hstep
            d = o.value(wc, rho, cells=sel, shift=shift).imag / hstep
            assert abs(gw[i] - d) <= 1e-12 * np.abs(gw).max(), i
        for _ in range(24):
            e, p, k = rng.integers(m.nel), rng.integers(4), rng.integers(16)
            tc = tab.astype(complex)
            step = hstep * max(abs(tab[e, p, k]), 1e-12)
            tc[e, p, k] += 1j * step
            d = o.value(w, rho, cells=sel, table=tc, shift=shift).imag / step
            scale = np.abs(gt[:, :, k]).max()
            assert abs(gt[e, p, k] - d) <= 1e-12 * scale, (e, p, k)
        assert abs(o.value(w.astype(complex), rho, cells=sel, shift=shift).real - K) <= 1e-13 * abs(K)
        if sel is not None:
            off = np.setdiff1d(np.arange(m.nel), cells)
            assert np.all(gt[off] == 0.0)


def test_bounds_of_the_aggregate_and_the_zero_state():
    m = wing_skin_mesh(3, 4)
    rng = np.random.default_rng(2)
    o = oracle_of(m, rng, uhat=False)
    t, ang = random_plies(m.nel, 2, rng)
    o.set_ply_table(table_of(t, ang), 4)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    for rho in (1.0, 100.0, 1e4):
        for sel, alpha in ((None, None), (np.arange(3, 9), None), (None, 7.5)):
            K = o.value(w, rho, alpha=alpha, cells=sel)
            lo, hi = o.bounds(w, rho, alpha=alpha, cells=sel)
            if alpha is None:
                assert lo <= K <= hi
            else:                       # a given alpha moves both bounds together
                a0 = o.area(sel)
                assert lo <= K <= hi + np.log(a0 / alpha) / rho + 1e-15
            assert np.isfinite(K)
    # w = 0 with F1 = F2 = 0: every FI is zero and K = 1/rho log(area / alpha) = 0 with the reference area
    tab = o.ply.copy()
    tab[:, :, 10:12] = 0.0
    o.set_ply_table(tab, 4)
    assert abs(o.value(np.zeros(m.ndof), 100.0)) <= 1e-15
    assert np.all(o.field(np.zeros(m.ndof)) == 0.0)
