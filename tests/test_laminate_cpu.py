"""CPU checks of the laminate layer: classical lamination theory (femo_alpha_amd.laminate) against closed forms, its thickness
Jacobian against central differences, the in-plane rotation, and the CPU laminate reference (tests/laminate_ref.py) against the
single-layer oracle.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                     # noqa: E402

CFRP = dict(E1=135e9, E2=10e9, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)


def plies(angles, t=1.25e-4, **mat):
    p = dict(CFRP, **mat)
    n = len(angles)
    return lm.clt_from_plies(*(np.full(n, p[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")), np.full(n, t), np.asarray(angles, float))


def test_one_isotropic_ply_is_the_single_layer_law():
    E, nu, h = 7e10, 0.33, 2e-3
    G = E / 2 / (1 + nu)
    A, B, D, As = lm.clt_from_plies([E], [E], [G], [nu], [G], [G], [h], [30.0])     # any angle: isotropic
    C = E / (1 - nu ** 2) * np.array([[1, nu, 0], [nu, 1, 0], [0, 0, 0.5 * (1 - nu)]])
    assert np.allclose(A[0], h * C, rtol=1e-14, atol=1e-14 * E * h)
    assert np.abs(B).max() <= 1e-14 * E * h * h
    assert np.allclose(D[0], h ** 3 / 12 * C, rtol=1e-13, atol=1e-14 * E * h ** 3)
    assert np.allclose(As[0], 0.833 * G * h * np.eye(2), rtol=1e-14, atol=1e-14 * G * h)


def test_symmetric_layup_has_no_coupling():
    A, B, D, As = plies([0, 45, -45, 90, 90, -45, 45, 0])
    assert np.abs(B).max() <= 1e-12 * np.abs(A).max() * 1e-3


def test_cross_ply_coupling_in_closed_form():
    t = 1.25e-4
    A, B, D, As = plies([0, 90], t=t)
    p = CFRP
    den = 1 - p["nu12"] ** 2 * p["E2"] / p["E1"]
    Q11, Q22 = p["E1"] / den, p["E2"] / den
    # ply 0 at z in [-t, 0], ply 90 at [0, t]; the strain at height z is eps - z kappa, so B = -int z Qbar dz:
    # B11 = -1/2 (Q11 (0 - t^2) + Q22 (t^2 - 0)) = (Q11 - Q22) t^2 / 2
    assert np.isclose(B[0, 0, 0], 0.5 * (Q11 - Q22) * t * t, rtol=1e-13)
    assert np.isclose(B[0, 1, 1], -B[0, 0, 0], rtol=1e-13)
    assert abs(B[0, 0, 1]) <= 1e-12 * abs(B[0, 0, 0]) and abs(B[0, 2, 2]) <= 1e-12 * abs(B[0, 0, 0])


def test_angle_ply_pair_has_no_a16_but_b16():
    A, B, D, As = plies([30, -30])
    assert abs(A[0, 0, 2]) <= 1e-12 * A[0, 0, 0] and abs(A[0, 1, 2]) <= 1e-12 * A[0, 0, 0]
    assert abs(B[0, 0, 2]) > 1e-3 * abs(A[0, 0, 0]) * 1.25e-4


def test_thickness_jacobian_against_central_differences():
    rng = np.random.default_rng(3)
    nel, nply = 3, 4
    t = 1e-4 * (1 + rng.uniform(0, 1, (nel, nply)))
    ang = rng.uniform(-90, 90, (nel, nply))
    mat = [np.full((nel, nply), CFRP[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")]
    _, jac = lm.clt_from_plies(*mat, t, ang, jacobian=True)
    for j in range(nply):
        dt = 1e-7 * t[:, j].mean()
        tp, tm = t.copy(), t.copy()
        tp[:, j] += dt; tm[:, j] -= dt
        fp, fm = lm.clt_from_plies(*mat, tp, ang), lm.clt_from_plies(*mat, tm, ang)
        for k in range(4):
            fd = (fp[k] - fm[k]) / (2 * dt)
            scale = np.abs(jac[k]).max()
            assert np.abs(jac[k][:, j] - fd).max() <= 1e-8 * scale, (j, k)


def test_rotation_by_a_full_turn_and_by_the_ply_angles():
    clt = plies([0, 35, -60, 90])
    back = lm.rotate_clt(clt, 360.0)
    for a, b in zip(clt, back):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max() + 1e-300
    turned = lm.rotate_clt(clt, -90.0)
    ref = plies([-90, -55, -150, 0])
    for a, b in zip(turned, ref):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def test_pack_applies_the_reference_drilling_default():
    A, B, D, As = plies([0, 90])
    p = lm.pack(np.repeat(A, 4, 0), np.repeat(B, 4, 0), np.repeat(D, 4, 0), np.repeat(As, 4, 0))
    assert p.shape == (4, 32)
    assert np.all(p[:, 31] == 12 * D.max())
    A2, B2, D2, As2, cd = lm.unpack(p)
    assert np.array_equal(A2[0], A[0]) and np.array_equal(B2[1], B[0]) and np.array_equal(As2[2], As[0])


@pytest.mark.parametrize("kind", ["warped quads", "triangles CG2CR1"])
def test_laminate_reference_reproduces_the_single_layer_oracle(kind):
    from laminate_ref import LaminateOracle
    from femo_alpha_amd.mesh import ShellMesh, quads_to_triangles, wing_skin_mesh
    from oracle.rm_shell_oracle import ShellOracle
    m = wing_skin_mesh(4, 6)
    if kind != "warped quads":
        t = quads_to_triangles(m)
        m = ShellMesh(t.nodes, t.cells, "CG2CR1")
    rng = np.random.default_rng(1)
    h = 0.01 * (1 + 0.3 * rng.uniform(-1, 1, m.nel))
    E = 7e10 * (1 + 0.2 * rng.uniform(-1, 1, m.nel))
    nu = 0.3 + 0.05 * rng.uniform(-1, 1, m.nel)
    uhat = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    o = ShellOracle(m, element_wise_material=True)
    o.set_fields(h=h, E=E, nu=nu, uhat=uhat)
    lo = LaminateOracle(m, element_wise_material=True)
    lo.set_fields(h=h, E=E, nu=nu, uhat=uhat)
    lo.set_laminate(lm.isotropic(h, E, nu))
    K0, K1 = o.element_matrices(), lo.element_matrices()
    assert np.abs(K1 - K0).max() <= 1e-13 * np.abs(K0).max()


def test_offset_single_layer_is_the_reference_bottom_layer():
    """The reference's single layer on top of its reference surface (getSingleLayerCLT with BOT, linear_shell_model.py:147-151):
    A = h C, B = -h^2/2 C, D = h^3/3 C -- one isotropic ply moved by the documented offset transform, o = h / 2."""
    E, nu, h = 7e10, 0.33, 2e-3
    G = E / 2 / (1 + nu)
    clt = lm.clt_from_plies([E], [E], [G], [nu], [G], [G], [h], [0.0])
    A, B, D, As = lm.offset(clt, 0.5 * h)
    C = E / (1 - nu ** 2) * np.array([[1, nu, 0], [nu, 1, 0], [0, 0, 0.5 * (1 - nu)]])
    assert np.allclose(A[0], h * C, rtol=1e-14, atol=0)
    assert np.allclose(B[0], -h ** 2 / 2 * C, rtol=1e-13, atol=1e-14 * E * h * h)
    assert np.allclose(D[0], h ** 3 / 3 * C, rtol=1e-13, atol=1e-14 * E * h ** 3)


def test_coupling_sign_follows_the_through_thickness_strain():
    """B against the energy integrated through the thickness: 1/2 int (eps - z kappa).Qbar (eps - z kappa) dz, plies bottom to top."""
    rng = np.random.default_rng(7)
    angles, t = [0.0, 90.0, 30.0], np.array([1e-4, 2e-4, 1.5e-4])
    n = len(angles)
    mat = [np.full(n, CFRP[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")]
    A, B, D, _ = lm.clt_from_plies(*mat, t, np.asarray(angles))
    Qb, _ = lm.ply_stiffness(*mat, np.asarray(angles))
    eps, kap = rng.uniform(-1, 1, 3) * 1e-3, rng.uniform(-1, 1, 3)
    z = np.concatenate([[0.0], np.cumsum(t)]) - 0.5 * t.sum()
    xg, wg = np.polynomial.legendre.leggauss(4)
    energy = 0.0
    for k in range(n):
        zq = 0.5 * (z[k] + z[k + 1]) + 0.5 * (z[k + 1] - z[k]) * xg
        for zz, ww in zip(zq, 0.5 * (z[k + 1] - z[k]) * wg):
            s = eps - zz * kap
            energy += 0.5 * ww * s @ Qb[k] @ s
    packed = 0.5 * (eps @ A[0] @ eps + eps @ B[0] @ kap + kap @ B[0] @ eps + kap @ D[0] @ kap)
    assert abs(packed - energy) <= 1e-12 * abs(energy)
