"""Ply failure aggregate and field of laminated shells on the GPU (femo_set_ply_table, "ply_failure", femo_ply_failure_field) against
the numpy reference tests/ply_failure_ref.py, closed-form identities, central differences with re-solves, and the handling of the
table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh                       # noqa: E402
from oracle.rm_shell_oracle import degree4_rule                                  # noqa: E402
from test_gpu_laminate import BETA, CLAMP, PLY, ROOT_EDGE, _mesh, block_scale, random_laminate, tight   # noqa: E402

pytestmark = pytest.mark.gpu

STRENGTH = dict(Xt=1.5e6, Xc=1.2e6, Yt=5e4, Yc=2e5, S=7e4)
MAT = ("E1", "E2", "G12", "nu12")


def random_table(nel, rng, nply=2, h=0.05):
    """Per cell nply plies of random angles and thicknesses, recovery points at the bottom and top of every ply (npt = 2 nply)."""
    t = h / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    ang = rng.uniform(-90, 90, (nel, nply))
    return lm.ply_table(*[np.full((nel, nply), PLY[k]) for k in MAT], t, ang, lm.tsai_wu(**STRENGTH))


def _pair(kind, bc=None, uhat=True, seed=0, nply=2):
    from femo_alpha_amd.backend import ShellContext
    from ply_failure_ref import PlyFailureOracle
    m = _mesh(kind)
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (m.nn, 3))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3)) if uhat else None
    clt = random_laminate(m.nel, rng)
    tab = random_table(m.nel, rng, nply)
    o = PlyFailureOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f, uhat=uh)
    o.set_ply_table(tab, 2 * nply)
    c = ShellContext(m)
    for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=f).items():
        c.set_field(k, v)
    if uh is not None:
        c.set_field("uhat", uh)
    if bc == "penalty":
        c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_table(tab)
    return m, o, c, rng, clt, tab


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("kind", ["warped", "tri", "quad CG1CG1", "tri CG2CR1"])
def test_field_value_and_partials_against_the_reference(kind, sub):
    """uhat != 0, a random state; whole mesh with the reference area, or a tagged sub-domain with a given alpha.  1e-11 relative to the
    largest entry (the operator-level bar); for the scalar K the yardstick is the largest failure index."""
    m, o, c, rng, _, tab = _pair(kind)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    rho = 30.0
    c.set_state(w)
    c.set_ply_failure_params(rho)
    cells, alpha = None, None
    if sub:
        tags = (np.arange(m.nel) % 3).astype(np.int32)
        c.set_cell_tags(tags, 3)
        c.select_subdomain(1)
        alpha = 2.5
        c.set_stress_alpha(alpha, 1)
        cells = np.where(tags == 1)[0]
    fr = o.field(w)
    fg = c.ply_failure_field()
    print(f"{kind} sub={sub}: max FI {np.abs(fr).max():.3e}")
    assert fg.shape == fr.shape and np.abs(fg - fr).max() <= 1e-11 * np.abs(fr).max()
    Kr = o.value(w, rho, alpha=alpha, cells=cells)
    K = c.functional("ply_failure")
    print(f"  K {K:.15e} reference {Kr:.15e}")
    assert abs(K - Kr) <= 1e-11 * np.abs(fr).max()
    gwr, gtr = o.gradients(w, rho, cells=cells)
    gw = c.dfunctional("ply_failure", "disp_solid")
    gt = c.dfunctional("ply_failure", "ply_table").reshape(gtr.shape)
    print(f"  dK/dw {np.abs(gw - gwr).max() / np.abs(gwr).max():.2e}  dK/dtable (per entry kind) "
          f"{max(np.abs(gt[..., k] - gtr[..., k]).max() / np.abs(gtr[..., k]).max() for k in range(16)):.2e}")
    assert np.abs(gw - gwr).max() <= 1e-11 * np.abs(gwr).max()
    for k in range(16):          # the 16 entries of a point have different units: each against its own largest
        assert np.abs(gt[..., k] - gtr[..., k]).max() <= 1e-11 * np.abs(gtr[..., k]).max(), k
    for name in ("laminate", "thickness", "E", "nu", "density", "F_solid"):
        assert not np.any(c.dfunctional("ply_failure", name))
    c.close()


def test_isotropic_ply_field_is_the_squared_von_mises_ratio():
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
    fg = c.ply_failure_field()
    for p, zf in ((0, -0.5), (1, 0.5)):
        ref = ((o.von_mises_top(w, zf=zf)[0] / X) ** 2).max(axis=1)
        assert np.abs(fg[:, p] - ref).max() <= 1e-11 * ref.max()
    c.close()


def test_large_exponent_stays_finite_within_the_bounds_and_repeats_bit_for_bit():
    m, o, c, rng, _, tab = _pair("warped", uhat=False)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    fi = o.field(w)
    s = 1e3 / np.abs(fi).max()                 # failure indices of order 1e3: scale the quadratic and the linear coefficients
    tab = tab.copy(); tab[:, :, 10:12] *= s; tab[:, :, 12:16] *= s
    c.set_field("ply_table", tab)
    o.set_ply_table(tab, 4)
    rho = 1e4
    c.set_ply_failure_params(rho)
    K = c.functional("ply_failure")
    lo, hi = o.bounds(w, rho)
    print(f"rho = 1e4: max FI {np.abs(o.field(w)).max():.3e}, K {K:.6e} in [{lo:.6e}, {hi:.6e}]")
    assert np.isfinite(K) and lo <= K <= hi
    Kr = o.value(w, rho)
    assert abs(K - Kr) <= 1e-11 * abs(hi)
    calls = [lambda: np.array([c.functional("ply_failure")]), lambda: c.dfunctional("ply_failure", "disp_solid"),
             lambda: c.dfunctional("ply_failure", "ply_table"), lambda: c.ply_failure_field()]
    for call in calls:
        a, b = call(), call()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    # w = 0 with F1 = F2 = 0: K = 0
    tab0 = tab.copy(); tab0[:, :, 10:12] = 0.0
    c.set_field("ply_table", tab0)
    c.set_state(np.zeros(m.ndof))
    assert abs(c.functional("ply_failure")) <= 1e-15
    c.close()


def _pipeline(m, t, ang, c_drill):
    """Laminate and recovery points of the same plies."""
    nel, nply = t.shape
    mat = [np.full((nel, nply), PLY[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")]
    clt, dclt = lm.clt_from_plies(*mat, t, ang, jacobian=True)
    tab, dz = lm.ply_table(*mat[:4], t, ang, lm.tsai_wu(**STRENGTH), jacobian=True)
    return lm.pack(*clt, c_drill), tab, dclt, dz


def test_total_gradients_against_central_differences_with_re_solves():
    from femo_alpha_amd.backend import ShellContext
    m = _mesh("warped")
    rng = np.random.default_rng(6)
    nply = 2
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (m.nel, nply)))
    ang = rng.uniform(-90, 90, (m.nel, nply))
    clt, tab, dclt, dz = _pipeline(m, t, ang, 50.0)
    f = rng.uniform(-1, 1, (m.nn, 3))
    c = ShellContext(m)
    for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=f, uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE), BETA)
    c.set_laminate(clt)
    c.set_ply_table(tab)
    tight(c)

    def solved():
        c.solve_state(True)
        return c.functional("ply_failure")
    solved()
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())        # rho FI of order 5: every point contributes
    solved()
    gl = c.total_gradient("ply_failure", "laminate")[0].reshape(m.nel, 32)
    bar = lambda g, fd, G: abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()
    for e, k in [(0, 0), (5, 10), (7, 13), (2, 18), (3, 22), (4, 27), (1, 31)]:
        d = clt.copy()
        s = 1e-5 * block_scale(clt, e, k)
        d[e, k] += s; c.set_laminate(d); jp = solved()
        d[e, k] -= 2 * s; c.set_laminate(d); jm = solved()
        c.set_laminate(clt)
        assert bar(gl[e, k], (jp - jm) / (2 * s), gl), ("laminate", e, k)
    solved()
    gt = c.total_gradient("ply_failure", "ply_table")[0].reshape(tab.shape)
    assert np.array_equal(gt, c.dfunctional("ply_failure", "ply_table").reshape(tab.shape))      # the explicit partial alone
    # at the three recovery points with the largest failure index: elsewhere the aggregate moves by less than its own rounding
    # (K carries ~1e-16 / rho of noise) under a step small enough for a central difference
    fld = c.ply_failure_field()
    top = [np.unravel_index(i, fld.shape) for i in np.argsort(fld.ravel())[::-1][:3]]
    for (e, p), k in zip(top * 3, [0, 4, 8, 9, 10, 12, 14, 15, 2]):
        d = tab.copy()
        # K carries ~1e-18 of rounding (1e-16 of S over rho ~ 5e3), so a difference must reach ~1e-12 to be read to 1e-6; FI moves
        # by at most 2e-4 of itself under this step, which leaves (rho dFI)^2 / 6 < 2e-7 of truncation
        s = 1e-4 * np.abs(tab[:, :, k]).max()
        d[e, p, k] += s; c.set_field("ply_table", d); jp = c.functional("ply_failure")
        d[e, p, k] -= 2 * s; c.set_field("ply_table", d); jm = c.functional("ply_failure")
        c.set_field("ply_table", tab)
        assert bar(gt[e, p, k], (jp - jm) / (2 * s), gt[:, :, k]), ("ply_table", e, p, k)
    gf = c.total_gradient("ply_failure", "F_solid")[0]
    f0 = c.get_field("F_solid")
    for i in (4, 31, 77):
        s = 1e-5
        x = f0.copy(); x[i] += s; c.set_field("F_solid", x); jp = solved()
        x[i] -= 2 * s; c.set_field("F_solid", x); jm = solved()
        c.set_field("F_solid", f0)
        assert bar(gf[i], (jp - jm) / (2 * s), gf), ("F_solid", i)
    # the ply-thickness chain through both inputs
    solved()
    dlam = lm.pack(dclt[0].reshape(-1, 3, 3), dclt[1].reshape(-1, 3, 3), dclt[2].reshape(-1, 3, 3), dclt[3].reshape(-1, 2, 2),
                   0.0).reshape(m.nel, nply, 32)
    g_t = np.einsum("ep,pj->ej", gt[:, :, 9], dz) + np.einsum("ek,ejk->ej", gl, dlam)
    for e, j in [(0, 0), (3, 1), (8, 0), (11, 1)]:
        s = 1e-4 * t[e, j]           # a re-solved K repeats to ~5e-18: the difference must reach ~1e-11 to be read at the bar
        vals = []
        for sg in (1, -1):
            tt = t.copy(); tt[e, j] += sg * s
            cl, tb, _, _ = _pipeline(m, tt, ang, 50.0)
            c.set_laminate(cl); c.set_field("ply_table", tb)
            vals.append(solved())
        assert bar(g_t[e, j], (vals[0] - vals[1]) / (2 * s), g_t), ("t", e, j)
    c.close()


def test_grouped_totals_equal_the_separate_ones():
    m, o, c, rng, clt, tab = _pair("warped", bc="penalty")
    c.use_direct_solver()
    tags = (np.arange(m.nel) % 3).astype(np.int32)
    c.set_cell_tags(tags, 3)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    names, subs = ["compliance", "ply_failure", "elastic_energy", "ply_failure"], [-1, -1, -1, 1]
    G = c.total_gradients(names, "laminate", subdomains=subs)[0]
    for i, (n, s) in enumerate(zip(names, subs)):
        c.select_subdomain(s)
        g = c.total_gradient(n, "laminate")[0]
        assert np.abs(G[i] - g).max() <= 1e-10 * np.abs(g).max(), (n, s)
    c.select_subdomain(-1)
    c.close()


def test_table_handling_and_refusals():
    from femo_alpha_amd._lib import FemoHipError
    from femo_alpha_amd.backend import ShellContext
    m = plate_mesh(2.0, 10.0, 4, 20)
    rng = np.random.default_rng(4)
    clt, tab = random_laminate(m.nel, rng), random_table(m.nel, rng)
    c = ShellContext(m)
    for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.use_direct_solver()
    assert c.lib.femo_field_size(c._h, b"ply_table") == -1
    with pytest.raises(FemoHipError, match="laminate mode"):
        c.set_ply_table(tab)
    c.set_laminate(clt)
    for call in (lambda: c.functional("ply_failure"), lambda: c.dfunctional("ply_failure", "disp_solid"), lambda: c.ply_failure_field(),
                 lambda: c.total_gradient("ply_failure", "laminate"), lambda: c.total_gradients(["compliance", "ply_failure"], "laminate"),
                 lambda: c.set_field("ply_table", tab)):
        with pytest.raises(FemoHipError, match="femo_set_ply_table"):
            call()
    with pytest.raises(FemoHipError, match="npt must be 1..32"):
        c.set_ply_table(np.zeros((m.nel, 33, 16)))
    with pytest.raises(FemoHipError, match="npt must be 1..32"):
        c.set_ply_table(np.zeros(0), npt=0)
    with pytest.raises(FemoHipError, match=r"x 4 points x 80 cells = 5120, got 5104"):
        c.set_ply_table(tab.ravel()[:-16], npt=4)
    bad = tab.copy(); bad[7, 2, 9] = np.inf
    with pytest.raises(FemoHipError, match="value 9 of recovery point 2 of cell 7 is not finite"):
        c.set_ply_table(bad)
    with pytest.raises(FemoHipError, match="rho must be finite and > 0"):
        c.set_ply_failure_params(0.0)
    # the context is still usable; setting a table does not trigger a re-factorisation
    c.solve_state(True)
    w, info = c.get_state(), c.frontal_info()
    c.set_ply_table(tab)
    assert c.field_size("ply_table") == tab.size and np.array_equal(c.get_field("ply_table"), tab.ravel())
    c.solve_state(True)
    assert c.frontal_info() == info              # the measured times of the one factorisation: no second one has replaced them
    assert np.abs(c.get_state() - w).max() <= 1e-12 * np.abs(w).max()
    K = c.functional("ply_failure")
    assert np.isfinite(K)
    for call in (lambda: c.dfunctional("ply_failure", "uhat"), lambda: c.total_gradient("ply_failure", "uhat"),
                 lambda: c.total_gradients(["ply_failure"], "uhat")):
        with pytest.raises(FemoHipError, match="shape derivative"):
            call()
    assert c.functional("ply_failure") == K
    # the table survives new laminate values and goes with the laminate
    c.set_field("laminate", clt * 1.01)
    assert c.field_size("ply_table") == tab.size and np.array_equal(c.get_field("ply_table"), tab.ravel())
    c.set_ply_table(None)
    assert c.lib.femo_field_size(c._h, b"ply_table") == -1
    c.set_ply_table(tab)
    c.set_laminate(None)
    assert c.lib.femo_field_size(c._h, b"ply_table") == -1
    with pytest.raises(FemoHipError, match="femo_set_ply_table"):
        c.functional("ply_failure")
    c.close()


@pytest.mark.parametrize("renumber", [False, True])
def test_reverse_mode_through_the_model_matches_the_backend_totals(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel = mesh.nn, mesh.nel
    rng = np.random.default_rng(8)
    clt, tab = random_laminate(nel, rng), random_table(nel, rng)
    tab[:, :, 10:12] *= 1e-3; tab[:, :, 12:16] *= 1e-6           # failure indices of order one under this load
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    pressure = csdl.Variable(value=np.tile([0.5, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=0.05 * np.ones(nn), name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=np.ones(nn), name="density")
    node_disp = csdl.Variable(value=np.zeros((nn, 3)), name="node_disp")
    lam = csdl.Variable(value=clt, name="laminate")
    ply = csdl.Variable(value=tab.reshape(nel, -1), name="ply_table")
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, ply_failure=4, rho=20)
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, laminate=lam, ply_table=ply)
    recorder.stop()
    ctx = model.shell_pde.ctx
    assert np.array_equal(ctx.get_field("ply_table").reshape(nel, -1), tab.reshape(nel, -1)[model.cell_of_new])
    for var, arg, width in ((lam, "laminate", 32), (ply, "ply_table", 64)):
        got = np.asarray(recorder.compute_totals(out.ply_failure, var)).reshape(nel, width)
        ref = np.empty((nel, width))
        ref[model.cell_of_new] = ctx.total_gradient("ply_failure", arg)[0].reshape(nel, width)     # solver order -> caller order
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), arg
    with pytest.raises(ValueError):
        model.evaluate(pressure, thickness, E, nu, density, node_disp, laminate=lam)
    with pytest.raises(ValueError):
        RMShellModel(mesh, shell_bc_func=CLAMP, record=False, ply_failure=4)


def test_full_size_bounds_and_a_directional_derivative():
    """wing1m with the isotropic-equivalent laminate split into 8 plies (npt = 16): the bounds of K against the field, and the
    derivative of K along a random laminate direction by central differences with re-solves."""
    from bench import make_workload
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, _ = make_workload("wing1m")
    rng = np.random.default_rng(11)
    h = 1.27e-3 * (1 + 0.2 * rng.uniform(-1, 1, m.nel))
    E, nu = float(fields["E"][0]), float(fields["nu"][0])
    X = 3e8
    nply = 8
    col = lambda v: np.full((m.nel, nply), v)
    tab = lm.ply_table(col(E), col(E), col(E / 2 / (1 + nu)), col(nu), h[:, None] / nply * np.ones((1, nply)), col(0.0),
                       lm.tsai_wu(X, X, X, X, X / np.sqrt(3.0)))
    clt = lm.isotropic(h, E, nu)
    c = ShellContext(m, element_wise_material=True)
    for k, v in dict(fields, thickness=h).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.set_laminate(clt)
    c.set_ply_table(tab)
    c.use_direct_solver(rtol=1e-13)
    c.solve_state(True)
    fld = c.ply_failure_field()
    assert fld.shape == (m.nel, 16) and np.all(np.isfinite(fld))
    mx = fld.max()
    rho = 20.0 / mx
    c.set_ply_failure_params(rho)
    K = c.functional("ply_failure")
    # w det at the points of the degree-4 rule from the oracle's geometry (uhat = 0 in this workload: J = 1)
    from ply_failure_ref import PlyFailureOracle
    o = PlyFailureOracle(m, element_wise_material=True, nquad=degree4_rule(m))
    wd = np.concatenate([o.wts[None, :] * o._geometry(sl, o.N1, o.dN1)["det"] for sl in o._chunks()])
    lo = mx + np.log(wd.min() / (wd.sum() * 16)) / rho
    print(f"wing1m: max FI {mx:.4e}, rho {rho:.4e}, K {K:.6e} in [{lo:.6e}, {mx:.6e}]")
    assert lo <= K <= mx
    g = c.total_gradient("ply_failure", "laminate")[0].reshape(m.nel, 32)
    d = clt * rng.uniform(-1, 1, (m.nel, 1))                     # a random scaling of every cell's laminate
    s = 1e-5
    vals = []
    for sg in (1, -1):
        c.set_laminate(clt + sg * s * d)
        c.solve_state(True)
        vals.append(c.functional("ply_failure"))
    fd = (vals[0] - vals[1]) / (2 * s)
    gd = float(np.sum(g * d))
    print(f"  directional derivative {gd:.8e}, central difference {fd:.8e}")
    assert abs(gd - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(g * d).max()
    c.close()
