"""Max-displacement KS aggregate over the transient history (the lpc example's max_disp = csdl.maximum(csdl.absolute(s W), rho) / s,
ex_lpc_gust_response_opt.py:457-459, 770-772) and the tip displacement history (reference plate_sim.py:22-23, 323-328), on the GPU:
value, per-level values, partials and totals against the numpy restatement (tests/disp_history_ref.py), the host route and finite
differences; bitwise repeatability, the seeded adjoint, the untouched march state, errors; the tip probe against the downloaded
history; BASELINE config 5 against its golden."""
import os

import numpy as np
import pytest

import disp_history_ref as R
from femo_alpha_amd import csdl
from femo_alpha_amd.mesh import plate_mesh

pytestmark = pytest.mark.gpu

E, NU, RHO, DT, N = 1e8, 0.3, 10.0, 0.01, 12
CASES = [(False, "CG2CG1"), (True, "CG2CG1"), (False, "CG1CG1"), (False, "CG2CR1")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gust(time_levels, nn, dt):
    # the load of tests/test_gpu_stress_history.py: 1-cosine gust of ex_simple_dynamic_shell_opt.py:45-95, scaled
    t = np.arange(time_levels) * dt
    fz = np.where((t >= 0.02) & (t <= 0.14), 0.1 * 50 * (1 - np.cos(2 * np.pi * (t - 0.02) / 0.12)), 0.0)
    F = np.zeros((time_levels, nn, 3))
    F[:, :, 2] = fz[:, None]
    return F.reshape(time_levels, -1)


def _mesh(element):
    from femo_alpha_amd.mesh import ShellMesh, quads_to_triangles
    mesh = plate_mesh(2.0, 10.0, 4, 12)
    if element == "CG2CR1":
        tri = quads_to_triangles(mesh)
        return ShellMesh(tri.nodes, tri.cells, element)
    if element != "CG2CG1":
        return ShellMesh(mesh.nodes, mesh.cells, element)
    return mesh


class Case:
    """A marched 2 x 10 plate under the gust (the cases of tests/test_gpu_stress_history.py)."""

    def __init__(self, ewt, element, rtol=1e-12, seed=0, mesh=None, bc=None, quad_deg=3):
        from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
        self.mesh = mesh = _mesh(element) if mesh is None else mesh
        self.ps = PlateSim(mesh, E, NU, RHO, DT, N, element_wise_thickness=ewt, quad_deg=quad_deg, leaf_size=8, rtol=rtol,
                           custom_bc_func=bc)
        self.n_t = mesh.nel if ewt else mesh.nn
        self.rng = np.random.default_rng(seed)
        self.t0 = 0.1 * (1 + 0.2 * self.rng.uniform(-1, 1, self.n_t))
        self.F = _gust(N + 1, mesh.nn, DT)
        self.ps.update_t(self.t0)
        self.ps.update_f_history(self.F)
        self.W = self.ps.solve_dynamic_problem()          # (fe_dofs, time_levels)

    def march(self, t, F=None):
        self.ps.update_t(t)
        self.ps.update_f_history(self.F if F is None else F)
        return self.ps.solve_dynamic_problem()


def _settings(W, ndof_u):
    """(rho, s) pairs: s > 0 and s < 0, rho such that rho |s| max|w| = 50 over the selected entries."""
    out = []
    for comp in ("all", "translations"):
        wmax = np.abs(R.selected(W.T, ndof_u, comp)).max()
        for s in (1.0 / wmax, -2.5 / wmax):
            out.append((comp, 50.0 / (abs(s) * wmax), s))
    return out


@pytest.mark.parametrize("ewt,element", CASES)
def test_value_and_per_level_values_against_the_restatement(ewt, element):
    c = Case(ewt, element)
    ps, W, nu = c.ps, c.W, c.mesh.ndof_u
    other = 1.3 * W * (1 + 0.1 * c.rng.uniform(-1, 1, W.shape))
    for comp, rho, s in _settings(W, nu):
        for Wx, arg in ((W, None), (other, other)):
            M = ps.max_displacement_history(rho, s, comp, W=arg)
            P = ps.max_displacement_history(rho, s, comp, per_level=True, W=arg)
            ref, ref_l = R.ks_value(Wx.T, rho, s, nu, comp)
            assert abs(M - ref) <= 1e-13 * abs(ref), (comp, rho, s, M, ref)
            assert P.shape == (N + 1,)
            assert np.abs(P - ref_l).max() <= 1e-13 * np.abs(ref_l).max(), (comp, s)
            assert np.sign(M) == np.sign(s)


@pytest.mark.parametrize("ewt,element", CASES)
def test_partials_against_the_restatement_and_finite_differences(ewt, element):
    c = Case(ewt, element)
    ps, W, rng, nu = c.ps, c.W, c.rng, c.mesh.ndof_u
    for comp, rho, s in _settings(W, nu):
        G = ps.max_displacement_history_partials(rho, s, comp)
        assert G.shape == (ps.fe_dofs, N + 1)
        ref = R.ks_grad(W.T, rho, s, nu, comp).T
        assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max(), (comp, s)
        assert np.all(G[W == 0.0] == 0.0)
        if comp == "translations":
            assert np.all(G[nu:, :] == 0.0)
        Mx = lambda Wx: ps.max_displacement_history(rho, s, comp, W=Wx)
        for _ in range(2):
            d = rng.uniform(-1, 1, W.shape) * W       # every entry relative to itself; zero entries stay zero (the kink of |w|)
            eps = 1e-6
            fd = (Mx(W + eps * d) - Mx(W - eps * d)) / (2 * eps)
            assert abs(np.sum(G * d) - fd) <= 1e-6 * abs(fd) + 1e-12 * abs(Mx(W)), (comp, s, np.sum(G * d), fd)


@pytest.mark.parametrize("ewt,element", CASES)
def test_total_gradient_against_the_host_route_and_finite_differences(ewt, element):
    c = Case(ewt, element)
    ps, rng, nu = c.ps, c.rng, c.mesh.ndof_u
    W = c.W
    comp, rho, s = _settings(W, nu)[0]
    g_dev, gF_dev = ps.max_displacement_history_total_gradient(rho, s, comp)
    assert g_dev.shape == (c.n_t,) and gF_dev.shape[0] == N + 1
    # the route an example takes today: history on the host, numpy gradient, adjoint from the host, residual products
    G = R.ks_grad(W.T, rho, s, nu, comp).T
    ps.adjoint_history(G)
    g_h, dF_h = ps.residual_T_products()
    assert np.abs(g_dev + g_h).max() <= 1e-10 * np.abs(g_h).max()
    assert np.abs(gF_dev + dF_h).max() <= 1e-10 * np.abs(dF_h).max()
    # central differences of march + aggregate (marches to rtol 1e-12)
    J = lambda t, F=None: (c.march(t, F), ps.max_displacement_history(rho, s, comp))[1]
    for i in rng.choice(c.n_t, 3, replace=False):
        st = 1e-4 * c.t0[i]
        tp = c.t0.copy(); tp[i] += st
        tm = c.t0.copy(); tm[i] -= st
        fd = (J(tp) - J(tm)) / (2 * st)
        assert abs(g_dev[i] - fd) < 2e-5 * np.abs(g_dev).max(), (i, g_dev[i], fd)
    k, node = 5, c.mesh.nn // 2
    for dof in (3 * node + 2, 3 * node):
        Fp = c.F.copy(); Fp[k, dof] += 1e-3
        Fm = c.F.copy(); Fm[k, dof] -= 1e-3
        fd = (J(c.t0, Fp) - J(c.t0, Fm)) / 2e-3
        assert abs(gF_dev[k, dof] - fd) < 1e-5 * np.abs(gF_dev).max(), (dof, gF_dev[k, dof], fd)


@pytest.mark.parametrize("ewt,element", [(False, "CG2CG1"), (True, "CG2CG1")])
def test_csdl_operation_totals_and_check_totals(ewt, element):
    from femo_alpha_amd.dynamic_rm_shell.operations import MaxDisplacementHistoryOperation, StateOperation
    c = Case(ewt, element)
    ps = c.ps
    wmax = np.abs(c.ps.tip_disp_history).max()
    s = 1.0 / wmax                                   # the example's scaler 1 / max(tip_disp_history)
    rho = 50.0 / (s * np.abs(c.W).max())
    rec = csdl.Recorder(inline=True); rec.start()
    grp = csdl.VariableGroup()
    grp.thickness = csdl.Variable(value=c.t0, name="thickness")
    grp.force_history = csdl.Variable(value=c.F, name="force_history")
    grp.disp_history = StateOperation(ps).evaluate(grp)
    md = MaxDisplacementHistoryOperation(ps, rho=rho, scaler=s).evaluate(grp)
    rec.stop()
    W = grp.disp_history.value.reshape((c.mesh.ndof, N + 1), order="F")
    assert md.value[0] == pytest.approx(R.ks_value(W.T, rho, s)[0], rel=1e-13)
    g = rec.compute_totals(md, grp.thickness)
    gF = rec.compute_totals(md, grp.force_history)
    g_dev, gF_dev = ps.max_displacement_history_total_gradient(rho, s)
    assert np.abs(g_dev - g).max() <= 1e-10 * np.abs(g).max()
    assert np.abs(gF_dev.reshape(gF.shape) - gF).max() <= 1e-10 * np.abs(gF).max()
    i0 = int(np.argmax(np.abs(g)))
    rows = rec.check_totals(md, grp.thickness, step=1e-4, indices=[i0, c.n_t // 3])
    for i, ana, fd, rel in rows:
        assert abs(ana - fd) <= 1e-5 * np.abs(g).max(), (i, ana, fd, rel)


def test_repeatability_seeded_adjoint_and_untouched_march_state():
    c = Case(False, "CG2CG1", rtol=1e-8)
    ps, ctx, W, nu = c.ps, c.ps.ctx, c.W, c.mesh.ndof_u
    T = ps.time_levels
    comp, rho, s = _settings(W, nu)[0]
    M1 = ps.max_displacement_history(rho, s); G1 = ps.max_displacement_history_partials(rho, s)
    M2 = ps.max_displacement_history(rho, s); G2 = ps.max_displacement_history_partials(rho, s)
    assert M1 == M2 and np.array_equal(G1, G2)
    Mg, _ = ctx.newmark_disp_aggregate_grad(T, rho, s)
    assert Mg == M1                                   # the gradient call's value: the same bits as the value call
    ctx.set_option("disp_history_chunk", 5)           # the host gradient staged in chunks of 5 levels: the same bits
    assert np.array_equal(ps.max_displacement_history_partials(rho, s), G1)
    ctx.set_option("disp_history_chunk", 0)
    # the seeded adjoint against the same G passed from the host
    _, Gs = ctx.newmark_disp_aggregate_grad(T, rho, s, seed_adjoint=True)
    assert np.array_equal(Gs, G1.T)
    ctx.newmark_adjoint_seeded(T)
    L1 = ctx.newmark_history(2)
    ctx.newmark_adjoint(Gs)
    L2 = ctx.newmark_history(2)
    ctx.newmark_adjoint(Gs)
    L3 = ctx.newmark_history(2)
    if np.array_equal(L2, L3):                        # the solve repeats bit for bit: so must the shared sweep
        assert np.array_equal(L1, L2)
    else:                                             # atomics in the sweeps of the factor: equal to the solve's own rounding
        assert np.abs(L1 - L2).max() <= 10 * np.abs(L2 - L3).max()
    assert np.abs(L1).max() > 0
    # a caller's history leaves the march's resident history and the stress aggregate alone, interleaved either way
    W0 = ctx.newmark_history(0)
    S0 = ps.pnorm_stress_history(m=1e-6, rho=6.0)
    other = 1.7 * W
    Mo = ps.max_displacement_history(rho, s, W=other)
    assert Mo == pytest.approx(R.ks_value(other.T, rho, s)[0], rel=1e-13)
    assert ps.pnorm_stress_history(m=1e-6, rho=6.0) == S0
    ps.pnorm_stress_history(m=1e-6, rho=6.0, W=other)
    assert ps.max_displacement_history(rho, s) == M1
    ps.max_displacement_history_partials(rho, s, W=other)
    assert ps.pnorm_stress_history(m=1e-6, rho=6.0) == S0
    assert np.array_equal(ctx.newmark_history(0), W0)
    assert ps.max_displacement_history(rho, s) == M1


def test_errors_name_the_parameter_and_the_context_stays_usable():
    from femo_alpha_amd import _lib
    c = Case(True, "CG2CG1", rtol=1e-8)
    ps, W = c.ps, c.W
    comp, rho, s = _settings(W, c.mesh.ndof_u)[0]
    M = ps.max_displacement_history(rho, s)
    for bad_rho in (0.0, -3.0):
        with pytest.raises(_lib.FemoHipError, match="rho"):
            ps.max_displacement_history(bad_rho, s)
        assert ps.max_displacement_history(rho, s) == M
    for bad_s in (0.0, np.inf):
        with pytest.raises(_lib.FemoHipError, match="scaler"):
            ps.max_displacement_history_partials(rho, bad_s)
        assert ps.max_displacement_history(rho, s) == M
    Wn = W.copy(); Wn[7, 5] = np.nan
    with pytest.raises(_lib.FemoHipError, match="level 5"):
        ps.max_displacement_history(rho, s, W=Wn)
    with pytest.raises(_lib.FemoHipError, match="level 5"):
        ps.max_displacement_history_partials(rho, s, W=Wn)
    with pytest.raises(ValueError, match="components"):
        ps.max_displacement_history(rho, s, components="rotations")
    assert ps.max_displacement_history(rho, s) == M
    G = ps.max_displacement_history_partials(rho, s)
    assert np.all(np.isfinite(G))


def test_tip_history_at_a_vertex_and_by_default():
    c = Case(False, "CG2CG1")
    ps, mesh = c.ps, c.mesh
    # no set-up: the reference's default point [10, 0, 0], a vertex of this plate
    v0 = int(np.argmin(np.linalg.norm(mesh.nodes - [10.0, 0.0, 0.0], axis=1)))
    assert np.array_equal(ps.tip_disp_history, c.W[3 * v0 + 2, :])
    v = int(np.argmin(np.linalg.norm(mesh.nodes - [10.0, 2.0, 0.0], axis=1)))
    ps.set_up_tip_dofs(mesh.nodes[v])
    assert ps.x_tip is not None and ps.cell_tip is None
    W = ps.solve_dynamic_problem()
    tip = ps.tip_disp_history
    assert tip.shape == (N + 1,) and tip[0] == 0.0 and np.abs(tip).max() > 0
    assert np.array_equal(tip, W[3 * v + 2, :])
    # refreshed by a second march with a new thickness
    ps.update_t(1.5 * c.t0)
    W2 = ps.solve_dynamic_problem()
    assert np.array_equal(ps.tip_disp_history, W2[3 * v + 2, :])
    assert not np.array_equal(ps.tip_disp_history, tip)
    # a mesh without the default point records zeros, no error
    from femo_alpha_amd.mesh import plate_mesh
    c2 = Case(False, "CG2CG1", mesh=plate_mesh(1.0, 4.0, 2, 6))
    assert np.array_equal(c2.ps.tip_disp_history, np.zeros(N + 1))


def test_tip_history_inside_a_warped_cell():
    from femo_alpha_amd.mesh import unstructured_quad_skin_mesh
    mesh = unstructured_quad_skin_mesh(3, 8)
    # quad_deg 6: the strain energies on the mesh's own rule (warped cells ask for more points than a reduced rule can sit beside)
    c = Case(False, "CG2CG1", mesh=mesh, bc=lambda x: np.isclose(x[1], 0.0, atol=1e-6), quad_deg=6)
    ps = c.ps
    rng = np.random.default_rng(4)
    tip_cell = int(np.argmax(mesh.nodes[mesh.cells].mean(axis=1)[:, 1]))       # a cell at the free end of the span
    Nn, _ = mesh._geometry(rng.uniform(-0.7, 0.7, 2))
    x = Nn @ mesh.nodes[mesh.cells[tip_cell]]
    for cell in (tip_cell, None):
        ps.set_up_tip_dofs(x, cell_tip=cell)
        W = ps.solve_dynamic_problem()
        dofs, w = mesh.point_evaluation(x, cell=tip_cell)
        ref = w @ W[dofs, :]
        assert ps.cell_tip == cell
        assert np.abs(ps.tip_disp_history - ref).max() <= 1e-14 * np.abs(ref).max() and np.abs(ref).max() > 0
        assert np.abs(ps.tip_displacement_history(W) - ref).max() <= 1e-14 * np.abs(ref).max()
        assert ps.tip_disp_history[0] == 0.0


def test_config5_tip_history_and_aggregate_against_the_golden():
    """BASELINE config 5 (bench.dynamic_case: 508 734 DOF, 101 levels) against tests/golden/config5_plate500k_dynamic.npz, at the
    tolerance of tests/test_gpu_goldens.py::test_config5_march_against_the_full_size_golden.  The golden's tip vertex is the corner at
    x = 10, y = 2 (the plate spans x in [0, 10], y in [0, 2])."""
    import bench
    from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
    TOL = 1e-8
    g = np.load(os.path.join(GOLDEN, "config5_plate500k_dynamic.npz"))
    mesh, dt, F = bench.dynamic_case(nsteps=int(g["nsteps"]))
    assert np.array_equal(mesh.nodes[int(g["tip_vertex"])], [10.0, 2.0, 0.0])
    ps = PlateSim(mesh, 1e8, 0.3, 10.0, dt, int(g["nsteps"]), quad_deg=3, leaf_size=mesh.recommended_leaf_size())
    ps.update_t(np.full(mesh.nn, 0.1))
    ps.update_f_history(F)
    ps.set_up_tip_dofs([10.0, 2.0, 0.0])
    ps.solve_dynamic_problem()
    tip, ref = ps.tip_disp_history, g["tip_history"]
    assert tip.shape == ref.shape and tip[0] == 0.0
    assert np.abs(tip - ref).max() < TOL * np.abs(ref).max()
    # the example's setting: scaler 1 / max(tip history), rho = 300
    s, rho = 1.0 / np.max(tip), 300.0
    P = ps.max_displacement_history(rho, s, per_level=True)
    wl = float(g["w_last_maxabs"])
    lo, hi = wl, wl + np.log(mesh.ndof) / (rho * s)
    assert lo * (1 - TOL) <= P[-1] <= hi * (1 + TOL), (P[-1], lo, hi)
    M = ps.max_displacement_history(rho, s)
    Wh = ps.ctx.newmark_history(0)
    ref_M, ref_l = R.ks_value(Wh, rho, s)
    assert abs(M - ref_M) <= 1e-12 * abs(ref_M)
    assert np.abs(P - ref_l).max() <= 1e-12 * np.abs(ref_l).max()
    ps.ctx.close()
