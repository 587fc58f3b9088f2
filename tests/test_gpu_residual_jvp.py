"""Forward mode of the static shell on the GPU: (dR/d arg) v (femo_residual_jvp) and the forward chain (femo_total_jvp) against the
numpy reference tests/residual_jvp_ref.py, against the existing transposed products (<lam, J v> = <J^T lam, v>), against central
differences of the oracle for the mesh motion, and against the adjoint totals; the operator surface and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import residual_jvp_ref as ref                                                    # noqa: E402
from femo_alpha_amd.mesh import plate_mesh                                         # noqa: E402
from test_gpu_laminate import BETA, ROOT_EDGE, random_laminate                     # noqa: E402
from test_gpu_laminate import _mesh as _lam_mesh                                   # noqa: E402
from test_gpu_laminate import _pair as _lam_pair                                   # noqa: E402
from test_gpu_parity import CLAMP                                                  # noqa: E402
from test_gpu_parity import _mesh as _par_mesh                                     # noqa: E402

pytestmark = pytest.mark.gpu

ISO_ARGS = ("thickness", "E", "nu", "F_solid")
ONAME = dict(thickness="h", E="E", nu="nu")


def _mesh(kind):
    if kind == "plate80":            # 80 cells: two workgroups of 64 cells, the second partly filled
        return plate_mesh(2.0, 10.0, 4, 20)
    if kind in ("quad CG1CG1", "tri CG2CR1"):
        return _lam_mesh(kind)
    return _par_mesh(kind)


def _pair(kind, ewm=False, ewp=False, uhat=True, bc="penalty", beta=BETA, seed=0):
    """The seeded pair of the parity tests (tests/test_gpu_parity.py::_pair) on this file's meshes."""
    from femo_alpha_amd.backend import ShellContext
    from oracle.rm_shell_oracle import ShellOracle
    m = _mesh(kind)
    rng = np.random.default_rng(seed)
    nT = m.nel if ewm else m.nn
    nF = m.nel if ewp else m.nn
    fields = dict(thickness=0.05 * (1 + 0.3 * rng.uniform(-1, 1, nT)), E=3e7 * (1 + 0.2 * rng.uniform(-1, 1, nT)),
                  nu=0.3 + 0.05 * rng.uniform(-1, 1, nT), density=10 * (1 + 0.1 * rng.uniform(-1, 1, nT)),
                  F_solid=rng.uniform(-1, 1, (nF, 3)))
    if uhat:
        fields["uhat"] = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    marker = CLAMP if kind.startswith("plate") else ROOT_EDGE
    pf = m.penalty_facets(marker) if bc == "penalty" else None
    sd = m.locate_dofs_geometrical(marker) if bc == "strong" else None
    o = ShellOracle(m, element_wise_material=ewm, elementwise_pressure=ewp, penalty_facets=pf, strong_dofs=sd, beta=beta)
    o.set_fields(h=fields["thickness"], E=fields["E"], nu=fields["nu"], rho=fields["density"], f=fields["F_solid"], uhat=fields.get("uhat"))
    c = ShellContext(m, element_wise_material=ewm, elementwise_pressure=ewp)
    for k, v in fields.items():
        c.set_field(k, v)
    if pf is not None:
        c.set_penalty_facets(pf, beta)
    if sd is not None:
        c.set_strong_dofs(sd)
    return m, o, c, rng


def _dist(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max()


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("kind,ewm,ewp,uhat,bc", [("warped", False, False, True, "penalty"), ("warped", True, True, False, "strong"),
                                                  ("tri", False, False, True, "strong"), ("quad CG1CG1", False, False, True, "penalty"),
                                                  ("tri CG2CR1", True, False, True, "strong"), ("plate", False, False, False, "strong"),
                                                  ("plate80", True, False, True, "penalty")])
def test_field_and_load_products_against_the_reference(kind, ewm, ewp, uhat, bc):
    m, o, c, rng = _pair(kind, ewm, ewp, uhat, bc)
    w = rng.uniform(-1, 1, m.ndof) * 1e-3                        # strong entries non-zero: the residual's operator does not see them
    c.set_state(w)
    for arg in ISO_ARGS:
        v = rng.uniform(-1, 1, c.field_size(arg))
        got = c.dRdarg(arg, v)
        want = ref.jvp_load(o, v) if arg == "F_solid" else ref.jvp_field(o, ONAME[arg], w, v)
        d = _dist(got, want)
        print(f"dRdarg [{kind}, {arg}]: {d:.1e}")
        assert d <= 1e-11, arg
        assert np.all(got[o.strong_dofs] == 0.0)
    assert np.all(c.dRdarg("density", rng.uniform(-1, 1, c.field_size("density"))) == 0.0)
    c.close()


@pytest.mark.parametrize("kind,bc", [("warped", "penalty"), ("tri", "strong"), ("quad CG1CG1", "strong"), ("tri CG2CR1", "penalty")])
def test_laminate_product_against_the_reference(kind, bc):
    m, o, c, rng, clt = _lam_pair(kind, bc=bc)
    w = rng.uniform(-1, 1, m.ndof) * 1e-3
    c.set_state(w)
    v = rng.uniform(-1, 1, (m.nel, 32)) * np.abs(clt).max(axis=1, keepdims=True)          # not symmetric
    got = c.dRdarg("laminate", v.ravel())
    d = _dist(got, ref.jvp_laminate(o, w, v))
    print(f"dRdarg [{kind}, laminate]: {d:.1e}")
    assert d <= 1e-11
    assert np.all(got[o.strong_dofs] == 0.0)
    for arg in ("thickness", "E", "nu"):                         # the laminate replaces them inside R: exact zeros, as their transposes
        assert np.all(c.dRdarg(arg, rng.uniform(-1, 1, c.field_size(arg))) == 0.0)
        assert np.all(c.dRdarg_T(arg, rng.uniform(-1, 1, m.ndof)) == 0.0)
    c.close()


# ------------------------------------------------------------------------------------------ 2. exact transposition
def _transposition(m, c, rng, strong, args):
    w = rng.uniform(-1, 1, m.ndof) * 1e-3
    w[strong] = 0.0                                              # the transposed products read the state as it is stored
    c.set_state(w)
    dofs = m.cell_dofs()
    for arg in args:
        n = c.field_size(arg)
        pairs = [(rng.uniform(-1, 1, m.ndof), rng.uniform(-1, 1, n)) for _ in range(3)]
        # a lambda on the DOFs of one cell and a v on one entry of it: a sign or slot error cannot average out
        e = m.nel // 2
        lam = np.zeros(m.ndof); lam[dofs[e]] = rng.uniform(-1, 1, dofs.shape[1])
        v = np.zeros(n)
        if arg == "laminate":
            v[32 * e + rng.integers(32)] = 1.0
        elif arg == "uhat":
            v[3 * m.cells[e, 1]] = 1.0                           # in-plane on the flat plates, where a normal motion moves neither F^-1 E_a nor J
        elif arg == "F_solid":
            v[3 * (e if n == 3 * m.nel else m.cells[e, 1]) + 1] = 1.0
        else:
            v[e if n == m.nel else m.cells[e, 1]] = 1.0
        pairs.append((lam, v))
        for lam, v in pairs:
            lam = lam.copy(); lam[strong] = 0.0
            Jv = c.dRdarg(arg, v)
            JTl = c.dRdarg_T(arg, lam)
            gap = abs(lam @ Jv - JTl @ v)
            scale = np.linalg.norm(lam) * np.linalg.norm(Jv)
            print(f"transposition [{arg}]: |<lam, J v> - <J^T lam, v>| = {gap:.2e}, bound {1e-11 * scale:.2e}")
            assert scale > 0, arg
            assert gap <= 1e-11 * scale, arg


@pytest.mark.parametrize("kind,ewm,ewp,bc", [("warped", False, False, "penalty"), ("tri", True, True, "penalty"),
                                             ("quad CG1CG1", False, False, "penalty"), ("tri CG2CR1", False, False, "penalty"),
                                             ("plate80", False, False, "strong")])
def test_exact_transposition(kind, ewm, ewp, bc):
    m, o, c, rng = _pair(kind, ewm, ewp, True, bc)
    _transposition(m, c, rng, o.strong_dofs, ISO_ARGS + ("uhat",))
    c.close()


@pytest.mark.parametrize("kind", ["warped", "tri", "quad CG1CG1", "tri CG2CR1"])
def test_exact_transposition_in_laminate_mode(kind):
    m, o, c, rng, _ = _lam_pair(kind, bc="penalty")
    _transposition(m, c, rng, o.strong_dofs, ("laminate", "F_solid", "uhat"))
    c.close()


def test_exact_transposition_with_prescribed_penalty_values():
    m, o, c, rng = _pair("warped", bc="penalty")
    c.set_field("dirichlet", rng.uniform(-1, 1, m.ndof) * 1e-3)
    _transposition(m, c, rng, o.strong_dofs, ("uhat",))
    c.close()


# ------------------------------------------------------------------------------------------ 3. uhat against the oracle
@pytest.mark.parametrize("kind,bc", [("warped", "penalty"), ("tri", "penalty"), ("plate", "strong")])
def test_shape_product_against_central_differences_of_the_oracle(kind, bc):
    """As tests/test_gpu_parity.py::test_shape_sensitivities_vs_oracle_finite_differences forms the residual: K @ w - load_vector()
    at uhat +- 1e-6 v, and its bar."""
    m, o, c, rng = _pair(kind, uhat=True, bc=bc, beta=1e6)
    w = rng.uniform(-1, 1, m.ndof) * 1e-3
    w[o.strong_dofs] = 0.0
    c.set_state(w)
    u0 = o.uhat.copy()
    v = rng.uniform(-1, 1, u0.shape)
    Jv = c.dRdarg("uhat", v.ravel())
    step = 1e-6

    def R(u):
        o.set_fields(uhat=u)
        r = o.assemble_K(with_strong=False) @ w - o.load_vector()
        r[o.strong_dofs] = 0.0
        return r
    fd = (R(u0 + step * v) - R(u0 - step * v)) / (2 * step)
    o.set_fields(uhat=u0)
    err = np.abs(Jv - fd)
    print(f"uhat product [{kind}]: largest error {err.max():.2e} of {np.abs(Jv).max():.2e}")
    assert np.all(err <= 2e-6 * np.abs(Jv).max() + 1e-9 * np.abs(fd))
    assert np.all(Jv[o.strong_dofs] == 0.0)
    c.close()


# ------------------------------------------------------------------------------------------ 4. linearity and repeatability
@pytest.mark.parametrize("lam", [False, True])
def test_linearity_and_repeatability(lam):
    if lam:
        m, o, c, rng, _ = _lam_pair("warped", bc="penalty")
        args = ("laminate", "F_solid", "uhat")
    else:
        m, o, c, rng = _pair("plate80", bc="penalty")
        args = ISO_ARGS + ("uhat",)
    c.set_state(rng.uniform(-1, 1, m.ndof) * 1e-3)
    for arg in args:
        V = rng.uniform(-1, 1, (3, c.field_size(arg)))
        got = c.dRdarg(arg, V)
        assert got.shape == (3, m.ndof) and np.abs(got).max() > 0
        for k in range(3):
            assert np.array_equal(got[k], c.dRdarg(arg, V[k])), arg             # three directions in one call: the same bits
        assert np.array_equal(got, c.dRdarg(arg, V)), arg                       # a second identical call: the same bits
        assert np.array_equal(c.dRdarg(arg, 2.0 * V[0]), 2.0 * got[0]), arg     # a power of two commutes with every rounding
    c.close()


# ------------------------------------------------------------------------------------------ 5. totals
def _tight(c):
    c.use_direct_solver(rtol=1e-12)


def _check_totals(c, arg, V, functionals, label):
    dW, dJ, it, rr = c.total_jvp(arg, V, functionals)
    G, _, _ = c.total_gradients(list(functionals), arg)
    want = G @ V.T
    for i, fn in enumerate(functionals):
        for k in range(V.shape[0]):
            if want[i, k] == 0.0:                                # no dependence at all (the mass on E, say): exact zeros on both sides
                assert dJ[i, k] == 0.0, (fn, arg, k)
                continue
            d = abs(dJ[i, k] - want[i, k]) / abs(want[i, k])
            print(f"total_jvp against total_gradients . v [{label}, {fn}, {arg}, direction {k}]: {d:.1e}")
            assert d <= 1e-8, (fn, arg, k)
    return dW


@pytest.mark.parametrize("kind,ewm,bc", [("warped", False, "penalty"), ("plate80", True, "strong")])
def test_totals_against_the_adjoint_chain(kind, ewm, bc):
    m, o, c, rng = _pair(kind, ewm=ewm, uhat=True, bc=bc)
    _tight(c)
    c.set_stress_params(1e-6, 6.0)
    c.solve_state()
    fns = ("compliance", "elastic_energy", "mass", "pnorm_stress")
    for arg in ("thickness", "E", "F_solid", "uhat"):
        base = c.get_field(arg)
        scale = np.abs(base).max() if arg != "uhat" else 0.02
        V = scale * rng.uniform(0.5, 1.0, (2, base.size))                      # one-signed directions: g . v does not cancel
        _check_totals(c, arg, V, fns, kind)
    c.close()


def test_totals_of_the_ply_failure_in_laminate_mode():
    from test_gpu_ply_failure import _pair as _ply_pair
    m, o, c, rng, clt, tab = _ply_pair("warped", bc="penalty")
    _tight(c)
    c.solve_state()
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    V = clt.reshape(1, -1) * rng.uniform(0.5, 1.0, (2, clt.size))
    _check_totals(c, "laminate", V, ("ply_failure", "elastic_energy"), "laminate")
    c.close()


def test_tangent_state_against_differences_of_re_solved_states_and_group_sizes():
    """dW = -K^-1 (dR/dh) v against central differences of two re-solved states at eps and eps / 2, combined by Richardson extrapolation as
    tests/test_gpu_dynamic.py does for the march (truncation O(eps^4)), with that test's bar; then groups of 1, 2, 4 and 5 directions
    against one at a time."""
    m, o, c, rng = _pair("plate80", uhat=True, bc="strong")
    c.use_direct_solver(rtol=1e-15, maxit=20)                    # refined to the rounding floor (tests/test_gpu_laminate.py::tight)
    c.set_option("strict", 0)
    h0 = c.get_field("thickness")
    d = rng.uniform(-1, 1, h0.size) * h0

    def solved(h):
        c.set_field("thickness", h); c.solve_state()
        return c.get_state()
    cd = lambda e: (solved(h0 + e * d) - solved(h0 - e * d)) / (2 * e)
    eps = 2e-3
    fd1, fd2 = cd(eps), cd(eps / 2)
    fd = (4.0 * fd2 - fd1) / 3.0
    solved(h0)
    dW, _, it, rr = c.total_jvp("thickness", d)
    dist = np.abs(dW - fd).max() / np.abs(fd).max()
    print(f"tangent state against the extrapolated difference: {dist:.1e} (differences at {eps:g} and {eps / 2:g} differ by "
          f"{np.abs(fd1 - fd2).max() / np.abs(fd).max():.1e})")
    assert dist < 2e-9
    assert np.all(dW[o.strong_dofs] == 0.0)
    V = rng.uniform(-1, 1, (5, h0.size)) * h0
    single = np.array([c.total_jvp("thickness", v)[0] for v in V])
    for g in (1, 2, 4, 5):
        dWg, dJg, it, rr = c.total_jvp("thickness", V[:g], ("compliance",))
        assert dWg.shape == (g, m.ndof) and dJg.shape == (1, g) and it.shape == (g,)
        dd = np.abs(dWg - single[:g]).max() / np.abs(single).max()
        print(f"group of {g} against one at a time: {dd:.1e}")
        assert dd <= 1e-8
    assert c.total_jvp("thickness", V[:2], ("compliance",), want_states=False)[0] is None
    c.close()


# ------------------------------------------------------------------------------------------ 6. operator surface
def test_forward_mode_through_the_operator_surface():
    from femo_alpha_amd import csdl
    from femo_alpha_amd.csdl_alpha_opt.state_operation import StateOperation
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn = mesh.nn
    rng = np.random.default_rng(5)
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    pressure = csdl.Variable(value=np.tile([0.0, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=0.1 * (1 + 0.2 * rng.uniform(-1, 1, nn)), name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=10.0 * np.ones(nn), name="density")
    node_disp = csdl.Variable(value=0.01 * rng.uniform(-1, 1, (nn, 3)), name="node_disp")
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=True)
    model.evaluate(pressure, thickness, E, nu, density, node_disp, debug_mode=False, is_pressure=True)
    recorder.stop()
    fea, ctx = model.fea, model.shell_pde.ctx
    ctx.use_direct_solver(rtol=1e-12)
    op = StateOperation(fea=fea, args_name_list=fea.states_dict["disp_solid"]["arguments"], state_name="disp_solid")
    inputs = {name: fea.inputs_dict[name]["function"].x.array.copy() for name in fea.states_dict["disp_solid"]["arguments"]}
    outputs = {}
    fea.opt_iter = 0
    op.solve_residual_equations(inputs, outputs)
    for arg in ("thickness", "uhat"):
        v = rng.uniform(-1, 1, inputs[arg].size) * (0.1 if arg == "thickness" else 0.01)
        seed = rng.uniform(-1, 1, mesh.ndof)
        d_res = {"disp_solid": seed.copy()}
        op.compute_jacvec_product(inputs, outputs, {arg: v}, {}, d_res, "fwd")
        Jv = ctx.dRdarg(arg, v)
        assert np.abs(Jv).max() > 0
        assert np.array_equal(d_res["disp_solid"], seed + Jv)                   # J v is ADDED into d_residuals
        d_out = {}
        op.apply_inverse_jacobian(inputs, outputs, d_out, {"disp_solid": Jv}, "fwd")
        dW = ctx.total_jvp(arg, v)[0]
        dd = np.abs(-d_out["disp_solid"] - dW).max() / np.abs(dW).max()
        print(f"operator surface [{arg}]: K^-1 (J v) against -total_jvp's tangent: {dd:.1e}")
        assert dd <= 1e-8


# ------------------------------------------------------------------------------------------ 7. refusals and state preservation
def test_refusals_leave_the_context_as_it_was():
    from femo_alpha_amd._lib import FemoHipError
    m, o, c, rng = _pair("warped", bc="penalty")
    _tight(c)
    c.solve_state()
    w0, info0 = c.get_state(), c.frontal_info()
    h0 = c.get_field("thickness")
    v = rng.uniform(-1, 1, m.nn)
    ref_Jv = c.dRdarg("thickness", v)
    with pytest.raises(FemoHipError, match="unknown argument 'pressure'"):
        c.dRdarg("pressure", v)
    with pytest.raises(FemoHipError, match="unknown argument 'laminate'"):       # outside laminate mode, as femo_dRdarg_T answers
        c.dRdarg("laminate", np.zeros(32 * m.nel))
    with pytest.raises(FemoHipError, match="unknown field 'laminate'"):           # the transposed product sizes its result first
        c.dRdarg_T("laminate", np.zeros(m.ndof))
    with pytest.raises(FemoHipError, match="wrong length"):
        c.dRdarg("thickness", np.zeros(m.nn + 1))
    with pytest.raises(FemoHipError, match="wrong length"):
        c.total_jvp("uhat", np.zeros(m.nn))
    with pytest.raises(FemoHipError, match="unknown functional"):
        c.total_jvp("thickness", v, ("stiffness",))
    with pytest.raises(FemoHipError, match="unknown sub-domain"):
        c.total_jvp("thickness", v, ("compliance",), subdomains=[3])
    with pytest.raises(FemoHipError, match="femo_set_ply_table"):
        c.total_jvp("thickness", v, ("ply_failure",))
    assert np.array_equal(c.get_state(), w0) and np.array_equal(c.get_field("thickness"), h0)
    assert np.array_equal(c.frontal_info(), info0)
    assert np.array_equal(c.dRdarg("thickness", v), ref_Jv)
    dW, dJ, it, rr = c.total_jvp("thickness", v, ("compliance", "mass"))
    assert np.array_equal(c.frontal_info(), info0)               # a tangent re-uses the factor of the state solve
    assert np.array_equal(c.get_state(), w0)
    assert np.all(np.isfinite(dW)) and dJ.shape == (2,) and np.all(it >= 1)
    c.close()


def test_ply_failure_keeps_refusing_the_shape_derivative_and_strict_reports_status_4():
    from femo_alpha_amd._lib import FemoHipError
    from test_gpu_ply_failure import _pair as _ply_pair
    m, o, c, rng, clt, tab = _ply_pair("warped", bc="penalty")
    _tight(c)
    c.solve_state()
    v = rng.uniform(-1, 1, 3 * m.nn)
    with pytest.raises(FemoHipError, match="shape derivative"):
        c.total_jvp("uhat", v, ("ply_failure",))
    w0 = c.get_state()
    c.set_solver(preconditioner=2, rtol=1e-300, maxit=1, check_every=1)          # cannot be met: strict makes it an error (status 4)
    with pytest.raises(FemoHipError, match="did not converge"):
        c.total_jvp("laminate", rng.uniform(-1, 1, (2, clt.size)) * 1e-3 * np.abs(clt).max())
    c.set_option("strict", 0)
    dW = c.total_jvp("laminate", rng.uniform(-1, 1, (2, clt.size)) * 1e-3 * np.abs(clt).max())[0]
    assert np.all(np.isfinite(dW)) and np.array_equal(c.get_state(), w0)
    c.close()
