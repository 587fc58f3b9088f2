"""Forward mode of the field outputs on the GPU (csrc/field_jvp.h; femo_field_output_jvp, femo_field_total_jvp): the matrix-free
tangents of the DG1 von Mises fields against the partial Jacobian of the older kernels and against the reverse products, the
tangent of the ply failure field against the numpy reference tests/field_jvp_ref.py, the forward chain for fields against the
adjoint chain and against differences of re-solved states, the operator surface and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_jvp_ref import fi_gap, ply_field_tangent                                 # noqa: E402
from femo_alpha_amd.mesh import plate_mesh, wing_skin_mesh                         # noqa: E402
from test_gpu_laminate import BETA, ROOT_EDGE, random_laminate, tight              # noqa: E402
from test_gpu_ply_failure import _pair as _ply_pair                                # noqa: E402
from test_gpu_ply_failure import random_table                                      # noqa: E402
from test_gpu_stress_field_derivatives import ARGS, FAMILIES, NAMES, _context, _direction, rel     # noqa: E402

pytestmark = pytest.mark.gpu

PLY_KINDS = ["warped", "tri", "quad CG1CG1", "tri CG2CR1"]
ZERO_ARGS_PLY = ("laminate", "thickness", "E", "nu", "density", "F_solid")
BIG_SEED = 1          # wing_skin_mesh(10, 24), seeds 0-2 tried on the CPU: the smallest gap between the two largest FI of an entry is 2.4e-5 max|FI|


def _one_hot(m, c, arg, rng):
    """A direction on one entry of one cell (tests/test_gpu_residual_jvp.py::_transposition): a slot or sign error cannot average out."""
    e = m.nel // 2
    n = c.arg_size(arg)
    v = np.zeros(n)
    if arg == "disp_solid":
        v[m.cell_dofs()[e][0]] = 1e-4                            # an in-plane displacement: it strains the flat plates too
    elif arg == "uhat":
        v[3 * m.cells[e, 1]] = 0.05                              # in-plane on the flat plates, where a normal motion moves nothing
    else:
        i = e if n == m.nel else m.cells[e, 1]
        v[i] = abs(c.get_field(arg)[i])
    return v


# ------------------------------------------------------------------------------------------ 1. partials against the Jacobian
@pytest.mark.parametrize("family,ewm,uhat", FAMILIES)
def test_partials_against_the_existing_jacobian(family, ewm, uhat):
    """field_output_jvp(name, wrt, d) against field_output_jacobian(name, wrt) @ d (older kernels: an independent reference) for every
    name x argument, random and one-hot directions; the bar the reverse products are held to against that matrix, 1e-12."""
    m, c, fields, rng = _context(family, ewm, uhat)
    c.set_state(rng.uniform(-1, 1, m.ndof) * 1e-4)
    for name in NAMES:
        for arg in ARGS:
            J = c.field_output_jacobian(name, arg)
            for d in (_direction(c, arg, rng), _one_hot(m, c, arg, rng)):
                got = c.field_output_jvp(name, arg, d)
                assert got.shape == (m.nvc * m.nel,)
                if name == "stress_mid" and arg == "thickness":
                    assert np.all(got == 0.0)
                    continue
                want = J @ d
                print(f"{family} ewm={ewm} [{name}, {arg}]: {rel(got, want):.1e}")
                assert np.abs(want).max() > 0.0
                assert rel(got, want) < 1e-12, (name, arg, rel(got, want))
        for arg in ("F_solid", "density"):
            assert np.all(c.field_output_jvp(name, arg, np.ones(c.arg_size(arg))) == 0.0)
    c.close()


# ------------------------------------------------------------------------------------------ 2. transposition
@pytest.mark.parametrize("family,ewm,uhat", [("warped", False, True), ("tri", True, False), ("cr1", False, True), ("cg1", True, False)])
def test_exact_transposition_with_the_reverse_products(family, ewm, uhat):
    """|<cbar, J v> - <J^T cbar, v>| <= 1e-11 |cbar| |J v| (the bar of test_gpu_residual_jvp.py::test_exact_transposition): three random
    pairs and a one-hot pair for every argument."""
    m, c, fields, rng = _context(family, ewm, uhat, seed=7)
    c.set_state(rng.uniform(-1, 1, m.ndof) * 1e-4)
    nc = m.nvc * m.nel
    for name in NAMES:
        for arg in ARGS:
            if name == "stress_mid" and arg == "thickness":
                continue
            pairs = [(rng.uniform(-1, 1, nc), _direction(c, arg, rng)) for _ in range(3)]
            cb = np.zeros(nc); cb[m.nvc * (m.nel // 2): m.nvc * (m.nel // 2 + 1)] = rng.uniform(-1, 1, m.nvc)
            pairs.append((cb, _one_hot(m, c, arg, rng)))
            for cb, v in pairs:
                Jv = c.field_output_jvp(name, arg, v)
                JTc = c.field_output_vjp(name, arg, cb)
                gap, scale = abs(cb @ Jv - JTc @ v), np.linalg.norm(cb) * np.linalg.norm(Jv)
                print(f"transposition [{family}, {name}, {arg}]: {gap:.2e}, bound {1e-11 * scale:.2e}")
                assert scale > 0 and gap <= 1e-11 * scale, (name, arg)
    c.close()


# ------------------------------------------------------------------------------------------ 3. linearity and repeatability
@pytest.mark.parametrize("family,ewm,uhat", [("warped", False, True), ("tri", True, True)])
def test_linearity_and_repeatability(family, ewm, uhat):
    m, c, fields, rng = _context(family, ewm, uhat, seed=3)
    c.set_state(rng.uniform(-1, 1, m.ndof) * 1e-4)
    for name in NAMES:
        for arg in ARGS:
            V = np.array([_direction(c, arg, rng) for _ in range(5)])
            got = c.field_output_jvp(name, arg, V[:3])
            assert got.shape == (3, m.nvc * m.nel)
            for k in range(3):
                assert np.array_equal(got[k], c.field_output_jvp(name, arg, V[k])), (name, arg, k)
            assert np.array_equal(got, c.field_output_jvp(name, arg, V[:3]))
            assert np.array_equal(c.field_output_jvp(name, arg, V)[4], c.field_output_jvp(name, arg, V[4]))     # a second pass of four
            assert np.array_equal(c.field_output_jvp(name, arg, 2.0 * V[0]), 2.0 * got[0]), (name, arg)       # a power of two commutes
    c.close()


# ------------------------------------------------------------------------------------------ 4. ply failure field
def _ply_big(seed=BIG_SEED):
    """The construction of test_gpu_ply_failure.py::_pair on wing_skin_mesh(10, 24): 240 cells, four one-wave blocks, the last partly filled."""
    from femo_alpha_amd.backend import ShellContext
    from oracle.rm_shell_oracle import degree4_rule
    from ply_failure_ref import PlyFailureOracle
    m = wing_skin_mesh(10, 24)
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (m.nn, 3))
    uh = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    clt = random_laminate(m.nel, rng)
    tab = random_table(m.nel, rng, 2)
    o = PlyFailureOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f, uhat=uh)
    o.set_ply_table(tab, 4)
    c = ShellContext(m)
    for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=f, uhat=uh).items():
        c.set_field(k, v)
    c.set_laminate(clt)
    c.set_ply_table(tab)
    return m, o, c, rng, clt, tab


@pytest.mark.parametrize("kind", PLY_KINDS + ["big"])
def test_ply_failure_field_tangents_against_the_reference(kind):
    """State and table tangents at the reference's maximiser, 1e-11 of the largest entry (the operator-level bar of
    test_gpu_ply_failure.py); entries whose two largest FI agree to 1e-6 max|FI| have no defined maximiser and are left out (at most 1 %;
    none for the four small kinds).  Exact zeros for the six arguments the field does not depend on; linearity and repeatability."""
    m, o, c, rng, _, tab = _ply_big() if kind == "big" else _ply_pair(kind)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    dw = 2e-3 * rng.uniform(-1, 1, (3, m.ndof))
    dt = tab[None] * rng.uniform(-1, 1, (3,) + tab.shape)
    for wrt, V in (("disp_solid", dw), ("ply_table", dt.reshape(3, -1))):
        got = c.field_output_jvp("ply_failure_field", wrt, V)
        assert got.shape == (3, m.nel * tab.shape[1])
        for k in range(3):
            want, gap, fmax = ply_field_tangent(o, w, tab, dw=dw[k] if wrt == "disp_solid" else None, dtable=dt[k] if wrt == "ply_table" else None)
            keep = gap >= 1e-6 * fmax
            out = 1.0 - keep.mean()
            err = np.abs(got[k].reshape(want.shape) - want)[keep].max() / np.abs(want).max()
            print(f"{kind} [{wrt}, direction {k}]: {err:.1e}; smallest gap {gap.min() / fmax:.1e} max|FI|, left out {100 * out:.2f} %")
            assert out <= 0.01
            if kind != "big":
                assert out == 0.0
            assert err <= 1e-11
            assert np.array_equal(got[k], c.field_output_jvp("ply_failure_field", wrt, V[k]))
        assert np.array_equal(got, c.field_output_jvp("ply_failure_field", wrt, V))
        assert np.array_equal(c.field_output_jvp("ply_failure_field", wrt, 2.0 * V[0]), 2.0 * got[0])
    for arg in ZERO_ARGS_PLY:
        assert not np.any(c.field_output_jvp("ply_failure_field", arg, np.ones(c.arg_size(arg)))), arg
    for name in NAMES:                                    # the stress fields keep the single-layer recovery in laminate mode
        for arg in ("laminate", "ply_table"):
            assert not np.any(c.field_output_jvp(name, arg, np.ones(c.arg_size(arg)))), (name, arg)
    c.close()


def test_ply_failure_field_tangent_against_central_differences_of_the_field():
    """ply_failure_field() itself along a table direction: step 1e-6 relative, bar 1e-6, as the stress fields' difference test."""
    m, o, c, rng, _, tab = _ply_pair("warped")
    c.set_state(2e-3 * rng.uniform(-1, 1, m.ndof))
    d = tab * rng.uniform(-1, 1, tab.shape)
    got = c.field_output_jvp("ply_failure_field", "ply_table", d.ravel()).reshape(m.nel, -1)
    eps = 1e-6
    c.set_field("ply_table", tab + eps * d); fp = c.ply_failure_field()
    c.set_field("ply_table", tab - eps * d); fm = c.ply_failure_field()
    c.set_field("ply_table", tab)
    fd = (fp - fm) / (2 * eps)
    print(f"table tangent against central differences: {rel(got, fd):.1e}")
    assert rel(got, fd) < 1e-6
    c.close()


# ------------------------------------------------------------------------------------------ 5. totals
def _totals_context(case):
    if case == "warped":
        m, c, fields, rng = _context("warped", False, True, seed=11, beta=BETA)
    elif case == "plate80":
        from femo_alpha_amd.backend import ShellContext
        from test_gpu_stress_field_derivatives import _fields
        m = plate_mesh(2.0, 10.0, 4, 20)
        fields, rng = _fields(m, True, True, 11)
        c = ShellContext(m, element_wise_material=True)
        for k, v in fields.items():
            c.set_field(k, v)
        c.set_strong_dofs(m.locate_dofs_geometrical(lambda x: np.less(x[0], 3e-16)))
    else:
        m, c, fields, rng = _context("tri", True, False, seed=11, beta=BETA)
    c.use_direct_solver(rtol=1e-12)
    c.solve_state()
    return m, c, rng


@pytest.mark.parametrize("case", ["warped", "plate80", "tri"])
def test_totals_against_the_adjoint_chain(case):
    """cbar . field_total_jvp(...)[name][k] against (field_total_gradients(name, cbar, arg) @ V.T)[., k], 1e-8 of sum |cbar_i dfield_i| (the
    1e-8 of test_gpu_residual_jvp.py::test_totals_against_the_adjoint_chain, robust to cancellation).  All three names in ONE call, with
    the iteration counts of a single-name call: one solve per direction, not one per field."""
    m, c, rng = _totals_context(case)
    nc = m.nvc * m.nel
    for arg in ("thickness", "E", "F_solid", "uhat"):
        base = c.get_field(arg)
        scale = np.abs(base).max() if arg != "uhat" else 0.02
        V = scale * rng.uniform(0.5, 1.0, (2, base.size))
        res, dW, it, rr = c.field_total_jvp(NAMES, arg, V, want_states=True)
        one, _, it1, _ = c.field_total_jvp(NAMES[:1], arg, V)
        assert np.array_equal(it, it1) and it.shape == (2,)
        assert dW.shape == (2, m.ndof) and rel(one["stress"], res["stress"]) <= 1e-8
        cbs = rng.uniform(-1, 1, (3, nc))
        for name in NAMES:
            assert res[name].shape == (2, nc)
            G, _, _ = c.field_total_gradients(name, cbs, arg)
            want = G @ V.T
            for i in range(3):
                for k in range(2):
                    got, bound = cbs[i] @ res[name][k], 1e-8 * np.abs(cbs[i] * res[name][k]).sum()
                    print(f"{case} [{name}, {arg}, cotangent {i}, direction {k}]: {abs(got - want[i, k]):.2e}, bound {bound:.2e}")
                    assert bound > 0 and abs(got - want[i, k]) <= bound, (name, arg, i, k)
    c.close()


def test_totals_in_laminate_mode_and_group_sizes():
    """arg = "laminate", names ("ply_failure_field", "stress") in one call.  The ply part has no reverse counterpart: Richardson-
    extrapolated central differences of the field at re-solved states (eps and eps / 2), construction and bar 2e-9 of the largest entry of
    test_gpu_residual_jvp.py::test_tangent_state_against_differences_of_re_solved_states_and_group_sizes.  A difference of max_q FI is the
    derivative of one branch only where every state of the stencil selects that branch by a clear margin: entries are kept where the two
    largest FI differ by 1e-6 max|FI| at all four perturbed states and the maximiser is the base state's (from the reference alone; at
    most 1 % left out).  The stress part against the adjoint chain, composed from the existing calls (femo_field_total_gradients does
    not take "laminate").  Then groups of 1, 2, 4 and 5 directions against one at a time."""
    m, o, c, rng, clt, tab = _ply_pair("warped", bc="penalty")
    tight(c)
    names = ("ply_failure_field", "stress")
    d = clt * rng.uniform(-1, 1, clt.shape)
    keep = np.ones((m.nel, tab.shape[1]), bool)
    fmax = None

    def solved(L):
        nonlocal keep, fmax
        c.set_field("laminate", L); c.solve_state()
        fi = o.failure_index(c.get_state())[0]
        if fmax is None:                                  # the base state comes first
            fmax, solved.q0 = np.abs(fi).max(), fi.argmax(axis=1)
        keep &= (fi_gap(fi) >= 1e-6 * fmax) & (fi.argmax(axis=1) == solved.q0)
        return c.ply_failure_field()
    solved(clt)
    cd = lambda e: (solved(clt + e * d) - solved(clt - e * d)) / (2 * e)
    eps = 2e-3
    fd1, fd2 = cd(eps), cd(eps / 2)
    fd = (4.0 * fd2 - fd1) / 3.0
    solved(clt)
    res, _, it, rr = c.field_total_jvp(names, "laminate", d.ravel())
    got = res["ply_failure_field"].reshape(fd.shape)
    out = 1.0 - keep.mean()
    dist = np.abs(got - fd)[keep].max() / np.abs(fd).max()
    print(f"ply failure field tangent against the extrapolated difference: {dist:.1e}, left out {100 * out:.2f} %")
    assert out <= 0.01
    assert dist < 2e-9
    cbs = rng.uniform(-1, 1, (3, m.nvc * m.nel))
    for cb in cbs:
        lam = c.solve_linear(c.field_output_vjp("stress", "disp_solid", cb))[0]
        want = -c.dRdarg_T("laminate", lam) @ d.ravel()
        gotS, bound = cb @ res["stress"], 1e-8 * np.abs(cb * res["stress"]).sum()
        print(f"stress total along the laminate direction: {abs(gotS - want):.2e}, bound {bound:.2e}")
        assert bound > 0 and abs(gotS - want) <= bound
    V = clt.reshape(1, -1) * rng.uniform(-1, 1, (5, clt.size))
    single = [c.field_total_jvp(names, "laminate", v)[0] for v in V]
    for g in (1, 2, 4, 5):
        resg, dWg, itg, _ = c.field_total_jvp(names, "laminate", V[:g], want_states=True)
        assert dWg.shape == (g, m.ndof) and itg.shape == (g,)
        for n in names:
            ref = np.array([s[n] for s in single[:g]])
            dd = np.abs(resg[n] - ref).max() / np.abs(ref).max()
            print(f"group of {g} against one at a time [{n}]: {dd:.1e}")
            assert dd <= 1e-8
    c.close()


# ------------------------------------------------------------------------------------------ 6. surface
def test_operator_surface_and_caller_order():
    """computeMatVecProductFwd(computePartials(field_form, f), v) is ctx.field_output_jvp bit for bit; FEA.field_tangents on a renumbered
    model takes directions and answers in caller order: against assemble(partial, dim=2) @ v and the tangent state, mapped by hand."""
    from femo_alpha_amd import csdl
    from femo_alpha_amd.fea.fea_hip import assemble, computeMatVecProductFwd, computePartials
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
    model = RMShellModel(mesh, shell_bc_func=lambda x: np.less(x[0], 3e-16), record=False, renumber=True)
    model.evaluate(pressure, thickness, E, nu, density, node_disp, debug_mode=False, is_pressure=True)
    recorder.stop()
    fea, ctx = model.fea, model.shell_pde.ctx
    ctx.use_direct_solver(rtol=1e-12)
    ctx.solve_state()
    form = fea.outputs_field_dict["stress"]["form"]
    for arg in ("thickness", "disp_solid"):
        func = fea.states_dict[arg]["function"] if arg == "disp_solid" else fea.inputs_dict[arg]["function"]
        partial = computePartials(form, func)
        v = rng.uniform(-1, 1, func.function_space.dim) * (1e-4 if arg == "disp_solid" else 0.1)
        assert np.array_equal(computeMatVecProductFwd(partial, v), ctx.field_output_jvp("stress", arg, v))
    assert not np.array_equal(model.cell_of_new, np.arange(mesh.nel))
    for arg, width in (("thickness", 1), ("uhat", 3)):
        partial = computePartials(form, fea.inputs_dict[arg]["function"])
        Jw = assemble(computePartials(form, fea.states_dict["disp_solid"]["function"]), dim=2)
        v_caller = rng.uniform(-1, 1, (nn, width)) * (0.1 if arg == "thickness" else 0.01)
        v_solver = v_caller[model.vertex_of_new].ravel()
        dW = ctx.total_jvp(arg, v_solver)[0]
        want = (Jw @ dW + assemble(partial, dim=2) @ v_solver).reshape(mesh.nel, -1)[model.new_of_cell].ravel()
        got = fea.field_tangents(["stress"], arg, v_caller.ravel())["stress"]
        print(f"field_tangents in caller order [{arg}]: {rel(got, want):.1e}")
        assert got.shape == want.shape and rel(got, want) < 1e-10


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_as_it_was():
    from femo_alpha_amd._lib import FemoHipError
    m, c, fields, rng = _context("warped", False, True, seed=2, beta=BETA)
    c.use_direct_solver(rtol=1e-12)
    c.solve_state()
    nc = m.nvc * m.nel
    v = rng.uniform(-1, 1, m.nn)
    w0, info0, h0, u0 = c.get_state(), c.frontal_info(), c.get_field("thickness"), c.get_field("uhat")
    ref = c.field_output_jvp("stress", "thickness", v)
    with pytest.raises(FemoHipError, match="unknown field output"):
        c.field_output_jvp("stress_side", "thickness", v)
    with pytest.raises(FemoHipError, match="unknown field output"):
        c.field_total_jvp(("stress", "stress_side"), "thickness", v)
    with pytest.raises(FemoHipError, match="unknown argument 'pressure'"):
        c.field_output_jvp("stress", "pressure", v)
    with pytest.raises(FemoHipError, match="unknown argument 'pressure'"):
        c.field_total_jvp(("stress",), "pressure", v)
    with pytest.raises(FemoHipError, match="wrong length"):
        c.field_output_jvp("stress", "thickness", np.zeros(m.nn + 1))
    with pytest.raises(FemoHipError, match="wrong length"):
        c.field_total_jvp(("stress",), "uhat", v)
    with pytest.raises(FemoHipError, match="femo_set_ply_table"):
        c.field_output_jvp("ply_failure_field", "disp_solid", np.zeros(m.ndof))
    with pytest.raises(FemoHipError, match="femo_set_ply_table"):
        c.field_total_jvp(("stress", "ply_failure_field"), "thickness", v)
    import ctypes as C
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.full(nc + 1, 7.0)
    assert c.lib.femo_field_output_jvp(c._h, b"stress", b"thickness", 1, p(v), v.size, p(out), nc + 1) != 0          # a wrong nout
    assert "nvc * nel" in c.lib.femo_last_error(c._h).decode()
    assert c.lib.femo_field_output_jvp(c._h, b"stress", b"thickness", 0, p(v), v.size, p(out), nc) != 0              # ndir < 1
    names = (C.c_char_p * 1)(b"stress")
    assert c.lib.femo_field_total_jvp(c._h, 1, names, b"thickness", 1, p(v), v.size, p(out), nc + 1, None, None, None) != 0
    assert "nout" in c.lib.femo_last_error(c._h).decode()
    assert np.all(out == 7.0)                                                    # a refused call writes nothing
    c.set_solver(preconditioner=2, rtol=1e-300, maxit=1, check_every=1)          # cannot be met: strict makes it an error (status 4)
    with pytest.raises(FemoHipError, match="did not converge"):
        c.field_total_jvp(NAMES, "thickness", v)
    c.use_direct_solver(rtol=1e-12)
    assert np.array_equal(c.get_state(), w0) and np.array_equal(c.frontal_info(), info0)
    assert np.array_equal(c.get_field("thickness"), h0) and np.array_equal(c.get_field("uhat"), u0)
    assert np.array_equal(c.field_output_jvp("stress", "thickness", v), ref)
    res, dW, it, rr = c.field_total_jvp(("stress",), "thickness", v)
    assert dW is None and res["stress"].shape == (nc,) and np.all(it >= 1)
    assert np.array_equal(c.get_state(), w0) and np.array_equal(c.frontal_info(), info0)
    c.close()


def test_the_ply_failure_field_refuses_the_shape_derivative():
    from femo_alpha_amd._lib import FemoHipError
    m, o, c, rng, clt, tab = _ply_pair("warped", bc="penalty")
    tight(c)
    c.set_option("strict", 1)
    c.solve_state()
    w0, info0, t0 = c.get_state(), c.frontal_info(), c.get_field("ply_table")
    ref = c.field_output_jvp("ply_failure_field", "disp_solid", w0)
    v = rng.uniform(-1, 1, 3 * m.nn)
    with pytest.raises(FemoHipError, match="shape derivative"):
        c.field_output_jvp("ply_failure_field", "uhat", v)
    with pytest.raises(FemoHipError, match="shape derivative"):
        c.field_total_jvp(("stress", "ply_failure_field"), "uhat", v)
    assert np.array_equal(c.get_state(), w0) and np.array_equal(c.frontal_info(), info0) and np.array_equal(c.get_field("ply_table"), t0)
    assert np.array_equal(c.field_output_jvp("ply_failure_field", "disp_solid", w0), ref)
    res = c.field_total_jvp(("stress", "ply_failure_field"), "ply_table", t0)[0]     # the explicit partial alone: dW = 0
    assert np.array_equal(res["ply_failure_field"], c.field_output_jvp("ply_failure_field", "ply_table", t0))
    assert not np.any(res["stress"])
    c.close()
