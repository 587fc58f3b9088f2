"""Reverse mode of the ply failure field on the GPU (csrc/ply_field_rev.h; femo_field_output_vjp, femo_field_output_jacobian and
femo_field_total_gradients under the name "ply_failure_field"): the products against the numpy reference tests/ply_field_rev_ref.py,
exact transposition with the forward mode, the sparse Jacobian, repeatability, the totals against the forward chain, against the
chain by hand and through the layup, the refusals, and FEA.field_gradients on a renumbered model."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_jvp_ref import fi_gap                                                   # noqa: E402
from femo_alpha_amd.mesh import plate_mesh                                         # noqa: E402
from ply_field_rev_ref import ply_field_jacobians                                  # noqa: E402
from test_gpu_field_jvp import PLY_KINDS, _ply_big                                 # noqa: E402
from test_gpu_laminate import CLAMP, random_laminate, tight                        # noqa: E402
from test_gpu_layup import WRT, _ctx                                               # noqa: E402
from test_gpu_ply_failure import _pair, random_table                               # noqa: E402

pytestmark = pytest.mark.gpu

PF = "ply_failure_field"
ZERO_ARGS = ("laminate", "thickness", "E", "nu", "density", "F_solid")
dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _state(kind):
    """Context, oracle and the random state of test_ply_failure_field_tangents_against_the_reference (drawn first after the pair)."""
    m, o, c, rng, clt, tab = _ply_big() if kind == "big" else _pair(kind)
    w = 2e-3 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    return m, o, c, rng, tab, w


def _one_hot_pair(m, tab, wrt):
    """A cotangent on one (cell, point) and a direction on one entry of the same cell: a slot or sign error cannot average out."""
    npt = tab.shape[1]
    e, p = m.nel // 2, 1
    cb = np.zeros(m.nel * npt)
    cb[e * npt + p] = 1.0
    if wrt == "disp_solid":
        v = np.zeros(m.ndof)
        v[m.cell_dofs()[e][0]] = 1e-4
    else:
        v = np.zeros(tab.size)
        v[16 * (e * npt + p)] = tab[e, p, 0]
    return cb, v


def _directions(rng, m, tab, wrt, n):
    if wrt == "disp_solid":
        return 2e-3 * rng.uniform(-1, 1, (n, m.ndof))
    return (tab[None] * rng.uniform(-1, 1, (n,) + tab.shape)).reshape(n, -1)


# ------------------------------------------------------------------------------------------ 1. products against the reference
@pytest.mark.parametrize("kind", PLY_KINDS + ["big"])
def test_products_against_the_reference(kind):
    """(d field / d w)^T cbar against J_w^T cbar and (d field / d table)^T cbar against J_t^T cbar, 1e-11 of the largest entry (the
    operator-level bar of test_gpu_ply_failure.py): three random cotangents and a one-hot.  A reverse product mixes entries, so an
    entry without a defined maximiser (the two largest FI agree to 1e-6 max|FI|, from the reference alone) is left out by zeroing its
    cotangent: at most 1 % for "big", none for the small kinds.  With these inputs the smallest gap is 1.2e-3 / 1.2e-3 / 7.5e-4 /
    1.3e-3 max|FI| on the small kinds and 2.4e-5 on "big": nothing is left out in any of the five."""
    m, o, c, rng, tab, w = _state(kind)
    npt = tab.shape[1]
    nc = m.nel * npt
    Jw, Jt = ply_field_jacobians(o, w, tab)
    fi = o.failure_index(w)[0]
    gap, fmax = fi_gap(fi), np.abs(fi).max()
    keep = (gap >= 1e-6 * fmax).ravel()
    out = 1.0 - keep.mean()
    print(f"{kind}: smallest gap {gap.min() / fmax:.1e} max|FI|, left out {100 * out:.2f} %")
    assert out <= 0.01
    if kind != "big":
        assert out == 0.0
    hot = _one_hot_pair(m, tab, "disp_solid")[0]
    assert keep[np.flatnonzero(hot)[0]]
    cbs = np.vstack([rng.uniform(-1, 1, (3, nc)), hot]) * keep
    for wrt, J in (("disp_solid", Jw), ("ply_table", Jt)):
        got = c.field_output_vjp(PF, wrt, cbs)
        assert got.shape == (4, J.shape[1])
        for k in range(4):
            want = J.T @ cbs[k]
            err = rel(got[k], want)
            print(f"{kind} [{wrt}, cotangent {k}]: {err:.1e}")
            assert np.abs(want).max() > 0 and err <= 1e-11, (wrt, k)
    c.close()


# ------------------------------------------------------------------------------------------ 2. transposition
@pytest.mark.parametrize("kind", PLY_KINDS + ["big"])
def test_exact_transposition_with_the_forward_mode(kind):
    """|<cbar, J v> - <J^T cbar, v>| <= 1e-11 |cbar| |J v| (the bar of test_gpu_field_jvp.py): three random pairs and a one-hot pair
    per argument.  No entry is left out: both modes take the same branch, ties included."""
    m, o, c, rng, tab, w = _state(kind)
    nc = m.nel * tab.shape[1]
    for wrt in ("disp_solid", "ply_table"):
        pairs = list(zip(rng.uniform(-1, 1, (3, nc)), _directions(rng, m, tab, wrt, 3))) + [_one_hot_pair(m, tab, wrt)]
        for cb, v in pairs:
            Jv = c.field_output_jvp(PF, wrt, v)
            JTc = c.field_output_vjp(PF, wrt, cb)
            gap, scale = abs(cb @ Jv - JTc @ v), np.linalg.norm(cb) * np.linalg.norm(Jv)
            print(f"transposition [{kind}, {wrt}]: {gap:.2e}, bound {1e-11 * scale:.2e}")
            assert scale > 0 and gap <= 1e-11 * scale, wrt
    c.close()


# ------------------------------------------------------------------------------------------ 3. Jacobian
@pytest.mark.parametrize("kind", PLY_KINDS + ["big"])
def test_jacobian_shape_pattern_and_products(kind):
    """Rows nel npt; ld entries per row for the state with the columns among the cell's own dofs, 16 for the table at the columns of
    the row's own recovery point, none for the six arguments the field does not depend on.  J v against the jvp and J^T cbar against
    the vjp, 1e-12 of the largest entry (the bar the stress fields' products are held to against their matrix)."""
    m, o, c, rng, tab, w = _state(kind)
    npt = tab.shape[1]
    nc, ld = m.nel * npt, o.dofs.shape[1]
    for wrt, width in (("disp_solid", ld), ("ply_table", 16)):
        J = c.field_output_jacobian(PF, wrt)
        assert J.shape == (nc, c.arg_size(wrt)) and J.nnz == nc * width
        assert np.array_equal(J.indptr, width * np.arange(nc + 1))
        cols = J.indices.reshape(m.nel, npt, width)
        if wrt == "disp_solid":
            assert np.array_equal(np.sort(cols, axis=2), np.broadcast_to(np.sort(o.dofs, axis=1)[:, None, :], cols.shape))
        else:
            assert np.array_equal(cols.ravel(), np.arange(tab.size))
        V = np.vstack([_directions(rng, m, tab, wrt, 2), _one_hot_pair(m, tab, wrt)[1]])
        cbs = np.vstack([rng.uniform(-1, 1, (2, nc)), _one_hot_pair(m, tab, wrt)[0]])
        for v, cb in zip(V, cbs):
            fwd, rev = rel(c.field_output_jvp(PF, wrt, v), J @ v), rel(c.field_output_vjp(PF, wrt, cb), J.T @ cb)
            print(f"{kind} [{wrt}]: J v {fwd:.1e}, J^T cbar {rev:.1e}")
            assert fwd <= 1e-12 and rev <= 1e-12, wrt
    for wrt in ZERO_ARGS:
        J = c.field_output_jacobian(PF, wrt)
        assert J.shape == (nc, c.arg_size(wrt)) and J.nnz == 0 and not np.any(J.indptr), wrt
    c.close()


# ------------------------------------------------------------------------------------------ 4. repeatability
@pytest.mark.parametrize("kind", ["warped", "tri CG2CR1", "big"])
def test_repeatability_linearity_zeros_and_the_subdomain(kind):
    m, o, c, rng, tab, w = _state(kind)
    nc = m.nel * tab.shape[1]
    cbs = rng.uniform(-1, 1, (3, nc))
    first = {}
    for wrt in ("disp_solid", "ply_table"):
        got = c.field_output_vjp(PF, wrt, cbs)
        assert np.array_equal(got, c.field_output_vjp(PF, wrt, cbs))                              # two calls: the same bits
        for k in range(3):
            assert np.array_equal(got[k], c.field_output_vjp(PF, wrt, cbs[k])), (wrt, k)         # rows equal single calls
        assert np.array_equal(c.field_output_vjp(PF, wrt, 2.0 * cbs[0]), 2.0 * got[0]), wrt      # a power of two commutes
        first[wrt] = got
    for wrt in ZERO_ARGS:
        z = c.field_output_vjp(PF, wrt, cbs)
        assert z.shape == (3, c.arg_size(wrt)) and not np.any(z), wrt
    c.set_cell_tags((np.arange(m.nel) % 3).astype(np.int32), 3)                                   # the field ignores the selection
    c.select_subdomain(1)
    for wrt in ("disp_solid", "ply_table"):
        assert np.array_equal(c.field_output_vjp(PF, wrt, cbs), first[wrt]), wrt
    c.close()


# ------------------------------------------------------------------------------------------ 5. totals against the forward chain
def _solved_pair():
    m, o, c, rng, clt, tab = _pair("warped", bc="penalty")
    tight(c)
    c.solve_state()
    return m, o, c, rng, clt, tab


def test_totals_against_the_forward_chain_and_group_sizes():
    """cbar . field_total_jvp([field], arg, V)[k] against (field_total_gradients(field, cbars, arg) @ V.T)[., k] within
    1e-8 sum |cbar_i dfield_i| (the bar of test_gpu_field_jvp.py::test_totals_against_the_adjoint_chain), for 1, 3 and 5 cotangents (a
    group of four and one more); the rows of a grouped call against single calls, 1e-10.  No solve where R does not see the argument."""
    m, o, c, rng, clt, tab = _solved_pair()
    nc = m.nel * tab.shape[1]
    cbs = rng.uniform(-1, 1, (5, nc))
    dirs = {"laminate": clt.reshape(1, -1) * rng.uniform(-1, 1, (2, clt.size)), "ply_table": _directions(rng, m, tab, "ply_table", 2),
            "F_solid": rng.uniform(-1, 1, (2, c.arg_size("F_solid")))}
    for arg, V in dirs.items():
        res = c.field_total_jvp([PF], arg, V)[0][PF]
        assert res.shape == (2, nc)
        single = np.array([c.field_total_gradients(PF, cb, arg)[0][0] for cb in cbs])
        for nb in (1, 3, 5):
            G, it, rr = c.field_total_gradients(PF, cbs[:nb], arg)
            assert G.shape == (nb, c.arg_size(arg)) and it.shape == (nb,) and rr.shape == (nb,)
            assert np.all(it == 0) and np.all(rr == 0) if arg == "ply_table" else np.all(it >= 1)
            d = rel(G, single[:nb])
            print(f"[{arg}] group of {nb} against one at a time: {d:.1e}")
            assert d <= 1e-10
            want = G @ V.T
            for i in range(nb):
                for k in range(2):
                    got, bound = cbs[i] @ res[k], 1e-8 * np.abs(cbs[i] * res[k]).sum()
                    print(f"[{arg}, {nb} cotangents, cotangent {i}, direction {k}]: {abs(got - want[i, k]):.2e}, bound {bound:.2e}")
                    assert bound > 0 and abs(got - want[i, k]) <= bound, (arg, nb, i, k)
    for arg in ("thickness", "E", "nu", "density"):                       # R does not depend on them in laminate mode, nor does the field
        G, it, rr = c.field_total_gradients(PF, cbs[:2], arg)
        assert G.shape == (2, c.arg_size(arg)) and not np.any(G) and np.all(it == 0) and np.all(rr == 0), arg
    c.close()


# ------------------------------------------------------------------------------------------ 6. totals against the chain by hand
def test_totals_against_the_chain_by_hand():
    """lambda = K^-1 (d field / d w)^T cbar from the public solve, then -(dR / d laminate)^T lambda: 1e-10 of the largest entry."""
    m, o, c, rng, clt, tab = _solved_pair()
    for cb in rng.uniform(-1, 1, (2, m.nel * tab.shape[1])):
        lam = c.solve_linear(c.field_output_vjp(PF, "disp_solid", cb))[0]
        want = -c.dRdarg_T("laminate", lam)
        got = c.field_total_gradients(PF, cb, "laminate")[0][0]
        print(f"laminate total against the chain by hand: {rel(got, want):.1e}")
        assert np.abs(want).max() > 0 and rel(got, want) <= 1e-10
    c.close()


# ------------------------------------------------------------------------------------------ 7. layup
@pytest.mark.parametrize("kind,layup", [("4x20", "2 bot/top"), ("tri", "16 bot/top"), ("5x13", "1 top")])
def test_gradients_with_respect_to_the_layup(kind, layup):
    """Totals with respect to ply thickness and angle against the host's pull-back R.jtu of the totals with respect to the laminate
    and the table, and the partial against the pull-back of the table cotangent alone: 1e-10 of the largest entry (the bar of
    test_gpu_layup.py's reverse totals).  "16 bot/top" has 32 recovery points (the most a cell can hold), "1 top" has one."""
    m, c, R, rng = _ctx(kind, layup, seed=2)
    tight(c)
    c.solve_state(True)
    nc = c.field_size_of(PF)
    assert nc == m.nel * R.npt
    cbs = rng.uniform(-1, 1, (2, nc))
    Gl = c.field_total_gradients(PF, cbs, "laminate")[0]
    Gt = c.field_total_gradients(PF, cbs, "ply_table")[0]
    tb = c.field_output_vjp(PF, "ply_table", cbs)
    for wrt in WRT:
        G, it, rr = c.field_total_gradients(PF, cbs, wrt)
        P = c.field_output_vjp(PF, wrt, cbs)
        assert G.shape == P.shape == (2, c.field_size(wrt)) and np.all(it >= 1)
        for k in range(2):
            ref, refp = R.jtu(wrt, Gl[k], Gt[k]).ravel(), R.jtu(wrt, None, tb[k]).ravel()
            print(f"[{kind}, {layup}, {wrt}, cotangent {k}]: total {rel(G[k], ref):.1e}, partial {rel(P[k], refp):.1e}")
            assert np.abs(ref).max() > 0 and rel(G[k], ref) <= 1e-10, (wrt, k)
            assert np.abs(refp).max() > 0 and rel(P[k], refp) <= 1e-10, (wrt, k)
            assert np.array_equal(P[k], c.field_output_vjp(PF, wrt, cbs[k]))
    c.close()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_context_as_it_was():
    from femo_alpha_amd._lib import FemoHipError
    m, o, c, rng, clt, tab = _solved_pair()
    nc = m.nel * tab.shape[1]
    cb = rng.uniform(-1, 1, nc)
    w0, info0, t0 = c.get_state(), c.frontal_info(), c.get_field("ply_table")
    ref_w, ref_t = c.field_output_vjp(PF, "disp_solid", cb), c.field_output_vjp(PF, "ply_table", cb)
    ref_g = c.field_total_gradients(PF, cb, "ply_table")[0]

    def unchanged():
        assert np.array_equal(c.get_state(), w0) and np.array_equal(c.frontal_info(), info0) and np.array_equal(c.get_field("ply_table"), t0)
        assert np.array_equal(c.field_output_vjp(PF, "disp_solid", cb), ref_w)
        assert np.array_equal(c.field_output_vjp(PF, "ply_table", cb), ref_t)
        assert np.array_equal(c.field_total_gradients(PF, cb, "ply_table")[0], ref_g)
    for call in (lambda: c.field_output_vjp(PF, "uhat", cb), lambda: c.field_output_jacobian(PF, "uhat"),
                 lambda: c.field_total_gradients(PF, cb, "uhat")):
        with pytest.raises(FemoHipError, match="shape derivative"):
            call()
    unchanged()
    for call in (lambda: c.field_output_vjp("stress_side", "disp_solid", np.zeros(m.nvc * m.nel)), lambda: c.field_output_jacobian("stress_side", "disp_solid")):
        with pytest.raises(FemoHipError, match="unknown field output"):
            call()
    with pytest.raises(FemoHipError, match="unknown argument 'pressure'"):
        c._chk(c.lib.femo_field_output_vjp(c._h, PF.encode(), b"pressure", dptr(cb), 1, dptr(np.empty(m.nn)), m.nn))
    # lengths: a cotangent that is no whole number of rows, an output of the wrong length (nothing is written)
    with pytest.raises(ValueError, match="wrong length"):
        c.field_output_vjp(PF, "disp_solid", cb[:-1])
    with pytest.raises(ValueError, match="wrong length"):
        c.field_total_gradients(PF, np.zeros(m.nvc * m.nel + 1), "laminate")
    out = np.full(m.ndof + 1, 7.0)
    assert c.lib.femo_field_output_vjp(c._h, PF.encode(), b"disp_solid", dptr(cb), 1, dptr(out), m.ndof + 1) != 0
    assert "wrong length" in c.lib.femo_last_error(c._h).decode()
    assert c.lib.femo_field_total_gradients(c._h, PF.encode(), 1, dptr(cb), b"laminate", dptr(out), clt.size + 1, None, None) != 0
    assert "wrong length" in c.lib.femo_last_error(c._h).decode()
    assert c.lib.femo_field_output_vjp(c._h, PF.encode(), b"disp_solid", dptr(cb), 0, dptr(out), m.ndof) != 0            # nbar < 1
    assert "nel * npt" in c.lib.femo_last_error(c._h).decode()
    # the state is not an argument of the totals
    assert c.lib.femo_field_total_gradients(c._h, PF.encode(), 1, dptr(cb), b"disp_solid", dptr(out), m.ndof, None, None) != 0
    assert "not an argument" in c.lib.femo_last_error(c._h).decode()
    assert np.all(out == 7.0)
    unchanged()
    # the stress fields keep their argument set: the laminate is still refused for them
    with pytest.raises(FemoHipError, match="unknown argument 'laminate'"):
        c.field_total_gradients("stress", np.zeros(m.nvc * m.nel), "laminate")
    unchanged()
    # without a table every entry point names femo_set_ply_table
    c.set_ply_table(None)
    for call in (lambda: c.field_output_vjp(PF, "disp_solid", cb), lambda: c.field_output_jacobian(PF, "disp_solid"),
                 lambda: c.field_total_gradients(PF, cb, "laminate")):
        with pytest.raises(FemoHipError, match="femo_set_ply_table"):
            call()
    c.set_ply_table(tab)
    unchanged()
    c.close()


def test_the_sparse_jacobian_with_respect_to_the_layup_stays_refused():
    from femo_alpha_amd._lib import FemoHipError
    m, c, R, rng = _ctx("4x20", "2 bot/top", seed=2)
    cb = rng.uniform(-1, 1, c.field_size_of(PF))
    ref = c.field_output_vjp(PF, "ply_thickness", cb)
    for wrt in WRT:
        with pytest.raises(FemoHipError, match="not provided"):
            c.field_output_jacobian(PF, wrt)
    with pytest.raises(FemoHipError, match="wrong length"):
        c._chk(c.lib.femo_field_output_vjp(c._h, PF.encode(), b"ply_angle", dptr(cb), 1, dptr(np.empty(ref.size + 1)), ref.size + 1))
    assert np.array_equal(c.field_output_vjp(PF, "ply_thickness", cb), ref)
    c.close()


# ------------------------------------------------------------------------------------------ 9. FEA.field_gradients
def _model(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel = mesh.nn, mesh.nel
    rng = np.random.default_rng(8)
    clt, tab = random_laminate(nel, rng), random_table(nel, rng)
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    pressure = csdl.Variable(value=np.tile([0.5, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=0.05 * (1 + 0.2 * rng.uniform(-1, 1, nn)), name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=np.ones(nn), name="density")
    node_disp = csdl.Variable(value=np.zeros((nn, 3)), name="node_disp")
    lam = csdl.Variable(value=clt, name="laminate")
    ply = csdl.Variable(value=tab.reshape(nel, -1), name="ply_table")
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, ply_failure=4, rho=20)
    model.evaluate(pressure, thickness, E, nu, density, node_disp, laminate=lam, ply_table=ply)
    recorder.stop()
    ctx = model.shell_pde.ctx
    tight(ctx)
    ctx.solve_state(True)
    return mesh, model, ctx, rng


def test_field_gradients_through_the_model_in_caller_order():
    """FEA.field_gradients takes cotangents and answers in caller order: the same gradients from a renumbered model as from a plain
    one (1e-10), and for "stress" ShellContext.field_total_gradients mapped by hand.  The partial of the field form transposes through
    computeMatVecProductBwd, and assemble(partial, dim=2) is the Jacobian."""
    from femo_alpha_amd.fea.fea_hip import assemble, computeMatVecProductBwd, computePartials
    results = []
    for renumber in (False, True):
        mesh, model, ctx, rng = _model(renumber)
        fea, nel = model.fea, mesh.nel
        cb_ply = rng.uniform(-1, 1, (2, nel * 4))
        cb_vm = rng.uniform(-1, 1, (2, mesh.nvc * nel))
        got = {}
        for arg in ("laminate", "ply_table"):
            got[arg] = fea.field_gradients(PF, cb_ply, arg)
            assert got[arg].shape == (2, ctx.arg_size(arg))
            assert fea.last_solve[0] == 0 if arg == "ply_table" else fea.last_solve[0] >= 1           # R does not see the table: no solve
            one = fea.field_gradients(PF, cb_ply[0], arg)
            assert one.shape == (ctx.arg_size(arg),) and rel(one, got[arg][0]) <= 1e-10
        got["stress"] = fea.field_gradients("stress", cb_vm, "thickness")
        assert fea.last_solve[0] >= 1
        # by hand: cotangent rows caller -> solver order, vertex gradients solver -> caller order
        cell_of_new = np.arange(nel) if fea.cell_of_new is None else fea.cell_of_new
        vertex_of_new = np.arange(mesh.nn) if fea.vertex_of_new is None else fea.vertex_of_new
        if renumber:
            assert not np.array_equal(cell_of_new, np.arange(nel))
        g = ctx.field_total_gradients("stress", cb_vm.reshape(2, nel, -1)[:, cell_of_new].reshape(2, -1), "thickness")[0]
        want = np.empty_like(g)
        want[:, vertex_of_new] = g
        print(f"renumber={renumber}: stress / thickness against the backend mapped by hand: {rel(got['stress'], want):.1e}")
        assert rel(got["stress"], want) <= 1e-10
        form = model.ply_failure_field_form
        for role in ("disp_solid", "ply_table"):
            func = fea.states_dict[role]["function"] if role == "disp_solid" else fea.inputs_dict[role]["function"]
            partial = computePartials(form, func)
            cbs = cb_ply.reshape(2, nel, -1)[:, cell_of_new].reshape(2, -1)                      # the backend's own order
            assert np.array_equal(computeMatVecProductBwd(partial, cbs[0]), ctx.field_output_vjp(PF, role, cbs[0]))
            J = assemble(partial, dim=2)
            assert J.shape == (nel * 4, func.function_space.dim) and rel(J.T @ cbs[0], ctx.field_output_vjp(PF, role, cbs[0])) <= 1e-12
        results.append(got)
    for key in ("laminate", "ply_table", "stress"):
        d = rel(results[1][key], results[0][key])
        print(f"renumbered against plain, caller order [{key}]: {d:.1e}")
        assert np.abs(results[0][key]).max() > 0 and d <= 1e-10, key
