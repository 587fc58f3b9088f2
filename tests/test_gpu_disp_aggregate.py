"""The static max-displacement aggregates on the GPU (femo_set_disp_aggregate; "max_disp", "max_disp1", "max_disp2", "max_disp3"): value
and gradient against tests/disp_aggregate_ref.py, the range of rho x, sub-domains and empty block slots, zero-norm nodes, the four
slots in grouped reverse and forward totals, the exact zeros, repeatability, the handling of the parameters, and the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import disp_aggregate_ref as ref                                                  # noqa: E402
from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles         # noqa: E402
from test_gpu_laminate import BETA, CLAMP, tight                                  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["max_disp", "max_disp1", "max_disp2", "max_disp3"]
D = (0.3, -0.2, 1.0)
# (scaler, direction): norm mode, direction mode with both signs
MODES = [(1.0, None), (2.5, None), (1.0, D), (-1.5, D)]
KINDS = ["quad 4x20", "tri 4x20", "quad 8x40", "tri 8x40", "quad 4x20 CG1CG1"]


def _mesh(kind):
    """plate_mesh(2, 10, 4, 20): 105 vertices and 369 P2 nodes, one block of 256 for the vertices and a ragged last wave either way;
    plate_mesh(2, 10, 8, 40): 369 vertices and 1377 P2 nodes, several blocks."""
    p = plate_mesh(2.0, 10.0, 8, 40) if "8x40" in kind else plate_mesh(2.0, 10.0, 4, 20)
    if kind.startswith("tri"):
        return quads_to_triangles(p)
    return ShellMesh(p.nodes, p.cells, "CG1CG1") if kind.endswith("CG1CG1") else p


def _xmax(w, m, sel, s, d):
    u = w[: 3 * m.nP2].reshape(-1, 3)[sel]
    return abs(s) * (np.linalg.norm(u, axis=1) if d is None else np.abs(u @ np.array(d))).max()


def _check(c, m, w, cells, nodes, s, d, rho, tag=""):
    """Value to 1e-13 relative and gradient to 1e-12 of its largest entry (the bars tests/test_gpu_disp_history.py holds the transient
    kernels to); rotation entries exactly zero."""
    sel = ref.selected_nodes(m, cells, nodes)
    c.set_disp_aggregate(0, rho, s, d, nodes)
    M, Mr = c.functional("max_disp"), ref.value(w, m, sel, rho, s, d)
    g, gr = c.dfunctional("max_disp", "disp_solid"), ref.gradient(w, m, sel, rho, s, d)
    ev, eg = abs(M - Mr) / abs(Mr), np.abs(g - gr).max() / np.abs(gr).max()
    print(f"[{tag}, {nodes}, s {s}, d {d}, rho x {rho * _xmax(w, m, sel, s, d):.3g}, N {sel.size}] value {ev:.1e}, gradient {eg:.1e}")
    assert ev <= 1e-13
    assert eg <= 1e-12
    assert g.size == m.ndof and np.all(g[3 * m.nP2:] == 0.0)
    unsel = np.setdiff1d(np.arange(m.nP2), sel)
    assert np.all(g[: 3 * m.nP2].reshape(-1, 3)[unsel] == 0.0)
    return M, g


def _plain_ctx(m, **kw):
    from femo_alpha_amd.backend import ShellContext
    return ShellContext(m, **kw)


def _solvable(m, seed=0, bc="penalty", **kw):
    """A context with fields, a load and a clamp, ready to solve; (context, thickness, load)."""
    c = _plain_ctx(m, **kw)
    rng = np.random.default_rng(seed)
    nT = m.nel if kw.get("element_wise_material") else m.nn
    h = 0.1 * (1 + 0.2 * rng.uniform(-1, 1, nT))
    f = np.tile([0.5, 0.2, 5.0], (m.nn, 1)) * (1 + 0.3 * rng.uniform(-1, 1, (m.nn, 3)))
    for k, v in dict(thickness=h, E=[1e8], nu=[0.3], density=[1.0], F_solid=f).items():
        c.set_field(k, v)
    if bc == "penalty":
        c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    else:
        c.set_strong_dofs(m.locate_dofs_geometrical(CLAMP))
    return c, h, f


# ------------------------------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("kind", KINDS)
def test_value_and_state_gradient_against_the_reference(kind):
    """Random states set with set_state (no solve); both modes, both node kinds, both signs of the scaler; rho |s| max x = 50."""
    m = _mesh(kind)
    c = _plain_ctx(m)
    rng = np.random.default_rng(1)
    w = 1e-2 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    for nodes in ("vertices", "all"):
        sel = ref.selected_nodes(m, None, nodes)
        for s, d in MODES:
            _check(c, m, w, None, nodes, s, d, 50.0 / _xmax(w, m, sel, s, d), kind)
    c.close()


# ------------------------------------------------------------------------------------------ 2. range
@pytest.mark.parametrize("kind", ["quad 4x20", "tri 8x40"])
def test_rho_x_of_ten_thousand_where_an_unshifted_exponential_overflows(kind):
    m = _mesh(kind)
    c = _plain_ctx(m)
    rng = np.random.default_rng(2)
    w = 1e-2 * rng.uniform(-1, 1, m.ndof)
    c.set_state(w)
    for nodes in ("vertices", "all"):
        sel = ref.selected_nodes(m, None, nodes)
        for s, d in MODES:
            rho = 1e4 / _xmax(w, m, sel, s, d)
            c.set_disp_aggregate(0, rho, s, d, nodes)
            M, Mr = c.functional("max_disp"), ref.value(w, m, sel, rho, s, d)
            g = c.dfunctional("max_disp", "disp_solid")
            print(f"[{kind}, {nodes}, s {s}, d {d}] value {abs(M - Mr) / abs(Mr):.1e}")
            assert np.isfinite(M) and abs(M - Mr) <= 1e-13 * abs(Mr)
            assert np.all(np.isfinite(g))
    c.close()


# ------------------------------------------------------------------------------------------ 3. selection and empty slots
def test_subdomains_empty_block_slots_and_an_empty_tag():
    """Three cells of the last rows of the larger mesh: their nodes carry high indices, so the leading blocks hold only empty pairs
    (and with nodes = 'vertices' the blocks beyond the vertices too).  A second sub-domain elsewhere, and a third without cells."""
    from femo_alpha_amd._lib import FemoHipError
    for kind in ("quad 8x40", "tri 8x40"):
        m = _mesh(kind)
        c = _plain_ctx(m)
        rng = np.random.default_rng(3)
        w = 1e-2 * rng.uniform(-1, 1, m.ndof)
        c.set_state(w)
        tags = -np.ones(m.nel, dtype=np.int32)
        tags[m.nel - 3:] = 0
        tags[m.nel // 3: m.nel // 3 + 41] = 1
        c.set_cell_tags(tags, 3)
        first = ref.selected_nodes(m, np.flatnonzero(tags == 0), "all")
        assert first.min() >= 256                                                  # block 0 of the node kernels is empty
        for sub in (0, 1, -1):
            cells = None if sub < 0 else np.flatnonzero(tags == sub)
            c.select_subdomain(sub)
            for nodes in ("vertices", "all"):
                sel = ref.selected_nodes(m, cells, nodes)
                for s, d in (MODES[0], MODES[3]):
                    _check(c, m, w, cells, nodes, s, d, 50.0 / _xmax(w, m, sel, s, d), f"{kind}, sub {sub}")
        # N of the whole mesh from the zero state: M = log N / (rho s)
        c.select_subdomain(-1)
        c.set_state(np.zeros(m.ndof))
        for nodes, N in (("vertices", m.nn), ("all", m.nP2)):
            c.set_disp_aggregate(0, 10.0, 2.0, None, nodes)
            assert abs(np.exp(c.functional("max_disp") * 20.0) - N) <= 1e-9 * N
        c.set_state(w)
        c.select_subdomain(2)
        for call in (lambda: c.functional("max_disp"), lambda: c.dfunctional("max_disp", "disp_solid"),
                     lambda: c.dfunctional("max_disp", "thickness")):
            with pytest.raises(FemoHipError, match="sub-domain 2"):
                call()
        # new tags: the kept masks are dropped, the same selections answer for the new cells
        tags2 = np.roll(tags, 7)
        c.set_cell_tags(tags2, 3)
        c.select_subdomain(1)
        cells = np.flatnonzero(tags2 == 1)
        sel = ref.selected_nodes(m, cells, "all")
        _check(c, m, w, cells, "all", 1.0, None, 50.0 / _xmax(w, m, sel, 1.0, None), f"{kind}, new tags")
        c.close()


# ------------------------------------------------------------------------------------------ 4. zero-norm nodes
def test_zero_state_and_strongly_clamped_nodes_after_a_solve():
    m = _mesh("quad 4x20")
    c, h, f = _solvable(m, seed=4, bc="strong")
    c.set_state(np.zeros(m.ndof))
    for nodes, N in (("vertices", m.nn), ("all", m.nP2)):
        for rho, s in ((100.0, 1.0), (7.0, 3.0)):
            c.set_disp_aggregate(0, rho, s, None, nodes)
            M = c.functional("max_disp")
            assert abs(M - np.log(N) / (rho * s)) <= 1e-13 * M
            assert not np.any(c.dfunctional("max_disp", "disp_solid"))
    c.use_direct_solver()
    c.solve_state(True)
    w = c.get_state()
    u = w[: 3 * m.nP2].reshape(-1, 3)
    clamped = np.flatnonzero(np.linalg.norm(u, axis=1) == 0.0)
    assert clamped.size >= 5                                                      # the clamped edge: exact zeros
    for nodes in ("vertices", "all"):
        sel = ref.selected_nodes(m, None, nodes)
        rho = 5.0 / _xmax(w, m, sel, 1.0, None)
        M, g = _check(c, m, w, None, nodes, 1.0, None, rho, "clamped")
        assert np.isfinite(M) and np.all(np.isfinite(g))
        assert np.all(g[: 3 * m.nP2].reshape(-1, 3)[clamped] == 0.0)
    c.close()


# ------------------------------------------------------------------------------------------ 5. four slots in one grouped call
GROUP = ["compliance", "max_disp", "max_disp1", "pnorm_stress", "max_disp2"]


def _set_group_slots(c, m, w):
    """Slot 0: the magnitude over the vertices; slot 1: an upper limit on every node of sub-domain 0; slot 2: a lower limit on the
    vertices of sub-domain 1; slot 3: a skewed direction on every node.  rho |s| max x = 5: every node contributes.  Returns per name
    (sub-domain, cells, nodes, s, d, rho)."""
    tags = (np.arange(m.nel) % 3 - 1).astype(np.int32)                              # -1, 0, 1
    c.set_cell_tags(tags, 2)
    spec = {}
    for slot, (sub, nodes, s, d) in enumerate([(-1, "vertices", 1.0, None), (0, "all", 1.0, (0.0, 0.0, 1.0)),
                                               (1, "vertices", -1.0, (0.0, 0.0, 1.0)), (-1, "all", 2.0, D)]):
        cells = None if sub < 0 else np.flatnonzero(tags == sub)
        sel = ref.selected_nodes(m, cells, nodes)
        rho = 5.0 / _xmax(w, m, sel, s, d)
        c.set_disp_aggregate(slot, rho, s, d, nodes)
        spec[NAMES[slot]] = (sub, sel, s, d, rho)
    return spec


def _by_hand(c, name, sub, arg):
    """The route through the public calls one functional at a time: dJ/dw, one adjoint solve, dJ/d arg - (dR/d arg)^T lambda."""
    c.select_subdomain(sub)
    lam = c.solve_linear(c.dfunctional(name, "disp_solid"))[0]
    g = c.dfunctional(name, arg) - c.dRdarg_T(arg, lam)
    c.select_subdomain(-1)
    return g


def test_grouped_totals_against_the_public_route_and_the_cpu_oracle():
    """1e-10 of the largest entry against the route by hand (the project's bar for this comparison) and 1e-7 against the CPU oracle's
    adjoint seeded with the reference gradient (the bar test_rm_shell_model_protocol uses for totals against the oracle)."""
    from oracle.rm_shell_oracle import ShellOracle
    m = _mesh("quad 4x20")
    c, h, f = _solvable(m, seed=5)
    tight(c)
    c.solve_state(True)
    w = c.get_state()
    c.set_stress_params(1.0 / c.field_output("stress").max(), 10.0)               # (m vm) of order one: a stress gradient that is not zero
    spec = _set_group_slots(c, m, w)
    subs = [-1, spec["max_disp"][0], spec["max_disp1"][0], -1, spec["max_disp2"][0]]
    o = ShellOracle(m, penalty_facets=m.penalty_facets(CLAMP), beta=BETA)
    o.set_fields(h=h, E=1e8, nu=0.3, rho=1.0, f=f)
    o.factorize()
    for arg in ("thickness", "E", "F_solid"):
        G, its, rrs = c.total_gradients(GROUP, arg, subdomains=subs)
        for i, name in enumerate(GROUP):
            hand = _by_hand(c, name, subs[i], arg)
            err = np.abs(G[i] - hand).max() / np.abs(hand).max()
            print(f"grouped against the public route [{name}, {arg}, sub {subs[i]}]: {err:.1e}")
            assert np.abs(hand).max() > 0 and err <= 1e-10, (name, arg)
            if name in spec:
                sub, sel, s, d, rho = spec[name]
                lam = o.solve_adjoint(ref.gradient(w, m, sel, rho, s, d))
                orc = -o.dRdf_T(lam) if arg == "F_solid" else -o.dRdfield_T("h" if arg == "thickness" else arg, w, lam)
                err = np.abs(G[i] - orc).max() / np.abs(orc).max()
                print(f"grouped against the oracle's adjoint [{name}, {arg}]: {err:.1e}")
                assert err <= 1e-7, (name, arg)
    c.close()


def test_grouped_totals_in_layup_mode_against_the_composed_host_route():
    """d/d ply_thickness = J^T (d/d laminate, d/d ply_table) with the host Jacobian of tests/layup_ref.py, as
    tests/test_gpu_layup.py composes it; 1e-10 of the largest entry."""
    from test_gpu_layup import _ctx as _layup_ctx
    m, c, R, rng = _layup_ctx("4x20", "2 bot/top", seed=5)
    tight(c)
    c.solve_state(True)
    w = c.get_state()
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    spec = _set_group_slots(c, m, w)
    names = ["max_disp", "ply_failure", "max_disp1", "max_disp2", "max_disp3"]
    subs = [spec[n][0] if n in spec else -1 for n in names]
    Gl = c.total_gradients(names, "laminate", subdomains=subs)[0]
    Gt = c.total_gradients(names, "ply_table", subdomains=subs)[0]
    for wrt in ("ply_thickness", "ply_angle"):
        G = c.total_gradients(names, wrt, subdomains=subs)[0]
        for i, name in enumerate(names):
            want = R.jtu(wrt, Gl[i], Gt[i]).ravel()
            err = np.abs(G[i] - want).max() / np.abs(want).max()
            print(f"layup totals [{name}, {wrt}, sub {subs[i]}]: {err:.1e}")
            assert np.abs(want).max() > 0 and err <= 1e-10, (name, wrt)
    for name in NAMES:                                                             # the explicit partials: exact zeros
        for wrt in ("laminate", "ply_table", "ply_thickness", "ply_angle"):
            g = c.dfunctional(name, wrt)
            assert g.size == c.arg_size(wrt) and not np.any(g), (name, wrt)
    c.close()


# ------------------------------------------------------------------------------------------ 6. forward mode
def test_forward_mode_equals_the_reverse_totals():
    """total_jvp of the four names along two random thickness directions = total_gradients . v to 1e-8 (tests/test_gpu_layup.py)."""
    m = _mesh("quad 4x20")
    c, h, f = _solvable(m, seed=6)
    tight(c)
    c.solve_state(True)
    spec = _set_group_slots(c, m, c.get_state())
    subs = [spec[n][0] for n in NAMES]
    G = c.total_gradients(NAMES, "thickness", subdomains=subs)[0]
    rng = np.random.default_rng(6)
    V = rng.uniform(0.5, 1.0, (2, m.nn)) * h
    dW, dJ, _, _ = c.total_jvp("thickness", V, NAMES, subdomains=subs)
    want = G @ V.T
    for i, name in enumerate(NAMES):
        for k in range(2):
            err = abs(dJ[i, k] - want[i, k]) / abs(want[i, k])
            print(f"total_jvp against total_gradients . v [{name}, direction {k}]: {err:.1e}")
            assert err <= 1e-8, (name, k)
    c.close()


# ------------------------------------------------------------------------------------------ 7. exact zeros
def test_every_argument_but_the_state_gives_exact_zeros():
    from femo_alpha_amd._lib import FemoHipError, dptr
    m = _mesh("tri 4x20")
    c, h, f = _solvable(m, seed=7)
    c.set_field("uhat", 0.02 * np.random.default_rng(7).uniform(-1, 1, (m.nn, 3)))
    c.use_direct_solver()
    c.solve_state(True)
    _set_group_slots(c, m, c.get_state())
    for name in NAMES:
        assert np.any(c.dfunctional(name, "disp_solid"))
        for wrt in ("thickness", "E", "nu", "density", "F_solid", "uhat"):
            g = c.dfunctional(name, wrt)
            assert g.size == c.arg_size(wrt) and not np.any(g), (name, wrt)
        for wrt in ("laminate", "tickness"):                                      # no field outside laminate mode; no field at all
            with pytest.raises(FemoHipError, match="unknown argument"):
                c._chk(c.lib.femo_dfunctional(c._h, name.encode(), wrt.encode(), dptr(np.zeros(8)), 8))
    with pytest.raises(FemoHipError, match="unknown functional"):
        c.functional("max_disp4")
    c.close()


# ------------------------------------------------------------------------------------------ 8. repeatability
def test_value_gradient_and_grouped_totals_repeat_bit_for_bit():
    """The value and the gradient on the larger mesh (several block slots, merged in block order), for all four slots.

    The grouped totals repeat bit for bit where the solves behind them do, so they are checked with the matrix-free Jacobi-PCG on a small
    strongly clamped plate with a thickness per cell: its dot products sum at most two non-zero block results (either order gives the
    same bits), the operator sums element results in a fixed order, there is no penalty term, and every cell owns its entry of the
    thickness gradient -- whatever differed between two calls would come from the aggregate's kernels or from the grouping.  With the
    multifrontal solver the same comparison gives 1e-15 of the largest entry on the rows of "compliance" and of the aggregates alike:
    its forward sweep adds the contributions of sibling fronts with float atomics (csrc/sweeps_multi.h), which is repeatable to
    rounding only (tests/test_gpu_dynamic.py says the same of the transient path)."""
    m = _mesh("tri 8x40")
    c = _plain_ctx(m)
    w = 1e-2 * np.random.default_rng(8).uniform(-1, 1, m.ndof)
    c.set_state(w)
    spec = _set_group_slots(c, m, w)
    for name in NAMES:
        c.select_subdomain(spec[name][0])
        M, g = c.functional(name), c.dfunctional(name, "disp_solid")
        for _ in range(2):
            assert c.functional(name) == M and np.array_equal(c.dfunctional(name, "disp_solid"), g), name
    c.close()
    m = plate_mesh(2.0, 10.0, 3, 7)
    assert m.ndof <= 512 and m.nel <= 64
    c, h, f = _solvable(m, seed=8, bc="strong", element_wise_material=True)
    c.set_solver(preconditioner=0, rtol=1e-12, maxit=200000, check_every=50)
    its, rr = c.solve_state(True)
    spec = _set_group_slots(c, m, c.get_state())
    subs = [-1, spec["max_disp"][0], spec["max_disp1"][0], -1, spec["max_disp2"][0]]
    G1, it1, _ = c.total_gradients(GROUP, "thickness", subdomains=subs)
    G2, it2, _ = c.total_gradients(GROUP, "thickness", subdomains=subs)
    print(f"Jacobi-PCG: state in {its} iterations (relres {rr:.1e}), adjoints in {it1.tolist()}")
    for i, name in enumerate(GROUP):
        print(f"grouped totals, second call [{name}]: {np.abs(G1[i] - G2[i]).max() / np.abs(G1[i]).max():.1e}")
    assert np.all(np.abs(G1).max(axis=1) > 0) and np.array_equal(it1, it2)
    assert np.array_equal(G1, G2)
    c.close()


# ------------------------------------------------------------------------------------------ 9. handling
def test_refusals_change_nothing_and_ghost_and_dist_contexts_are_not_provided():
    from femo_alpha_amd._lib import FemoHipError
    m = _mesh("quad 4x20")
    c, h, f = _solvable(m, seed=9)
    c.use_direct_solver()
    c.solve_state(True)
    # the defaults before any call: rho = 100, s = 1, no direction, the vertices
    w = c.get_state()
    sel = ref.selected_nodes(m, None, "vertices")
    for name in NAMES:
        Mr = ref.value(w, m, sel, 100.0)
        assert abs(c.functional(name) - Mr) <= 1e-13 * abs(Mr), name
    spec = _set_group_slots(c, m, w)
    info = c.frontal_info()

    def snapshot():
        out = [c.get_state()] + [c.get_field(k) for k in ("thickness", "E", "nu", "density", "F_solid", "uhat")]
        for name in NAMES:
            c.select_subdomain(spec[name][0])
            out += [np.array([c.functional(name)]), c.dfunctional(name, "disp_solid")]
        c.select_subdomain(-1)
        return out
    before = snapshot()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(slot=-1), "slot"), (dict(slot=4), "slot"), (dict(rho=0.0), "rho"), (dict(rho=-1.0), "rho"), (dict(rho=nan), "rho"),
           (dict(rho=inf), "rho"), (dict(scaler=0.0), "scaler"), (dict(scaler=nan), "scaler"), (dict(scaler=inf), "scaler"),
           (dict(scaler=-1.0), "direction"), (dict(direction=(0.0, 0.0, 0.0)), "direction"), (dict(direction=(0.0, nan, 1.0)), "direction"),
           (dict(direction=(inf, 0.0, 1.0)), "direction")]
    for slot in range(4):
        for kw, match in bad:
            args = dict(slot=slot, rho=3.0, scaler=0.5, direction=None, nodes="all")
            args.update(kw)
            with pytest.raises(FemoHipError, match=match):
                c.set_disp_aggregate(**args)
    with pytest.raises(FemoHipError, match="nodes"):
        c._chk(c.lib.femo_set_disp_aggregate(c._h, 0, 3.0, 0.5, None, 2))
    with pytest.raises(ValueError):
        c.set_disp_aggregate(0, nodes="edges")
    after = snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert c.frontal_info() == info                                                # the operator never saw the parameters or the calls
    # a non-finite translation at a selected node: the value call fails with a message; at an unselected node it is not looked at
    w2 = w.copy()
    w2[3 * (m.nP2 - 1) + 1] = nan                                                 # the last P2 node is no vertex
    c.set_state(w2)
    c.set_disp_aggregate(0, 10.0, 1.0, None, "all")
    with pytest.raises(FemoHipError, match="non-finite"):
        c.functional("max_disp")
    c.set_disp_aggregate(0, 10.0, 1.0, None, "vertices")
    assert np.isfinite(c.functional("max_disp"))
    c.close()
    # ghost entries and the element-partitioned driver: replicated separator nodes would be counted once per partition
    g = _plain_ctx(m, nghost=3)
    d = _plain_ctx(m)
    d.use_direct_solver()
    d.dist_setup(np.zeros(0, dtype=np.int32), 1, 0, np.zeros(0, dtype=np.int32))
    for ctx in (g, d):
        for call in (lambda: ctx.functional("max_disp"), lambda: ctx.dfunctional("max_disp2", "disp_solid"),
                     lambda: ctx.dfunctional("max_disp1", "thickness")):
            with pytest.raises(FemoHipError, match="not provided"):
                call()
        ctx.close()


# ------------------------------------------------------------------------------------------ 10. the model
def _model_inputs(csdl, nn, h0):
    pressure = csdl.Variable(value=np.tile([0.0, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=h0, name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=10.0 * np.ones(nn), name="density")
    node_disp = csdl.Variable(value=np.zeros((nn, 3)), name="node_disp")
    return pressure, thickness, E, nu, density, node_disp


@pytest.mark.parametrize("renumber", [False, True])
def test_outputs_and_totals_through_the_model(renumber):
    """A magnitude over the whole mesh and a lower limit (direction z, scaler -1) on a tagged tip, at rho |s| max x = 5.  One
    check_totals row on the largest gradient entry for the new output and for "compliance", same step, same case: both finite
    differences share the solves and the truncation of the step; the aggregate adds the curvature of the KS function at rho s x = 5,
    which the factor ten covers."""
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel = mesh.nn, mesh.nel
    rng = np.random.default_rng(10)
    h0 = 0.1 * (1 + 0.2 * rng.uniform(-1, 1, nn))
    tip = np.flatnonzero(mesh.nodes[mesh.cells].mean(axis=1)[:, 0] > 8.0)
    root = np.flatnonzero(mesh.nodes[mesh.cells].mean(axis=1)[:, 0] < 2.0)
    assert tip.size and root.size
    mesh_tags = {"root": root, "tip": tip}
    # the deflection first, for rho: a plain model
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    plain = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, mesh_tags=mesh_tags, renumber=renumber)
    out0 = plain.evaluate(*_model_inputs(csdl, nn, h0))
    recorder.stop()
    parent_outputs = ["compliance", "mass", "elastic_energy", "pnorm_stress", "pnorm_stress_root", "pnorm_stress_tip"]
    assert list(plain.fea.outputs_dict) == parent_outputs                         # without the keyword: the outputs of the parent
    assert getattr(out0, "max_disp") is None
    umax = np.linalg.norm(out0.disp_extracted.value, axis=1).max()
    rho = 5.0 / umax
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    inputs = _model_inputs(csdl, nn, h0)
    thickness = inputs[1]
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, mesh_tags=mesh_tags, renumber=renumber,
                         max_disp=[dict(rho=rho), dict(rho=rho, direction=(0, 0, 1), scaler=-1, tag="tip", name="tip_low")])
    out = model.evaluate(*inputs)
    recorder.stop()
    assert list(model.fea.outputs_dict) == parent_outputs + ["max_disp", "tip_low"]
    assert model.fea.outputs_dict["tip_low"]["arguments"] == ["disp_solid"]
    ctx, sm = model.shell_pde.ctx, model.mesh                                     # the solver's mesh and order
    w = out.disp_solid.value
    cases = [("max_disp", "max_disp", -1, None, 1.0, None), ("tip_low", "max_disp1", model.association_table["tip"], model.mesh_tags["tip"], -1.0, (0.0, 0.0, 1.0))]
    G = ctx.total_gradients([c[1] for c in cases], "thickness", subdomains=[c[2] for c in cases])[0]
    for i, (name, fn, sub, cells, s, d) in enumerate(cases):
        sel = ref.selected_nodes(sm, cells, "vertices")
        M, Mr = float(np.ravel(getattr(out, name).value)[0]), ref.value(w, sm, sel, rho, s, d)
        print(f"[model, renumber {renumber}, {name}] value {M:.6e}, against the reference {abs(M - Mr) / abs(Mr):.1e}")
        assert abs(M - Mr) <= 1e-13 * abs(Mr), name
        got = np.asarray(recorder.compute_totals(getattr(out, name), thickness)).ravel()
        want = np.zeros(nn)
        want[model.vertex_of_new] = G[i]                                          # solver order -> caller order
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"[model, renumber {renumber}, {name}] compute_totals against total_gradients: {err:.1e}")
        assert err <= 1e-10, name
    # the lower limit sits below the smallest z displacement of the tip, within log N / (rho |s|)
    uz = w[: 3 * sm.nn].reshape(-1, 3)[ref.selected_nodes(sm, model.mesh_tags["tip"], "vertices"), 2]
    low = float(np.ravel(out.tip_low.value)[0])
    assert uz.min() - np.log(uz.size) / rho <= low <= uz.min()
    if not renumber:
        dA = np.asarray(recorder.compute_totals(out.max_disp, thickness)).ravel()
        i0 = int(np.argmax(np.abs(dA)))
        row_m = recorder.check_totals(out.max_disp, thickness, step=1e-3, indices=[i0])[0]
        row_c = recorder.check_totals(out.compliance, thickness, step=1e-3, indices=[i0])[0]
        print(f"check_totals at entry {i0}, step 1e-3: max_disp {row_m[3]:.2e} ({row_m[1]:.8e} against {row_m[2]:.8e}), "
              f"compliance {row_c[3]:.2e} ({row_c[1]:.8e} against {row_c[2]:.8e})")
        assert row_m[3] <= 10.0 * row_c[3]


def test_the_model_refuses_bad_specifications_and_works_with_a_layup():
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    from test_gpu_layup import _layup
    from test_layup_cpu import _plies
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel, nply = mesh.nn, mesh.nel, 2
    for bad in ([dict()] * 5, [], dict(tag="tip"), dict(colour=1), [dict(name="a"), dict(name="a")], dict(name="compliance")):
        with pytest.raises(ValueError, match="max_disp"):
            RMShellModel(mesh, shell_bc_func=CLAMP, record=False, max_disp=bad)
    rng = np.random.default_rng(11)
    pc = _plies(nply, rng)
    t, theta = _layup(nel, nply, rng)
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    inputs = _model_inputs(csdl, nn, 0.05 * np.ones(nn))
    ply_t = csdl.Variable(value=t, name="ply_thickness")
    ply_a = csdl.Variable(value=theta, name="ply_angle")
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=True, laminate=True,
                         layup=dict(plies=pc, t=t[0], theta=theta[0], surfaces=()), max_disp=dict(rho=20.0, nodes="all"))
    out = model.evaluate(*inputs, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    ctx, sm = model.shell_pde.ctx, model.mesh
    sel = ref.selected_nodes(sm, None, "all")
    M, Mr = float(np.ravel(out.max_disp.value)[0]), ref.value(out.disp_solid.value, sm, sel, 20.0)
    assert abs(M - Mr) <= 1e-13 * abs(Mr)
    got = np.asarray(recorder.compute_totals(out.max_disp, ply_t)).reshape(nel, nply)
    want = np.empty((nel, nply))
    want[model.cell_of_new] = ctx.total_gradient("max_disp", "ply_thickness")[0].reshape(nel, nply)
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
