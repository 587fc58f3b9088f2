"""The tail-delay pass of the symbolic analysis (csrc/symbolic.cpp section 3b, solver/symbolic.py ``_tail_delay``): whole tree levels
hand the pivots of a short last outer panel (128 columns) to their parents, so that the level's lock-step factorisation has one
chain step fewer.  Host only: the C++ plan against its numpy twin, the invariants of a plan, the cases in which the pass must
refuse, and the numbers through the CPU multifrontal factorisation (both plans factorise the same matrix exactly)."""
import numpy as np
import pytest

from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles
from femo_alpha_amd.solver import _native, symbolic

NBO = 128


def _two_plates(nx, ny):
    a = plate_mesh(2.0, 10.0, nx, ny)
    return ShellMesh(np.vstack([a.nodes, a.nodes + [0.0, 12.0, 0.0]]), np.vstack([a.cells, a.cells + a.nn]))


# name -> (mesh, leaf size).  Largest pivot count per level without the pass (found by building the plans):
#   plate16x80   300  45  72  90 150 150 150      level 4 has a tail of 22 DOFs: in (128, 160]
#   plate14x70   270  54  72  90 132 132 132      tails of 14, 4, 4: a cascade over three levels
#   refuse26x65  105  39  54  72  90 117 153 240 240   level 6 (153) would put 240 + 2 x 27 pivots into its parents: over 256, refused
#   tri16x80     300  45  72  90 150 150 150      CG2CG1 triangles
#   cg1_24x120   144  42  48  72  90 150 150 150  CG1CG1: every node carries six DOFs
#   two30x30     225  45  81  81 135 135 276 0    two components, an empty root: the component roots (276) have nowhere to delay to
CASES = {
    "plate16x80": (lambda: plate_mesh(2.0, 10.0, 16, 80), 24),
    "plate14x70": (lambda: plate_mesh(2.0, 10.0, 14, 70), 28),
    "refuse26x65": (lambda: plate_mesh(2.0, 10.0, 26, 65), 12),
    "tri16x80": (lambda: quads_to_triangles(plate_mesh(2.0, 10.0, 16, 80)), 48),
    "cg1_24x120": (lambda: plate_mesh(2.0, 10.0, 24, 120, element="CG1CG1"), 24),
    "two30x30": (lambda: _two_plates(30, 30), 24),
}
SHRINKS = {"plate16x80": [4], "plate14x70": [0, 4, 5], "tri16x80": [4], "cg1_24x120": [0, 5], "two30x30": [4, 5]}   # at tail_max 32
PLAN_ARRAYS = ("npiv", "nf", "parent", "left", "right", "front_dofs", "up_map", "elem_front", "elem_map", "height", "eorder", "dof_off",
               "front_off")
_cache = {}


def _mesh(name):
    if name not in _cache:
        _cache[name] = CASES[name][0]()
    return _cache[name]


def _plan(name, tail_max, impl="native"):
    key = (name, tail_max, impl)
    if key not in _cache:
        _cache[key] = symbolic.build_plan(_mesh(name), CASES[name][1], impl=impl, tail_max=tail_max)
    return _cache[key]


def _same_plan(a, b):
    for k in ("ntree", "nlevels", "nleaves"):
        assert getattr(a, k) == getattr(b, k), k
    for k in PLAN_ARRAYS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.shape == y.shape and np.array_equal(x, y), k
    assert len(a.level_nodes) == len(b.level_nodes)
    for x, y in zip(a.level_nodes, b.level_nodes):
        assert np.array_equal(x, y)


def _panels(plan):
    return [int(-(-int(plan.npiv[l].max()) // NBO)) for l in plan.level_nodes]


@pytest.mark.parametrize("tail_max", [0, 16, 32])
@pytest.mark.parametrize("name", sorted(CASES))
def test_native_plan_equals_the_numpy_plan(name, tail_max):
    a, b = _plan(name, tail_max, "python"), _plan(name, tail_max)
    _same_plan(a, b)
    for k in ("dofs", "saved"):
        assert np.array_equal(a.tail_delay[k], b.tail_delay[k]), k
    assert tuple(a.tail_delay["flops3"]) == tuple(b.tail_delay["flops3"])
    assert a.summary() == b.summary()


@pytest.mark.parametrize("name,depth", [("plate16x80", 1), ("plate14x70", 2), ("tri16x80", 1)])
def test_native_tree_equals_the_numpy_tree_and_the_partition_boundary_holds(name, depth):
    """With a forced partition depth a front at depth <= min_depth never delays: the replicated top and the boundaries (Schur blocks)
    of the subtree roots are those of the plain tree; a subtree root may receive pivots from its own subtree, in front of its own."""
    m, leaf = _mesh(name), CASES[name][1]
    a = symbolic.analyse(m, leaf, min_depth=depth, impl="python", tail_max=32)
    b = symbolic.analyse(m, leaf, min_depth=depth, tail_max=32)
    off = symbolic.analyse(m, leaf, min_depth=depth)
    for k in ("lo", "hi", "left", "right", "parent", "depth", "height", "eorder", "epos", "owner"):
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    for t in range(a.ntree):
        assert np.array_equal(a.piv_nodes[t], b.piv_nodes[t])
        assert np.array_equal(a.bnd_nodes[t], b.bnd_nodes[t])
        if b.depth[t] < depth:
            assert np.array_equal(b.piv_nodes[t], off.piv_nodes[t]) and np.array_equal(b.bnd_nodes[t], off.bnd_nodes[t])
        if b.depth[t] == depth:
            assert np.array_equal(b.bnd_nodes[t], off.bnd_nodes[t])
            assert np.array_equal(b.piv_nodes[t][b.piv_nodes[t].size - off.piv_nodes[t].size:], off.piv_nodes[t])


@pytest.mark.parametrize("tail_max", [16, 32])
@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_invariants_with_the_pass_on(name, tail_max):
    m, p, off = _mesh(name), _plan(name, tail_max), _plan(name, 0)
    # every DOF is a pivot of exactly one front
    assert int(p.npiv.sum()) == m.ndof
    piv = np.concatenate([p.front_dofs[p.dof_off[t]:p.dof_off[t] + p.npiv[t]] for t in range(p.ntree)])
    assert np.array_equal(np.sort(piv), np.arange(m.ndof))
    for t in range(p.ntree):
        fd = p.front_dofs[p.dof_off[t]:p.dof_off[t + 1]]
        assert np.unique(fd).size == fd.size
        par = p.parent[t]
        bd = fd[p.npiv[t]:]
        if par < 0:
            assert bd.size == 0
            continue
        # the boundary rows of a front are rows of its parent, at the places up_map names, in increasing order
        rows = p.up_map[p.dof_off[t] + p.npiv[t]:p.dof_off[t + 1]]
        assert np.all(rows >= 0) and np.all(rows < p.nf[par])
        assert np.array_equal(p.front_dofs[p.dof_off[par] + rows], bd)
        assert np.all(np.diff(rows) > 0), "node_order 1: a child's rows rise along the parent's"
        assert np.all(p.up_map[p.dof_off[t]:p.dof_off[t] + p.npiv[t]] == -1)
    # a parent front is exactly its pivots and what its children pass up
    for t in np.nonzero(p.left >= 0)[0]:
        kids = set(np.concatenate([p.front_dofs[p.dof_off[c] + p.npiv[c]:p.dof_off[c + 1]] for c in (p.left[t], p.right[t])]).tolist())
        fd = p.front_dofs[p.dof_off[t]:p.dof_off[t + 1]]
        assert set(fd.tolist()) == kids | set(fd[:p.npiv[t]].tolist()) and set(fd[p.npiv[t]:].tolist()) <= kids
    # leaves keep all their DOFs: the assembly does not change
    cd = m.cell_dofs()
    for e in range(0, m.nel, 5):
        t = p.elem_front[e]
        assert np.array_equal(p.front_dofs[p.dof_off[t] + p.elem_map[e]], cd[e])
    leaves = np.nonzero(p.left < 0)[0]
    assert np.array_equal(p.nf[leaves], off.nf[leaves]) and np.array_equal(p.elem_map, off.elem_map)
    # panels per level: never more than without the pass, fewer where the plan says so
    pa, pb = _panels(off), _panels(p)
    assert all(b <= a for a, b in zip(pa, pb))
    saved = np.asarray(p.tail_delay["saved"])
    assert [a - b for a, b in zip(pa, pb)] == saved.tolist()
    assert np.array_equal(np.asarray(p.tail_delay["dofs"]) > 0, saved > 0)
    f0, f1 = p.tail_delay["flops3"]
    assert f1 <= 1.01 * f0
    fl = lambda q: int(np.sum(3 * q.npiv.astype(object) * q.nf.astype(object) ** 2 - 3 * q.npiv.astype(object) ** 2 * q.nf.astype(object)
                              + q.npiv.astype(object) ** 3))
    assert (f0, f1) == (fl(off), fl(p))
    if tail_max == 32 and name in SHRINKS:
        assert np.nonzero(saved)[0].tolist() == SHRINKS[name]
        assert "delayed_dofs" in p.summary() and p.summary()["delayed_dofs"] == int(np.sum(p.tail_delay["dofs"]))


def test_a_level_with_a_short_tail_loses_its_last_panel():
    off, on = _plan("plate16x80", 0), _plan("plate16x80", 32)
    lev = off.level_nodes[4]
    assert 128 < int(off.npiv[lev].max()) <= 160 and int(on.npiv[lev].max()) <= 128
    # at the child npiv shrinks and nf stays; at the parent both grow by what the children hand up
    for t in lev:
        d = int(off.npiv[t] - on.npiv[t])
        assert d >= 0 and on.nf[t] == off.nf[t]
        if d:
            assert d >= int(off.npiv[t]) - 128 and d < int(off.npiv[t]) - 128 + 6, "whole nodes: at most five DOFs more than the tail"
    for par in np.unique(off.parent[lev]):
        kids = [c for c in (off.left[par], off.right[par])]
        up = sum(int(off.npiv[c] - on.npiv[c]) for c in kids)
        assert on.npiv[par] - off.npiv[par] == up and on.nf[par] - off.nf[par] == up
        # the delayed DOFs come first among the parent's pivots, the left child's before the right one's
        got = on.front_dofs[on.dof_off[par]:on.dof_off[par] + up]
        want = np.concatenate([off.front_dofs[off.dof_off[c] + on.npiv[c]:off.dof_off[c] + off.npiv[c]] for c in kids])
        assert np.array_equal(got, want)
    # tail_max below the tail: nothing happens
    _same_plan(_plan("plate16x80", 16), off)


def test_a_delay_that_would_cost_the_parent_level_a_panel_is_refused():
    off, on = _plan("refuse26x65", 0), _plan("refuse26x65", 32)
    h = 6
    lev = off.level_nodes[h]
    mx = int(off.npiv[lev].max())
    P = -(-mx // NBO)
    tails = np.maximum(off.npiv[lev].astype(np.int64) - NBO * (P - 1), 0)
    assert P >= 2 and 0 < tails.max() <= 32, "the level's own conditions hold"
    grown = off.npiv.astype(np.int64).copy()
    np.add.at(grown, off.parent[lev], tails)
    up = off.level_nodes[h + 1]
    assert -(-int(grown[up].max()) // NBO) > -(-int(off.npiv[up].max()) // NBO), "the parents would need a further panel"
    _same_plan(on, off)
    assert int(np.sum(on.tail_delay["saved"])) == 0 and "delayed_dofs" not in on.summary()


def test_component_roots_do_not_delay_into_an_empty_root():
    off = _plan("two30x30", 0)
    root = int(np.nonzero(off.parent < 0)[0][0])
    top = off.level_nodes[-2]
    assert off.nf[root] == 0 and int(off.npiv[top].max()) == 276
    # tail_max 24: level 4's delay leaves level 5 a tail of 25 (refused), the component roots' tail of 20 is short enough -- but the root
    # level would go from no panel to one
    on = symbolic.build_plan(_mesh("two30x30"), CASES["two30x30"][1], tail_max=24)
    assert on.nf[root] == 0 and on.npiv[root] == 0
    assert np.array_equal(on.npiv[top], off.npiv[top]) and np.asarray(on.tail_delay["saved"]).tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert _plan("two30x30", 32).nf[root] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_tail_max_zero_is_the_plan_of_the_previous_entry_point(name):
    """femo_tail_delay_plan_build with tail_max 0 against femo_plan_build_ex2, every array of the C ABI bit for bit."""
    m, leaf = _mesh(name), CASES[name][1]
    old = _native.plan_arrays(m, leaf, 0, symbolic.AXIS_RULE, symbolic.GAP, symbolic.NODE_ORDER, tail_max=None)
    new = _native.plan_arrays(m, leaf, 0, symbolic.AXIS_RULE, symbolic.GAP, symbolic.NODE_ORDER, tail_max=0)
    assert sorted(old) == sorted(new)
    for k in old:
        assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
    assert not new["tail_delay_dofs"].any() and not new["tail_delay_saved"].any()


def test_the_entry_point_is_declared_exported_and_bound():
    """include/femo_symbolic.h declares femo_tail_delay_plan_build with the arguments of femo_plan_build_ex2 and tail_max, the library
    exports it and the ctypes table binds it with that signature."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "femo_symbolic.h")).read(), flags=re.S)
    decl = {n: a for n, a in re.findall(r"\bint\s+(femo_[a-z_0-9]+)\s*\(([^)]*)\)", text)}
    norm = lambda a: [" ".join(x.split()) for x in a.split(",")]
    assert norm(decl["femo_tail_delay_plan_build"]) == norm(decl["femo_plan_build_ex2"]) + ["int32_t tail_max"]
    lib = _native.load()
    assert list(_native.TAIL_DELAY_SIGNATURES) == ["femo_tail_delay_plan_build"]
    res, args = _native.TAIL_DELAY_SIGNATURES["femo_tail_delay_plan_build"]
    fn = lib.femo_tail_delay_plan_build
    assert fn.restype is res and list(fn.argtypes) == list(args) == list(_native.SIGNATURES["femo_plan_build_ex2"][1]) + [args[-1]]
    assert len(args) == len(norm(decl["femo_tail_delay_plan_build"]))


def test_contexts_ask_for_the_pass_and_build_plan_does_not():
    import inspect
    assert inspect.signature(symbolic.build_plan).parameters["tail_max"].default == 0
    assert inspect.signature(symbolic.analyse).parameters["tail_max"].default == 0
    assert symbolic.TAIL_MAX == 32


# ---- numbers: both plans are exact factorisations of the same matrix
NUMERIC = ["plate16x80", "plate14x70", "tri16x80", "two30x30"]


@pytest.fixture(scope="module")
def cpu_problem():
    cache = {}

    def get(name):
        if name not in cache:
            from oracle import cpu_baseline as cb
            from oracle.rm_shell_oracle import ShellOracle
            m = _mesh(name)
            rng = np.random.default_rng(5)
            o = ShellOracle(m, penalty_facets=m.penalty_facets(lambda x: np.less(x[0], 1e-12)))
            o.set_fields(h=0.1 * (1 + 0.2 * rng.uniform(-1, 1, m.nn)), E=1e8, nu=0.3, rho=10.0, f=rng.uniform(-1, 1, (m.nn, 3)))
            cs = cb.CpuShell(o)
            b = cs.load_vector(2)
            mf = cb.CpuMultifrontal(cs, _plan(name, 0), 2)
            mf.factorize()
            x0 = mf.solve(b)
            # the plain plan's own distance from the oracle's sparse direct solve of the same system: what rounding times conditioning
            # amounts to on this mesh
            xo = o.solve()
            cache[name] = (cs, b, x0, float(np.abs(x0 - xo).max() / np.abs(xo).max()))
        return cache[name]
    return get


@pytest.mark.parametrize("tail_max", [16, 32])
@pytest.mark.parametrize("name", NUMERIC)
def test_cpu_multifrontal_solution_is_that_of_the_plain_plan(cpu_problem, name, tail_max):
    from oracle import cpu_baseline as cb
    """1e-10 relative against the plain plan's solution: both are exact factorisations of one matrix and differ by rounding times
    conditioning.  Where the plain plan itself sits farther than 1e-11 from the oracle's direct solve (the penalty clamp costs digits),
    the bound is ten times that distance."""
    cs, b, x0, d0 = cpu_problem(name)
    mf = cb.CpuMultifrontal(cs, _plan(name, tail_max), 2)
    mf.factorize()
    x = mf.solve(b)
    err = np.abs(x - x0).max() / np.abs(x0).max()
    print(f"{name} tail_max {tail_max}: |x - x0| / |x0| = {err:.3e}; plain plan against the oracle's direct solve {d0:.3e}")
    assert err < max(1e-10, 10.0 * d0)
