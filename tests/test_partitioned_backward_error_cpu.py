"""The element-partitioned preconditioner checked by itself, not through PCG, on the CPU: the driver of femo_alpha_amd/parallel.py with
the numpy stand-in engine, all ranks as threads, ONE application z = M^-1 v (``dist_helpers.apply_preconditioner``: the steps of the PCG
loop between its collectives) against the single-domain oracle's K in the scaled backward error omega of tests/factor_check.py -- on
EVERY rank's view of the result, the replicated entries taken from that rank alone.  Pins the procedure and its negative control where
no GPU is needed; tests/test_gpu_partitioned_backward_error.py takes the same steps with the HIP engine.

Measured here (dense numpy on each rank's plan): wing 6.3e-14 at every world, plate16x80 4.8e-13; the first entry of one gathered Schur
block scaled by 1 + 1e-8 on one rank raises that rank's view to 1e-6 .. 1e-5."""
import numpy as np
import pytest

import dist_helpers as H
from factor_check import omega
from test_gpu_factor_backward_error import BOUND            # 1e-12: the project's bound on omega of one application

CLAMP = lambda x: np.less(x[0], 3e-16)
_cache = {}


def problem(name):
    """(mesh, marker, fields, leaf, K of the oracle, penalty-DOF mask), cached: shared with the GPU test."""
    if name not in _cache:
        from femo_alpha_amd.mesh import plate_mesh
        if name in ("wing", "wing_cr", "wing_ewm"):
            m, marker, fields = H.make_case("wing" if name == "wing_ewm" else name)
            leaf = 4
            if name == "wing_ewm":                    # element-wise material: the thickness is a cell field
                fields = dict(fields, thickness=0.02 * (1 + 0.2 * np.random.default_rng(8).uniform(-1, 1, m.nel)))
        else:
            m = {"plate16x80": lambda: plate_mesh(2.0, 10.0, 16, 80), "plate32x32": lambda: plate_mesh(2.0, 5.0, 32, 32)}[name]()
            marker, leaf = CLAMP, {"plate16x80": 24, "plate32x32": 8}[name]
            rng = np.random.default_rng(7)
            fields = dict(thickness=0.02 * (1 + 0.2 * rng.uniform(-1, 1, m.nn)), E=np.array([7e9]), nu=np.array([0.3]),
                          density=np.array([2700.0]), F_solid=rng.uniform(-1, 1, (m.nn, 3)) * 50)
        K, pen = H.oracle_matrix(m, marker, fields, element_wise_material=name == "wing_ewm")
        _cache[name] = (m, marker, fields, leaf, K, pen)
    return _cache[name]


def probes(n, k=4, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (k, n))


def omegas(name, world, engine, tail_max=0, comm_factory=None, k=4, rows=None):
    """omega of every rank's view (over ``rows``, default all), and the per-rank facts of ``dist_helpers.preconditioner_views``."""
    m, marker, fields, leaf, K, _ = problem(name)
    V = probes(m.ndof, k)
    views, facts = H.preconditioner_views(world, m, marker, fields, V, leaf_size=leaf, engine=engine, tail_max=tail_max,
                                          comm_factory=comm_factory, element_wise_material=name == "wing_ewm")
    return [omega(K, V.T, Z.T, rows=rows) for Z in views], facts


def thicker(name, factor=1.05):
    """(the thickness of ``name`` times ``factor``, K of the oracle with it), cached: the field change of the refactorisation case."""
    key = (name, "thicker", factor)
    if key not in _cache:
        m, marker, fields, _, _, _ = problem(name)
        t2 = fields["thickness"] * factor
        _cache[key] = (t2, H.oracle_matrix(m, marker, dict(fields, thickness=t2))[0])
    return _cache[key]


def omegas_after_a_field_change(name, world, engine):
    """Factorise, change the thickness, factorise again, apply once: omega of every rank's view against the NEW K and against the OLD
    one (a stub front or a replicated front that kept anything of the first factorisation shows in the first; the second proves that
    the change is large enough to be seen)."""
    m, marker, fields, leaf, K_old, _ = problem(name)
    t2, K_new = thicker(name)
    V = probes(m.ndof)

    def body(ds, comm):
        ds.set_fields(**fields)
        ds.factorize()
        ds.set_fields(thickness=t2)
        assert not ds.factored
        ds.factorize()
        return H.apply_preconditioner(ds, comm, V)
    views = H.global_views(H.run_ranks(world, m, marker, body, leaf_size=leaf, engine=engine, tail_max=0))
    return [omega(K_new, V.T, Z.T) for Z in views], [omega(K_old, V.T, Z.T) for Z in views]


def dots_and_operator(name, world, engine):
    """Through the partition, with v a global probe: (1) r.r as the PCG loop forms it -- ``pcg_start`` on b = v, ``precond_fwd``, the
    all-reduce, ``read`` -- against v.v: the weighted dot counts every replicated entry once over the ranks, ghosts included;
    (2) the partitioned operator -- the local apply, then the sum over the replicated entries -- as global views Y of K v.
    Returns (relative error of r.r per rank, omega(K, Y, v) per rank view)."""
    import math
    import torch
    m, marker, fields, leaf, K, _ = problem(name)
    v = probes(m.ndof, 1, seed=5)[0]
    vv = math.fsum(v * v)

    def body(ds, comm):
        ds.set_fields(**fields)
        ds.factorize()                                    # precond_fwd wants a factor
        eng, l2g = ds.eng, np.asarray(ds.info["l2g_dof"])
        loc = torch.as_tensor(np.ascontiguousarray(v[l2g]))
        with eng.on_stream():
            eng.vec("b").copy_(loc)
            eng.pcg_start("b", "state")
            eng.precond_fwd()
            if comm.size > 1:
                comm.allreduce_(eng.topbuf)
            rr = eng.read()[0]
            eng.vec("p").copy_(loc)
            (eng.ctx.op_apply_vec if hasattr(eng, "ctx") else eng.apply)("p", "Ap")
            ds._sum_top("Ap")
            y = eng.vec("Ap").cpu().numpy().copy()
        return dict(rr=rr, Z=y[None, :], l2g_dof=l2g, top_local=np.asarray(ds.info["top_local"]), nghost=int(ds.info["nghost"]))
    res = H.run_ranks(world, m, marker, body, leaf_size=leaf, engine=engine, tail_max=0)
    assert max(r["nghost"] for r in res) > 0
    return [abs(r["rr"] - vv) / vv for r in res], [omega(K, Y[0], v) for Y in H.global_views(res)]


# plate16x80: the tail-delay pass works below the partition depth only; at tail_max 32 it moves a panel at worlds 1 and 2
@pytest.mark.parametrize("name,world,tail_max,saved", [("wing", 1, 0, False), ("wing", 2, 0, False), ("wing", 4, 0, False),
                                                        ("wing", 8, 0, False), ("plate16x80", 1, 0, False), ("plate16x80", 2, 0, False),
                                                        ("plate16x80", 1, 32, True), ("plate16x80", 2, 32, True),
                                                        ("plate16x80", 4, 32, False)])
def test_floor_on_every_rank_view(name, world, tail_max, saved):
    w, facts = omegas(name, world, "numpy", tail_max)
    for q, x in enumerate(w):
        print(f"omega {name} tail_max {tail_max} world {world} rank-view {q} {x:.3e} (numpy engine)")
    assert len(w) == world and max(w) <= BOUND, w
    assert all((f["ntop"] > 0) == (world > 1) for f in facts), facts
    if world >= 4:
        assert max(f["nghost"] for f in facts) > 0, facts
    assert all((f["saved"] > 0) == saved for f in facts), facts


@pytest.mark.parametrize("world,receiver,source", [(2, 1, 0), (4, 2, 1), (8, 5, 6)])
def test_negative_control_one_exchanged_entry(world, receiver, source):
    """One entry of ONE receiving rank's copy of ONE other rank's packed Schur block, scaled by 1 + 1e-8: that rank's view must sit two
    decades above the bound (measured: six).  PCG at rtol 1e-12 does not notice such a factor."""
    comms = {}

    def factory(group, rank):
        comms[rank] = H.PerturbingComm(group, rank, receiver, source)
        return comms[rank]
    w, _ = omegas("wing", world, "numpy", comm_factory=factory)
    print(f"omega wing world {world}, entry 0 of rank {source}'s block scaled by 1 + 1e-8 on rank {receiver}: views " +
          " ".join(f"{x:.2e}" for x in w) + " (numpy engine)")
    assert comms[receiver].hits == 1
    assert w[receiver] >= 100 * BOUND, w


def test_refactorisation_after_a_field_change():
    new, old = omegas_after_a_field_change("wing", 4, "numpy")
    print("omega wing world 4 after a thickness change: new K " + " ".join(f"{x:.2e}" for x in new) + "  old K " +
          " ".join(f"{x:.2e}" for x in old) + " (numpy engine)")
    assert max(new) <= BOUND and min(old) >= 100 * BOUND


def test_dots_and_operator_through_the_partition():
    """Bounds as in the GPU test: 1e-13 on r.r (n u with n = 3174; an entry counted twice or not at all is O(1 / n)), 1e-10 on the
    operator (a wrong ghost or a separator entry summed twice is O(1))."""
    dots, op = dots_and_operator("wing", 4, "numpy")
    print(f"wing world 4: r.r against v.v {max(dots):.2e}, omega(K, Y, v) of the partitioned operator {max(op):.2e} (numpy engine)")
    assert max(dots) <= 1e-13 and max(op) <= 1e-10


def test_wing_cr_penalty_rows():
    """CG2CR1 with penalty facets: the rows of the DOFs the penalty facets hold (a few per cent) measure the conditioning of the penalty --
    a sparse LU of the oracle's own K leaves 3.3e-12 on them --, every other row the factor."""
    m, _, _, _, K, pen = problem("wing_cr")
    assert 0 < pen.mean() < 0.05
    for world in (1, 2, 4):
        w, _ = omegas("wing_cr", world, "numpy", rows=~pen)
        wp, _ = omegas("wing_cr", world, "numpy", rows=pen)
        print(f"omega wing_cr world {world}: rows off the penalty facets {max(w):.2e}, the {int(pen.sum())} of {pen.size} on them "
              f"{max(wp):.2e} (numpy engine)")
        assert max(w) <= BOUND


def test_the_stand_in_fronts_decide_level_0():
    """What makes plate32x32 the case it is meant to be, read from the rank plans at world 4: on level 0 the largest front and by far
    the largest Schur block (294 against 108) belong to a stand-in front without pivots, so the level's maxima -- and with them the
    launch shapes and the LDS of its sweeps -- are decided by fronts that eliminate nothing; the replicated top (582 DOF, a root of
    294 pivots) spans more than one 128-column panel; half of the replicated entries are ghosts."""
    from femo_alpha_amd.solver.symbolic import analyse, rank_plan
    m, _, _, leaf, _, _ = problem("plate32x32")
    T = analyse(m, leaf, min_depth=2)
    for rank in range(4):
        _, plan, info = rank_plan(m, T, rank, 4)
        l0 = np.asarray(plan.level_nodes[0])
        nf, npiv = np.asarray(plan.nf)[l0], np.asarray(plan.npiv)[l0]
        big = int(np.argmax(nf))
        assert npiv[big] == 0 and l0[big] in info["stub_fronts"] and l0[big] != info["root_front"], (rank, int(nf[big]))
        assert nf[big] > nf[npiv > 0].max() and nf[big] > 2 * (nf - npiv)[npiv > 0].max()
        assert min(info["schur_sizes"]) > 256 and info["n_top"] > 512 and info["nghost"] > 128
        assert int(np.asarray(plan.npiv)[np.asarray(plan.level_nodes[-1])].max()) > 256


def test_views_keep_one_ranks_top_apart():
    """``global_views`` on made-up pieces: view q carries rank q's replicated entries and everybody's interior ones."""
    a = dict(Z=np.array([[1.0, 2.0, 3.0]]), l2g_dof=np.array([0, 4, 2]), top_local=np.array([2]))
    b = dict(Z=np.array([[5.0, 6.0, 7.0]]), l2g_dof=np.array([2, 1, 3]), top_local=np.array([0]))
    va, vb = H.global_views([a, b])
    assert np.array_equal(va, [[1.0, 6.0, 3.0, 7.0, 2.0]]) and np.array_equal(vb, [[1.0, 6.0, 5.0, 7.0, 2.0]])


def test_omega_row_mask():
    import scipy.sparse as sp
    K = sp.diags([2.0, 3.0, 4.0]).tocsr()
    v = np.array([2.0, 3.0, 4.0])
    z = np.array([1.0, 1.0 + 1e-6, 1.0])
    assert omega(K, v, z) > 1e-7
    assert omega(K, v, z, rows=np.array([True, False, True])) == 0.0
    assert omega(K, v, z, rows=np.array([False, True, False])) == omega(K, v, z)
    with pytest.raises(ValueError):
        omega(K, v, z, rows=np.zeros(3, bool))
