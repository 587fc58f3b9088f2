"""The element-partitioned preconditioner of the HIP engine checked by itself, not through PCG: all ranks as threads of this process on
the one card, ONE application z = M^-1 v through the calls of the PCG loop (femo_dist_precond_fwd, the all-reduce, femo_dist_precond_rest)
against the single-domain oracle's K in the scaled backward error omega of tests/factor_check.py, on EVERY rank's view of the result
(interior entries from their owners, the replicated entries from that rank alone).  PCG at rtol 1e-12 converges to the same solution
in the same iterations with a Schur block that is wrong in its 8th digit; omega sees it (the negative control below).

What only the partitioned path runs, and these cases reach: pivot-free stand-in fronts on level 0 beside the leaves (they are the
largest fronts of that level), the packed exchange (k_tril_pack / k_tril_unpack), the split sweeps with k_top_delta / k_top_restore
around the collective, the weighted dots over ghost entries.  The procedure and its negative control are pinned without a GPU in
tests/test_partitioned_backward_error_cpu.py, whose helpers this module shares.  Every measured value is printed as
"omega <case> world <P> rank-view <q> <value>".

Measured on the MI355X (smallest .. largest over the rank views of two runs; the bound is 1e-12):

    case                                 world 1     world 2     world 4               world 8
    wing, default sweeps                 1.3e-14     1.3e-14     1.3e-14               1.3e-14 .. 2.1e-14
    wing, wide_cnt=0                                             3.8e-15 .. 1.6e-14    1.2e-14 .. 3.3e-14
    plate32x32, default sweeps           6.1e-15     4.4e-15     6.0e-15 .. 4.9e-14
    plate32x32, wide_cnt=0 / 20                      2.0e-15     1.6e-14 .. 2.1e-14 (wide_cnt=20)
    plate16x80, tail_max 0               3.4e-14     2.3e-14
    plate16x80, tail_max 32              5.2e-14     2.0e-14 (wide_cnt=0: 1.4e-15)
    wing, element-wise material                      9.7e-15     9.7e-15
    second factorisation, new K                      5.5e-15 (plate32x32)  5.6e-15 (wing)
    second factorisation, OLD K                      7.2e-02 (plate32x32)  1.8e-02 (wing)
    wing_cr, rows off the penalty facets 3.0e-15     2.6e-15     3.0e-15 .. 4.3e-15
    wing_cr, rows on them (123 of 4323)  2.7e-15     2.9e-15     2.9e-15   (numpy engine 1.5e-10, single context 4.0e-15)
    one exchanged entry * (1 + 1e-8)                 2.0e-06 on the receiving rank's view (the other view 1.4e-06)
    world 4 on wing: r.r against v.v 2.1e-16; omega(K, Y, v) of the partitioned operator 2.0e-15

The numpy engine leaves 6.3e-14 (wing), 4.8e-13 (plate16x80) and 3.9e-13 (plate32x32) on the same cases: the device sits a factor 3 to
200 below it.  (The emulator's floor is its own: it solves with the triangular factors by general LU; with triangular solves it
leaves 5e-16 on plate32x32.)"""
import numpy as np
import pytest

import dist_helpers as H
import test_partitioned_backward_error_cpu as P
from factor_check import omega
from test_gpu_factor_backward_error import BOUND

pytestmark = pytest.mark.gpu


def _report(case, world, w):
    for q, x in enumerate(w):
        print(f"omega {case} world {world} rank-view {q} {x:.3e}")


# ------------------------------------------------------------------ case 1: one application, every partitioning
D, S, S20 = "default", "wide_cnt=0", "wide_cnt=20"


@pytest.mark.parametrize("name,world,tail_max,sweeps", [
    ("wing", 1, 0, D), ("wing", 2, 0, D), ("wing", 4, 0, D), ("wing", 8, 0, D), ("wing", 4, 0, S), ("wing", 8, 0, S),
    ("plate32x32", 1, 0, D), ("plate32x32", 2, 0, D), ("plate32x32", 4, 0, D), ("plate32x32", 2, 0, S), ("plate32x32", 4, 0, S20),
    ("plate16x80", 1, 0, D), ("plate16x80", 2, 0, D), ("plate16x80", 1, 32, D), ("plate16x80", 2, 32, D), ("plate16x80", 2, 32, S),
    ("wing_ewm", 2, 0, D), ("wing_ewm", 4, 0, D)])
def test_one_application_on_every_rank_view(name, world, tail_max, sweeps, monkeypatch):
    """wing: unequal partitions, many ghosts.  plate32x32 (leaf 8): subtree-root Schur blocks of 294 DOF and a replicated top of 582
    DOF at world 4 -- the stand-in fronts are by far the largest fronts of level 0 (tests/test_partitioned_backward_error_cpu.py reads
    that from the plans).  plate16x80 (leaf 24): the tail-delay pass moves a panel below the partition depth with tail_max 32.
    wing_ewm: cell fields.

    Which sweep kernels: no level of these meshes has more than 512 fronts, so by default ("wide_cnt" 512) EVERY level, level 0 with
    its stand-in fronts included, takes the wide forms (k_sweep_gemv_n / _t, k_sweep_bnd_cols; the factorisation keeps L11^-1).  With
    "wide_cnt=0" every level takes the one-workgroup-per-front forms instead (k_front_fwd_small / k_front_bwd_small; no pivot block
    here exceeds "wide_np" 512), whose LDS on level 0 is sized by a stand-in front -- the forms level 0 of a large partition takes.
    "wide_cnt=20" on plate32x32 at world 4 gives level 0 (35 fronts, 3 of them stand-ins) those forms and leaves the levels above
    it, 16 fronts and fewer, wide: the split a large partition has, whose top levels are always wide.  Forcing the two replicated top
    levels of that case through the one-workgroup forms as well ("wide_cnt=0", a path no plan takes by default) was measured at
    1.3e-14 .. 7e-13 over seven runs, changing from run to run, against 8e-15 .. 5e-14 for the two settings tested here.

    What a view measures beyond the factor: every rank sweeps the replicated top on its own, and where two top fronts add into a
    third with atomics the ranks round in different orders, so their replicated entries differ by a forward error (measured: 1e-15
    .. 9e-15 of the largest entry at world 4; exactly 0 at world 2, whose top is one front).  A view joins one rank's top to the
    other ranks' interiors, which were swept back from THEIR tops, and the ill-conditioned top of the plate turns that difference
    into a residual.  The numpy engine with triangular solves sits at 5e-16 at every world and shows the same: rounding-sized
    (1e-16) relative noise on the contributions of the local sweeps leaves it there, the same noise on the top sweeps, drawn
    differently on every rank, gives 1e-14 .. 5e-13 at world 4.  Probes supported on the root separator alone, or on the other
    replicated entries alone, stay at 1e-15 on the device: the exchanged blocks, the top factor and the top sweeps are exact."""
    if sweeps != "default":
        monkeypatch.setenv("FEMO_OPTIONS", sweeps)            # read by every context made from here on
    w, facts = P.omegas(name, world, "hip", tail_max)
    _report(f"{name} tail_max {tail_max} sweeps {sweeps}", world, w)
    assert all(f["repaired"] == 0 for f in facts), facts
    assert all((f["ntop"] > 0) == (world > 1) for f in facts), facts
    if world >= 4:
        assert max(f["nghost"] for f in facts) > 0, facts
    if name == "plate16x80":
        assert all((f["saved"] > 0) == (tail_max > 0) for f in facts), facts
    assert len(w) == world and max(w) <= BOUND, w


# ------------------------------------------------------------------ case 2: factorise twice
@pytest.mark.parametrize("name,world", [("wing", 4), ("plate32x32", 2)])
def test_second_factorisation_leaves_nothing_stale(name, world):
    new, old = P.omegas_after_a_field_change(name, world, "hip")
    _report(f"{name} after a thickness change, new K", world, new)
    _report(f"{name} after a thickness change, OLD K", world, old)
    assert max(new) <= BOUND, new
    assert min(old) >= 100 * BOUND, old


# ------------------------------------------------------------------ case 3: the exchange is exact
@pytest.mark.parametrize("world", [2, 4])
def test_packed_exchange_is_exact(world):
    """After the factorisation of the rank's own levels: femo_front_schur_pack hands out the column-major lower triangle of the root
    front's Schur block bit for bit; after femo_front_block_unpack the stand-in front of rank q holds rank q's lower triangle bit for
    bit (only the lower triangle of a front is maintained); a front with pivots is never overwritten."""
    import torch
    from femo_alpha_amd._lib import FemoHipError
    m, marker, fields, leaf, _, _ = P.problem("plate32x32")

    def square(ctx, front, n):
        S = torch.empty(n * n, dtype=torch.float64, device="cuda")
        ctx.front_schur_get(front, S)
        return S.cpu().numpy().reshape(n, n).T              # column-major on the device

    def body(ds, comm):
        ds.set_fields(**fields)
        eng, info, ctx = ds.eng, ds.info, ds.eng.ctx
        sizes, root = info["schur_sizes"], info["root_front"]
        with eng.on_stream():
            eng.factor(0, ds.nl, True)
            mine = eng.new_tensor(max(n * (n + 1) // 2 for n in sizes))
            eng.schur_pack(root, mine)
            gathered = comm.allgather(mine)
            for q in range(comm.size):
                if q != comm.rank:
                    eng.block_unpack(info["stub_fronts"][q], gathered[q])
            out = dict(packed=mine.cpu().numpy().copy(), own=square(ctx, root, sizes[comm.rank]),
                       stubs={q: square(ctx, info["stub_fronts"][q], sizes[q]) for q in range(comm.size) if q != comm.rank})
            with pytest.raises(FemoHipError):
                eng.block_unpack(root, gathered[comm.rank])
        return out
    res = H.run_ranks(world, m, marker, body, leaf_size=leaf, tail_max=0)
    for p, r in enumerate(res):
        S = r["own"]
        n = S.shape[0]
        tri = np.concatenate([S[j:, j] for j in range(n)])
        assert n > 128 and np.count_nonzero(tri) > tri.size // 2
        assert np.array_equal(r["packed"][: tri.size], tri), p
        for q, A in r["stubs"].items():
            assert np.array_equal(np.tril(A), np.tril(res[q]["own"])), (p, q)


# ------------------------------------------------------------------ case 4: CG2CR1 in partitions
_cr_numpy = {}


@pytest.mark.parametrize("world", [1, 2, 4])
def test_wing_cr_off_and_on_the_penalty_rows(world):
    """CG2CR1 with penalty facets.  The rows of the DOFs the penalty facets hold (123 of 4323, asserted below 5 %) measure the
    conditioning of the 1e15 penalty, not the factor: a sparse LU of the oracle's own K leaves 3.3e-12 on them, the numpy engine
    1.55e-10.  So: every other row within BOUND; the penalty rows within 4 x the numpy engine's value on the same rows (both are
    dominated by the same conditioning and differ by the order of summation).  Measured: the device leaves 3e-15 on the penalty rows as
    on all others, in partitions and in a single context -- the emulator's 1.55e-10 is the emulator's (general LU on the triangular
    factors), so the mask costs the device nothing and the second bar is far from tight."""
    m, _, _, _, K, pen = P.problem("wing_cr")
    share = pen.mean()
    print(f"wing_cr: {int(pen.sum())} of {pen.size} rows belong to penalty facets ({100 * share:.2f} %)")
    assert 0 < share < 0.05
    if world not in _cr_numpy:
        _cr_numpy[world] = max(P.omegas("wing_cr", world, "numpy", rows=pen)[0])
    m, marker, fields, leaf, _, _ = P.problem("wing_cr")
    V = P.probes(m.ndof)
    views, facts = H.preconditioner_views(world, m, marker, fields, V, leaf_size=leaf, engine="hip", tail_max=0)
    off = [omega(K, V.T, Z.T, rows=~pen) for Z in views]
    on = [omega(K, V.T, Z.T, rows=pen) for Z in views]
    _report("wing_cr rows off the penalty facets", world, off)
    _report("wing_cr rows on the penalty facets", world, on)
    print(f"omega wing_cr world {world} rows on the penalty facets, numpy engine {_cr_numpy[world]:.3e}")
    assert all(f["repaired"] == 0 for f in facts), facts
    assert max(off) <= BOUND, off
    assert max(on) <= 4 * _cr_numpy[world], (on, _cr_numpy[world])


def test_wing_cr_single_context_on_the_same_rows():
    """What the single-context path (ShellContext.frontal_apply) leaves on the same mesh with the same penalty facets: no other test
    measures CG2CR1 with penalty facets by omega.  The rows off the penalty facets within BOUND; the value on them is printed."""
    from femo_alpha_amd.backend import ShellContext
    m, marker, fields, leaf, K, pen = P.problem("wing_cr")
    c = ShellContext(m)
    try:
        for k, v in fields.items():
            c.set_field(k, v)
        c.set_penalty_facets(m.penalty_facets(marker))
        c.enable_frontal(leaf)
        c.set_solver(preconditioner=2, rtol=1e-12, maxit=30, check_every=1)
        V = P.probes(m.ndof)
        Z = c.frontal_apply(V)
        assert c.frontal_info()["pivots_repaired"] == 0
    finally:
        c.close()
    off, on = omega(K, V.T, Z.T, rows=~pen), omega(K, V.T, Z.T, rows=pen)
    print(f"omega wing_cr single context rows off the penalty facets {off:.3e} on them {on:.3e}")
    assert off <= BOUND


# ------------------------------------------------------------------ case 5: the dots and the operator through the partition
def test_dots_and_operator_through_the_partition():
    """World 4 on wing (ghost entries on some rank, asserted).  r.r of the PCG loop (k_wdot: replicated entries weighted 1 / P, ghosts
    included) against v.v to 1e-13 -- n u with n = 3174; an entry counted twice or not at all is O(1 / n).  The partitioned operator
    (local apply, then the sum over the replicated entries; gathered per owner, the top from each rank in turn) against the oracle:
    omega(K, Y, v) <= 1e-10, the same function with the roles of its two arguments exchanged -- a condition that separates rounding
    from an index error (a wrong ghost or a separator entry summed twice is O(1)), not a measured floor."""
    dots, op = P.dots_and_operator("wing", 4, "hip")
    for q, (d, o) in enumerate(zip(dots, op)):
        print(f"wing world 4 rank {q}: r.r against v.v {d:.3e}  omega(K, Y, v) of the partitioned operator, rank-view {q} {o:.3e}")
    assert max(dots) <= 1e-13, dots
    assert max(op) <= 1e-10, op


# ------------------------------------------------------------------ case 6: negative control
def test_negative_control_one_exchanged_entry():
    """Entry 0 of rank 0's packed Schur block scaled by 1 + 1e-8 in rank 1's copy alone: rank 1's view must sit two decades above the
    bound (the numpy engine gives 2e-6).  Every test of the partitioned path through PCG passes with this factor."""
    comms = {}

    def factory(group, rank):
        comms[rank] = H.PerturbingComm(group, rank, receiver=1, source=0)
        return comms[rank]
    w, _ = P.omegas("wing", 2, "hip", comm_factory=factory)
    _report("wing, one exchanged entry scaled by 1 + 1e-8 on rank 1,", 2, w)
    assert comms[1].hits == 1 and comms[0].hits == 0
    assert w[1] >= 100 * BOUND, w
