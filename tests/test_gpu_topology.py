"""The solver on the meshes of tests/topology_meshes.py: two components, a cut-out, a vertex of valence 70 and 70 (1100) cells on one
edge.  What they reach that no generated plate, skin or tee beam does (tests/test_topology_cpu.py pins it on the host):

  * pivot-free fronts (npiv == 0) mixed among ordinary fronts, at the leaves and in the middle of the tree -- the launch ranges
    frontal_factorize_range derives from a level's fronts sorted by pivot count then start behind a run of zeros;
  * a front with nf == 0 (the root above two components): a level whose extend-add gathers nothing;
  * CSR runs of 70 .. 2200 contributions to one matrix entry: runs that fill a 64-lane chunk of k_csr_segmented, are carried through
    several chunks, and hold a whole 512-contribution wave in their middle;
  * penalty facets and operator penalty terms on edges with 70 incident cells.

Every comparison is with the oracle on the same mesh, in the metrics and at the bounds the suite already holds the solver to
(tests/factor_check.py, test_gpu_factor_backward_error.py, test_gpu_parity.py, test_gpu_goldens.py); helpers are imported from
those files.  Measured omegas are printed as "omega <case> <value>"."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_factor_backward_error as bw
import test_gpu_parity as par
import topology_meshes as tm
from factor_check import omega, omega_fit
from test_gpu_factor_backward_error import BOUND, SCHEDULES

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 8)
# (case, leaf) -> the plan must hold pivot-free fronts (the table of tests/test_topology_cpu.py), so no case passes by not occurring
PIVOT_FREE = {("islands", 1), ("islands", 2), ("islands", 8), ("holed", 1), ("holed", 2), ("fan70", 1), ("fan70", 2),
              ("book70", 1), ("book70", 2), ("book70", 8)}


def _assert_plan(name, leaf, plan):
    npiv, nf = np.asarray(plan.npiv), np.asarray(plan.nf)
    base = tm.base(name)
    if base.startswith("islands"):
        root = int(np.asarray(plan.level_nodes[-1])[0])
        assert npiv[root] == 0 and nf[root] == 0, (name, leaf)
    if (base, leaf) in PIVOT_FREE:
        assert (npiv == 0).any(), (name, leaf)
    return int((npiv == 0).sum())


# ------------------------------------------------------------------ a. the factor by itself
FACTOR_CASES = ["islands", "holed", "fan70", "book70",                 # penalty clamps
                "islands_strong", "book70_strong",                     # strong DOFs
                "islands_tri", "holed_tri",                            # triangles
                "fan70_cg1", "fan70_cr1"]                              # the other elements


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", FACTOR_CASES)
def test_factor_backward_error(name, leaf):
    """One application of the factor to 4 probes: omega <= BOUND, no pivot repaired, and the plan really holds the pivot-free fronts.

    fan70_cr1 (CG2CR1, penalty clamp of the outer ring) at leaf 2 and 8 is the case that found the unsymmetric penalty block of
    k_facet_matrices: omega was 7.0e-9 and 1.29e-8 there (proportional to the penalty weight, the same under every schedule and
    sweep option, 9.6e-15 at leaf 1), because the 3 x 3 rotation block kept rounding residues of its own in (a, b) and (b, a) and
    the fronts, which keep one triangle, factorised a matrix that differed from the operator's by 3e-3 in entries the free mode of
    the penalty (stiffness 1e-8 of the penalty) does not forgive."""
    m, K, c = bw._context(name, leaf)
    try:
        n0 = _assert_plan(name, leaf, c.plan)
        w = bw._omega_of(f"{name} leaf {leaf} ({n0} pivot-free fronts of {c.plan.ntree})", c, K)
    finally:
        c.close()
    assert w <= BOUND, (name, leaf, w)


# ------------------------------------------------------------------ b. the options that change which kernels see the pivot-free fronts
OPTIONS_POST = [("assemble_fc 0", dict(assemble_fc=0)), ("assemble_fc 2", dict(assemble_fc=2))] + \
               [s for s in SCHEDULES if s[0] in ("trailing 0", "trailing 1", "trailing 2", "all left-looking", "all right-looking")] + \
               [("sweep_graph 0", dict(sweep_graph=0)), ("sweep_graph 1", dict(sweep_graph=1))]
OPTIONS_PRE = [("no wide level", dict(wide_cnt=0, wide_np=100000)), ("wide_cnt 100000", dict(wide_cnt=100000)),
               ("swork_slots 2", dict(swork_slots=2))]


@pytest.mark.parametrize("name", ["book70", "islands"])
def test_factor_through_the_schedule_and_sweep_options(name):
    assert len(OPTIONS_POST) == 9
    bad = []
    for what, pre, post in [(w, None, p) for w, p in OPTIONS_POST] + [(w, p, None) for w, p in OPTIONS_PRE]:
        m, K, c = bw._context(name, 2, pre=pre, post=post)
        try:
            _assert_plan(name, 2, c.plan)
            w = bw._omega_of(f"{name} leaf 2 {what}", c, K)
        finally:
            c.close()
        if not w <= BOUND:
            bad.append((what, w))
    # "sweep_ahead": the first application of a cold solve, through one PCG iteration (x_1 = alpha M^-1 b)
    for ahead in (0, 2):
        m, K, c = bw._context(name, 2, post=dict(sweep_ahead=ahead, strict=0))
        try:
            c.set_solver(preconditioner=2, rtol=1e-12, maxit=1, check_every=1)
            b = bw._probes(m.ndof, 1, seed=9)[0]
            x1, it, _ = c.solve_linear(b)
            assert it == 1
            w = omega_fit(K, b, x1)
            print(f"omega {name} leaf 2 sweep_ahead {ahead} (fitted) {w:.3e}")
        finally:
            c.close()
        if not w <= BOUND:
            bad.append((f"sweep_ahead {ahead}", w))
    assert not bad, bad


# ------------------------------------------------------------------ c. grouped sweeps
@pytest.mark.parametrize("pre", [dict(wide_np=100000, wide_cnt=0), None], ids=["no wide level", "default"])
def test_several_vectors_column_by_column(pre):
    bw._several_vectors("book70", leaf=2, pre=pre, post={})


# ------------------------------------------------------------------ d. Schur blocks level by level
@pytest.mark.parametrize("name", ["holed", "fan24"])
def test_schur_blocks_level_by_level(name):
    """A front without pivots must show the plain sum of its children's blocks (of its own cells' matrices at a leaf)."""
    assert bw._schur_blocks_level_by_level(name, "default", leaf=2) >= 1


# ------------------------------------------------------------------ e. whole solve and gradients
TOL = 1e-8               # the bar of test_gpu_goldens and test_gpu_multi_rhs


def _device_problem(name, o):
    from femo_alpha_amd.backend import ShellContext
    m = o.mesh
    c = ShellContext(m)
    for k, v in bw._fields(m).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(tm.clamp(name)))
    return c


_refs = {}


def _reference(name):
    """Oracle, state, compliance and the total gradients of the compliance with respect to thickness and E: once per mesh."""
    if name not in _refs:
        m, o = tm.oracle_problem(name)
        w, J, dJdh = o.forward_adjoint()
        lam = o.solve_adjoint(o.dcompliance_du(w))
        _refs[name] = (m, o, w, J, dJdh, -o.dRdfield_T("E", w, lam))
    return _refs[name]


@pytest.mark.parametrize("leaf", [2, None], ids=["leaf 2", "default leaf"])
@pytest.mark.parametrize("name", ["islands", "holed", "fan70", "book70"])
def test_solve_and_total_gradients(name, leaf):
    m, o, w_ref, J_ref, gh_ref, gE_ref = _reference(name)
    c = _device_problem(name, o)
    try:
        c.use_direct_solver(leaf, rtol=1e-12)
        it, rr = c.solve_state(zero_guess=True)
        w = c.get_state()
        gh, it_h, _ = c.total_gradient("compliance", "thickness")
        gE, it_E, _ = c.total_gradient("compliance", "E")
        e = (par.rel(w, w_ref), abs(c.functional("compliance") - J_ref) / abs(J_ref), par.rel(gh, gh_ref), par.rel(gE, gE_ref))
        print(f"solve {name} leaf {leaf}: iterations {it}/{it_h}/{it_E}, displacement {e[0]:.1e}, compliance {e[1]:.1e}, "
              f"d/dh {e[2]:.1e}, d/dE {e[3]:.1e} from the oracle")
        assert c.frontal_info()["pivots_repaired"] == 0
        assert max(it, it_h, it_E) <= 4 and rr <= 1e-12
        assert max(e) < TOL, e
    finally:
        c.close()


@pytest.mark.parametrize("name,vertices", [("fan70", (0,)), ("book70_spine", (2,))], ids=["fan70 centre", "book70 spine"])
def test_shape_sensitivities(name, vertices):
    """As test_gpu_parity.test_shape_sensitivities_vs_oracle_finite_differences, also at the vertex of valence 70 and at vertices of
    the clamped spine (70 penalty facets on each of its edges: the penalty's shape term)."""
    m = tm.mesh(name)
    if name == "book70_spine":
        pf = m.penalty_facets(tm.clamp(name))
        assert pf.shape[0] == 210 and m.edge_count.max() == 70
        assert np.all(np.hypot(m.nodes[list(vertices), 0], m.nodes[list(vertices), 2]) == 0.0)
    else:
        assert np.bincount(m.cells.ravel())[0] == 70
    par._shape_sensitivities(name, "penalty", vertices=vertices, nrandom=1)


# ------------------------------------------------------------------ f. operator and penalty
@pytest.mark.parametrize("name", ["fan70", "book70_spine"])
def test_operator_and_diagonal(name):
    m, o, c, rng = par._pair(name)
    try:
        K = o.assemble_K()
        for _ in range(2):
            x = rng.uniform(-1, 1, m.ndof)
            assert par.rel(c.apply_K(x), K @ x) < 1e-11
        assert par.rel(c.diagonal(), K.diagonal()) < 1e-11
        # the penalty term by itself (the rows of the clamped edges carry 1e15 beside 1e4: the elastic part hides there)
        Kp = K - o.assemble_K(with_penalty=False)
        rows = np.unique(Kp.nonzero()[0])
        assert rows.size > 0
        x = np.zeros(m.ndof); x[rows] = rng.uniform(-1, 1, rows.size)
        assert par.rel(c.apply_K(x)[rows], (K @ x)[rows]) < 1e-11
    finally:
        c.close()


# ------------------------------------------------------------------ g. CSR
def _run_scale(m, o, cm):
    """Per CSR entry: the sum of the absolute element contributions that land there, and their number."""
    Ke = o.element_matrices()
    return np.bincount(cm["dest"], weights=np.abs(Ke.ravel()[cm["perm"]]), minlength=cm["nnz"]), np.bincount(cm["dest"], minlength=cm["nnz"])


@pytest.mark.parametrize("name,longest", [("fan70", 65), ("book70", 129), ("book1100", 1023)])
def test_csr_assembly_with_long_runs(name, longest):
    from femo_alpha_amd.backend import ShellContext
    from femo_alpha_amd.csr import build_csr_map
    from oracle.rm_shell_oracle import ShellOracle
    m = tm.book(1100, 1) if name == "book1100" else tm.mesh(name)
    f = bw._fields(m)
    o = ShellOracle(m)
    o.set_fields(h=f["thickness"], E=f["E"], nu=0.3, rho=2700.0, f=f["F_solid"])
    c = ShellContext(m)
    try:
        for k, v in f.items():
            c.set_field(k, v)
        info = c.enable_csr()
        K = c.assemble_csr()
        Kref = sp.csr_matrix(o.assemble_K(with_penalty=False, with_strong=False))
        Kref.sort_indices()
        assert info["nnz"] == Kref.nnz
        assert abs(K - Kref).max() < 1e-11 * abs(Kref).max()
        K2 = c.assemble_csr()
        assert abs(K2 - K).max() <= 1e-13 * abs(Kref).max()
        # the device-built map against the numpy one
        cm = build_csr_map(m)
        assert np.array_equal(info["rowptr"], cm["rowptr"]) and np.array_equal(info["colidx"], cm["colidx"])
        assert np.array_equal(Kref.indptr, cm["rowptr"]) and np.array_equal(Kref.indices, cm["colidx"])
        scale, runs = _run_scale(m, o, cm)
        assert runs.max() >= longest
        # (1) The long runs (longer than a 64-lane chunk) entry by entry against the oracle, relative to the entry's own sum of absolute
        # contributions: a dropped or doubled partial sum of a run of n is ~1 / n of that, and may be far below 1e-11 of the largest
        # entry.  Entries whose contributions are rounding residue of the element integrals themselves (flat pages: sums of exact zeros
        # in the oracle, 1e-16 of the element's largest entry on the device) have no scale of their own to be relative to: they are
        # left to (2); "of their own" = at least 1e-3 of the largest scale among the long runs.
        long_runs = (runs > 64) & (scale >= 1e-3 * scale[runs > 64].max())
        assert long_runs.sum() >= 9                      # at least the 3 x 3 diagonal block of one node
        # (2) Every entry against the device's OWN element matrices summed in extended precision: what is left is the order of the
        # scatter's additions, bounded for any order by (n - 1) u sum |x_i| (u = 2^-53).
        Kd = c.element_matrices().ravel()[cm["perm"]]
        heads = np.concatenate([[0], np.cumsum(runs)[:-1]])
        own = np.add.reduceat(Kd.astype(np.longdouble), heads)
        own_scale = np.add.reduceat(np.abs(Kd), heads)
        for what, Kdev in (("device map", K), ("device map, again", K2)):
            err = np.abs(Kdev.data - Kref.data)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(scale > 0, err / scale, 0.0)
            k = int(np.argmax(np.where(long_runs, ratio, 0.0)))
            print(f"csr {name} {what}: long runs ({int(long_runs.sum())} entries, up to {runs.max()}) worst {ratio[k]:.2e} of their contributions "
                  f"(a run of {runs[k]}); all entries with a scale {ratio.max():.2e}")
            assert np.all(err[long_runs] <= 1e-13 * scale[long_runs]), (what, k, int(runs[k]), ratio[k])
            err_own = np.abs(Kdev.data.astype(np.longdouble) - own).astype(np.float64)
            slack = err_own - (runs - 1) * 2.0 ** -53 * 1.01 * own_scale
            print(f"csr {name} {what}: against its own element matrices, worst {np.max(err_own / np.maximum(own_scale, 1e-300)):.2e} of the contributions")
            assert slack.max() <= 0.0, (what, int(np.argmax(slack)), int(runs[np.argmax(slack)]))
        host = c.enable_csr(host_map=True)
        assert np.array_equal(info["rowptr"], host["rowptr"]) and np.array_equal(info["colidx"], host["colidx"])
        Kh = c.assemble_csr()
        assert abs(Kh - K).max() <= 1e-13 * abs(Kref).max()
        assert np.all(np.abs(Kh.data - Kref.data)[long_runs] <= 1e-13 * scale[long_runs])
    finally:
        c.close()
