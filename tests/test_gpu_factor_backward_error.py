"""The multifrontal factor checked by itself, not through PCG: one application M^-1 v (femo_frontal_apply, the route of the PCG loop,
no Krylov iteration) against the oracle's K in the scaled backward error omega of tests/factor_check.py, for every operator variant,
every factorisation schedule, every sweep form and every number of right-hand sides; the first application of a cold solve with
"sweep_ahead" through one PCG iteration; the Schur block of every front, level by level, against the subtree's Schur complement.

PCG with rtol 1e-12 converges in the same number of iterations to the same solution with a factor whose entries are wrong by 1e-8, so
the other GPU tests do not see such a factor; omega does (an exact factor leaves ~1e-14, one entry off by 1e-10 ~1e-11 and more:
tests/test_factor_check_cpu.py).  Measured GPU floors are printed as "omega <case> <value>"."""
import numpy as np
import pytest
import scipy.sparse as sp

from factor_check import omega, omega_fit
from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles, tee_beam_mesh, wing_skin_mesh

pytestmark = pytest.mark.gpu

BOUND = 1e-12            # omega of one application; the GPU floor is 1e-15 .. 8e-14 (2e-13 fitted after one PCG step)
SCHUR_BOUND = 2e-11      # max |S - S_ref|_ij / sqrt(S_ii S_jj) of a front's Schur block; the GPU floor is 3.5e-12
CLAMP = lambda x: np.less(x[0], 3e-16)
ROOT = lambda x: np.less(x[1], 1e-9)

_cache = {}
_plans = {}


def _mesh(name):
    if name == "plate":
        return plate_mesh(2.0, 5.0, 64, 64)
    if name == "wing":
        return wing_skin_mesh(32, 96, shuffle=True).renumbered()[0]
    if name == "plate_small":
        return plate_mesh(2.0, 5.0, 24, 24)
    if name == "wing_small":
        return wing_skin_mesh(8, 20, shuffle=True).renumbered()[0]
    if name == "tri":
        return quads_to_triangles(wing_skin_mesh(10, 30))
    if name == "tri_cr1":
        t = quads_to_triangles(wing_skin_mesh(10, 30))
        return ShellMesh(t.nodes, t.cells, "CG2CR1")
    if name == "cg1":
        return wing_skin_mesh(12, 36, element="CG1CG1")
    if name == "tee":
        return tee_beam_mesh(nw=8, nh=4, nl=40)
    if name == "wing_mid":
        return wing_skin_mesh(12, 36)
    import topology_meshes as tm
    if tm.base(name) in tm.MESHES:            # disjoint, holed, high-valence and branched meshes (tests/test_gpu_topology.py)
        return tm.mesh(tm.base(name))
    raise KeyError(name)


def _strong(name):
    import topology_meshes as tm
    if tm.base(name) in tm.MESHES:
        return name.endswith("_strong")
    return not name.startswith("plate")


def _marker(name, strong):
    """The clamped set: the root section (strong DOFs) or the x = 0 edge (penalty facets); the topology meshes bring their own."""
    import topology_meshes as tm
    if tm.base(name) in tm.MESHES:
        return tm.clamp(tm.base(name))
    return ROOT if strong else CLAMP


def _fields(m, ewm=False):
    r = np.random.default_rng(1)
    n = m.nel if ewm else m.nn
    return dict(thickness=0.02 * (1 + 0.3 * r.uniform(-1, 1, n)), E=7e10 * (1 + 0.2 * r.uniform(-1, 1, n)), nu=[0.3], density=[2700.0],
                F_solid=r.uniform(-1, 1, (m.nn, 3)))


def _problem(name, ewm=False, uhat=False, nred=0, laminate=False, operator=None):
    """(mesh, K of the oracle, what the context needs) of one operator, cached."""
    key = (name, ewm, uhat, nred, laminate, operator)
    if key not in _cache:
        from oracle.rm_shell_oracle import ShellOracle
        m = _mesh(name)
        f = _fields(m, ewm)
        uh = 0.02 * np.random.default_rng(2).uniform(-1, 1, (m.nn, 3)) if uhat else None
        strong = _strong(name)
        sd = m.locate_dofs_geometrical(_marker(name, strong)) if strong else None
        pf = None if strong else m.penalty_facets(_marker(name, strong))
        clt = None
        if laminate:
            from laminate_ref import LaminateOracle
            from test_gpu_laminate import random_laminate
            clt = random_laminate(m.nel, np.random.default_rng(4))
            o = LaminateOracle(m, element_wise_material=ewm, penalty_facets=pf, strong_dofs=sd, nred=nred)
            o.set_laminate(clt)
        else:
            o = ShellOracle(m, element_wise_material=ewm, penalty_facets=pf, strong_dofs=sd, nred=nred)
        E = f["E"]
        o.set_fields(h=f["thickness"], E=E, nu=0.3, rho=2700.0, f=f["F_solid"], uhat=uh)
        if operator is None:
            K = o.assemble_K()
        else:
            aK, aM = operator
            K = o._apply_strong((aK * o.assemble_K(with_strong=False) + aM * o.assemble_M()).tocsr()) if strong else \
                (aK * o.assemble_K() + aM * o.assemble_M())
        _cache[key] = (m, sp.csr_matrix(K), dict(f=f, uh=uh, sd=sd, pf=pf, clt=clt, ewm=ewm, nred=nred, operator=operator))
    return _cache[key]


def _context(name, leaf=8, pre=None, post=None, plan=None, **variant):
    from femo_alpha_amd.backend import ShellContext
    m, K, d = _problem(name, **variant)
    c = ShellContext(m, element_wise_material=d["ewm"])
    for k, v in d["f"].items():
        c.set_field(k, v)
    if d["uh"] is not None:
        c.set_field("uhat", d["uh"])
    if d["nred"]:
        c.set_strain_quadrature(d["nred"])
    if d["sd"] is not None:
        c.set_strong_dofs(d["sd"])
    else:
        c.set_penalty_facets(d["pf"])
    if d["clt"] is not None:
        c.set_laminate(d["clt"])
    if d["operator"] is not None:
        c.set_operator(*d["operator"])
    for k, v in (post or {}).items():
        c.set_option(k, v)
    if plan is None:
        if (name, leaf) not in _plans:
            from femo_alpha_amd.solver.symbolic import build_plan
            _plans[(name, leaf)] = build_plan(m, leaf)
        plan = _plans[(name, leaf)]
    c.enable_frontal(leaf, plan=plan, **(pre or {}))
    c.set_solver(preconditioner=2, rtol=1e-12, maxit=30, check_every=1)
    return m, K, c


def _probes(n, k=4, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (k, n))


def _omega_of(what, c, K, k=4):
    """omega of one application to k random probes (all columns at once); no pivot may have been repaired."""
    V = _probes(K.shape[0], k)
    Z = c.frontal_apply(V)
    assert c.frontal_info()["pivots_repaired"] == 0, what
    w = omega(K, V.T, Z.T)
    print(f"omega {what} {w:.3e}")
    return w


def _check(name, what, leaf=8, pre=None, post=None, plan=None, bound=BOUND, **variant):
    m, K, c = _context(name, leaf, pre, post, plan, **variant)
    try:
        w = _omega_of(f"{name} {what}", c, K)
    finally:
        c.close()
    assert w <= bound, (name, what, w)
    return w


# ------------------------------------------------------------------ operators and variants, default schedule
@pytest.mark.parametrize("name", ["plate", "wing", "tri", "tri_cr1", "cg1", "tee"])
def test_operators_default_schedule(name):
    _check(name, "default")


@pytest.mark.parametrize("what,variant", [("element-wise material + uhat", dict(ewm=True, uhat=True)),
                                          ("laminate + uhat", dict(laminate=True, uhat=True)),
                                          ("laminate reduced strain rule", dict(laminate=True, nred=2)),
                                          ("reduced strain rule", dict(nred=2)),
                                          ("transient operator", dict(operator=(0.5, 2.0 / 1e-3 ** 2)))])
def test_operator_variants(what, variant):
    _check("wing_mid", what, **variant)


@pytest.mark.parametrize("name", ["plate", "wing"])
@pytest.mark.parametrize("fc", [0, 1, 2])
def test_front_assembly_forms(name, fc):
    _check(name, f"assemble_fc {fc}", post=dict(assemble_fc=fc))
    if name == "wing":
        _check("wing_mid", f"laminate assemble_fc {fc}", post=dict(assemble_fc=fc), laminate=True)


# ------------------------------------------------------------------ factorisation schedules, one option at a time
SP = dict(trailing=2, super_panel_cnt=100000)
SCHEDULES = [
    ("trailing 0", dict(trailing=0)), ("trailing 1", dict(trailing=1)), ("trailing 2", dict(trailing=2)),
    ("all left-looking", dict(trailing=0, left_min=1, left_max=100000)), ("all right-looking", dict(trailing=0, left_min=100000)),
    ("super_panel 200", dict(SP, super_panel=200)), ("super_panel 256", dict(SP, super_panel=256)),
    ("super_panel 384", dict(SP, super_panel=384)), ("super_panel 512", dict(SP, super_panel=512)),
    ("diag_v1 1", dict(diag_v1=1, diag_v1_cnt=1)), ("diag_v1 2", dict(diag_v1=2, diag_v1_cnt=1)),
    ("fuse_rows 0", dict(fuse_rows=0)), ("fuse_rows everywhere", dict(fuse_rows=1, fuse_rows_cnt=1, fuse_rows_np=256)),
    ("rows fine", dict(rows_fine_wg=100000, narrow_fine_wg=100000)),
    ("lookahead 0", dict(trailing=2, lookahead=0, super_panel=0)), ("lookahead 1", dict(trailing=2, lookahead=1, lookahead_cnt=1000, super_panel=0)),
    ("fused_schur 0", dict(fused_schur=0)),
    ("grid_chunk 3", dict(grid_chunk=3)), ("xinv_small_cnt 0", dict(xinv_small_cnt=0)), ("xinv_small_cnt all", dict(xinv_small_cnt=100000)),
    ("equilibrate 1", dict(equilibrate=1)), ("equilibrate 2", dict(equilibrate=2)),
]


@pytest.mark.parametrize("name", ["plate", "wing"])
def test_factorisation_schedules(name):
    bad = []
    for what, post in SCHEDULES:
        m, K, c = _context(name, post=post)
        try:
            w = _omega_of(f"{name} {what}", c, K)
        finally:
            c.close()
        if not w <= BOUND:
            bad.append((what, w))
    for what, pre in (("swork_slots 2", dict(swork_slots=2)),):
        m, K, c = _context(name, pre=pre)
        try:
            w = _omega_of(f"{name} {what}", c, K)
        finally:
            c.close()
        if not w <= BOUND:
            bad.append((what, w))
    from femo_alpha_amd.solver.symbolic import build_plan
    m = _mesh(name)
    _m, K, c = _context(name, plan=build_plan(m, 8, node_order=0))
    try:
        w = _omega_of(f"{name} node_order 0", c, K)
    finally:
        c.close()
    if not w <= BOUND:
        bad.append(("node_order 0", w))
    assert not bad, bad


# ------------------------------------------------------------------ sweeps
SWEEPS_PRE = [("wide_cnt 0", dict(wide_cnt=0)), ("wide_cnt 100000", dict(wide_cnt=100000)), ("wide_np 64", dict(wide_np=64)),
              ("wide_np 100000", dict(wide_np=100000)), ("no wide level", dict(wide_np=100000, wide_cnt=0))]
SWEEPS_POST = [("bnd_tiled_nb 0", dict(bnd_tiled_nb=0)), ("sweep_w", dict(sweep_w=1))] + \
              [(f"sweep_butterfly {b}", dict(sweep_butterfly=b)) for b in range(4)] + \
              [("sweep_graph 0", dict(sweep_graph=0)), ("sweep_graph 1", dict(sweep_graph=1))]


@pytest.mark.parametrize("name", ["plate", "wing"])
def test_sweep_forms(name):
    bad = []
    for what, pre, post in [(w, p, None) for w, p in SWEEPS_PRE] + [(w, None, p) for w, p in SWEEPS_POST]:
        m, K, c = _context(name, pre=pre, post=post)
        try:
            w = _omega_of(f"{name} {what}", c, K)
        finally:
            c.close()
        if not w <= BOUND:
            bad.append((what, w))
    assert not bad, bad


@pytest.mark.parametrize("name", ["plate", "wing"])
@pytest.mark.parametrize("post", [{}, dict(sweep_graph=1), dict(multi_rhs=0), dict(equilibrate=1)])
def test_several_vectors_column_by_column(name, post):
    """nrhs = 1 .. 6 through femo_frontal_apply: groups of up to four interleaved vectors (3 ride as 4, 5 = 4 + 1, 6 = 4 + 2), or one
    at a time where the grouped sweeps do not apply; every column against K and against the one-vector application."""
    _several_vectors(name, post=post)


def _several_vectors(name, leaf=8, pre=None, post=None):
    m, K, c = _context(name, leaf, pre=pre, post=post)
    try:
        V = _probes(m.ndof, 6, seed=7)
        Z1 = np.stack([c.frontal_apply(v) for v in V])
        for k in range(1, 7):
            Z = c.frontal_apply(V[:k])
            assert Z.shape == (k, m.ndof)
            for j in range(k):
                w = omega(K, V[j], Z[j])
                assert w <= BOUND, (k, j, w)
                assert np.abs(Z[j] - Z1[j]).max() <= 1e-12 * np.abs(Z1[j]).max(), (k, j)
        print(f"omega {name} nrhs 1..6 {pre or ''} {post} {omega(K, V.T, Z.T):.3e}")
        assert c.frontal_info()["pivots_repaired"] == 0
    finally:
        c.close()


# ------------------------------------------------------------------ sweep_ahead: the first application inside a cold PCG solve
@pytest.mark.parametrize("name", ["plate", "wing"])
def test_first_application_of_a_cold_solve(name):
    """With one PCG iteration from x = 0, x_1 = alpha M^-1 b: omega_fit sees the factor of the application "sweep_ahead" splits between
    the factorisation's side stream and the solve (0 = off; 50 = more levels than the tree has: off as well)."""
    for ahead in (0, 1, 2, 50):
        m, K, c = _context(name, post=dict(sweep_ahead=ahead, strict=0))
        try:
            c.set_solver(preconditioner=2, rtol=1e-12, maxit=1, check_every=1)
            b = _probes(m.ndof, 1, seed=9)[0]
            _, _, d = _problem(name)
            if d["sd"] is not None:
                b[np.asarray(d["sd"])] = 0.0              # PCG works on the masked right-hand side
            x1, it, _ = c.solve_linear(b)
            assert it == 1
            w = omega_fit(K, b, x1)
            print(f"omega {name} sweep_ahead {ahead} (fitted) {w:.3e}")
            assert w <= BOUND, (ahead, w)
        finally:
            c.close()


# ------------------------------------------------------------------ negative control
@pytest.mark.parametrize("nq", [4, 3])
def test_negative_control_lighter_front_quadrature(nq):
    """Fronts assembled with fewer Gauss points than the operator's 5 x 5 factor a slightly different matrix: omega must see it."""
    w = _check("wing", "default", bound=np.inf)
    wq = _check("wing", f"precond_nquad {nq}", post=dict(precond_nquad=nq), bound=np.inf)
    print(f"omega wing precond_nquad {nq}: {wq:.3e} = {wq / BOUND:.1e} x the bound ({wq / w:.1e} x the floor)")
    assert wq >= 100 * BOUND


# ------------------------------------------------------------------ grouped sweeps beyond the LDS of four interleaved vectors
def test_grouped_sweeps_of_a_front_too_large_for_four_vectors():
    """No wide level and leaves of 256 cells: the largest leaf front needs more LDS than four interleaved vectors may take (the plan
    upload lets the grouped application fall back to pairs); grouped applications and grouped solves stay exact and take the iterations
    of single solves."""
    m, K, c = _context("plate", leaf=256, pre=dict(wide_np=100000, wide_cnt=0))
    try:
        p = c.plan
        need = max(int(max(np.asarray(p.npiv)[list(l)])) + int(max((np.asarray(p.nf) - np.asarray(p.npiv))[list(l)])) for l in p.level_nodes) + 512
        assert need * 4 * 8 > 150 * 1024 >= need * 2 * 8, need
        V = _probes(m.ndof, 4, seed=3)
        Z = c.frontal_apply(V)
        w = omega(K, V.T, Z.T)
        print(f"omega plate leaf 256 no wide level, 4 vectors {w:.3e}")
        assert w <= BOUND
        Z1 = np.stack([c.frontal_apply(v) for v in V])
        assert np.abs(Z - Z1).max() <= 1e-12 * np.abs(Z1).max()
        X, its, _ = c.solve_linear_multi(V[:3])
        single = [c.solve_linear(v) for v in V[:3]]
        for j in range(3):
            assert its[j] == single[j][1], (its, [s[1] for s in single])
            assert np.abs(X[j] - single[j][0]).max() <= 1e-10 * np.abs(single[j][0]).max()
    finally:
        c.close()


# ------------------------------------------------------------------ NaN right-hand sides
@pytest.mark.parametrize("nrhs", [1, 3, 4])
def test_nan_right_hand_side_is_an_error(nrhs):
    from femo_alpha_amd._lib import FemoHipError
    m, K, c = _context("wing_mid")
    try:
        V = _probes(m.ndof, nrhs, seed=5)
        V[nrhs // 2, 17] = np.nan
        with pytest.raises(FemoHipError):
            if nrhs == 1:
                c.solve_linear(V[0])
            else:
                c.solve_linear_multi(V)
        V[nrhs // 2, 17] = 0.5
        X, its, rr = c.solve_linear_multi(V)
        assert np.all(rr <= 1e-12) and np.all(its >= 1)
        for j in range(nrhs):
            x, it, _ = c.solve_linear(V[j])
            assert it == its[j] and np.abs(x - X[j]).max() <= 1e-10 * np.abs(X[j]).max()
    finally:
        c.close()


# ------------------------------------------------------------------ per-front Schur blocks, level by level
@pytest.mark.parametrize("name", ["plate_small", "wing_small"])
@pytest.mark.parametrize("sched", ["default", "trailing 2 super_panel 256"])
def test_schur_blocks_level_by_level(name, sched):
    """After femo_factorize_range(l, l + 1) the Schur block of every front of level l is D - B A^-1 B^T of its subtree's own matrix
    (the element matrices of the subtree's cells; strong-BC rows and columns emptied, a unit diagonal where a constrained DOF is
    eliminated inside the subtree), in the scaled metric |S - S_ref|_ij / sqrt(S_ii S_jj).  A failure names the level and the front."""
    _schur_blocks_level_by_level(name, sched)


def _schur_blocks_level_by_level(name, sched, leaf=8):
    """Returns the number of fronts compared that have no pivots (their block is the plain sum of their children's blocks, or of
    their own cells' matrices: nothing is eliminated in them)."""
    import scipy.sparse.linalg as spla
    import torch
    from oracle.rm_shell_oracle import ShellOracle
    post = {"default": {}, "trailing 2 super_panel 256": dict(trailing=2, super_panel=256, super_panel_cnt=100000)}[sched]
    m, K, c = _context(name, leaf, post=post)
    pivot_free = 0
    try:
        _, _, d = _problem(name)
        o = ShellOracle(m, penalty_facets=d["pf"], strong_dofs=d["sd"])
        o.set_fields(h=d["f"]["thickness"], E=d["f"]["E"], nu=0.3, rho=2700.0, f=d["f"]["F_solid"])
        Ke = o.element_matrices()
        cd = m.cell_dofs()
        masked = np.zeros(m.ndof, bool)
        if d["sd"] is not None:
            masked[o.strong_dofs] = True
        plan = c.plan
        L = plan.nlevels
        level_of = np.empty(plan.ntree, int)
        for l, nodes in enumerate(plan.level_nodes):
            level_of[np.asarray(nodes)] = l
        parent = np.asarray(plan.parent)
        # penalty blocks belong to the subtree that holds all their DOFs (the facet's cell)
        pen = o._penalty_blocks()
        per_facet = max(len(pen) // max(o.penalty_facets.shape[0], 1), 1)      # blocks of one facet, one after the other
        keep = sp.diags((~masked).astype(float))
        worst = []
        for l in range(L):
            c.factorize_range(l, l + 1, l == 0)
            if l == L - 1:
                break                                          # the root has no Schur block
            top = np.asarray(plan.elem_front).copy()
            while True:
                up = np.where(level_of[top] < l, parent[top], top)
                if np.array_equal(up, top):
                    break
                top = up
            wl = 0.0
            for t in np.asarray(plan.level_nodes[l]):
                cells = np.nonzero(top == t)[0]
                dofs = np.asarray(plan.front_dofs[plan.dof_off[t]:plan.dof_off[t + 1]])
                npv = int(plan.npiv[t]); nb = dofs.size - npv
                if nb == 0:
                    continue
                bnd = dofs[npv:]
                rows = np.repeat(cd[cells], cd.shape[1], axis=1).ravel(); cols = np.tile(cd[cells], (1, cd.shape[1])).ravel()
                R, Cc, Vv = [rows], [cols], [Ke[cells].ravel()]
                cellset = set(cells.tolist())
                for i, (pd, blk) in enumerate(pen):
                    if int(o.penalty_facets[i // per_facet, 0]) in cellset:
                        R.append(np.repeat(pd, pd.size)); Cc.append(np.tile(pd, pd.size)); Vv.append(blk.ravel())
                Ks = sp.coo_matrix((np.concatenate(Vv), (np.concatenate(R), np.concatenate(Cc))), shape=K.shape).tocsr()
                interior = np.setdiff1d(np.unique(cd[cells]), bnd)
                unit = np.zeros(m.ndof); unit[interior[masked[interior]]] = 1.0
                Ks = (keep @ Ks @ keep + sp.diags(unit)).tocsr()
                A = Ks[interior][:, interior].tocsc(); B = Ks[bnd][:, interior]; D = Ks[bnd][:, bnd].toarray()
                # (a subtree that eliminates nothing -- a pivot-free leaf -- has no A: its block is D itself)
                S_ref = D - B @ spla.splu(A).solve(B.T.toarray()) if interior.size else D
                pivot_free += npv == 0
                S = torch.empty(nb * nb, dtype=torch.float64, device="cuda")
                c.front_schur_get(int(t), S)
                S = S.cpu().numpy().reshape(nb, nb).T              # column-major on the device; the lower triangle is maintained
                dg = np.abs(np.diag(S_ref)); dg = np.where(dg > 0, dg, 1.0)
                lo = np.tril_indices(nb)
                err = (np.abs(S - S_ref) / np.sqrt(np.outer(dg, dg)))[lo].max()
                wl = max(wl, err)
                assert err <= SCHUR_BOUND, (name, sched, "level", l, "front", int(t), err)
            worst.append(wl)
        print(f"schur {name} {sched} per level " + " ".join(f"{x:.1e}" for x in worst))
        V = _probes(m.ndof, 4)
        w = omega(K, V.T, c.frontal_apply(V).T)
        print(f"omega {name} {sched} after the level-by-level factorisation {w:.3e}")
        assert w <= BOUND
    finally:
        c.close()
    return pivot_free
