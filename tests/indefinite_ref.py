"""Host reference of the not-positive-definite verdict (tests/test_indefinite_cpu.py pins it, tests/test_gpu_indefinite.py uses it).

For a symmetric matrix eliminated without pivoting in the plan's order the number of negative pivots is the number of negative
eigenvalues (Sylvester), and the position of the first one is a property of the matrix and the order alone: a front's pivots
depend only on its own subtree, so in the level-major order of the plan the first non-positive pivot lies on the lowest tree level
that has one -- the level at which a factorisation taken level by level has to fail.  With K - sigma M (set_operator(1, -sigma))
sigma chooses how many negative pivots there are and how high in the tree the first one falls; one cell of negative modulus puts
them into that cell's leaf front.

Every case handed out keeps a margin (MARGIN): in units of the pivots d0 of K itself, the first non-positive pivot is below
-MARGIN and every pivot before it above +MARGIN, so that rounding (the GPU's factor is exact to ~1e-14) cannot move the verdict to
another level."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from test_gpu_factor_backward_error import _fields, _marker, _mesh, _plans, _strong

NBO, NB = 128, 32        # outer panel and sub-block of the numeric phase (csrc/frontal.h)
MARGIN = 1e-3
LEAF = 8
ONE_NEGATIVE_THETAS = (0.5, 0.35, 0.25, 0.15)     # sigma = lambda_1 + theta (lambda_2 - lambda_1), the first that serves

_base, _shifted, _cells = {}, {}, {}


def plan_of(name, leaf=LEAF):
    """build_plan(mesh, leaf): the plan _context(name, leaf) hands to the device (one cache for both)."""
    if (name, leaf) not in _plans:
        from femo_alpha_amd.solver.symbolic import build_plan
        _plans[(name, leaf)] = build_plan(_mesh(name), leaf)
    return _plans[(name, leaf)]


def elimination_order(plan):
    """The pivot DOFs of every front, level by level in the order of plan.level_nodes, and per position the level, the front, the
    column inside the front, its 128-column panel and its 32-column sub-block inside the panel."""
    dofs, level, front, column = [], [], [], []
    for l, nodes in enumerate(plan.level_nodes):
        for t in np.asarray(nodes):
            npv = int(plan.npiv[t])
            if npv == 0:
                continue
            o = int(plan.dof_off[t])
            dofs.append(np.asarray(plan.front_dofs[o:o + npv], dtype=np.int64))
            level.append(np.full(npv, l)); front.append(np.full(npv, int(t))); column.append(np.arange(npv))
    out = dict(dofs=np.concatenate(dofs), level=np.concatenate(level), front=np.concatenate(front), column=np.concatenate(column))
    out["panel"] = out["column"] // NBO
    out["sub"] = out["column"] % NBO // NB
    return out


def pivots_in_plan_order(A, plan, order=None):
    """The pivots of the elimination of ``A`` in the plan's order, no pivoting (SuperLU: natural order, threshold 0)."""
    p = (elimination_order(plan) if order is None else order)["dofs"]
    n = A.shape[0]
    assert p.size == n and np.array_equal(np.sort(p), np.arange(n)), "every DOF is the pivot of exactly one front"
    B = sp.csc_matrix(sp.csr_matrix(A)[p][:, p])
    lu = spla.splu(B, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    assert np.array_equal(lu.perm_r, np.arange(n)) and np.array_equal(lu.perm_c, np.arange(n))
    return lu.U.diagonal()


def _oracle(name, ewm=False, E=None):
    """The oracle of _problem(name, ewm=ewm) (same mesh, fields and clamp), optionally with another modulus."""
    from oracle.rm_shell_oracle import ShellOracle
    m = _mesh(name)
    f = _fields(m, ewm)
    strong = _strong(name)
    sd = m.locate_dofs_geometrical(_marker(name, strong)) if strong else None
    pf = None if strong else m.penalty_facets(_marker(name, strong))
    o = ShellOracle(m, element_wise_material=ewm, penalty_facets=pf, strong_dofs=sd)
    o.set_fields(h=f["thickness"], E=f["E"] if E is None else E, nu=0.3, rho=2700.0, f=f["F_solid"])
    return m, o, f, strong


def _pencil(name):
    if name not in _base:
        m, o, f, strong = _oracle(name)
        K = o.assemble_K(with_strong=False) if strong else o.assemble_K()
        M = o.assemble_M()
        free = np.setdiff1d(np.arange(m.ndof), o.strong_dofs) if strong else np.arange(m.ndof)
        order = elimination_order(plan_of(name))
        _base[name] = dict(o=o, K=K, M=M, strong=strong, free=free, order=order)
        _base[name]["d0"] = pivots_in_plan_order(matrix(name, 0.0), plan_of(name), order)
        assert np.all(_base[name]["d0"] > 0)
    return _base[name]


def matrix(name, sigma):
    """K - sigma M as _problem(name, operator=(1.0, -sigma)) builds it."""
    b = _pencil(name)
    aK, aM = 1.0, -sigma
    return sp.csr_matrix(b["o"]._apply_strong((aK * b["K"] + aM * b["M"]).tocsr()) if b["strong"] else (aK * b["K"] + aM * b["M"]))


def lowest_eigenvalues(name, k=8):
    """The k lowest eigenvalues of the pencil (K, M) on the free DOFs (shift-invert at 0)."""
    b = _pencil(name)
    fr = b["free"]
    Kf = sp.csc_matrix(sp.csr_matrix(b["K"])[fr][:, fr]); Mf = sp.csc_matrix(sp.csr_matrix(b["M"])[fr][:, fr])
    lam = spla.eigsh(Kf, k=k, M=Mf, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-10,
                     v0=np.random.default_rng(0).uniform(-1, 1, fr.size))
    return np.sort(lam)


def record(label, d, d0, order, **more):
    """What the pivots ``d`` say (``d0``: those of the positive definite operator): number of negative pivots, where the first one
    lies, and the two margins."""
    ratio = d / d0
    neg = np.nonzero(~(d > 0))[0]
    r = dict(label=label, count=int(neg.size), min_ratio_before=float(ratio.min()), **more)
    if neg.size == 0:
        r.update(level=None, front=None, column=None, panel=None, sub=None, npiv_front=None, first_ratio=None)
        return r
    k = int(neg[0])
    t = int(order["front"][k])
    r.update(level=int(order["level"][k]), front=t, column=int(order["column"][k]), panel=int(order["panel"][k]), sub=int(order["sub"][k]),
             npiv_front=int(np.sum(order["front"] == t)), first_ratio=float(ratio[k]),
             min_ratio_before=float(ratio[:k].min()) if k else np.inf,
             negatives=[(int(order["level"][i]), int(order["front"][i]), int(order["column"][i])) for i in neg[:8]])
    return r


def has_margin(r):
    if r["count"] == 0:
        return r["min_ratio_before"] >= MARGIN
    return r["first_ratio"] <= -MARGIN and r["min_ratio_before"] >= MARGIN


def _shift_record(name, label, sigma):
    b = _pencil(name)
    return record(label, pivots_in_plan_order(matrix(name, sigma), plan_of(name), b["order"]), b["d0"], b["order"], sigma=float(sigma))


def shifted_cases(name, scan=True):
    """(lowest eigenvalues of the pencil, cases) of K - sigma M on the problem ``name`` of test_gpu_factor_backward_error._problem:
    the near miss lambda_1 / 2, one negative pivot (between lambda_1 and lambda_2), three ((lambda_3 + lambda_4) / 2) and, with ``scan``,
    one sigma for every further tree level that can be reached: a geometric scan upwards from lambda_8, then bisection (the first
    negative position never moves up the tree as sigma grows).  Every case keeps MARGIN (asserted)."""
    if (name, scan) in _shifted:
        return _shifted[(name, scan)]
    lam = lowest_eigenvalues(name, 8)
    nlev = plan_of(name).nlevels
    # one negative pivot: any sigma between lambda_1 and lambda_2; the middle, unless the pivot then opens a 128-column panel (its first
    # 32-column sub-block) -- a smaller shift moves it towards the end of the root front
    for theta in ONE_NEGATIVE_THETAS:
        one = _shift_record(name, "one negative", lam[0] + theta * (lam[1] - lam[0]))
        if one["count"] == 1 and one["level"] == nlev - 1 and one["sub"] > 0 and has_margin(one):
            break
    cases = [_shift_record(name, "near miss", 0.5 * lam[0]), one, _shift_record(name, "three negative", 0.5 * (lam[2] + lam[3]))]
    if scan:
        seen = {}                                              # sigma -> record
        s = lam[7]
        while True:
            seen[s] = _shift_record(name, "scan", s)
            if seen[s]["level"] == 0 or s > 1e8 * lam[7]:
                break
            s *= 4.0
        have = {c["level"] for c in cases[1:]}
        for target in range(min(have) - 1, -1, -1):
            ok = []
            for _ in range(40):
                ok = [r for r in seen.values() if r["level"] == target and has_margin(r)]
                if ok:
                    break
                sig = sorted(seen)
                above = [x for x in sig if seen[x]["level"] > target]          # too small a shift
                below = [x for x in sig if seen[x]["level"] < target]          # too large a one
                hit = [x for x in sig if seen[x]["level"] == target]           # on the level, but short of the margin: look beside them
                if not above or not (below or hit):
                    break
                if not hit:
                    gaps = [(max(above), min(below))]
                else:
                    gaps = [(max(above), min(hit))] + ([(max(hit), min(below))] if below else [(max(hit), 2.0 * max(hit))])
                lo, hi = max(gaps, key=lambda g: g[1] / g[0])
                if hi / lo < 1 + 1e-6:
                    break                                                      # the level cannot be reached (or not with the margin)
                mid = float(np.sqrt(lo * hi))
                seen[mid] = _shift_record(name, "scan", mid)
            if ok:
                r = dict(min(ok, key=lambda r: r["sigma"]))
                r["label"] = f"level {target}"
                cases.append(r)
    for r in cases:
        assert has_margin(r), r
    assert cases[0]["count"] == 0 and cases[1]["count"] == 1 and cases[2]["count"] == 3, [c["count"] for c in cases[:3]]
    need = max(c["count"] for c in cases) + 4
    if need > 8:
        lam = lowest_eigenvalues(name, need)
    _shifted[(name, scan)] = (lam, cases)
    return _shifted[(name, scan)]


# ------------------------------------------------------------------ one cell of negative modulus (static operator)
CELL_FACTORS = (-1.0, -1e-3)


def cell_modulus(name, cell, factor):
    m = _mesh(name)
    E = _fields(m, True)["E"].copy()
    E[cell] *= factor
    return E


def negative_cell_cases(name="wing_small", want=2):
    """Static operator, element-wise material, E of one cell times -1 or -1e-3: the records of shifted_cases, with 'cell' and
    'factor' in place of 'sigma'; 'K' is the oracle's matrix.  ``want`` cells per factor, the first ones (from a fixed list spread
    over the mesh) whose first negative pivot keeps MARGIN."""
    if (name, want) in _cells:
        return _cells[(name, want)]
    plan = plan_of(name)
    order = elimination_order(plan)
    m, o, f, strong = _oracle(name, ewm=True)
    d0 = pivots_in_plan_order(o.assemble_K(), plan, order)
    assert np.all(d0 > 0)
    cases = []
    for factor in CELL_FACTORS:
        got = 0
        for cell in (np.arange(1, 24) * m.nel // 24 + 1):
            o.set_fields(E=cell_modulus(name, cell, factor))
            K = sp.csr_matrix(o.assemble_K())
            r = record(f"cell {cell} E x {factor:g}", pivots_in_plan_order(K, plan, order), d0, order, cell=int(cell), factor=factor)
            # (a pivot that belongs to the cell alone has d / d0 = factor exactly: 1.2 MARGIN keeps such a tie out of the choice)
            if r["count"] and has_margin(r) and r["first_ratio"] <= -1.2 * MARGIN and r["level"] == 0 and r["column"] > 0:
                r["K"] = K
                cases.append(r)
                got += 1
                if got == want:
                    break
        assert got == want, (factor, got)
    _cells[(name, want)] = cases
    return cases


def table(name, cases):
    rows = [f"{name}: {plan_of(name).nlevels} levels"]
    for r in cases:
        where = "none" if r["count"] == 0 else \
            f"level {r['level']} front {r['front']} column {r['column']} of {r['npiv_front']} (panel {r['panel']}, sub-block {r['sub']})"
        key = f"sigma {r['sigma']:.4e}" if "sigma" in r else f"cell {r['cell']}"
        fr = "" if r["count"] == 0 else f" first d/d0 {r['first_ratio']:.2e}"
        rows.append(f"  {r['label']:<22} {key:<18} negatives {r['count']:>4}  first: {where};{fr} smallest d/d0 before {r['min_ratio_before']:.2e}")
    return "\n".join(rows)
