"""The verdict "not positive definite" (status 5, FemoNotPositiveDefiniteError) of the multifrontal factorisation, checked where a
single non-positive pivot decides it: tests/indefinite_ref.py knows, from an elimination on the host in the plan's order, how many
negative pivots K - sigma M (or K with one cell of negative modulus) has and in which tree level, front, panel and sub-block the
first one lies (tests/test_indefinite_cpu.py pins that reference and the coverage of its cases).  Here: the verdict under every
factorisation schedule, the tree level that raises when the factorisation is taken level by level, every entry point that
factorises on demand, the repair mode, non-finite input -- and, each time, that an operator close to indefinite is accepted and that
the context recovers.  Measured values are printed as "omega <case> <value>" and "verdict <case> level <observed> (expected <e>)"."""
import time

import numpy as np
import pytest

import indefinite_ref as ref
from test_gpu_factor_backward_error import BOUND, SCHEDULES, _context, _mesh, _omega_of, _probes, _problem

pytestmark = pytest.mark.gpu

# level by level: the two schedules of test_schur_blocks_level_by_level, and k_diag_block on every level (by default the levels of
# these small trees have too few fronts for it: "diag_v1_cnt")
LEVEL_SCHEDULES = {"default": {}, "trailing 2 super_panel 256": dict(trailing=2, super_panel=256, super_panel_cnt=100000),
                   "diag_v1 1": dict(diag_v1=1, diag_v1_cnt=1)}
FUSE_ALL = dict(fuse_rows=1, fuse_rows_cnt=1, fuse_rows_np=256)


def _npd():
    from femo_alpha_amd.backend import FemoNotPositiveDefiniteError
    return FemoNotPositiveDefiniteError


def _raises_npd(call):
    """None if ``call`` raises FemoNotPositiveDefiniteError, else what happened instead."""
    try:
        call()
    except _npd():
        return None
    except Exception as e:                                   # another error is not the promised status
        return f"raised {type(e).__name__}: {e}"
    return "returned normally"


# ------------------------------------------------------------------ (a) the verdict under every schedule
def _plate_schedules():
    from femo_alpha_amd.solver.symbolic import build_plan
    out = [(what, dict(post=post)) for what, post in SCHEDULES if "equilibrate" not in post]
    out.append(("swork_slots 2", dict(pre=dict(swork_slots=2))))
    out.append(("node_order 0", dict(plan=build_plan(_mesh("plate"), 8, node_order=0))))
    out += [(f"fuse_rows everywhere diag_v1 {v}", dict(post=dict(FUSE_ALL, diag_v1=v, diag_v1_cnt=1))) for v in (0, 1, 2)]
    out += [(f"assemble_fc {fc}", dict(post=dict(assemble_fc=fc))) for fc in (0, 2)]
    return out


def _verdict_sequence(what, c, accepted, rejected, v):
    """Near misses are factorised and applied exactly (``accepted``: (label, switch, K)); every operator of ``rejected`` ((label,
    switch)) raises from factorize() and again from the frontal_apply() that follows.  Returns the list of what went wrong."""
    bad = []
    for label, switch, K in accepted:
        switch(c)
        try:
            info = c.factorize()
            w = _omega_of(f"{what}, {label}", c, K)
            if info["pivots_repaired"] != 0 or not w <= BOUND:
                bad.append((what, label, "omega", w, "pivots_repaired", info["pivots_repaired"]))
        except Exception as e:
            bad.append((what, label, f"{type(e).__name__}: {e}"))
    for label, switch in rejected:
        switch(c)
        for step, call in (("factorize", c.factorize), ("frontal_apply after the failure", lambda: c.frontal_apply(v))):
            r = _raises_npd(call)
            if r is not None:
                bad.append((what, label, step, r))
    return bad


def test_verdict_under_every_schedule():
    """64 x 64 plate, K - sigma M: the near miss (sigma = lambda_1 / 2) is accepted and exact, ONE negative pivot late in the root front
    (582 pivots: fourth 128-column panel, second 256-column super-panel, third sub-block) and then three (level 8 and the root) are
    refused by factorize() and by the frontal_apply() that follows; back at sigma = 0 the same context factorises exactly."""
    t0 = time.perf_counter()
    lam, cases = ref.shifted_cases("plate", scan=False)
    near, one, three = cases[:3]
    K_near = ref.matrix("plate", near["sigma"])
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    v = _probes(K_near.shape[0], 1, seed=11)[0]
    shift = lambda s: (lambda c: c.set_operator(1.0, -s))
    bad = []
    for what, kw in _plate_schedules():
        m, K0, c = _context("plate", **kw)
        try:
            bad += _verdict_sequence(f"plate {what}", c, [("near miss", shift(near["sigma"]), K_near)],
                                     [("one negative", shift(one["sigma"])), ("three negative", shift(three["sigma"]))], v)
            c.set_operator(1.0, 0.0)
            w = _omega_of(f"plate {what}, sigma 0 after the failures", c, K0)
            if not w <= BOUND:
                bad.append((what, "sigma 0 after the failures", w))
        except Exception as e:
            bad.append((what, f"{type(e).__name__}: {e}"))
        finally:
            c.close()
    print(f"time verdict_under_every_schedule: reference {t_cpu:.1f} s, contexts and GPU {time.perf_counter() - t0:.1f} s")
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.parametrize("eq", [1, 2])
def test_verdict_with_equilibration(eq):
    """"equilibrate" refuses an inertia term: the static operator with one cell of negative modulus instead (wing_small,
    element-wise material), the modulus restored afterwards."""
    cases = ref.negative_cell_cases("wing_small")
    m, K0, c = _context("wing_small", post=dict(equilibrate=eq), ewm=True)
    try:
        E0 = _problem("wing_small", ewm=True)[2]["f"]["E"]
        v = _probes(m.ndof, 1, seed=11)[0]
        assert _omega_of(f"wing_small equilibrate {eq}", c, K0) <= BOUND
        cell = lambda r: (lambda c: c.set_field("E", ref.cell_modulus("wing_small", r["cell"], r["factor"])))
        bad = _verdict_sequence(f"wing_small equilibrate {eq}", c, [], [(r["label"], cell(r)) for r in cases], v)
        c.set_field("E", E0)
        w = _omega_of(f"wing_small equilibrate {eq}, modulus restored", c, K0)
        assert not bad and w <= BOUND, "\n".join(map(str, bad + [w]))
    finally:
        c.close()


# ------------------------------------------------------------------ (b) the level that raises
def _level_that_raises(c):
    """Factorise level by level; the level whose range raises the verdict (None: the whole tree went through)."""
    for l in range(c.plan.nlevels):
        try:
            c.factorize_range(l, l + 1, l == 0)
        except _npd():
            return l
    return None


@pytest.mark.parametrize("name", ["plate_small", "wing_small"])
@pytest.mark.parametrize("sched", list(LEVEL_SCHEDULES))
def test_the_level_that_raises(name, sched):
    """femo_factorize_range(l, l + 1) for l = 0, 1, ...: every range below the level of the first non-positive pivot returns normally,
    the range of that level raises.  A later verdict is a missed pivot that only the NaNs it spread exposed, an earlier one a false
    positive.  Cases: every shift of indefinite_ref.shifted_cases (the root, level 0 and the levels between that a shift can reach; the
    near miss raises nowhere) and, on wing_small, one cell of negative modulus (level 0, in the middle of a leaf front)."""
    t0 = time.perf_counter()
    lam, cases = ref.shifted_cases(name)
    cells = ref.negative_cell_cases(name) if name == "wing_small" else []
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    bad = []
    m, K0, c = _context(name, post=LEVEL_SCHEDULES[sched])
    try:
        for r in cases:
            c.set_operator(1.0, -r["sigma"])
            got = _level_that_raises(c)
            print(f"verdict {name} {sched} {r['label']} (sigma {r['sigma']:.4e}, {r['count']} negative): level {got} (expected {r['level']})")
            if got != r["level"]:
                bad.append(dict(case=r["label"], schedule=sched, expected_level=r["level"], observed_level=got,
                                front=r["front"], column=r["column"]))
        c.set_operator(1.0, 0.0)
        assert _level_that_raises(c) is None
        assert _omega_of(f"{name} {sched} sigma 0 after the level-by-level failures", c, K0) <= BOUND
    finally:
        c.close()
    if cells:
        m, K0, c = _context(name, post=LEVEL_SCHEDULES[sched], ewm=True)
        try:
            for r in cells:
                c.set_field("E", ref.cell_modulus(name, r["cell"], r["factor"]))
                got = _level_that_raises(c)
                print(f"verdict {name} {sched} {r['label']} ({r['count']} negative, first at column {r['column']}): level {got} (expected 0)")
                if got != 0:
                    bad.append(dict(case=r["label"], schedule=sched, expected_level=0, observed_level=got, front=r["front"], column=r["column"]))
            c.set_field("E", _problem(name, ewm=True)[2]["f"]["E"])
            assert _level_that_raises(c) is None
            assert _omega_of(f"{name} {sched} modulus restored after the level-by-level failures", c, K0) <= BOUND
        finally:
            c.close()
    print(f"time the_level_that_raises {name} {sched}: reference {t_cpu:.1f} s, contexts and GPU {time.perf_counter() - t0:.1f} s")
    assert not bad, "\n".join(map(str, bad))


# ------------------------------------------------------------------ (c) every entry point that factorises on demand
def _entry_points(c, m):
    rng = np.random.default_rng(21)
    B = rng.uniform(-1, 1, (4, m.ndof))
    dh = rng.uniform(-1, 1, c.field_size("thickness"))

    def solve_state(ahead):
        def call():
            c.set_option("sweep_ahead", ahead)
            c.solve_state(zero_guess=True)
        return call
    return [(f"solve_state sweep_ahead {a}", solve_state(a)) for a in (0, 1, 2, 50)] + [
        ("solve_linear", lambda: c.solve_linear(B[0])),
        ("solve_linear_multi 3", lambda: c.solve_linear_multi(B[:3])),
        ("frontal_apply 1", lambda: c.frontal_apply(B[0])),
        ("frontal_apply 4", lambda: c.frontal_apply(B)),
        ("total_gradient", lambda: c.total_gradient("compliance", "thickness")),
        ("total_jvp", lambda: c.total_jvp("thickness", dh, functionals=("compliance",))),
        ("factorize_profile", lambda: c.factorize_profile()),
    ]


@pytest.mark.parametrize("family", ["shift", "cell"])
def test_every_entry_point_passes_the_verdict_on(family):
    """wing_small with one negative pivot (root front, column 73 of 78) or one cell of negative modulus, a cold factor each time: every
    entry point that factorises on demand raises FemoNotPositiveDefiniteError.  After each one the positive definite operator is
    restored, and the next cold solve_state(zero_guess=True) -- the reuse path after a failed factorisation, with the forward sweep
    of "sweep_ahead" started beside it -- takes the iterations of a fresh context and agrees with its state to 1e-10."""
    t0 = time.perf_counter()
    ewm = family == "cell"
    if ewm:
        r = ref.negative_cell_cases("wing_small")[-1]                     # E x -1e-3: the fewest negative pivots
        E0 = _problem("wing_small", ewm=True)[2]["f"]["E"]
        spoil = lambda c: c.set_field("E", ref.cell_modulus("wing_small", r["cell"], r["factor"]))
        restore = lambda c: c.set_field("E", E0)
    else:
        r = ref.shifted_cases("wing_small")[1][1]
        assert r["count"] == 1
        spoil = lambda c: c.set_operator(1.0, -r["sigma"])
        restore = lambda c: c.set_operator(1.0, 0.0)
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    m, K0, fresh = _context("wing_small", ewm=ewm)
    try:
        it0, rr0 = fresh.solve_state(zero_guess=True)
        w0 = fresh.get_state()
    finally:
        fresh.close()
    assert rr0 <= 1e-12 and np.all(np.isfinite(w0))
    m, K0, c = _context("wing_small", ewm=ewm)
    bad = []
    try:
        c.solve_state(zero_guess=True)                                    # a state for the derivative entry points
        for what, call in _entry_points(c, m):
            spoil(c)                                                      # invalidates the factor: the call meets a cold one
            res = _raises_npd(call)
            if res is not None:
                bad.append((family, what, res))
            restore(c)
            it, rr = c.solve_state(zero_guess=True)
            err = np.abs(c.get_state() - w0).max() / np.abs(w0).max()
            print(f"verdict wing_small {r['label']} {what}: {'raised' if res is None else res}; recovery {it} iterations (fresh {it0}), "
                  f"state off by {err:.1e}")
            if it != it0 or not err <= 1e-10:
                bad.append((family, what, "recovery", it, it0, err))
            if c.frontal_info()["pivots_repaired"] != 0:
                bad.append((family, what, "pivots_repaired after the recovery", c.frontal_info()["pivots_repaired"]))
    finally:
        c.close()
    print(f"time every_entry_point {family}: reference {t_cpu:.1f} s, contexts and GPU {time.perf_counter() - t0:.1f} s")
    assert not bad, "\n".join(map(str, bad))


# ------------------------------------------------------------------ (d) repair mode
@pytest.mark.parametrize("diag_v1", [1, 2])
def test_repair_mode_counts_and_recovers(diag_v1):
    """"allow_pivot_repair" with k_diag_block (diag_v1 1) and k_diag_block2<true> (diag_v1 2) on wing_small: the near miss repairs
    nothing; one negative pivot in the root, and the case whose first one lies at level 0, repair at least one, and the application of
    the repaired factor is finite; the next positive definite factorisation reports 0 again.  The exact count is not asserted: after
    the first repair the matrix that is eliminated is a different one, and Sylvester's count no longer applies to it."""
    lam, cases = ref.shifted_cases("wing_small")
    near, one = cases[0], cases[1]
    leaf = [r for r in cases if r["level"] == 0][0]
    m, K0, c = _context("wing_small", post=dict(allow_pivot_repair=1, diag_v1=diag_v1, diag_v1_cnt=1))
    try:
        v = _probes(m.ndof, 4, seed=13)
        c.set_operator(1.0, -near["sigma"])
        assert c.factorize()["pivots_repaired"] == 0
        assert _omega_of(f"wing_small repair mode diag_v1 {diag_v1}, near miss", c, ref.matrix("wing_small", near["sigma"])) <= BOUND
        for r in (one, leaf):
            c.set_operator(1.0, -r["sigma"])
            n = c.factorize()["pivots_repaired"]
            z = c.frontal_apply(v)
            print(f"verdict wing_small repair mode diag_v1 {diag_v1} {r['label']}: {n} repaired ({r['count']} negative pivots in the reference)")
            assert n >= 1, (r["label"], n)
            assert np.all(np.isfinite(z)), r["label"]
        c.set_operator(1.0, 0.0)
        assert c.factorize()["pivots_repaired"] == 0
        assert _omega_of(f"wing_small repair mode diag_v1 {diag_v1}, sigma 0 after the repairs", c, K0) <= BOUND
    finally:
        c.close()


# ------------------------------------------------------------------ (e) non-finite input
def test_nan_thickness_is_an_error_and_the_context_recovers():
    from femo_alpha_amd._lib import FemoHipError
    m, K0, fresh = _context("wing_small")
    try:
        it0, rr0 = fresh.solve_state(zero_guess=True)
        w0 = fresh.get_state()
    finally:
        fresh.close()
    m, K0, c = _context("wing_small")
    try:
        h0 = _problem("wing_small")[2]["f"]["thickness"]
        h = h0.copy()
        h[m.nn // 2] = np.nan
        with pytest.raises(FemoHipError):
            c.set_field("thickness", h)
            c.factorize()
        with pytest.raises(FemoHipError):
            c.solve_state(zero_guess=True)
        c.set_field("thickness", h0)
        it, rr = c.solve_state(zero_guess=True)
        err = np.abs(c.get_state() - w0).max() / np.abs(w0).max()
        print(f"verdict wing_small NaN thickness: recovery {it} iterations (fresh {it0}), state off by {err:.1e}")
        assert it == it0 and err <= 1e-10
        assert _omega_of("wing_small after a NaN thickness", c, K0) <= BOUND
    finally:
        c.close()
