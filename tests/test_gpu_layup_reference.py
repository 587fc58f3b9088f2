"""Layups about an offset reference surface on the GPU (femo_set_layup_reference): the laminate and the ply table built on the device
against the host step of femo_alpha_amd/laminate.py, the chain kernels against tests/layup_reference_ref.py, the totals against the
host contraction of the device's own totals with respect to "laminate" and "ply_table" and against finite differences of the oracle's
solve, the handling of the mode, and the model."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh                                       # noqa: E402
from layup_reference_ref import LayupReferenceRef                                # noqa: E402
from test_gpu_laminate import BETA, CLAMP, ROOT_EDGE, _mesh, tight               # noqa: E402
from test_gpu_layup import _layup                                                # noqa: E402
from test_layup_cpu import _plies                                                # noqa: E402

pytestmark = pytest.mark.gpu

MESHES = {"3x7": lambda: plate_mesh(2.0, 10.0, 3, 7), "5x13": lambda: plate_mesh(2.0, 10.0, 5, 13), "warped": lambda: _mesh("warped"),
          "tri": lambda: _mesh("tri")}
LAYUPS = {"1 top": (1, ("top",)), "5 bot/mid/top": (5, ("bot", "mid", "top")), "16 bot/top": (16, ("bot", "top")), "32 none": (32, ())}
REFS = ("bot", "top", "0.3 + c", "mid + 0")
WRT = ("ply_thickness", "ply_angle")
H0 = 0.05
# every (layup, reference) pair on the 65 cells of one wave plus one cell; on the other meshes a Latin square of the two
CASES = [("5x13", l, r) for l in LAYUPS for r in REFS] + \
        [(k, l, REFS[(i + j) % 4]) for i, k in enumerate(("3x7", "warped", "tri")) for j, l in enumerate(LAYUPS)]


def _reference(name, nel, rng):
    """(reference, offset) of a case; the per-cell c is of the order of H, either sign, and not constant."""
    if name == "0.3 + c":
        return 0.3, H0 * rng.uniform(-1, 1, nel)
    if name == "mid + 0":
        return "mid", np.zeros(nel)
    return name, None


def _ctx(kind, layup, ref, seed=0, shear=False):
    from femo_alpha_amd.backend import ShellContext
    m = MESHES[kind]()
    nply, surfaces = LAYUPS[layup]
    rng = np.random.default_rng(seed)
    pc = _plies(nply, rng)
    t, theta = _layup(m.nel, nply, rng, h=H0)
    reference, off = _reference(ref, m.nel, rng)
    c = ShellContext(m)
    fields = dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=rng.uniform(-1, 1, (m.nn, 3)),
                  uhat=0.02 * rng.uniform(-1, 1, (m.nn, 3)))
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE if kind in ("warped", "tri") else CLAMP), BETA)
    S = 5e4 * (1 + 0.3 * rng.uniform(0, 1, (nply, 2))) if shear else None
    c.set_layup(pc, t, theta, surfaces, reference=reference, offset=off, shear_strength=S)
    kw = dict(reference=reference, offset=0.0 if off is None else off)
    D = lm.clt_from_plies(*[np.broadcast_to(pc[:, k], t.shape) for k in range(6)], t, theta, **kw)[2]
    R = LayupReferenceRef(pc, t, theta, surfaces, c_drill=12.0 * float(np.max(D)), **kw)        # 12 max(D) about the chosen surface
    R.fields, R.S = fields, S
    return m, c, R, rng


def _built(c, R):
    lam = c.get_field("laminate").reshape(R.nel, 32)
    tab = c.get_field("ply_table").reshape(R.nel, R.npt, 16) if R.ns else None
    return lam, tab


# ------------------------------------------------------------------------------------------ 4. build parity
def _build_distance(R, lam, tab):
    """test_gpu_layup._build_distance with the extent Z_e = max_i |z_i| of the cell about its reference surface in place of H: A:
    max|A| of the cell, B: Z max|A|, D: Z^2 max|A|, A_s: max|A_s|, G: max|G| of the point, z: Z."""
    lr, tr = R.values()
    Z = np.abs(R.interfaces()).max(axis=1)
    a = np.abs(lr[:, 0:9]).max(axis=1)
    d = {"A": np.abs(lam[:, 0:9] - lr[:, 0:9]).max(axis=1) / a,
         "B": np.abs(lam[:, 9:18] - lr[:, 9:18]).max(axis=1) / (Z * a),
         "D": np.abs(lam[:, 18:27] - lr[:, 18:27]).max(axis=1) / (Z * Z * a),
         "A_s": np.abs(lam[:, 27:31] - lr[:, 27:31]).max(axis=1) / np.abs(lr[:, 27:31]).max(axis=1)}
    assert np.array_equal(lam[:, 31], lr[:, 31])                                  # c_drill: 12 max(D) about the surface, a constant
    if tr is not None:
        d["G"] = np.abs(tab[..., 0:9] - tr[..., 0:9]).max(axis=2) / np.abs(tr[..., 0:9]).max(axis=2)
        d["z"] = np.abs(tab[..., 9] - tr[..., 9]) / Z[:, None]
        assert np.array_equal(tab[..., 10:16], tr[..., 10:16])                    # the strength coefficients: the same bits
    return {k: float(np.max(v)) for k, v in d.items()}


@pytest.mark.parametrize("kind,layup,ref", CASES)
def test_build_parity(kind, layup, ref):
    """1e-13 of the block's scale, the rounding argument of test_gpu_layup.py (<= 32 products of <= 7 factors) with the extent of the
    cell about its reference surface as the length scale."""
    m, c, R, rng = _ctx(kind, layup, ref)
    lam, tab = _built(c, R)
    d = _build_distance(R, lam, tab)
    print(f"build parity [{kind}, {layup}, {ref}]: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
    for k, v in d.items():
        assert v <= 1e-13, k
    if ref in ("bot", "top"):                                                      # a stack about its bottom or top couples: B != 0
        assert np.abs(lam[:, 9:18]).max() > 0.1 * np.abs(R.interfaces()).max() * np.abs(lam[:, 0:9]).max()
    r, off = c.get_layup_reference()
    assert r == R.r and np.array_equal(off, R.offset)
    # new thicknesses keep the surface, and move it with H where r != 0
    t2 = R.t * (1 + 0.1 * rng.uniform(-1, 1, R.t.shape))
    c.set_field("ply_thickness", t2)
    R2 = LayupReferenceRef(R.pc, t2, R.theta, R.surfaces, R.c_drill, R.r, R.offset)
    for k, v in _build_distance(R2, *_built(c, R2)).items():
        assert v <= 1e-13, k
    c.close()


@pytest.mark.parametrize("kind,layup", [("5x13", "5 bot/mid/top"), ("tri", "16 bot/top"), ("3x7", "32 none")])
def test_the_default_and_an_explicit_mid_surface_without_offsets_give_the_same_bits(kind, layup):
    m, a, R, rng = _ctx(kind, layup, "mid + 0")
    nply, surfaces = LAYUPS[layup]
    from femo_alpha_amd.backend import ShellContext
    b = ShellContext(m)
    for k, v in R.fields.items():
        b.set_field(k, v)
    b.set_penalty_facets(m.penalty_facets(ROOT_EDGE if kind == "tri" else CLAMP), BETA)
    b.set_layup(R.pc, R.t, R.theta, surfaces)                                      # never told about a reference surface
    assert b.get_layup_reference()[0] == 0.0 and not np.any(b.get_layup_reference()[1])
    for x, y in zip(_built(a, R), _built(b, R)):
        assert x is None and y is None or np.array_equal(x, y)
    ul = rng.uniform(-1, 1, (m.nel, 32))
    ut = rng.uniform(-1, 1, (m.nel, R.npt, 16)) if surfaces else None
    for wrt in WRT:
        V = rng.uniform(-1, 1, (2, m.nel, nply)) * (R.t if wrt == "ply_thickness" else 10.0)
        for x, y in zip(a.layup_jvp(wrt, V), b.layup_jvp(wrt, V)):
            assert x is None and y is None or np.array_equal(x, y)
        assert np.array_equal(a.layup_vjp(wrt, ul, ut), b.layup_vjp(wrt, ul, ut))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------ 5. chain kernels
@pytest.mark.parametrize("kind,layup,ref", CASES)
def test_chain_kernels_against_the_host_jacobians(kind, layup, ref):
    """J v and J^T u for both arguments against the dense per-cell Jacobians of the host: 1e-13 of |J| |v| and |J|^T |u| with the
    heights about the reference surface; <J v, u> = <v, J^T u> to the same bar; two identical calls return the same bits."""
    m, c, R, rng = _ctx(kind, layup, ref, seed=1)
    nply, surfaces = LAYUPS[layup]
    nel, npt = m.nel, R.npt
    for wrt in WRT:
        V = rng.uniform(-1, 1, (2, nel, nply)) * (R.t if wrt == "ply_thickness" else 10.0)
        dl, dt = c.layup_jvp(wrt, V)
        worst = 0.0
        for k in range(2):
            rl, rt = R.jv(wrt, V[k])
            al, at = R.jv(wrt, V[k], absolute=True)
            worst = max(worst, np.max(np.abs(dl[k] - rl) / np.where(al > 0, al, 1.0)))
            if surfaces:
                worst = max(worst, np.max(np.abs(dt[k] - rt) / np.where(at > 0, at, 1.0)))
            ok = np.all(np.abs(dl[k] - rl) <= 1e-13 * al) and (not surfaces or np.all(np.abs(dt[k] - rt) <= 1e-13 * at))
            if not ok:
                print(f"chain kernels [{kind}, {layup}, {ref}, {wrt}]: J v {worst:.1e}")
            assert ok, (wrt, k)
        again = c.layup_jvp(wrt, V)
        assert np.array_equal(again[0], dl) and (not surfaces or np.array_equal(again[1], dt))
        ul = rng.uniform(-1, 1, (nel, 32))
        ut = rng.uniform(-1, 1, (nel, npt, 16)) if surfaces else None
        worst_T = 0.0
        for lb, tb in ((ul, ut), (ul, None), (None, ut)):
            if lb is None and tb is None:
                continue
            g = c.layup_vjp(wrt, lb, tb)
            want, bound = R.jtu(wrt, lb, tb), R.jtu(wrt, lb, tb, absolute=True)
            worst_T = max(worst_T, np.max(np.abs(g - want) / np.where(bound > 0, bound, 1.0)))
            if not np.all(np.abs(g - want) <= 1e-13 * bound):
                print(f"chain kernels [{kind}, {layup}, {ref}, {wrt}]: J^T u {worst_T:.1e}")
            assert np.all(np.abs(g - want) <= 1e-13 * bound), (wrt, lb is None, tb is None)
            assert np.array_equal(c.layup_vjp(wrt, lb, tb), g)
        g = c.layup_vjp(wrt, ul, ut)
        for k in range(2):
            lhs = np.sum(dl[k] * ul) + (np.sum(dt[k] * ut) if surfaces else 0.0)
            al, at = R.jv(wrt, V[k], absolute=True)
            bound = np.sum(al * np.abs(ul)) + (np.sum(at * np.abs(ut)) if surfaces else 0.0)
            assert abs(lhs - np.sum(V[k] * g)) <= 1e-13 * bound, (wrt, k)
        print(f"chain kernels [{kind}, {layup}, {ref}, {wrt}]: J v {worst:.1e}, J^T u {worst_T:.1e} of the absolute-value sums")
    c.close()


# ------------------------------------------------------------------------------------------ 6. totals
NAMES = ["compliance", "ply_failure", "ply_shear_failure", "max_disp"]
PF = "ply_failure_field"


def _ready(c):
    tight(c)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())            # rho FI of order 5: every point contributes
    c.set_ply_shear_params(5.0 / c.ply_shear_failure_field().max())


def _shear_chain(R, Gs):
    """(d shear table / d ply_angle)^T Gs, (nel, nply): the shear table sees the ply angles alone, never the reference surface."""
    shape = R.theta.shape
    dG = lm.ply_shear_table_dtheta(np.broadcast_to(R.pc[:, 4], shape), np.broadcast_to(R.pc[:, 5], shape), R.theta)
    return np.einsum("epk,epk->ep", Gs.reshape(R.nel, R.nply, 6)[..., :4], dG.reshape(R.nel, R.nply, 4))


@pytest.mark.parametrize("kind,layup,ref", [("3x7", "5 bot/mid/top", "bot"), ("warped", "16 bot/top", "0.3 + c"), ("tri", "1 top", "top"),
                                            ("5x13", "5 bot/mid/top", "0.3 + c")])
def test_totals_against_the_host_contraction_and_forward_against_reverse(kind, layup, ref):
    """d/dx = (d laminate/dx)^T [d/d laminate] + (d table/dx)^T [d/d ply_table] (+ the shear table's own chain for the angles) with
    the host Jacobians about the reference surface and the device's own totals in the brackets: 1e-10 of the largest entry, the bar
    of test_gpu_layup.py.  total_jvp against the reverse totals: 1e-9 of sum |G_i v_i|."""
    m, c, R, rng = _ctx(kind, layup, ref, seed=2, shear=True)
    nply = R.nply
    _ready(c)
    Gl = c.total_gradients(NAMES, "laminate")[0]
    Gt = c.total_gradients(NAMES, "ply_table")[0]
    Gs = c.total_gradients(NAMES, "ply_shear_table")[0]
    cbs = rng.uniform(-1, 1, (2, m.nel * R.npt))
    Fl = c.field_total_gradients(PF, cbs, "laminate")[0]
    Ft = c.field_total_gradients(PF, cbs, "ply_table")[0]
    for wrt in WRT:
        G = c.total_gradients(NAMES, wrt)[0]
        for i, name in enumerate(NAMES):
            want = R.jtu(wrt, Gl[i], Gt[i])
            if wrt == "ply_angle":
                want = want + _shear_chain(R, Gs[i])
            err = np.abs(G[i] - want.ravel()).max() / np.abs(want).max()
            print(f"reverse totals [{kind}, {layup}, {ref}, {name}, {wrt}]: {err:.1e}")
            assert np.abs(want).max() > 0 and err <= 1e-10, (name, wrt)
        F = c.field_total_gradients(PF, cbs, wrt)[0]
        for k in range(2):
            want = R.jtu(wrt, Fl[k], Ft[k]).ravel()
            err = np.abs(F[k] - want).max() / np.abs(want).max()
            print(f"field totals [{kind}, {layup}, {ref}, {wrt}, cotangent {k}]: {err:.1e}")
            assert np.abs(want).max() > 0 and err <= 1e-10, (wrt, k)
        V = rng.uniform(0.5, 1.0, (2, m.nel * nply)) * (np.tile(R.t.ravel(), (2, 1)) if wrt == "ply_thickness" else 1.0)
        dJ = c.total_jvp(wrt, V, NAMES, want_states=False)[1]
        for i, name in enumerate(NAMES):
            for k in range(2):
                gap = abs(dJ[i, k] - G[i] @ V[k]) / np.abs(G[i] * V[k]).sum()
                print(f"total_jvp against total_gradients . v [{kind}, {layup}, {ref}, {name}, {wrt}, direction {k}]: {gap:.1e}")
                assert gap <= 1e-9, (name, wrt, k)
    c.close()


def test_compliance_total_about_the_bottom_against_differences_of_the_oracles_solve():
    """Independent of the chain: the oracle (tests/laminate_ref.py) with the host laminate about the bottom surface, solved at
    t +- s v and t +- 2 s v along two random thickness directions; the bar of test_gpu_ply_shear.py, 1e-6 |fd| + 1e-9 max|G|.
    The oracle's compliance carries about 1e-9 of itself in rounding (the penalty clamp at 1e10 in its sparse LU: a step of iterative
    refinement moves it by 6e-10), and the compliance goes like t^-6: a second-order difference has 56 (0.75 s)^2 / 6 of truncation
    against 1e-9 |J| / (s |fd|) of noise, which leaves 1e-6 at best (measured: 1.3e-6 at s = 1e-4).  The fourth-order central
    difference at s = 4e-3 has 5040 (0.75 s)^4 / 30 = 1.4e-8 of truncation and 1e-7 of noise."""
    from laminate_ref import LaminateOracle
    m, c, R, rng = _ctx("3x7", "5 bot/mid/top", "bot", seed=3)
    tight(c)
    c.solve_state(True)
    G = c.total_gradient("compliance", "ply_thickness")[0]
    o = LaminateOracle(m, penalty_facets=m.penalty_facets(CLAMP), beta=BETA)
    f = R.fields
    o.set_fields(h=np.full(m.nn, 0.05), E=np.full(m.nn, 1e8), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=f["F_solid"], uhat=f["uhat"])

    def J(t):
        o.set_laminate(R.values(t=t)[0])
        return o.compliance(spla.spsolve(o.assemble_K().tocsc(), o.load_vector()))
    assert abs(J(R.t) - c.functional("compliance")) <= 1e-8 * abs(c.functional("compliance"))       # the project's bar for a device solve
    for k in range(2):
        v = R.t * rng.uniform(0.5, 1.0, R.t.shape)
        s = 4e-3
        fd = (8 * (J(R.t + s * v) - J(R.t - s * v)) - (J(R.t + 2 * s * v) - J(R.t - 2 * s * v))) / (12 * s)
        g = float(G @ v.ravel())
        print(f"compliance total about the bottom, direction {k}: {g:.8e} against the oracle's {fd:.8e}")
        assert abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()
    c.close()


# ------------------------------------------------------------------------------------------ 7. handling
def test_refusals_and_the_life_of_the_reference_surface():
    from femo_alpha_amd._lib import FemoHipError
    from femo_alpha_amd.backend import ShellContext
    m = plate_mesh(2.0, 10.0, 3, 7)
    rng = np.random.default_rng(5)
    nply, surfaces = 3, ("bot", "top")
    pc = _plies(nply, rng)
    t, theta = _layup(m.nel, nply, rng)
    S = 5e4 * (1 + 0.3 * rng.uniform(0, 1, (nply, 2)))
    off = H0 * rng.uniform(-1, 1, m.nel)

    def fresh(**kw):
        c = ShellContext(m)
        for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
            c.set_field(k, v)
        c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
        tight(c)
        c.set_layup(pc, t, theta, surfaces, c_drill=3.0, density=np.ones(nply), shear_strength=S, **kw)
        return c
    c = fresh()
    c.set_layup(None)
    for call in (lambda: c.set_layup_reference("bot"), c.get_layup_reference):     # outside the mode
        with pytest.raises(FemoHipError, match=r"no layup is active \(femo_set_layup\)"):
            call()
    c.set_layup(pc, t, theta, surfaces, c_drill=3.0, density=np.ones(nply), shear_strength=S)
    assert c.get_layup_reference()[0] == 0.0                                       # entering the mode: the mid-surface
    c.set_layup_reference(0.3, off)
    c.solve_state(True)

    def snapshot():
        return [c.get_state(), c.get_field("laminate"), c.get_field("ply_table"), *c.get_layup_reference(),
                np.array(list(c.frontal_info().values()))]
    before = snapshot()
    bad = off.copy(); bad[11] = np.inf
    cases = [(lambda: c.set_layup_reference(np.nan), "finite"),
             (lambda: c._chk(c.lib.femo_set_layup_reference(c._h, np.inf, None, 0)), "not finite"),
             (lambda: c.set_layup_reference("bot", bad), "offset of cell 11 is not finite"),
             (lambda: c.set_layup_reference("bot", off[:-1]), f"length {m.nel} .* got {m.nel - 1}"),
             (lambda: c.set_layup_reference("top", np.zeros(2 * m.nel)), f"length {m.nel} .* got {2 * m.nel}")]
    for call, match in cases:
        with pytest.raises((FemoHipError, ValueError), match=match):
            call()
        assert all(np.array_equal(x, y) for x, y in zip(before, snapshot())), match
    with pytest.raises(ValueError, match="reference"):
        c.set_layup_reference("middle")
    with pytest.raises(ValueError, match="cell 11"):
        c.set_layup(pc, t, theta, surfaces, reference="bot", offset=bad)
    assert all(np.array_equal(x, y) for x, y in zip(before, snapshot()))
    # what does not see the surface keeps its bits; the next solve is that of a fresh context built about the new surface
    blind = lambda: [c.functional("layup_mass"), c.functional("layup_volume"), c.get_field("ply_shear_table"), c.get_field("laminate")[27::32]]
    b0 = blind()
    for reference, o in (("top", None), ("bot", off), (-0.2, 0.01), ("mid", None)):
        c.set_layup_reference(reference, o)
        assert all(np.array_equal(x, y) for x, y in zip(b0, blind()))
        c.solve_state(True)
        f = fresh(reference=reference, offset=o)
        assert np.array_equal(f.get_field("laminate"), c.get_field("laminate")) and np.array_equal(f.get_field("ply_table"), c.get_field("ply_table"))
        f.solve_state(True)
        w = f.get_state()
        d = np.abs(c.get_state() - w).max() / np.abs(w).max()
        print(f"state after a change to ({reference}, {'c' if o is not None else None}) against a fresh context: {d:.1e}")
        assert d <= 1e-12
        f.close()
    assert np.abs(c.get_state() - before[0]).max() > 1e-3 * np.abs(before[0]).max()          # the surface matters to the plate
    # the surface belongs to the mode: new thicknesses and a further layup, of another ply count too, keep it; leaving clears it
    c.set_layup_reference("top", off)
    c.set_field("ply_thickness", 1.1 * t)
    c.set_field("ply_angle", theta + 3.0)
    assert c.get_layup_reference()[0] == -0.5 and np.array_equal(c.get_layup_reference()[1], off)
    c.set_layup(pc[:2], t[:, :2], theta[:, :2], ("top",), c_drill=3.0)
    assert c.get_layup_reference()[0] == -0.5 and np.array_equal(c.get_layup_reference()[1], off)
    R = LayupReferenceRef(pc[:2], t[:, :2], theta[:, :2], ("top",), 3.0, "top", off)
    assert np.abs(c.get_field("ply_table").reshape(m.nel, 2, 16)[..., 9] - R.values()[1][..., 9]).max() <= 1e-13 * np.abs(R.interfaces()).max()
    c.set_layup(pc, t, theta, surfaces, c_drill=3.0, reference="mid")              # given anew: no offsets any more
    assert c.get_layup_reference()[0] == 0.0 and not np.any(c.get_layup_reference()[1])
    c.set_layup_reference("bot", 0.02)                                             # one value for every cell
    assert np.array_equal(c.get_layup_reference()[1], np.full(m.nel, 0.02))
    c.set_layup(None)
    c.set_layup(pc, t, theta, surfaces, c_drill=3.0)
    assert c.get_layup_reference()[0] == 0.0 and not np.any(c.get_layup_reference()[1])
    c.set_layup_reference("bot")
    c.set_laminate(None)
    c.set_layup(pc, t, theta, surfaces, c_drill=3.0)
    assert c.get_layup_reference()[0] == 0.0
    # c_drill=None: 12 max(D) about the chosen surface
    c.set_layup(pc, t, theta, surfaces, reference="bot")
    D = lm.clt_from_plies(*[np.broadcast_to(pc[:, k], t.shape) for k in range(6)], t, theta, reference="bot")[2]
    assert np.all(c.get_field("laminate")[31::32] == 12.0 * float(np.max(D)))
    c.close()


# ------------------------------------------------------------------------------------------ 8. the model
@pytest.mark.parametrize("renumber", [False, True])
def test_the_model_takes_the_surface_and_permutes_the_offsets(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel, nply = mesh.nn, mesh.nel, 3
    rng = np.random.default_rng(8)
    pc = _plies(nply, rng)
    pc[:, 6:8] *= 1e-3; pc[:, 8:12] *= 1e-6                      # failure indices of order one under this load
    t, theta = _layup(nel, nply, rng)
    off = H0 * rng.uniform(-1, 1, nel)                            # caller cell order
    recorder = csdl.Recorder(inline=True)
    recorder.start()
    pressure = csdl.Variable(value=np.tile([0.5, 0.0, 5.0], (nn, 1)), name="force_vector")
    thickness = csdl.Variable(value=0.05 * np.ones(nn), name="thickness")
    E = csdl.Variable(value=1e8 * np.ones(nn), name="E")
    nu = csdl.Variable(value=0.3 * np.ones(nn), name="nu")
    density = csdl.Variable(value=np.ones(nn), name="density")
    node_disp = csdl.Variable(value=np.zeros((nn, 3)), name="node_disp")
    ply_t = csdl.Variable(value=t, name="ply_thickness")
    ply_a = csdl.Variable(value=theta, name="ply_angle")
    model = RMShellModel(mesh, shell_bc_func=CLAMP, record=False, renumber=renumber, laminate=True, rho=20,
                         layup=dict(plies=pc, t=t[0], theta=theta[0], surfaces=("bot", "top"), c_drill=3.0, reference="top", offset=off))
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    ctx = model.shell_pde.ctx
    new = model.cell_of_new
    if renumber:
        assert not np.array_equal(new, np.arange(nel))
    r, got = ctx.get_layup_reference()
    assert r == -0.5 and np.array_equal(got, off[new])
    # the model's context holds the plate in solver order: values and thickness derivatives agree to 1e-10
    for name in ("compliance", "ply_failure"):
        val = float(np.ravel(getattr(out, name).value)[0])
        assert abs(val - ctx.functional(name)) <= 1e-10 * abs(ctx.functional(name)), name
        got = np.asarray(recorder.compute_totals(getattr(out, name), ply_t)).reshape(nel, nply)
        want = np.empty((nel, nply))
        want[new] = ctx.total_gradient(name, "ply_thickness")[0].reshape(nel, nply)        # solver order -> caller order
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"model against its context [{name}, renumber={renumber}]: {err:.1e}")
        assert err <= 1e-10, name
    # ... and that plate is the caller's: the laminate the context built is the host's for the caller's cells, taken in solver order
    R = LayupReferenceRef(pc, t, theta, ("bot", "top"), 3.0, "top", off)
    lam, tab = R.values()
    built = ctx.get_field("laminate").reshape(nel, 32)
    Z = np.abs(R.interfaces()).max()
    assert np.abs(built[:, 9:18] - lam[new, 9:18]).max() <= 1e-13 * Z * np.abs(lam[:, 0:9]).max()
    assert np.abs(ctx.get_field("ply_table").reshape(nel, -1, 16)[..., 9] - tab[new][..., 9]).max() <= 1e-13 * Z
    if renumber:                                                                   # the offsets in caller order would be another plate
        wrong = LayupReferenceRef(pc, t[new], theta[new], ("bot", "top"), 3.0, "top", off).values()[0]
        assert np.abs(built[:, 9:18] - wrong[:, 9:18]).max() > 1e-3 * Z * np.abs(lam[:, 0:9]).max()
