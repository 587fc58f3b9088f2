"""Layups on the GPU (femo_set_layup, "ply_thickness" / "ply_angle"): the laminate and the ply table built on the device against the
host step of femo_alpha_amd/laminate.py, the chain kernels against tests/layup_ref.py, the totals against the host contraction of the
totals with respect to "laminate" and "ply_table", forward mode against reverse mode, and the handling of the mode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm                                        # noqa: E402
from femo_alpha_amd.mesh import plate_mesh                                       # noqa: E402
from layup_ref import LayupRef                                                   # noqa: E402
from test_gpu_laminate import BETA, CLAMP, ROOT_EDGE, _mesh, tight               # noqa: E402
from test_layup_cpu import _plies                                                # noqa: E402

pytestmark = pytest.mark.gpu

MESHES = {"3x7": lambda: plate_mesh(2.0, 10.0, 3, 7), "4x20": lambda: plate_mesh(2.0, 10.0, 4, 20),
          "5x13": lambda: plate_mesh(2.0, 10.0, 5, 13), "warped": lambda: _mesh("warped"), "tri": lambda: _mesh("tri")}
LAYUPS = {"1 top": (1, ("top",)), "2 bot/top": (2, ("bot", "top")), "5 bot/mid/top": (5, ("bot", "mid", "top")),
          "16 bot/top": (16, ("bot", "top")), "32 none": (32, ())}
EXACT = [0.0, 90.0, 45.0, -45.0, 180.0, -270.0]
WRT = ("ply_thickness", "ply_angle")


def _layup(nel, nply, rng, uniform=False, h=0.05):
    """Thickness +-30 % per cell and random angles, the exact angles in the first cells; ``uniform``: one layup for every cell."""
    t = h / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    theta = rng.uniform(-180, 180, (nel, nply))
    for e in range(min(nel, 3)):
        theta[e] = np.resize(np.roll(EXACT, e), nply)
    if uniform:
        t, theta = np.tile(t[0], (nel, 1)), np.tile(theta[0], (nel, 1))
    return t, theta


def _ctx(kind, layup, seed=0, uniform=False, uhat=True):
    from femo_alpha_amd.backend import ShellContext
    m = MESHES[kind]()
    nply, surfaces = LAYUPS[layup]
    rng = np.random.default_rng(seed)
    pc = _plies(nply, rng)
    t, theta = _layup(m.nel, nply, rng, uniform)
    c = ShellContext(m)
    fields = dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=rng.uniform(-1, 1, (m.nn, 3)))
    if uhat:
        fields["uhat"] = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(ROOT_EDGE if kind in ("warped", "tri") else CLAMP), BETA)
    c.set_layup(pc, t, theta, surfaces)
    D = lm.clt_from_plies(*[np.broadcast_to(pc[:, k], t.shape) for k in range(6)], t, theta)[2]
    R = LayupRef(pc, t, theta, surfaces, c_drill=12.0 * float(np.max(D)))
    return m, c, R, rng


# ------------------------------------------------------------------------------------------ 1. build parity
def _build_distance(R, lam, tab):
    """Largest distance of the device's laminate and table from the host's, in units of the block scales: A: max|A| of the cell,
    B: H max|A|, D: H^2 max|A|, A_s: max|A_s|, G: max|G| of the point, z: H."""
    lr, tr = R.values()
    H = R.t.sum(axis=1)
    a = np.abs(lr[:, 0:9]).max(axis=1)
    d = {"A": np.abs(lam[:, 0:9] - lr[:, 0:9]).max(axis=1) / a,
         "B": np.abs(lam[:, 9:18] - lr[:, 9:18]).max(axis=1) / (H * a),
         "D": np.abs(lam[:, 18:27] - lr[:, 18:27]).max(axis=1) / (H * H * a),
         "A_s": np.abs(lam[:, 27:31] - lr[:, 27:31]).max(axis=1) / np.abs(lr[:, 27:31]).max(axis=1)}
    assert np.array_equal(lam[:, 31], lr[:, 31])                                  # c_drill: 12 max(D) of the initial layup, a constant
    if tr is not None:
        d["G"] = np.abs(tab[..., 0:9] - tr[..., 0:9]).max(axis=2) / np.abs(tr[..., 0:9]).max(axis=2)
        d["z"] = np.abs(tab[..., 9] - tr[..., 9]) / H[:, None]
        assert np.array_equal(tab[..., 10:16], tr[..., 10:16])                    # the strength coefficients: the same bits
    return {k: float(np.max(v)) for k, v in d.items()}


BUILD_CASES = [(k, l, False) for k in MESHES for l in LAYUPS] + [(k, l, True) for k in ("5x13", "tri") for l in LAYUPS]
CHAIN_CASES = [(k, l, False) for k in ("3x7", "4x20", "5x13", "tri") for l in LAYUPS] + [("5x13", l, True) for l in LAYUPS]


@pytest.mark.parametrize("kind,layup,uniform", BUILD_CASES)
def test_build_parity(kind, layup, uniform):
    """1e-13 of the block's scale: a sum of <= 32 products of <= 7 factors rounded to <= 2 ulp is <= 5e-15 of the sum of the absolute
    terms on each side.  Largest distances observed over all cases on an MI355X, in units of the scales: A 9.3e-16, B 3.0e-16,
    D 7.9e-17, A_s 7.6e-16, G 5.3e-16, z 1.5e-16 (the chain kernels: J v 1.8e-15, J^T u 2.2e-15 of the absolute-value sums)."""
    m, c, R, rng = _ctx(kind, layup, uniform=uniform)
    nply, surfaces = LAYUPS[layup]
    lam = c.get_field("laminate").reshape(m.nel, 32)
    assert np.array_equal(lam[:, 0:9].reshape(-1, 3, 3), lam[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1))      # symmetric by construction
    assert c.field_size("ply_thickness") == c.field_size("ply_angle") == m.nel * nply
    assert np.array_equal(c.get_field("ply_thickness").reshape(m.nel, nply), R.t)
    assert np.array_equal(c.get_field("ply_angle").reshape(m.nel, nply), R.theta)
    if surfaces:
        tab = c.get_field("ply_table").reshape(m.nel, R.npt, 16)
    else:
        tab = None
        assert c.lib.femo_field_size(c._h, b"ply_table") == -1
    d = _build_distance(R, lam, tab)
    print(f"build parity [{kind}, {layup}, uniform={uniform}]: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
    for k, v in d.items():
        assert v <= 1e-13, k
    # new values through the fields rebuild both
    t2 = R.t * (1 + 0.1 * rng.uniform(-1, 1, R.t.shape))
    th2 = R.theta + rng.uniform(-5, 5, R.theta.shape)
    c.set_field("ply_thickness", t2)
    c.set_field("ply_angle", th2)
    R2 = LayupRef(R.pc, t2, th2, surfaces, R.c_drill)
    lam2 = c.get_field("laminate").reshape(m.nel, 32)
    tab2 = c.get_field("ply_table").reshape(m.nel, R.npt, 16) if surfaces else None
    for k, v in _build_distance(R2, lam2, tab2).items():
        assert v <= 1e-13, k
    c.close()


@pytest.mark.parametrize("kind,layup", [("4x20", "2 bot/top"), ("warped", "5 bot/mid/top"), ("tri", "32 none")])
def test_state_in_layup_mode_equals_the_state_of_the_read_back_laminate(kind, layup):
    m, c, R, rng = _ctx(kind, layup)
    c.use_direct_solver()
    c.solve_state(True)
    w = c.get_state()
    assert np.abs(w).max() > 0
    lam = c.get_field("laminate")
    c.set_layup(None)
    assert np.array_equal(c.get_field("laminate"), lam)                            # what was built stays as ordinary values
    c.set_laminate(lam)
    c.solve_state(True)
    assert np.abs(c.get_state() - w).max() <= 1e-12 * np.abs(w).max()
    c.close()


# ------------------------------------------------------------------------------------------ 2. chain kernels
@pytest.mark.parametrize("kind,layup,uniform", CHAIN_CASES)
def test_chain_kernels_against_the_host_jacobians(kind, layup, uniform):
    m, c, R, rng = _ctx(kind, layup, seed=1, uniform=uniform)
    nply, surfaces = LAYUPS[layup]
    nel, npt = m.nel, R.npt
    for wrt in WRT:
        V = rng.uniform(-1, 1, (3, nel, nply)) * (R.t if wrt == "ply_thickness" else 10.0)
        dl, dt = c.layup_jvp(wrt, V)
        assert dl.shape == (3, nel, 32) and ((dt is None) if not surfaces else dt.shape == (3, nel, npt, 16))
        worst = 0.0
        for k in range(3):
            rl, rt = R.jv(wrt, V[k])
            al, at = R.jv(wrt, V[k], absolute=True)
            assert np.all(np.abs(dl[k] - rl) <= 1e-12 * al), (wrt, k)
            worst = max(worst, np.max(np.abs(dl[k] - rl) / np.where(al > 0, al, 1.0)))
            if surfaces:
                assert np.all(np.abs(dt[k] - rt) <= 1e-12 * at), (wrt, k)
                worst = max(worst, np.max(np.abs(dt[k] - rt) / np.where(at > 0, at, 1.0)))
            one = c.layup_jvp(wrt, V[k])
            assert np.array_equal(one[0], dl[k]) and (not surfaces or np.array_equal(one[1], dt[k]))       # ndir > 1: the same bits
        again = c.layup_jvp(wrt, V)
        assert np.array_equal(again[0], dl) and (not surfaces or np.array_equal(again[1], dt))
        # either output absent
        assert c.layup_jvp(wrt, V, table=False)[1] is None and np.array_equal(c.layup_jvp(wrt, V, table=False)[0], dl)
        if surfaces:
            only = c.layup_jvp(wrt, V, laminate=False)
            assert only[0] is None and np.array_equal(only[1], dt)
        ul = rng.uniform(-1, 1, (nel, 32))
        ut = rng.uniform(-1, 1, (nel, npt, 16)) if surfaces else None
        worst_T = 0.0
        for lb, tb in ((ul, ut), (ul, None), (None, ut)):
            if lb is None and tb is None:
                continue
            g = c.layup_vjp(wrt, lb, tb)
            ref, bound = R.jtu(wrt, lb, tb), R.jtu(wrt, lb, tb, absolute=True)
            assert g.shape == (nel, nply)
            assert np.all(np.abs(g - ref) <= 1e-12 * bound), (wrt, lb is None, tb is None)
            worst_T = max(worst_T, np.max(np.abs(g - ref) / np.where(bound > 0, bound, 1.0)))
            assert np.array_equal(c.layup_vjp(wrt, lb, tb), g)                      # two calls: the same bits
        g = c.layup_vjp(wrt, ul, ut)
        for k in range(3):
            lhs = np.sum(dl[k] * ul) + (np.sum(dt[k] * ut) if surfaces else 0.0)
            al, at = R.jv(wrt, V[k], absolute=True)
            bound = np.sum(al * np.abs(ul)) + (np.sum(at * np.abs(ut)) if surfaces else 0.0)
            assert abs(lhs - np.sum(V[k] * g)) <= 1e-12 * bound, (wrt, k)
        print(f"chain kernels [{kind}, {layup}, uniform={uniform}, {wrt}]: J v {worst:.1e}, J^T u {worst_T:.1e} of the absolute-value sums")
    c.close()


# ------------------------------------------------------------------------------------------ 3. reverse totals
NAMES = ["compliance", "elastic_energy", "ply_failure"]


def _solved(c):
    c.solve_state(True)
    return c


@pytest.mark.parametrize("kind,layup", [("4x20", "2 bot/top"), ("warped", "5 bot/mid/top"), ("tri", "16 bot/top"), ("5x13", "1 top")])
def test_reverse_totals_against_the_host_contraction(kind, layup):
    """The composition of tests/test_gpu_ply_failure.py (the chain rule by hand on the host) with the same adjoints; 1e-10 max|g|."""
    m, c, R, rng = _ctx(kind, layup, seed=2)
    tight(c)
    _solved(c)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())            # rho FI of order 5: every point contributes
    tags = (np.arange(m.nel) % 3).astype(np.int32)
    c.set_cell_tags(tags, 3)
    for subs in ([-1, -1, -1], [1, 1, 1]):
        Gl = c.total_gradients(NAMES, "laminate", subdomains=subs)[0]
        Gt = c.total_gradients(NAMES, "ply_table", subdomains=subs)[0]
        for wrt in WRT:
            G = c.total_gradients(NAMES, wrt, subdomains=subs)[0]
            for i, name in enumerate(NAMES):
                ref = R.jtu(wrt, Gl[i], Gt[i]).ravel()
                err = np.abs(G[i] - ref).max() / np.abs(ref).max()
                print(f"reverse totals [{kind}, {layup}, {name}, {wrt}, sub {subs[i]}]: {err:.1e}")
                assert err <= 1e-10, (name, wrt, subs[i])
            c.select_subdomain(subs[2])
            one = c.total_gradient("ply_failure", wrt)[0]
            c.select_subdomain(-1)
            assert np.abs(one - G[2]).max() <= 1e-10 * np.abs(G[2]).max()
    c.close()


def test_layup_without_recovery_points_totals():
    m, c, R, rng = _ctx("5x13", "32 none", seed=2)
    from femo_alpha_amd._lib import FemoHipError
    tight(c)
    _solved(c)
    names = NAMES[:2]
    Gl = c.total_gradients(names, "laminate")[0]
    for wrt in WRT:
        G = c.total_gradients(names, wrt)[0]
        for i in range(2):
            ref = R.jtu(wrt, Gl[i], None).ravel()
            assert np.abs(G[i] - ref).max() <= 1e-10 * np.abs(ref).max(), (names[i], wrt)
        with pytest.raises(FemoHipError, match="femo_set_ply_table"):
            c.total_gradients(NAMES, wrt)
    with pytest.raises(FemoHipError, match="femo_set_ply_table"):
        c.functional("ply_failure")
    c.close()


def test_angle_totals_against_central_differences_with_re_solves():
    """tests/test_gpu_ply_failure.py's bar: 1e-6 relative + 1e-9 of the largest entry."""
    m, c, R, rng = _ctx("warped", "2 bot/top", seed=3)
    tight(c)
    _solved(c)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    _solved(c)
    names = ["ply_failure", "elastic_energy"]
    G = c.total_gradients(names, "ply_angle")[0].reshape(2, m.nel, 2)
    Gt = c.total_gradients(names, "ply_thickness")[0].reshape(2, m.nel, 2)
    bar = lambda g, fd, G: abs(g - fd) <= 1e-6 * abs(fd) + 1e-9 * np.abs(G).max()
    # cells with random angles: at the exact angles 0 / 90 / 180 of the first cells the energy is nearly stationary in the angle
    # (dU/dtheta ~ 3e-12 against 1e-7 elsewhere), and a central difference of it measures its own truncation
    for e, j in [(5, 0), (3, 1), (8, 0), (11, 1), (17, 0)]:
        s = 1e-2                                                                  # degrees: (1.7e-4 rad)^2 4^2 / 6 ~ 8e-8 of truncation
        vals = []
        for sg in (1, -1):
            th = R.theta.copy(); th[e, j] += sg * s
            c.set_field("ply_angle", th)
            _solved(c)
            vals.append([c.functional(n) for n in names])
        c.set_field("ply_angle", R.theta)
        for i, n in enumerate(names):
            fd = (vals[0][i] - vals[1][i]) / (2 * s)
            print(f"angle totals [{n}, cell {e}, ply {j}]: {G[i, e, j]:.8e} against {fd:.8e}")
            assert bar(G[i, e, j], fd, G[i]), (n, e, j)
    for e, j in [(1, 0), (9, 1)]:
        s = 1e-4 * R.t[e, j]
        vals = []
        for sg in (1, -1):
            tt = R.t.copy(); tt[e, j] += sg * s
            c.set_field("ply_thickness", tt)
            _solved(c)
            vals.append([c.functional(n) for n in names])
        c.set_field("ply_thickness", R.t)
        for i, n in enumerate(names):
            assert bar(Gt[i, e, j], (vals[0][i] - vals[1][i]) / (2 * s), Gt[i]), (n, e, j)
    c.close()


# ------------------------------------------------------------------------------------------ 4. forward mode
@pytest.mark.parametrize("kind,layup", [("4x20", "2 bot/top"), ("warped", "5 bot/mid/top"), ("tri", "32 none")])
def test_forward_mode_against_the_laminate_product_and_the_reverse_totals(kind, layup):
    """The forward-versus-reverse bars of tests/test_gpu_residual_jvp.py: 1e-11 of the product's size for (dR/dx) v, 1e-8 relative for
    the totals along one-signed directions."""
    m, c, R, rng = _ctx(kind, layup, seed=4)
    nply, surfaces = LAYUPS[layup]
    c.use_direct_solver(rtol=1e-12)
    _solved(c)
    fns = NAMES if surfaces else NAMES[:2]
    if surfaces:
        c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    for wrt in WRT:
        V = rng.uniform(0.5, 1.0, (2, m.nel * nply)) * (np.tile(R.t.ravel(), (2, 1)) if wrt == "ply_thickness" else 1.0)
        got = c.dRdarg(wrt, V)
        for k in range(2):
            ref = c.dRdarg("laminate", R.jv(wrt, V[k])[0].ravel())
            assert np.abs(ref).max() > 0
            assert np.abs(got[k] - ref).max() <= 1e-11 * np.abs(ref).max(), (wrt, k)
            assert np.array_equal(c.dRdarg("laminate", c.layup_jvp(wrt, V[k])[0].ravel()), got[k])        # the device's own J v: the same bits
        lam = rng.uniform(-1, 1, m.ndof)
        gap = abs(lam @ got[0] - c.dRdarg_T(wrt, lam) @ V[0])
        assert gap <= 1e-11 * np.linalg.norm(lam) * np.linalg.norm(got[0]), wrt
        dW, dJ, _, _ = c.total_jvp(wrt, V, fns)
        G = c.total_gradients(list(fns), wrt)[0]
        want = G @ V.T
        for i, fn in enumerate(fns):
            for k in range(2):
                d = abs(dJ[i, k] - want[i, k]) / abs(want[i, k])
                print(f"total_jvp against total_gradients . v [{kind}, {layup}, {fn}, {wrt}, direction {k}]: {d:.1e}")
                assert d <= 1e-8, (fn, wrt, k)
    c.close()


# ------------------------------------------------------------------------------------------ 5. handling
def test_refusals_limits_and_the_life_of_the_mode():
    from femo_alpha_amd._lib import FemoHipError, dptr
    from femo_alpha_amd.backend import ShellContext
    m = plate_mesh(2.0, 10.0, 4, 20)
    rng = np.random.default_rng(5)
    nply, surfaces = 3, ("bot", "top")
    pc = _plies(nply, rng)
    t, theta = _layup(m.nel, nply, rng)
    c = ShellContext(m)
    for k, v in dict(thickness=[0.05], E=[1e8], nu=[0.3], density=[1.0], F_solid=np.tile([0.1, 0.0, 5.0], (m.nn, 1))).items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(CLAMP), BETA)
    c.use_direct_solver()
    # outside the mode the two names are unknown
    for name in WRT:
        assert c.lib.femo_field_size(c._h, name.encode()) == -1
        with pytest.raises(FemoHipError, match="unknown"):
            c.set_field(name, t)
    with pytest.raises(FemoHipError, match="no layup is active"):
        c._chk(c.lib.femo_layup_vjp(c._h, b"ply_thickness", None, None, None, 0))
    # a transient operator refuses the mode, as it refuses femo_set_laminate
    c.set_operator(1.0, 1.0)
    with pytest.raises(FemoHipError, match="inertia"):
        c.set_layup(pc, t, theta, surfaces)
    c.set_operator(1.0, 0.0)
    assert c.lib.femo_field_size(c._h, b"laminate") == -1
    c.set_layup(pc, t, theta, surfaces)                                            # enters laminate mode
    assert c.field_size("laminate") == 32 * m.nel and c.field_size("ply_table") == 16 * 6 * m.nel
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())

    def snapshot():
        return [c.get_state(), c.get_field("laminate"), c.get_field("ply_table"), c.get_field("ply_thickness"), c.get_field("ply_angle"),
                c.functional("ply_failure")]
    before = snapshot()

    def unchanged():
        after = snapshot()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    bad_t = t.copy(); bad_t[7, 1] = 0.0
    bad_a = theta.copy(); bad_a[3, 0] = np.nan
    bad_E = pc.copy(); bad_E[1, 1] = -1.0
    bad_nu = pc.copy(); bad_nu[2, 3] = 10.0                                        # 1 - nu12^2 E2 / E1 <= 0
    bad_F = pc.copy(); bad_F[0, 8] = np.inf
    cases = [
        (lambda: c.set_layup(_plies(11), *_layup(m.nel, 11, rng), ("bot", "mid", "top")), "33 recovery points"),
        (lambda: c.set_layup(_plies(33), *_layup(m.nel, 33, rng), ()), r"nply must be 1\.\.32"),
        (lambda: c.set_layup(pc, bad_t, theta, surfaces), "thickness of ply 1 of cell 7"),
        (lambda: c.set_layup(pc, t, bad_a, surfaces), "angle of ply 0 of cell 3"),
        (lambda: c.set_field("ply_thickness", bad_t), "thickness of ply 1 of cell 7"),
        (lambda: c.set_field("ply_thickness", -t), "thickness of ply 0 of cell 0"),
        (lambda: c.set_field("ply_angle", bad_a), "angle of ply 0 of cell 3"),
        (lambda: c.set_field("ply_angle", theta.ravel()[:-1]), "nel x nply"),
        (lambda: c.set_layup(bad_E, t, theta, surfaces), "moduli .* of ply 1"),
        (lambda: c.set_layup(bad_nu, t, theta, surfaces), "ply 2 has 1 - nu12"),
        (lambda: c.set_layup(bad_F, t, theta, surfaces), "constant 8 of ply 0 is not finite"),
        (lambda: c.set_layup(pc, t, theta, surfaces, c_drill=0.0), "c_drill"),
        (lambda: c.set_layup(pc, t, theta, surfaces, c_drill=-3.0), "c_drill"),
        # the laminate and the table belong to the layup
        (lambda: c.set_laminate(before[1]), "femo_set_layup"),
        (lambda: c.set_field("laminate", before[1]), "femo_set_layup"),
        (lambda: c.set_field("ply_table", before[2]), "femo_set_layup"),
        (lambda: c.set_ply_table(before[2].reshape(m.nel, 6, 16)), "femo_set_layup"),
        (lambda: c.set_ply_table(None), "femo_set_layup"),
    ]
    for i, (call, match) in enumerate(cases):
        with pytest.raises(FemoHipError, match=match):
            call()
            print(f"case {i} ({match}) was not refused")
        unchanged()
    with pytest.raises(ValueError, match="surfaces"):
        c.set_layup(pc, t, theta, ("top", "bot"))
    # the field entry points do not provide the two arguments (zeros would be wrong for the ply failure field)
    cbar = rng.uniform(-1, 1, m.nvc * m.nel)
    V = rng.uniform(-1, 1, m.nel * nply)
    for wrt in WRT:
        for call in (lambda: c.field_output_vjp("stress", wrt, cbar), lambda: c.field_output_jvp("stress", wrt, V),
                     lambda: c.field_output_jvp("ply_failure_field", wrt, V), lambda: c.field_output_jacobian("stress", wrt),
                     lambda: c.field_total_gradients("stress", cbar, wrt), lambda: c.field_total_jvp(["ply_failure_field"], wrt, V),
                     lambda: c.field_gradient_vec("compliance", wrt, "adjoint"),
                     lambda: c._chk(c.lib.femo_dist_gradient(c._h, b"compliance", wrt.encode(), 1, None, 0))):
            with pytest.raises(FemoHipError, match="not provided"):
                call()
        unchanged()
    # leaving keeps the values as ordinary ones; re-entering works; femo_set_laminate(NULL, 0) drops everything
    c.set_layup(None)
    assert c.lib.femo_field_size(c._h, b"ply_thickness") == -1 and c.lib.femo_field_size(c._h, b"ply_angle") == -1
    assert np.array_equal(c.get_field("laminate"), before[1]) and np.array_equal(c.get_field("ply_table"), before[2])
    buf = np.empty(m.nel * nply)
    with pytest.raises(FemoHipError, match="unknown argument"):
        c._chk(c.lib.femo_dfunctional(c._h, b"compliance", b"ply_thickness", dptr(buf), buf.size))
    c.set_field("laminate", before[1])                                             # ordinary fields again
    c.set_field("ply_table", before[2])
    c.solve_state(True)
    assert np.abs(c.get_state() - before[0]).max() <= 1e-12 * np.abs(before[0]).max()
    c.set_layup(pc, t, theta, surfaces)
    c.solve_state(True)
    assert np.array_equal(c.get_field("laminate"), before[1]) and c.functional("ply_failure") == pytest.approx(before[5], rel=1e-12)
    c.set_layup(pc[:2], t[:, :2], theta[:, :2], ())                                # another layup: no table any more
    assert c.field_size("ply_angle") == 2 * m.nel and c.lib.femo_field_size(c._h, b"ply_table") == -1
    c.set_laminate(None)
    for name in WRT + ("laminate", "ply_table"):
        assert c.lib.femo_field_size(c._h, name.encode()) == -1
    c.solve_state(True)                                                            # the single-layer law again
    assert np.isfinite(c.functional("compliance"))
    c.close()


# ------------------------------------------------------------------------------------------ 6. the model
@pytest.mark.parametrize("renumber", [False, True])
def test_reverse_and_forward_mode_through_the_model_match_the_backend_totals(renumber):
    from femo_alpha_amd import csdl
    from femo_alpha_amd.csdl_alpha_opt.output_operation import OutputOperation
    from femo_alpha_amd.csdl_alpha_opt.state_operation import StateOperation
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    mesh = plate_mesh(2.0, 10.0, 4, 20)
    nn, nel, nply = mesh.nn, mesh.nel, 3
    rng = np.random.default_rng(8)
    pc = _plies(nply, rng)
    pc[:, 6:8] *= 1e-3; pc[:, 8:12] *= 1e-6                      # failure indices of order one under this load
    t, theta = _layup(nel, nply, rng)
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
                         layup=dict(plies=pc, t=t[0], theta=theta[0], surfaces=("bot", "top")))
    out = model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a)
    recorder.stop()
    fea, ctx = model.fea, model.shell_pde.ctx
    assert np.array_equal(ctx.get_field("ply_thickness").reshape(nel, nply), t[model.cell_of_new])
    assert np.array_equal(ctx.get_field("ply_angle").reshape(nel, nply), theta[model.cell_of_new])
    for var, arg in ((ply_t, "ply_thickness"), (ply_a, "ply_angle")):
        for name in ("ply_failure", "elastic_energy", "compliance"):
            got = np.asarray(recorder.compute_totals(getattr(out, name), var)).reshape(nel, nply)
            ref = np.empty((nel, nply))
            ref[model.cell_of_new] = ctx.total_gradient(name, arg)[0].reshape(nel, nply)        # solver order -> caller order
            assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (name, arg)
    # forward mode through the operations: (dR/dx) v is added into the residual tangents, the tangent state and the outputs' tangents
    ctx.use_direct_solver(rtol=1e-12)
    args = fea.states_dict["disp_solid"]["arguments"]
    assert "ply_thickness" in args and "ply_angle" in args and "laminate" not in fea.inputs_dict and "ply_table" not in fea.inputs_dict
    op = StateOperation(fea=fea, args_name_list=args, state_name="disp_solid")
    inputs = {name: fea.inputs_dict[name]["function"].x.array.copy() for name in args}
    outputs = {}
    fea.opt_iter = 0
    op.solve_residual_equations(inputs, outputs)
    for arg in WRT:
        v = rng.uniform(0.5, 1.0, inputs[arg].size) * (inputs[arg] if arg == "ply_thickness" else 1.0)
        seed = rng.uniform(-1, 1, mesh.ndof)
        d_res = {"disp_solid": seed.copy()}
        op.compute_jacvec_product(inputs, outputs, {arg: v}, {}, d_res, "fwd")
        Jv = ctx.dRdarg(arg, v)
        assert np.abs(Jv).max() > 0 and np.array_equal(d_res["disp_solid"], seed + Jv)
        d_out = {}
        op.apply_inverse_jacobian(inputs, outputs, d_out, {"disp_solid": Jv}, "fwd")
        dW, dJ, _, _ = ctx.total_jvp(arg, v, ("ply_failure", "elastic_energy"))
        assert np.abs(-d_out["disp_solid"] - dW).max() <= 1e-8 * np.abs(dW).max(), arg
        for i, name in enumerate(("ply_failure", "elastic_energy")):
            oo = OutputOperation(fea=fea, args_name_list=fea.outputs_dict[name]["arguments"], output_name=name)
            vals = {a: (outputs["disp_solid"] if a == "disp_solid" else fea.inputs_dict[a]["function"].x.array.copy())
                    for a in fea.outputs_dict[name]["arguments"]}
            der = {}
            oo.compute_derivatives(vals, {}, der)
            tangent = float(np.ravel(der[name, "disp_solid"]) @ dW + np.ravel(der[name, arg]) @ v)
            assert abs(tangent - dJ[i]) <= 1e-8 * abs(dJ[i]), (name, arg)
    with pytest.raises(ValueError):
        model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t, ply_angle=ply_a, laminate=ply_t)
    with pytest.raises(ValueError):
        model.evaluate(pressure, thickness, E, nu, density, node_disp, ply_thickness=ply_t)
    with pytest.raises(ValueError):
        RMShellModel(mesh, shell_bc_func=CLAMP, record=False, layup=dict(plies=pc, t=t[0], theta=theta[0]))
