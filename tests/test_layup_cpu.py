"""CPU-side checks of the layup inputs: the host angle Jacobians of femo_alpha_amd/laminate.py against central differences, the
composition of the thickness and angle Jacobians in tests/layup_ref.py, and the presence of the API.  No compute call is made
without a GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd import laminate as lm          # noqa: E402
from layup_ref import LayupRef                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["femo_set_layup", "femo_layup_jvp", "femo_layup_vjp"]
PLY = dict(E1=1.35e8, E2=1.0e7, G12=5e6, nu12=0.3, G13=5e6, G23=3.5e6)
STRENGTH = dict(Xt=1.5e6, Xc=1.2e6, Yt=5e4, Yc=2e5, S=7e4)


def _plies(nply, rng=None):
    pc = np.tile([PLY[k] for k in ("E1", "E2", "G12", "nu12", "G13", "G23")] + list(lm.tsai_wu(**STRENGTH)), (nply, 1))
    if rng is not None:                                  # a different material in every ply
        pc[:, [0, 1, 2, 4, 5]] *= 1 + 0.3 * rng.uniform(-1, 1, (nply, 5))
    return pc


def _layup(nel, nply, rng):
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (nel, nply)))
    theta = rng.uniform(-180, 180, (nel, nply))
    theta[0, :] = np.resize([0.0, 90.0, 45.0, -45.0, 180.0, -270.0], nply)
    return t, theta


@pytest.mark.parametrize("nply", [1, 2, 5])
def test_angle_jacobians_against_central_differences(nply):
    """Step 1e-3 degree; 1e-7 of the largest entry of the block: the entries are degree-4 trigonometric polynomials, so truncation is
    <= (1.7e-5)^2 4^3 / 6 ~ 3e-9 and rounding ~ 6e-12 of it."""
    rng = np.random.default_rng(nply)
    nel = 7
    pc = _plies(nply, rng)
    t, theta = _layup(nel, nply, rng)
    mat = [np.broadcast_to(pc[:, k], (nel, nply)) for k in range(6)]
    d = lm.clt_dtheta(*mat, t, theta)
    dG = lm.ply_table_dtheta(*mat[:4], theta)
    s = 1e-3
    for k in range(nply):
        e = np.zeros(nply); e[k] = s
        p = lm.clt_from_plies(*mat, t, theta + e)
        m = lm.clt_from_plies(*mat, t, theta - e)
        for name, blk, fp, fm in zip("A B D A_s".split(), d, p, m):
            fd = (fp - fm) / (2 * s)
            err = np.abs(blk[:, k] - fd).max()
            assert err <= 1e-7 * np.abs(blk).max(), (name, k, err, np.abs(blk).max())
        tp = lm.ply_table(*mat[:4], t, theta + e, pc[:, 6:12], ("bot", "mid", "top"))
        tm = lm.ply_table(*mat[:4], t, theta - e, pc[:, 6:12], ("bot", "mid", "top"))
        fd = ((tp - tm) / (2 * s)).reshape(nel, nply, 3, 16)
        assert not np.any(fd[..., 9:])                               # z and the strengths do not move
        assert not np.any(np.delete(fd, k, axis=1))                  # other plies do not move
        for sfc in range(3):
            g = fd[:, k, sfc, :9].reshape(nel, 3, 3)
            assert np.abs(dG[:, k] - g).max() <= 1e-7 * np.abs(tp[..., :9]).max(), k
    dQ, dQs = lm.ply_stiffness_dtheta(*[pc[0, k] for k in range(6)], 30.0)
    Qp = lm.ply_stiffness(*[pc[0, k] for k in range(6)], 30.0 + s)
    Qm = lm.ply_stiffness(*[pc[0, k] for k in range(6)], 30.0 - s)
    assert np.abs(dQ - (Qp[0] - Qm[0]) / (2 * s)).max() <= 1e-7 * np.abs(Qp[0]).max()
    assert np.abs(dQs - (Qp[1] - Qm[1]) / (2 * s)).max() <= 1e-7 * np.abs(Qp[1]).max()


@pytest.mark.parametrize("surfaces", [("bot", "top"), ("bot", "mid", "top"), ("top",), ()])
@pytest.mark.parametrize("wrt", ["ply_thickness", "ply_angle"])
def test_reference_chain_composes(wrt, surfaces):
    """J v of tests/layup_ref.py against central differences of its values, and <J v, u> = <v, J^T u>; the absolute-value products
    bound the plain ones."""
    rng = np.random.default_rng(3)
    nel, nply = 5, 3
    t, theta = _layup(nel, nply, rng)
    R = LayupRef(_plies(nply, rng), t, theta, surfaces, c_drill=7.0)
    lam, tab = R.values()
    assert lam.shape == (nel, 32) and np.all(lam[:, 31] == 7.0)
    assert (tab is None) == (not surfaces) and (tab is None or tab.shape == (nel, nply * len(surfaces), 16))
    v = rng.uniform(-1, 1, (nel, nply)) * (t if wrt == "ply_thickness" else 1.0)
    dl, dt = R.jv(wrt, v)
    s = 1e-4 if wrt == "ply_thickness" else 1e-3
    vp = R.values(t + s * v, theta) if wrt == "ply_thickness" else R.values(t, theta + s * v)
    vm = R.values(t - s * v, theta) if wrt == "ply_thickness" else R.values(t, theta - s * v)
    fd = (vp[0] - vm[0]) / (2 * s)
    for a, b in ((0, 9), (9, 18), (18, 27), (27, 31)):
        assert np.abs(dl[:, a:b] - fd[:, a:b]).max() <= 1e-6 * np.abs(fd[:, a:b]).max(), (a, b)
    assert not np.any(dl[:, 31])
    if surfaces:
        fdt = (vp[1] - vm[1]) / (2 * s)
        for k in range(16):
            assert np.abs(dt[..., k] - fdt[..., k]).max() <= 1e-6 * max(np.abs(fdt[..., k]).max(), 1e-300), k
    ul = rng.uniform(-1, 1, (nel, 32))
    ut = rng.uniform(-1, 1, (nel, R.npt, 16)) if surfaces else None
    lhs = np.sum(dl * ul) + (np.sum(dt * ut) if surfaces else 0.0)
    g = R.jtu(wrt, ul, ut)
    al, at = R.jv(wrt, v, absolute=True)
    bound = np.sum(al * np.abs(ul)) + (np.sum(at * np.abs(ut)) if surfaces else 0.0)
    assert abs(lhs - np.sum(g * v)) <= 1e-13 * bound
    # the majorants bound the plain products entry by entry (the sums of absolute terms are never smaller than the terms' sum)
    assert np.all(np.abs(dl) <= al * (1 + 1e-12)) and np.all(np.abs(g) <= R.jtu(wrt, ul, ut, absolute=True) * (1 + 1e-12))
    if surfaces:
        assert np.all(np.abs(dt) <= at * (1 + 1e-12))


def test_entries_are_declared_listed_exported_and_documented():
    from femo_alpha_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "femo_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert name in integration, name
    _build.build()
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_methods_and_model_arguments_exist():
    import inspect
    from femo_alpha_amd.backend import ShellContext
    from femo_alpha_amd.rm_shell.rm_shell_model import RMShellModel
    for m in ("set_layup", "layup_jvp", "layup_vjp"):
        assert callable(getattr(ShellContext, m)), m
    assert "layup" in inspect.signature(RMShellModel.__init__).parameters
    for f in ("clt_dtheta", "ply_table_dtheta", "ply_stiffness_dtheta"):
        assert callable(getattr(lm, f)), f


def test_ply_constants_of_set_layup():
    from femo_alpha_amd.backend import ShellContext
    pc = ShellContext._layup_plies(dict(PLY, **STRENGTH), 3)
    assert pc.shape == (3, 12) and np.array_equal(pc[1, 6:], lm.tsai_wu(**STRENGTH)) and pc[2, 0] == PLY["E1"]
    assert np.array_equal(ShellContext._layup_plies(pc, 3), pc)
    with pytest.raises(ValueError):
        ShellContext._layup_plies(pc, 2)
    with pytest.raises(ValueError):
        ShellContext._layup_plies([dict(PLY, **STRENGTH)] * 2, 3)
