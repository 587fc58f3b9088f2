"""The numpy reference of the static max-displacement aggregate (tests/disp_aggregate_ref.py) against itself: a brute-force
log-sum-exp, complex-step derivatives of its own value, the bounds of the contract and the value at w = 0.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import disp_aggregate_ref as ref                                                  # noqa: E402
from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles         # noqa: E402

MESHES = {"quad": lambda: plate_mesh(2.0, 10.0, 4, 20), "tri": lambda: quads_to_triangles(plate_mesh(2.0, 10.0, 4, 20)),
          "quad CG1CG1": lambda: ShellMesh(plate_mesh(2.0, 10.0, 4, 20).nodes, plate_mesh(2.0, 10.0, 4, 20).cells, "CG1CG1")}
D = (0.3, -0.2, 1.0)
# (scaler, direction): norm mode, direction mode with both signs
MODES = [(1.0, None), (2.5, None), (1.0, D), (-1.5, D)]


def _state(m, rng, scale=1e-2):
    return scale * rng.uniform(-1, 1, m.ndof)


def _cases(m):
    cells = np.arange(m.nel)[m.nel // 3: m.nel // 2]
    return [(None, "vertices"), (None, "all"), (cells, "vertices"), (cells, "all")]


def test_the_plate_meshes_have_the_sizes_the_gpu_tests_count_on():
    m = plate_mesh(2.0, 10.0, 4, 20)
    assert (m.nn, m.nP2) == (105, 369)
    m = plate_mesh(2.0, 10.0, 8, 40)
    assert (m.nn, m.nP2) == (369, 1377)
    assert ref.selected_nodes(m, None, "vertices").size == 369 and ref.selected_nodes(m, None, "all").size == 1377


@pytest.mark.parametrize("kind", list(MESHES))
def test_value_against_a_brute_force_log_sum_exp(kind):
    """rho |s| max x = 50: exp(50) is far from overflow, and the two ways differ by rounding alone (1e-13)."""
    m = MESHES[kind]()
    rng = np.random.default_rng(0)
    w = _state(m, rng)
    for cells, nodes in _cases(m):
        sel = ref.selected_nodes(m, cells, nodes)
        assert sel.size > 0
        for s, d in MODES:
            u = w[: 3 * m.nP2].reshape(-1, 3)[sel]
            xmax = np.abs(s) * (np.linalg.norm(u, axis=1) if d is None else np.abs(u @ np.array(d))).max()
            rho = 50.0 / xmax
            M, B = ref.value(w, m, sel, rho, s, d), ref.brute_force(w, m, sel, rho, s, d)
            assert abs(M - B) <= 1e-13 * abs(B), (kind, nodes, s, d)


@pytest.mark.parametrize("kind", list(MESHES))
def test_gradient_against_complex_steps_of_the_value(kind):
    """No selected node has zero norm (random states).  A complex step of 1e-30 carries no subtraction: 1e-12 of the largest entry."""
    m = MESHES[kind]()
    rng = np.random.default_rng(1)
    w = _state(m, rng)
    for cells, nodes in _cases(m):
        sel = ref.selected_nodes(m, cells, nodes)
        for s, d in MODES:
            rho = 5.0 / (abs(s) * 1e-2)
            g = ref.gradient(w, m, sel, rho, s, d)
            assert np.all(g[3 * m.nP2:] == 0.0)
            unsel = np.setdiff1d(np.arange(m.nP2), sel)
            assert np.all(g[: 3 * m.nP2].reshape(-1, 3)[unsel] == 0.0)
            p = g[: 3 * m.nP2].reshape(-1, 3)[sel]
            if d is None:
                assert abs(np.linalg.norm(p, axis=1).sum() - 1.0) <= 1e-13                # sum p_i = 1
            idx = np.concatenate([3 * sel[:4], 3 * sel[-4:] + 2, [3 * int(sel[np.argmax(np.abs(p).sum(axis=1))]) + 1]])
            for k in idx:
                wc = w.astype(complex)
                wc[k] += 1e-30j
                cs = ref.value(wc, m, sel, rho, s, d).imag / 1e-30
                assert abs(cs - g[k]) <= 1e-12 * np.abs(g).max(), (kind, nodes, s, d, k)


@pytest.mark.parametrize("kind", list(MESHES))
def test_bounds_for_both_signs_of_the_scaler(kind):
    m = MESHES[kind]()
    rng = np.random.default_rng(2)
    w = _state(m, rng)
    for cells, nodes in _cases(m):
        sel = ref.selected_nodes(m, cells, nodes)
        N = sel.size
        u = w[: 3 * m.nP2].reshape(-1, 3)[sel]
        for rho in (10.0, 1e3, 1e6):
            for s, d in MODES:
                M = ref.value(w, m, sel, rho, s, d)
                slack = np.log(N) / (rho * abs(s))
                if s > 0:
                    top = (np.linalg.norm(u, axis=1) if d is None else u @ np.array(d)).max()
                    assert top - 1e-15 <= M <= top + slack + 1e-15
                else:
                    low = (u @ np.array(d)).min()
                    assert low - slack - 1e-15 <= M <= low + 1e-15


def test_zero_state_in_norm_mode():
    m = plate_mesh(2.0, 10.0, 4, 20)
    w = np.zeros(m.ndof)
    for nodes, N in (("vertices", 105), ("all", 369)):
        sel = ref.selected_nodes(m, None, nodes)
        for rho, s in ((100.0, 1.0), (7.0, 3.0)):
            assert abs(ref.value(w, m, sel, rho, s) - np.log(N) / (rho * s)) <= 1e-15
            assert not np.any(ref.gradient(w, m, sel, rho, s))
