"""CPU-side checks of the max-displacement aggregate and the tip history of the transient path: the entries are declared, listed in
the ctypes table, exported by the built library and named in INTEGRATION.md; the operation and the PlateSim / ShellContext methods
exist; ShellMesh.point_evaluation (the tip probe) against its defining properties on every element variant; the numpy restatement
of the KS aggregate (tests/disp_history_ref.py) against a brute-force log-sum-exp.  No compute call is made without a GPU."""
import os
import re

import numpy as np
import pytest

import disp_history_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["femo_newmark_disp_aggregate", "femo_newmark_disp_aggregate_grad"]


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


def test_operation_and_methods_exist():
    from femo_alpha_amd.backend import ShellContext
    from femo_alpha_amd.dynamic_rm_shell.operations import MaxDisplacementHistoryOperation
    from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
    from femo_alpha_amd.mesh import ShellMesh
    assert callable(MaxDisplacementHistoryOperation.compute) and callable(MaxDisplacementHistoryOperation.compute_derivatives)
    for m in ("newmark_disp_aggregate", "newmark_disp_aggregate_grad"):
        assert callable(getattr(ShellContext, m)), m
    for m in ("set_up_tip_dofs", "tip_displacement_history", "max_displacement_history", "max_displacement_history_partials",
              "max_displacement_history_total_gradient"):
        assert callable(getattr(PlateSim, m)), m
    assert callable(ShellMesh.point_evaluation)


def _meshes():
    from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles, unstructured_quad_skin_mesh, wing_skin_mesh
    tri = quads_to_triangles(plate_mesh(2.0, 10.0, 3, 7))
    return {
        "CG2CG1 quads": plate_mesh(2.0, 10.0, 3, 7),
        "CG1CG1 quads": plate_mesh(2.0, 10.0, 3, 7, element="CG1CG1"),
        "CG2CG1 triangles": tri,
        "CG2CR1 triangles": ShellMesh(tri.nodes, tri.cells, "CG2CR1"),
        "warped wing skin": wing_skin_mesh(6, 14),
        "warped unstructured quads": unstructured_quad_skin_mesh(4, 10),
        "warped unstructured quads CG1CG1": unstructured_quad_skin_mesh(4, 10, element="CG1CG1"),
    }


MESHES = _meshes()


def _random_ref(mesh, rng):
    if mesh.is_quad:
        return rng.uniform(-0.98, 0.98, 2)
    lam = 0.01 + 0.97 * rng.dirichlet(np.ones(3))        # barycentric coordinates, every one >= 0.01
    return lam[1:]


def _node_coords(mesh):
    return mesh.nodes if mesh.element == "CG1CG1" else mesh.p2_coords


@pytest.mark.parametrize("name", list(MESHES))
def test_point_evaluation_is_kronecker_at_the_nodes(name):
    mesh = MESHES[name]
    rng = np.random.default_rng(1)
    P = _node_coords(mesh)
    for c in rng.choice(mesh.nel, 6, replace=False):
        for a, p in enumerate(mesh.cell_p2[c]):
            for comp in (0, 2):
                dofs, w = mesh.point_evaluation(P[p], cell=c, component=comp)
                assert np.array_equal(dofs, 3 * mesh.cell_p2[c] + comp)
                e = np.zeros(mesh.npc); e[a] = 1.0
                assert np.abs(w - e).max() < 1e-12, (name, c, a, w)
        v = mesh.cells[c, 0]                      # a vertex probe gives the vertex's own DOF exactly
        dofs, w = mesh.point_evaluation(mesh.nodes[v], cell=c)
        assert w[0] == 1.0 and np.all(w[1:] == 0.0)


@pytest.mark.parametrize("name", list(MESHES))
def test_point_evaluation_reproduces_a_linear_field_inside_warped_cells(name):
    """f(x) = a.x + b interpolated at the nodes is bilinear in the reference coordinates of a (bi)linear cell, so the basis reproduces
    it exactly -- at the right reference point only: this pins the pull-back, not just the basis."""
    mesh = MESHES[name]
    rng = np.random.default_rng(2)
    a, b = rng.normal(size=3), rng.normal()
    w = np.zeros(mesh.ndof)
    w[3 * np.arange(mesh.nP2) + 2] = _node_coords(mesh) @ a + b
    for c in rng.choice(mesh.nel, 12, replace=False):
        N, _ = mesh._geometry(_random_ref(mesh, rng))
        x = N @ mesh.nodes[mesh.cells[c]]
        dofs, wt = mesh.point_evaluation(x, cell=c)
        assert abs(wt @ w[dofs] - (x @ a + b)) < 1e-12 * (1 + abs(x @ a + b)), (name, c)
        # located without the cell: a cell holding x (the same one, or a neighbour when x is on a shared edge) gives the same value
        dofs2, wt2 = mesh.point_evaluation(x)
        assert abs(wt2 @ w[dofs2] - (x @ a + b)) < 1e-12 * (1 + abs(x @ a + b)), (name, c)
        assert mesh.locate(x) == c


def test_point_evaluation_off_the_mesh_and_bad_arguments_raise():
    from femo_alpha_amd.mesh import plate_mesh
    mesh = plate_mesh(2.0, 10.0, 3, 7)
    with pytest.raises(ValueError, match="lies in no cell"):
        mesh.point_evaluation([12.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="lies in no cell"):
        mesh.point_evaluation([5.0, -0.5, 0.0])
    with pytest.raises(ValueError, match="cell"):
        mesh.point_evaluation([5.0, 1.0, 0.0], cell=mesh.nel)
    with pytest.raises(ValueError, match="component"):
        mesh.point_evaluation([5.0, 1.0, 0.0], component=3)
    assert mesh.locate([12.0, 1.0, 0.0]) is None
    # a point above the plate: located in the cell under it, evaluated at its projection
    dofs, w = mesh.point_evaluation([5.0, 1.0, 0.3])
    dofs0, w0 = mesh.point_evaluation([5.0, 1.0, 0.0])
    assert np.array_equal(dofs, dofs0) and np.abs(w - w0).max() < 1e-14


def test_ks_restatement_against_brute_force_and_its_bounds():
    rng = np.random.default_rng(3)
    T, n, nu = 5, 40, 25
    W = rng.normal(size=(T, n)) * np.logspace(-3, 0, n)
    W[0] = 0.0                                     # the zero initial level
    for rho in (3.0, 50.0):
        for s in (2.5, -0.7):
            for comp, ncol in (("all", n), ("translations", nu)):
                M, Ml = R.ks_value(W, rho, s, nu, comp)
                x = np.abs(s) * np.abs(W[:, :ncol])
                assert M == pytest.approx(np.log(np.sum(np.exp(rho * x))) / rho / s, rel=1e-13)
                for i in range(T):
                    assert Ml[i] == pytest.approx(np.log(np.sum(np.exp(rho * x[i]))) / rho / s, rel=1e-13)
                assert Ml[0] == pytest.approx(np.log(ncol) / (rho * s), rel=1e-13)
                if s > 0:
                    N = x.size
                    assert np.abs(W[:, :ncol]).max() <= M <= np.abs(W[:, :ncol]).max() + np.log(N) / (rho * s)
                else:
                    assert M < 0
                # the gradient against central differences of the brute force
                G = R.ks_grad(W, rho, s, nu, comp)
                assert np.all(G[:, ncol:] == 0.0) and np.all(G[0] == 0.0)
                assert np.all(np.abs(G) <= 1.0 + 1e-15)
                brute = lambda V: np.log(np.sum(np.exp(rho * np.abs(s) * np.abs(V[:, :ncol])))) / rho / s
                for _ in range(3):
                    d = rng.normal(size=W.shape)
                    d[0] = 0.0                     # away from the kink of |w| at zero
                    eps = 1e-6
                    fd = (brute(W + eps * d) - brute(W - eps * d)) / (2 * eps)
                    assert np.sum(G * d) == pytest.approx(fd, rel=1e-7, abs=1e-9)
                # softmax weights: they sum to 1 over the selected entries, the n zero entries of level 0 included
                assert np.sum(np.abs(G)) == pytest.approx(1.0 - ncol * np.exp(-rho * s * M), rel=1e-12)
