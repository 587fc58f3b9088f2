"""Meshes whose topology the generators of femo_alpha_amd.mesh never produce: several components, a cut-out, a vertex of high valence
and an edge shared by many cells.  Plain numpy, for the tests only (tests/test_topology_cpu.py pins what each of them does to the
elimination tree and to the CSR map; tests/test_gpu_topology.py runs the device code on them)."""
import numpy as np

from femo_alpha_amd.mesh import ShellMesh, plate_mesh, quads_to_triangles

SEED_PERM = 11


def _finish(nodes, cells, element, tri, shuffle):
    """Triangle variant (every quad cut along its 0-2 diagonal) and / or a fixed-seed permutation of the nodes and of the cells."""
    nodes = np.asarray(nodes, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    if tri and cells.shape[1] == 4:
        cells = quads_to_triangles(ShellMesh(nodes, cells)).cells.astype(np.int64)
    if shuffle:
        rng = np.random.default_rng(SEED_PERM)
        new_of_old = rng.permutation(nodes.shape[0])
        old_of_new = np.empty_like(new_of_old)
        old_of_new[new_of_old] = np.arange(new_of_old.size)
        nodes = nodes[old_of_new]
        cells = new_of_old[cells][rng.permutation(cells.shape[0])]
    return ShellMesh(nodes, cells, element)


def islands(n=4, gap=0.5, tri=False, shuffle=False, element="CG2CG1"):
    """Two n x 2n plates (1 wide in y, 2 long in x), the second shifted by 2 + gap along y: two components that both reach x = 0.

    Exists for the front with nf == 0: the first cut of the bisection falls in the gap, its separator has no nodes, and the root of
    the elimination tree has neither pivots nor a boundary (an extend-add over nothing, a level whose largest front is empty)."""
    a = plate_mesh(1.0, 2.0, n, 2 * n)
    nodes = np.vstack([a.nodes, a.nodes + [0.0, 2.0 + gap, 0.0]])
    cells = np.vstack([a.cells, a.cells + a.nn])
    return _finish(nodes, cells, element, tri, shuffle)


def plate_with_hole(n=10, tri=False, shuffle=False, element="CG2CG1"):
    """The unit n x n plate less the cells whose centroid lies within 0.17 of the centre in both coordinates, nodes compacted.

    Exists for pivot-free fronts in the MIDDLE of the tree: a cut through the hole separates two pieces that share no node there, so
    fronts above the leaf level have npiv == 0 (and a boundary that is the plain sum of their children's) beside ordinary fronts."""
    a = plate_mesh(1.0, 1.0, n, n)
    c = a.nodes[a.cells].mean(axis=1)
    keep = ~((np.abs(c[:, 0] - 0.5) < 0.17) & (np.abs(c[:, 1] - 0.5) < 0.17))
    cells = a.cells[keep]
    used = np.unique(cells)
    remap = -np.ones(a.nn, dtype=np.int64)
    remap[used] = np.arange(used.size)
    return _finish(a.nodes[used], remap[cells], element, tri, shuffle)


def fan(k=70, shuffle=False, element="CG2CG1"):
    """k triangles round a centre vertex (valence k) and a ring of 2 k triangles outside them; rings at radius 1 and 2,
    z = 0.2 cos(3 theta) r, so the surface is not flat.

    Exists for (a) pivot-free LEAVES beside ordinary leaves: with small leaves most cells of the inner ring own none of their nodes
    (the centre and the spokes belong to ancestors); (b) CSR runs of k contributions to one matrix entry (the centre's diagonal
    block), longer than a 64-lane chunk of k_csr_segmented for k >= 65; (c) nothing else about it is special: all edges have two cells."""
    th = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
    r1 = np.stack([np.cos(th), np.sin(th), 0.2 * np.cos(3.0 * th)], axis=1)
    nodes = np.vstack([[[0.0, 0.0, 0.0]], r1, 2.0 * r1])
    i = np.arange(k)
    j = (i + 1) % k
    cells = np.stack([np.stack([0 * i, 1 + i, 1 + j], axis=1), np.stack([1 + i, 1 + k + i, 1 + k + j], axis=1),
                      np.stack([1 + i, 1 + k + j, 1 + j], axis=1)], axis=1).reshape(-1, 3)
    return _finish(nodes, cells, element, False, shuffle)


def book(k=70, nl=3, tri=False, shuffle=False, element="CG2CG1"):
    """k pages at angles 2 pi p / k round a common spine on the y axis (0 <= y <= 1.5); a page is 2 quads across (radius 0.5 and 1)
    and nl quads along the spine.

    Exists for edges shared by k cells: the spine's edges (penalty facets with k incident cells each when the spine is clamped; CSR
    runs of k and 2 k contributions; pivot-free fronts even at usual leaf sizes, because the spine's nodes belong to the top of the
    tree).  book(1100, 1) has runs long enough that a whole 512-contribution wave of k_csr_segmented lies inside one of them."""
    ys = np.linspace(0.0, 1.5, nl + 1)
    nodes = [np.stack([0 * ys, ys, 0 * ys], axis=1)]
    cells = []
    jj = np.arange(nl)
    for p in range(k):
        a = 2.0 * np.pi * p / k
        base = (nl + 1) * (1 + 2 * p)
        for r in (0.5, 1.0):
            nodes.append(np.stack([r * np.cos(a) + 0 * ys, ys, r * np.sin(a) + 0 * ys], axis=1))
        cells.append(np.stack([jj, base + jj, base + jj + 1, jj + 1], axis=1))
        cells.append(np.stack([base + jj, base + nl + 1 + jj, base + nl + 2 + jj, base + jj + 1], axis=1))
    # cell order of a page: inner and outer quad of every spine segment, as a mesher walking along the page would give them
    cells = np.stack(cells, axis=0).reshape(k, 2, nl, 4).transpose(0, 2, 1, 3).reshape(-1, 4)
    return _finish(np.vstack(nodes), cells, element, tri, shuffle)


# markers of the clamped sets the tests use
CLAMP_X0 = lambda x: np.less(x[0], 1e-12)                                  # islands, holed: the x = 0 edge (both islands reach it)
CLAMP_Y0 = lambda x: np.less(x[1], 1e-12)                                  # book: the y = 0 edges of all pages
CLAMP_OUTER = lambda x: np.greater(x[0] ** 2 + x[1] ** 2, 3.9)              # fan: the outer ring (radius 2)
CLAMP_SPINE = lambda x: np.less(x[0] ** 2 + x[2] ** 2, 1e-20)               # book: the spine itself (k cells on every clamped edge)


# ------------------------------------------------------------------ the named cases of the tests
# name -> (generator call, marker of the clamped set); "_spine": the same mesh clamped along the spine
MESHES = {
    "islands": (lambda: islands(), CLAMP_X0),
    "islands_tri": (lambda: islands(tri=True), CLAMP_X0),
    "islands_shuffled": (lambda: islands(shuffle=True), CLAMP_X0),
    "holed": (lambda: plate_with_hole(), CLAMP_X0),
    "holed_tri": (lambda: plate_with_hole(tri=True), CLAMP_X0),
    "holed_shuffled": (lambda: plate_with_hole(shuffle=True), CLAMP_X0),
    "fan70": (lambda: fan(70), CLAMP_OUTER),
    "fan70_cg1": (lambda: fan(70, element="CG1CG1"), CLAMP_OUTER),
    "fan70_cr1": (lambda: fan(70, element="CG2CR1"), CLAMP_OUTER),
    "fan70_shuffled": (lambda: fan(70, shuffle=True), CLAMP_OUTER),
    "fan24": (lambda: fan(24), CLAMP_OUTER),
    "book70": (lambda: book(70, 3), CLAMP_Y0),
    "book70_shuffled": (lambda: book(70, 3, shuffle=True), CLAMP_Y0),
    "book70_spine": (lambda: book(70, 3), CLAMP_SPINE),
}
_meshes = {}


def base(name):
    """"<mesh>_strong" is <mesh> clamped through strong DOFs instead of penalty facets."""
    return name[:-len("_strong")] if name.endswith("_strong") else name


def mesh(name):
    if name not in _meshes:
        _meshes[name] = MESHES[name][0]()
    return _meshes[name]


def clamp(name):
    return MESHES[name][1]


def oracle_problem(name, strong=False, uhat=None, beta=None):
    """(mesh, oracle) of a named case with the fields of test_gpu_factor_backward_error._fields: nodal thickness and E with
    +-30 % / +-20 % noise and a random load; clamped by penalty facets, or by strong DOFs."""
    from oracle.rm_shell_oracle import ShellOracle
    from test_gpu_factor_backward_error import _fields
    m = mesh(name)
    f = _fields(m)
    kw = dict(strong_dofs=m.locate_dofs_geometrical(clamp(name))) if strong else dict(penalty_facets=m.penalty_facets(clamp(name)))
    if beta is not None:
        kw["beta"] = beta
    o = ShellOracle(m, **kw)
    o.set_fields(h=f["thickness"], E=f["E"], nu=0.3, rho=2700.0, f=f["F_solid"], uhat=uhat)
    return m, o
