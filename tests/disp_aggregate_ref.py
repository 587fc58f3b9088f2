"""numpy restatement of the static max-displacement aggregate (include/femo_hip.h, femo_set_disp_aggregate), written from the contract
and independent of the library:

    selected nodes i: members of a cell of the selection, of the kind asked for ('vertices': i < nn, 'all': every displacement node)
    x_i = s |u_i|  (norm mode)   or   x_i = s (d . u_i)  (direction mode, d as given)
    S = x_max + 1/rho log sum_i exp(rho (x_i - x_max)),   M = S / s,   p_i = exp(rho (x_i - S))
    dM/du_i = p_i u_i / |u_i|  (0 where |u_i| = 0)   or   p_i d

The value carries complex arithmetic (complex-step derivatives): the direction mode is linear in u, the norm is sqrt(u . u) without
abs, and the shift x_max is the entry of largest real part."""
import numpy as np


def selected_nodes(mesh, cells=None, nodes="vertices"):
    """Sorted indices of the selected displacement nodes; ``cells``: None for every cell, else the cell indices of the sub-domain."""
    cp2 = np.asarray(mesh.cell_p2)
    if cells is not None:
        cp2 = cp2[np.asarray(cells, dtype=np.int64)]
    sel = np.unique(cp2.ravel())
    sel = sel[sel < mesh.nP2]
    if nodes == "vertices":
        sel = sel[sel < mesh.nn]
    elif nodes != "all":
        raise ValueError("nodes must be 'vertices' or 'all'")
    return sel


def _x(u, s, direction):
    if direction is None:
        return s * np.sqrt(np.sum(u * u, axis=1))
    return s * (u @ np.asarray(direction, dtype=np.float64))


def value(w, mesh, sel, rho, s=1.0, direction=None):
    """M for the state vector ``w`` (real or complex) over the node indices ``sel``."""
    u = np.asarray(w)[: 3 * mesh.nP2].reshape(-1, 3)[sel]
    x = _x(u, s, direction)
    xm = x[np.argmax(x.real)]
    return (xm + np.log(np.sum(np.exp(rho * (x - xm)))) / rho) / s


def gradient(w, mesh, sel, rho, s=1.0, direction=None):
    """dM/dw, the length of ``w``: zeros on rotations and unselected nodes."""
    w = np.asarray(w, dtype=np.float64)
    u = w[: 3 * mesh.nP2].reshape(-1, 3)[sel]
    x = _x(u, s, direction)
    S = value(w, mesh, sel, rho, s, direction) * s
    p = np.exp(rho * (x - S))
    g = np.zeros(w.size)
    G = np.zeros((mesh.nP2, 3))
    if direction is None:
        r = np.sqrt(np.sum(u * u, axis=1))
        safe = np.where(r > 0, r, 1.0)
        G[sel] = np.where((r > 0)[:, None], p[:, None] * u / safe[:, None], 0.0)
    else:
        G[sel] = p[:, None] * np.asarray(direction, dtype=np.float64)[None, :]
    g[: 3 * mesh.nP2] = G.ravel()
    return g


def brute_force(w, mesh, sel, rho, s=1.0, direction=None):
    """The unshifted log-sum-exp, for moderate rho x only."""
    u = np.asarray(w, dtype=np.float64)[: 3 * mesh.nP2].reshape(-1, 3)[sel]
    x = _x(u, s, direction)
    return np.log(np.sum(np.exp(rho * x))) / (rho * s)
