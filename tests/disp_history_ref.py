"""numpy restatement of the max-displacement KS aggregate of the transient path (include/femo_hip.h, femo_newmark_disp_aggregate*),
written from the formula and independent of the library: the yardstick of tests/test_gpu_disp_history.py, itself checked against a
brute-force log-sum-exp in tests/test_disp_history_cpu.py.  W: (levels, ndof) level-major."""
import numpy as np


def selected(W, ndof_u, components):
    W = np.asarray(W, dtype=np.float64)
    if components == "all":
        return W
    if components == "translations":
        return W[:, :ndof_u]
    raise ValueError(components)


def _ks(x, rho):
    xm = x.max()
    return xm + np.log(np.sum(np.exp(rho * (x - xm)))) / rho


def ks_value(W, rho, s, ndof_u=None, components="all"):
    """(M, [M_i]): M = (x_max + 1/rho log sum exp(rho (x - x_max))) / s, x = |s| |w| over the selected entries of every level / of
    each level alone."""
    X = np.abs(s) * np.abs(selected(W, ndof_u, components))
    return _ks(X.ravel(), rho) / s, np.array([_ks(r, rho) / s for r in X])


def ks_grad(W, rho, s, ndof_u=None, components="all"):
    """dM/dW = sign(s) sign(w) exp(rho (x - s M)), zero where w = 0 and on the entries not selected; (levels, ndof)."""
    W = np.asarray(W, dtype=np.float64)
    M, _ = ks_value(W, rho, s, ndof_u, components)
    Ws = selected(W, ndof_u, components)
    G = np.zeros_like(W)
    G[:, :Ws.shape[1]] = np.sign(s) * np.sign(Ws) * np.exp(rho * (np.abs(s) * np.abs(Ws) - s * M))
    return G
