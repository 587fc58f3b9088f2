"""Backward error of an application of a Cholesky factor, the metric the factor tests assert.

PCG corrects any error of its preconditioner, so a factor that is wrong in its 8th digit still converges in the same number of
iterations to the same solution; and ``rel(K z, v)`` is dominated by the conditioning of the operator (1e10 .. 1e13 on the thin shells
here, 1e15 penalty rows), so it sits near 1e-9 for an exact factor and moves little when one entry is off.  The row-wise backward
error of Oettli and Prager after the symmetric diagonal scaling that Cholesky is invariant to is what sees a wrong factor:

    D = |diag K|,  K^ = D^-1/2 K D^-1/2,  z^ = D^1/2 z,  v^ = D^-1/2 v,
    omega(z) = max_i |v^ - K^ z^|_i / (|K^| |z^| + |v^|)_i

An exact factor leaves omega at a few units of rounding (~1e-14); a factor entry off by a relative 1e-10 raises it to 1e-11 and more
(tests/test_factor_check_cpu.py pins these numbers on two meshes)."""
import numpy as np
import scipy.sparse as sp


def _scaled(K):
    K = sp.csr_matrix(K)
    d = np.abs(K.diagonal())
    if not np.all(d > 0):
        raise ValueError("omega: K needs a non-zero diagonal")
    s = 1.0 / np.sqrt(d)
    S = sp.diags(s)
    return (S @ K @ S).tocsr(), s


def omega(K, V, Z, rows=None):
    """Row-wise scaled backward error of Z as the solution of K Z = V: the largest over the rows and over the columns of V / Z
    (vectors of K.shape[0] entries, or arrays (n, ncols)).  ``rows``: a boolean mask of K.shape[0] entries, the rows the largest is
    taken over (default: all of them; every row is computed with the whole of Z either way).  Returns one float."""
    Kh, s = _scaled(K)
    Ka = abs(Kh)
    V = np.asarray(V, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    if V.ndim == 1:
        V, Z = V[:, None], Z[:, None]
    if V.shape != Z.shape or V.shape[0] != Kh.shape[0]:
        raise ValueError("omega: V and Z must both be (n,) or (n, ncols)")
    zh = Z / s[:, None]
    vh = V * s[:, None]
    num = np.abs(vh - Kh @ zh)
    den = Ka @ np.abs(zh) + np.abs(vh)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    if rows is not None:
        rows = np.asarray(rows)
        if rows.dtype != bool or rows.shape != (Kh.shape[0],) or not rows.any():
            raise ValueError("omega: rows must be a boolean mask of K.shape[0] entries with at least one row set")
        r = r[rows]
    return float(r.max())


def omega_fit(K, v, x):
    """omega of s x, where the scalar s minimises || v^ - s K^ x^ ||_2: for an x known only up to a factor (the first PCG iterate
    x_1 = alpha M^-1 b)."""
    Kh, sc = _scaled(K)
    vh = np.asarray(v, dtype=np.float64) * sc
    kx = Kh @ (np.asarray(x, dtype=np.float64) / sc)
    s = float(kx @ vh) / float(kx @ kx)
    return omega(K, v, s * np.asarray(x, dtype=np.float64))


def rel(a, b):
    """The metric the factor was checked with before: max |a - b| / max |b|."""
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)
