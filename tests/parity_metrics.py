"""Row- and entry-scaled errors of operator-level quantities, the metrics tests/test_gpu_operator_rowscaled.py asserts.

The operator-level parity tests compare with ``rel(a, b) = max|a - b| / max|b|`` at 1e-11.  Where the clamp is the penalty beta = 1e15, the
largest entry of K x is a penalty row of ~4e14 beside interior rows of 1e3 .. 1e7: 95-96 % of the rows of K x lie below 1e-6 max|K x| (plate
and warped meshes of test_gpu_parity._pair), so 1e-11 of the largest row is an absolute 4e3 on rows whose whole value is that size or smaller.
Measured with the float64 oracle alone (tests/test_parity_metrics_cpu.py pins these):

  * every non-penalty row of K x times 1 + 1e-4 leaves rel at ~4e-12 on the plate (1.7e-11 on the warped mesh); times 1 + 1e-6, at 3.6e-14;
  * the thickness of one interior node changed by a relative 1e-7 moves rel(K x) by 7.6e-16 and rel(diag K) by 1.5e-15 -- and
    row_scaled(K x) to 3.8e-8, entrywise(diag K) to 1.1e-7;
  * without any penalty, the diagonal of one element matrix spans a factor 5e5 (rotations against translations): a 1e-9 thickness change
    shows at 1.5e-10 in rel(Ke) and at 1.1e-9 in entry_scaled(Ke).

The metrics below divide every row, entry or term by a scale of its own, so no row hides behind a larger one.  REFERENCE_FLOOR holds what
the float64 oracle itself reaches under each metric against a higher-precision evaluation of the same quantity; the GPU tests allow
BOUND_FACTOR times that."""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53                   # unit round-off of float64
BOUND_FACTOR = 50.0              # a kernel may be this many reference floors away from the oracle (test_gpu_operator_rowscaled.py)


def rel(a, b):
    """The metric the operator-level tests were checked with before: max |a - b| / max |b|."""
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def _ratio(num, den):
    """max_i num_i / den_i; an entry whose scale is zero must have a zero numerator, otherwise inf."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    if num.shape != den.shape:
        raise ValueError(f"scaled error: error {num.shape} and scale {den.shape} differ in shape")
    if not np.all(np.isfinite(num)) or np.any(np.isnan(den)):
        return float("inf")
    if np.any(den < 0):
        raise ValueError("scaled error: a scale is negative")
    if num.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    return float(r.max())


def _diff(a, b):
    """|a - b| in float64, formed in the wider of the two types (a reference may be numpy.longdouble)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError(f"scaled error: value {a.shape} and reference {b.shape} differ in shape")
    return np.abs(a - b).astype(np.float64)


def row_scaled(y, y_ref, K, x, extra=None):
    """Row-wise error of an operator application: max_i |y - y_ref|_i / (|K| |x| (+ extra))_i, K the oracle's assembled operator (penalty
    and strong rows included), ``extra`` a further non-negative term of the scale (the residual K w - F: extra = |F|).  A row whose scale
    is zero must hold y_i == y_ref_i exactly; otherwise the result is inf.  The denominator is the sum of the absolute values of the terms
    row i adds, so the metric is invariant to any scaling of the rows (D K with D diagonal: numerator and denominator of row i scale
    alike) -- a penalty row of 4e14 weighs as much as an interior row of 1e3.  ``rel`` divides all rows by the largest one: with every
    non-penalty row of K x off by 1e-4 it reads 4e-12, and with one interior thickness off by 1e-7 it moves by 7.6e-16, where this metric
    reads 3.8e-8."""
    K = sp.csr_matrix(K)
    x = np.asarray(x, dtype=np.float64)
    if K.shape[0] != K.shape[1] or x.shape != (K.shape[0],):
        raise ValueError("row_scaled: K must be square and x a vector of K.shape[0] entries")
    scale = abs(K) @ np.abs(x)
    if extra is not None:
        extra = np.asarray(extra, dtype=np.float64)
        if extra.shape != scale.shape or np.any(extra < 0):
            raise ValueError("row_scaled: extra must be a non-negative vector of K.shape[0] entries")
        scale = scale + extra
    return _ratio(_diff(y, y_ref), scale)


def entry_scaled(A, A_ref):
    """Entry-wise error of symmetric positive (semi-)definite matrices after the symmetric diagonal scaling: max_ij |A - A_ref|_ij /
    sqrt(A_ref_ii A_ref_jj), for element matrices (nel, ld, ld) -- each scaled by its own diagonal -- and for scipy sparse matrices of one
    pattern (the CSR values; the diagonal comes from the same matrix).  A zero (or negative) diagonal entry of the reference raises, as
    factor_check._scaled does.  Invariant to D A D with D diagonal, that is to the units of the DOFs: the diagonal of one element matrix
    spans a factor 5e5 between rotations and translations, so ``rel`` sees the rotation block three to six digits worse than this metric
    does (a 1e-9 thickness change: 1.5e-10 under rel, 1.1e-9 here), and with a penalty in the matrix not at all."""
    if sp.issparse(A_ref):
        A_ref = sp.csr_matrix(A_ref)
        if A_ref.shape[0] != A_ref.shape[1]:
            raise ValueError("entry_scaled: the matrices must be square")
        d = A_ref.diagonal()
        if not np.all(d > 0):
            raise ValueError("entry_scaled: the reference needs a positive diagonal")
        if not sp.issparse(A):
            # the values alone (they may be numpy.longdouble, which scipy does not hold), in the order of A_ref's sorted pattern
            if not A_ref.has_sorted_indices:
                raise ValueError("entry_scaled: values without a pattern need a reference with sorted indices")
            rows = np.repeat(np.arange(A_ref.shape[0]), np.diff(A_ref.indptr))
            return _ratio(_diff(A, A_ref.data), np.sqrt(d[rows] * d[A_ref.indices]))
        if A.shape != A_ref.shape:
            raise ValueError("entry_scaled: the matrices must be of one shape")
        E = abs(sp.csr_matrix(A) - A_ref).tocoo()
        if E.nnz == 0:
            return 0.0
        if not np.all(np.isfinite(E.data)):
            return float("inf")
        return _ratio(E.data, np.sqrt(d[E.row] * d[E.col]))
    A_ref = np.asarray(A_ref)
    if A_ref.ndim != 3 or A_ref.shape[1] != A_ref.shape[2]:
        raise ValueError("entry_scaled: element matrices are (nel, ld, ld)")
    d = np.einsum("eii->ei", A_ref).astype(np.float64)
    if not np.all(d > 0):
        raise ValueError("entry_scaled: the reference needs a positive diagonal")
    return _ratio(_diff(A, A_ref), np.sqrt(d[:, :, None] * d[:, None, :]))


def entrywise(d, d_ref):
    """Relative error of each entry by itself: max_i |d - d_ref|_i / |d_ref|_i, for the diagonal of K (sums of positive terms: the entry is
    its own scale).  Invariant to any scaling of the entries.  Under ``rel`` the 1e15 penalty entries set the scale, and one interior
    thickness off by 1e-7 moves rel(diag K) by 1.5e-15; this metric reads 1.1e-7.  A zero reference entry must be matched exactly."""
    return _ratio(_diff(d, d_ref), np.abs(np.asarray(d_ref, dtype=np.float64)))


def term_scaled(g, g_ref, scale):
    """Error of sums whose terms cancel: max_i |g - g_ref|_i / scale_i, ``scale`` the same sum with every term replaced by its absolute
    value (the oracle's ``absolute=True``: np.abs on B, dC, the shape-function tables, lam_e, w_e and f inside the same einsums).  For
    the transposed derivative products, the partial gradients of the functionals and the load vector.  Invariant to the scaling of any
    single entry (its terms and its scale move together), and what a summation in another order can move an entry by is a multiple of
    u scale_i whatever the cancellation.  ``rel`` divides by the largest entry of g: entries that are small because their terms cancel,
    or because their node carries little of the load, are checked to fewer digits the smaller they are."""
    scale = np.asarray(scale, dtype=np.float64)
    return _ratio(_diff(g, g_ref), scale.reshape(np.shape(g_ref)))


# REFERENCE_FLOOR[(quantity, case)]: the metric of the float64 oracle against a higher-precision evaluation of the same quantity
# (tests/rowscaled_cases.py names the cases and the quantities; tests/test_parity_metrics_cpu.py measures the value again and holds every
# constant between that and four times that).  Recorded as twice the value measured when the table was made.  Source of the higher
# precision, per entry of REFERENCE_SOURCE: "dd" = CpuShell.assemble_K_dd (double-double assembly: isotropic law, rotations on the
# vertices, penalty clamp or none), "ld" = the oracle's own methods in numpy.longdouble with the operands cast (node coordinates, fields
# and inputs: rowscaled_cases.extended -- geometry, B, C, einsums and scatter-adds all in extended precision; with B and C merely cast
# the floor misses the rounding of the oracle's own B, which on slender triangles is 50 to 130 times its summation error).  No case
# needed the third resort, the difference of the two float64 implementations.
REFERENCE_FLOOR = {
    # plate-penalty
    ("Ke", "plate-penalty"): 3.61e-15, ("Kx:uniform", "plate-penalty"): 2.28e-15, ("Kx:element", "plate-penalty"): 1.89e-15,
    ("Kx:free", "plate-penalty"): 1.58e-15, ("Kxvec:uniform", "plate-penalty"): 2.28e-15, ("diag", "plate-penalty"): 2.5e-15,
    ("residual", "plate-penalty"): 1.78e-15, ("load", "plate-penalty"): 2.15e-15, ("csr", "plate-penalty"): 2.5e-15,
    ("dRdT:thickness", "plate-penalty"): 1.12e-16, ("dRdT:E", "plate-penalty"): 1.16e-16, ("dRdT:nu", "plate-penalty"): 1.3e-16,
    ("dRdT:F_solid", "plate-penalty"): 8.82e-16, ("dJ:compliance:thickness", "plate-penalty"): 1.2e-16, ("dJ:compliance:disp_solid", "plate-penalty"): 1.29e-15,
    ("dJ:elastic_energy:disp_solid", "plate-penalty"): 1.79e-15, ("dJ:elastic_energy:thickness", "plate-penalty"): 3.61e-16,
    # warped-penalty
    ("Ke", "warped-penalty"): 6.41e-15, ("Kx:uniform", "warped-penalty"): 2.94e-15, ("Kx:element", "warped-penalty"): 6.75e-15,
    ("Kx:free", "warped-penalty"): 2.46e-15, ("Kxvec:uniform", "warped-penalty"): 2.94e-15, ("diag", "warped-penalty"): 4.68e-15,
    ("residual", "warped-penalty"): 3.28e-15, ("load", "warped-penalty"): 2.07e-15, ("csr", "warped-penalty"): 4.68e-15,
    ("dRdT:thickness", "warped-penalty"): 2.66e-16, ("dRdT:E", "warped-penalty"): 2.56e-16, ("dRdT:nu", "warped-penalty"): 2.15e-16,
    ("dRdT:F_solid", "warped-penalty"): 1.39e-15, ("dJ:compliance:thickness", "warped-penalty"): 3.37e-16, ("dJ:compliance:disp_solid", "warped-penalty"): 1.75e-15,
    ("dJ:elastic_energy:disp_solid", "warped-penalty"): 3.09e-15, ("dJ:elastic_energy:thickness", "warped-penalty"): 5.54e-16,
    # warped-ewm-ewp-strong
    ("Ke", "warped-ewm-ewp-strong"): 6.59e-15, ("Kx:uniform", "warped-ewm-ewp-strong"): 3.09e-15, ("Kx:element", "warped-ewm-ewp-strong"): 2.68e-14,
    ("Kx:free", "warped-ewm-ewp-strong"): 2.58e-15, ("Kxvec:uniform", "warped-ewm-ewp-strong"): 3.09e-15, ("diag", "warped-ewm-ewp-strong"): 5.97e-15,
    ("residual", "warped-ewm-ewp-strong"): 3.49e-15, ("load", "warped-ewm-ewp-strong"): 2.28e-15, ("csr", "warped-ewm-ewp-strong"): 5.97e-15,
    ("dRdT:thickness", "warped-ewm-ewp-strong"): 3.07e-16, ("dRdT:E", "warped-ewm-ewp-strong"): 3.96e-16, ("dRdT:nu", "warped-ewm-ewp-strong"): 2.25e-16,
    ("dRdT:F_solid", "warped-ewm-ewp-strong"): 1.22e-15, ("dJ:compliance:thickness", "warped-ewm-ewp-strong"): 2.31e-15, ("dJ:compliance:disp_solid", "warped-ewm-ewp-strong"): 1.46e-15,
    ("dJ:elastic_energy:disp_solid", "warped-ewm-ewp-strong"): 2.82e-15, ("dJ:elastic_energy:thickness", "warped-ewm-ewp-strong"): 9.88e-16,
    # warped-uhat-penalty
    ("Ke", "warped-uhat-penalty"): 6.7e-15, ("Kx:uniform", "warped-uhat-penalty"): 3.02e-15, ("Kx:element", "warped-uhat-penalty"): 9.96e-15,
    ("Kx:free", "warped-uhat-penalty"): 2.83e-15, ("Kxvec:uniform", "warped-uhat-penalty"): 3.02e-15, ("diag", "warped-uhat-penalty"): 5.05e-15,
    ("residual", "warped-uhat-penalty"): 2.4e-15, ("load", "warped-uhat-penalty"): 2.78e-15, ("csr", "warped-uhat-penalty"): 5.05e-15,
    ("dRdT:thickness", "warped-uhat-penalty"): 2.94e-16, ("dRdT:E", "warped-uhat-penalty"): 2.4e-16, ("dRdT:nu", "warped-uhat-penalty"): 1.72e-16,
    ("dRdT:F_solid", "warped-uhat-penalty"): 1.46e-15, ("dJ:compliance:thickness", "warped-uhat-penalty"): 3.37e-16, ("dJ:compliance:disp_solid", "warped-uhat-penalty"): 1.63e-15,
    ("dJ:elastic_energy:disp_solid", "warped-uhat-penalty"): 2.74e-15, ("dJ:elastic_energy:thickness", "warped-uhat-penalty"): 3.52e-16,
    # tri-penalty
    ("Ke", "tri-penalty"): 7.74e-14, ("Kx:uniform", "tri-penalty"): 4.48e-14, ("Kx:element", "tri-penalty"): 1.55e-13,
    ("Kx:free", "tri-penalty"): 4.85e-14, ("Kxvec:uniform", "tri-penalty"): 4.48e-14, ("diag", "tri-penalty"): 5.33e-14,
    ("residual", "tri-penalty"): 5.16e-14, ("load", "tri-penalty"): 8.63e-16, ("csr", "tri-penalty"): 5.33e-14,
    ("dRdT:thickness", "tri-penalty"): 3.27e-15, ("dRdT:E", "tri-penalty"): 3.42e-15, ("dRdT:nu", "tri-penalty"): 1.51e-15,
    ("dRdT:F_solid", "tri-penalty"): 3.51e-16, ("dJ:compliance:thickness", "tri-penalty"): 2.32e-15, ("dJ:compliance:disp_solid", "tri-penalty"): 6.55e-16,
    ("dJ:elastic_energy:disp_solid", "tri-penalty"): 5.11e-14, ("dJ:elastic_energy:thickness", "tri-penalty"): 9.62e-15,
    # tri-ewm-uhat-strong
    ("Ke", "tri-ewm-uhat-strong"): 7.94e-14, ("Kx:uniform", "tri-ewm-uhat-strong"): 4.08e-14, ("Kx:element", "tri-ewm-uhat-strong"): 7.42e-13,
    ("Kx:free", "tri-ewm-uhat-strong"): 4.27e-14, ("Kxvec:uniform", "tri-ewm-uhat-strong"): 4.08e-14, ("diag", "tri-ewm-uhat-strong"): 5.44e-14,
    ("residual", "tri-ewm-uhat-strong"): 4.68e-14, ("load", "tri-ewm-uhat-strong"): 4.39e-15, ("csr", "tri-ewm-uhat-strong"): 5.44e-14,
    ("dRdT:thickness", "tri-ewm-uhat-strong"): 1.14e-14, ("dRdT:E", "tri-ewm-uhat-strong"): 1.13e-14, ("dRdT:nu", "tri-ewm-uhat-strong"): 2.65e-15,
    ("dRdT:F_solid", "tri-ewm-uhat-strong"): 1.11e-15, ("dJ:compliance:thickness", "tri-ewm-uhat-strong"): 1.06e-15, ("dJ:compliance:disp_solid", "tri-ewm-uhat-strong"): 3.92e-15,
    ("dJ:elastic_energy:disp_solid", "tri-ewm-uhat-strong"): 4.68e-14, ("dJ:elastic_energy:thickness", "tri-ewm-uhat-strong"): 1.82e-14,
    # tee-uhat-penalty
    ("Ke", "tee-uhat-penalty"): 2.79e-15, ("Kx:uniform", "tee-uhat-penalty"): 1.37e-15, ("Kx:element", "tee-uhat-penalty"): 3.87e-15,
    ("Kx:free", "tee-uhat-penalty"): 1.63e-15, ("Kxvec:uniform", "tee-uhat-penalty"): 1.37e-15, ("diag", "tee-uhat-penalty"): 1.8e-15,
    ("residual", "tee-uhat-penalty"): 1.73e-15, ("load", "tee-uhat-penalty"): 9.5e-16, ("csr", "tee-uhat-penalty"): 1.8e-15,
    ("dRdT:thickness", "tee-uhat-penalty"): 2e-16, ("dRdT:E", "tee-uhat-penalty"): 1.98e-16, ("dRdT:nu", "tee-uhat-penalty"): 1.33e-16,
    ("dRdT:F_solid", "tee-uhat-penalty"): 6.31e-16, ("dJ:compliance:thickness", "tee-uhat-penalty"): 9.03e-17, ("dJ:compliance:disp_solid", "tee-uhat-penalty"): 9.29e-16,
    ("dJ:elastic_energy:disp_solid", "tee-uhat-penalty"): 1.69e-15, ("dJ:elastic_energy:thickness", "tee-uhat-penalty"): 2.32e-16,
    # delaunay-uhat-penalty
    ("Ke", "delaunay-uhat-penalty"): 6.31e-14, ("Kx:uniform", "delaunay-uhat-penalty"): 5.04e-14, ("Kx:element", "delaunay-uhat-penalty"): 7.1e-14,
    ("Kx:free", "delaunay-uhat-penalty"): 5.45e-14, ("Kxvec:uniform", "delaunay-uhat-penalty"): 5.04e-14, ("diag", "delaunay-uhat-penalty"): 5.67e-14,
    ("residual", "delaunay-uhat-penalty"): 4.11e-14, ("load", "delaunay-uhat-penalty"): 4.61e-15, ("csr", "delaunay-uhat-penalty"): 5.67e-14,
    ("dRdT:thickness", "delaunay-uhat-penalty"): 3.16e-15, ("dRdT:E", "delaunay-uhat-penalty"): 3.24e-15, ("dRdT:nu", "delaunay-uhat-penalty"): 2.93e-15,
    ("dRdT:F_solid", "delaunay-uhat-penalty"): 1.23e-15, ("dJ:compliance:thickness", "delaunay-uhat-penalty"): 3.18e-15, ("dJ:compliance:disp_solid", "delaunay-uhat-penalty"): 7.81e-15,
    ("dJ:elastic_energy:disp_solid", "delaunay-uhat-penalty"): 4.12e-14, ("dJ:elastic_energy:thickness", "delaunay-uhat-penalty"): 7.82e-15,
    # delaunay-ewm-ewp-strong
    ("Ke", "delaunay-ewm-ewp-strong"): 6.03e-14, ("Kx:uniform", "delaunay-ewm-ewp-strong"): 2.92e-14, ("Kx:element", "delaunay-ewm-ewp-strong"): 7.8e-13,
    ("Kx:free", "delaunay-ewm-ewp-strong"): 4.25e-14, ("Kxvec:uniform", "delaunay-ewm-ewp-strong"): 2.92e-14, ("diag", "delaunay-ewm-ewp-strong"): 4e-14,
    ("residual", "delaunay-ewm-ewp-strong"): 2.5e-14, ("load", "delaunay-ewm-ewp-strong"): 9.33e-16, ("csr", "delaunay-ewm-ewp-strong"): 4e-14,
    ("dRdT:thickness", "delaunay-ewm-ewp-strong"): 6.3e-15, ("dRdT:E", "delaunay-ewm-ewp-strong"): 6.35e-15, ("dRdT:nu", "delaunay-ewm-ewp-strong"): 3.75e-15,
    ("dRdT:F_solid", "delaunay-ewm-ewp-strong"): 7.42e-16, ("dJ:compliance:thickness", "delaunay-ewm-ewp-strong"): 9.43e-16, ("dJ:compliance:disp_solid", "delaunay-ewm-ewp-strong"): 5.73e-16,
    ("dJ:elastic_energy:disp_solid", "delaunay-ewm-ewp-strong"): 2.43e-14, ("dJ:elastic_energy:thickness", "delaunay-ewm-ewp-strong"): 8.31e-15,
    # cg1-penalty
    ("Ke", "cg1-penalty"): 5.2e-15, ("Kx:uniform", "cg1-penalty"): 2.22e-15, ("Kx:element", "cg1-penalty"): 5.09e-15,
    ("Kx:free", "cg1-penalty"): 2.15e-15, ("Kxvec:uniform", "cg1-penalty"): 2.22e-15, ("diag", "cg1-penalty"): 2.81e-15,
    ("residual", "cg1-penalty"): 1.98e-15, ("load", "cg1-penalty"): 1.76e-15, ("csr", "cg1-penalty"): 2.81e-15,
    ("dRdT:thickness", "cg1-penalty"): 2.84e-16, ("dRdT:E", "cg1-penalty"): 2.99e-16, ("dRdT:nu", "cg1-penalty"): 1.96e-16,
    ("dRdT:F_solid", "cg1-penalty"): 1.33e-15, ("dJ:compliance:thickness", "cg1-penalty"): 3.37e-16, ("dJ:compliance:disp_solid", "cg1-penalty"): 1.75e-15,
    ("dJ:elastic_energy:disp_solid", "cg1-penalty"): 1.86e-15, ("dJ:elastic_energy:thickness", "cg1-penalty"): 4.46e-16,
    # cg1-uhat-strong
    ("Ke", "cg1-uhat-strong"): 4.58e-15, ("Kx:uniform", "cg1-uhat-strong"): 1.91e-15, ("Kx:element", "cg1-uhat-strong"): 2.95e-15,
    ("Kx:free", "cg1-uhat-strong"): 1.82e-15, ("Kxvec:uniform", "cg1-uhat-strong"): 1.91e-15, ("diag", "cg1-uhat-strong"): 2.98e-15,
    ("residual", "cg1-uhat-strong"): 2.49e-15, ("load", "cg1-uhat-strong"): 1.61e-15, ("csr", "cg1-uhat-strong"): 2.98e-15,
    ("dRdT:thickness", "cg1-uhat-strong"): 4.32e-16, ("dRdT:E", "cg1-uhat-strong"): 4.09e-16, ("dRdT:nu", "cg1-uhat-strong"): 2.85e-16,
    ("dRdT:F_solid", "cg1-uhat-strong"): 1.35e-15, ("dJ:compliance:thickness", "cg1-uhat-strong"): 3.37e-16, ("dJ:compliance:disp_solid", "cg1-uhat-strong"): 1.28e-15,
    ("dJ:elastic_energy:disp_solid", "cg1-uhat-strong"): 1.73e-15, ("dJ:elastic_energy:thickness", "cg1-uhat-strong"): 7.78e-16,
    # cr1-uhat-penalty
    ("Ke", "cr1-uhat-penalty"): 1.11e-13, ("Kx:uniform", "cr1-uhat-penalty"): 5.6e-14, ("Kx:element", "cr1-uhat-penalty"): 1.69e-13,
    ("Kx:free", "cr1-uhat-penalty"): 8.35e-14, ("Kxvec:uniform", "cr1-uhat-penalty"): 5.6e-14, ("diag", "cr1-uhat-penalty"): 8.59e-14,
    ("residual", "cr1-uhat-penalty"): 5.52e-14, ("load", "cr1-uhat-penalty"): 8.18e-15, ("csr", "cr1-uhat-penalty"): 8.59e-14,
    ("dRdT:thickness", "cr1-uhat-penalty"): 4.57e-15, ("dRdT:E", "cr1-uhat-penalty"): 4.6e-15, ("dRdT:nu", "cr1-uhat-penalty"): 1.72e-15,
    ("dRdT:F_solid", "cr1-uhat-penalty"): 9.09e-16, ("dJ:compliance:thickness", "cr1-uhat-penalty"): 2.32e-15, ("dJ:compliance:disp_solid", "cr1-uhat-penalty"): 8.55e-15,
    ("dJ:elastic_energy:disp_solid", "cr1-uhat-penalty"): 5.53e-14, ("dJ:elastic_energy:thickness", "cr1-uhat-penalty"): 7.84e-15,
    # cr1-strong
    ("Ke", "cr1-strong"): 7.74e-14, ("Kx:uniform", "cr1-strong"): 4.48e-14, ("Kx:element", "cr1-strong"): 1.76e-13,
    ("Kx:free", "cr1-strong"): 4.53e-14, ("Kxvec:uniform", "cr1-strong"): 4.48e-14, ("diag", "cr1-strong"): 5.33e-14,
    ("residual", "cr1-strong"): 4.78e-14, ("load", "cr1-strong"): 8.63e-16, ("csr", "cr1-strong"): 5.33e-14,
    ("dRdT:thickness", "cr1-strong"): 4.01e-15, ("dRdT:E", "cr1-strong"): 3.7e-15, ("dRdT:nu", "cr1-strong"): 2.06e-15,
    ("dRdT:F_solid", "cr1-strong"): 3.48e-16, ("dJ:compliance:thickness", "cr1-strong"): 2.32e-15, ("dJ:compliance:disp_solid", "cr1-strong"): 7.9e-16,
    ("dJ:elastic_energy:disp_solid", "cr1-strong"): 4.78e-14, ("dJ:elastic_energy:thickness", "cr1-strong"): 6.22e-15,
    # laminate
    ("Ke", "laminate"): 2.25e-14, ("Kx:uniform", "laminate"): 1.11e-14, ("Kx:element", "laminate"): 2.26e-14,
    ("Kx:free", "laminate"): 6.85e-15, ("Kxvec:uniform", "laminate"): 1.11e-14, ("diag", "laminate"): 1.67e-14,
    ("residual", "laminate"): 1.22e-14, ("load", "laminate"): 2.78e-15, ("csr", "laminate"): 1.67e-14,
    ("dRdT:laminate", "laminate"): 9.23e-15, ("dRdT:F_solid", "laminate"): 1.46e-15, ("dJ:compliance:thickness", "laminate"): 3.37e-16,
    ("dJ:compliance:disp_solid", "laminate"): 1.63e-15, ("dJ:elastic_energy:disp_solid", "laminate"): 1.22e-14, ("dJ:elastic_energy:laminate", "laminate"): 1.16e-14,
    # nred2
    ("Ke", "nred2"): 1.16e-14, ("Kx:uniform", "nred2"): 5.67e-15, ("Kx:element", "nred2"): 1.42e-14,
    ("Kx:free", "nred2"): 4.16e-15, ("Kxvec:uniform", "nred2"): 5.67e-15, ("diag", "nred2"): 8.12e-15,
    ("residual", "nred2"): 6.36e-15, ("load", "nred2"): 2.07e-15, ("csr", "nred2"): 8.12e-15,
    ("dRdT:thickness", "nred2"): 3.32e-16, ("dRdT:E", "nred2"): 3.89e-16, ("dRdT:nu", "nred2"): 2.74e-16,
    ("dRdT:F_solid", "nred2"): 1.39e-15, ("dJ:compliance:thickness", "nred2"): 3.37e-16, ("dJ:compliance:disp_solid", "nred2"): 1.75e-15,
    ("dJ:elastic_energy:disp_solid", "nred2"): 6.55e-15, ("dJ:elastic_energy:thickness", "nred2"): 1.14e-15,
    # transient
    ("Kx:uniform", "transient"): 2.84e-15, ("Kx:element", "transient"): 6.06e-15, ("Kx:free", "transient"): 2.42e-15,
    # prescribed
    ("load", "prescribed"): 2.78e-15, ("residual", "prescribed"): 2.51e-15,
    # fan70
    ("Ke", "fan70"): 1.81e-13, ("Kx:uniform", "fan70"): 1.15e-13, ("Kx:element", "fan70"): 3.3e-12,
    ("Kx:free", "fan70"): 1.13e-13, ("Kxvec:uniform", "fan70"): 1.15e-13, ("diag", "fan70"): 1.38e-13,
    ("residual", "fan70"): 1.15e-13, ("load", "fan70"): 1.2e-15, ("csr", "fan70"): 1.38e-13,
    ("dRdT:thickness", "fan70"): 7.45e-15, ("dRdT:E", "fan70"): 7.91e-15, ("dRdT:nu", "fan70"): 5.02e-15,
    ("dRdT:F_solid", "fan70"): 5.13e-16, ("dJ:compliance:thickness", "fan70"): 9.3e-15, ("dJ:compliance:disp_solid", "fan70"): 1.07e-15,
    ("dJ:elastic_energy:disp_solid", "fan70"): 1.16e-13, ("dJ:elastic_energy:thickness", "fan70"): 1.78e-14,
}
# case -> the quantities whose floor comes from the double-double assembly ("dd"); every other one is "ld"
REFERENCE_SOURCE = {
    "plate-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "warped-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "warped-ewm-ewp-strong": (),
    "warped-uhat-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "tri-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "tri-ewm-uhat-strong": (),
    "tee-uhat-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "delaunay-uhat-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "delaunay-ewm-ewp-strong": (),
    "cg1-penalty": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "cg1-uhat-strong": (),
    "cr1-uhat-penalty": (),
    "cr1-strong": (),
    "laminate": (),
    "nred2": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
    "transient": (),
    "prescribed": (),
    "fan70": ('Kx:uniform', 'Kx:element', 'Kx:free', 'Kxvec:uniform', 'diag', 'csr'),
}
# widened single constants: (quantity, case) -> (bound, the argument); none may reach 1e-12
WIDENED = {}


def bound(quantity, case):
    """What a kernel may differ from the oracle by: BOUND_FACTOR reference floors, or the widened constant with its argument."""
    if (quantity, case) in WIDENED:
        b = WIDENED[(quantity, case)][0]
        assert b < 1e-12
        return b
    return BOUND_FACTOR * REFERENCE_FLOOR[(quantity, case)]
