"""The CSDL stand-in's reverse sweep through explicit operations whose output has several entries (a field output such as
``stress``): compute_totals propagates J^T bar for a dense or a scipy-sparse partial J, and the scalar branch is unchanged.
No GPU: a toy explicit operation in numpy."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import csdl_standin as csdl  # noqa: E402

A = np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 3.0], [4.0, 0.0, 0.5], [0.0, 0.0, 2.0]])


class _Linear(csdl.CustomExplicitOperation):
    """y = A x (4 entries) with the partial handed back dense or sparse."""

    def __init__(self, sparse):
        super().__init__()
        self.sparse = sparse

    def evaluate(self, x):
        self.declare_input("x", x)
        y = self.create_output("y", (A.shape[0],))
        self.declare_derivative_parameters("y", "*", dependent=True)
        self._finish_evaluate()
        return y

    def compute(self, input_vals, output_vals):
        output_vals["y"] = A @ input_vals["x"]

    def compute_derivatives(self, input_vals, output_vals, derivatives):
        derivatives["y", "x"] = sp.csr_matrix(A) if self.sparse else A.copy()


class _Norm2(csdl.CustomExplicitOperation):
    """s = |x|^2 (one entry): its partial is a gradient vector, taken by the scalar branch."""

    def evaluate(self, x):
        self.declare_input("x", x)
        s = self.create_output("s", (1,))
        self.declare_derivative_parameters("s", "*", dependent=True)
        self._finish_evaluate()
        return s

    def compute(self, input_vals, output_vals):
        output_vals["s"] = np.array([input_vals["x"] @ input_vals["x"]])

    def compute_derivatives(self, input_vals, output_vals, derivatives):
        derivatives["s", "x"] = 2.0 * input_vals["x"]


@pytest.mark.parametrize("sparse", [False, True])
def test_vector_output_propagates_the_transposed_jacobian(sparse):
    rec = csdl.Recorder(inline=True).start()
    x = csdl.Variable(value=np.array([0.3, -1.2, 2.0]), name="x")
    y = _Linear(sparse).evaluate(x)
    of = y[2]                                   # one entry of the field: d of / d x = row 2 of A
    w = y * 3.0                                 # an expression of the whole field, through the unary view
    s = _Norm2().evaluate(w)
    rec.stop()
    assert np.array_equal(rec.compute_totals(of, x), A[2])
    g = rec.compute_totals(s, x)                # d |3 A x|^2 / d x = A^T (18 A x)
    assert np.allclose(g, A.T @ (18.0 * (A @ x.value)), rtol=1e-14, atol=0)
    rows = rec.check_totals(of, x, step=1e-6)
    assert all(r[3] < 1e-8 for r in rows)


def test_scalar_branch_is_unchanged():
    rec = csdl.Recorder(inline=True).start()
    x = csdl.Variable(value=np.array([0.5, -2.0, 1.5, 4.0]), name="x")
    s = _Norm2().evaluate(x)
    t = s * 2.5
    rec.stop()
    assert np.array_equal(rec.compute_totals(s, x), 2.0 * x.value)
    assert np.array_equal(rec.compute_totals(t, x), 2.5 * (2.0 * x.value))
