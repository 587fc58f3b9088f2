"""The shape-sensitivity kernels against the extended-precision reference of tests/shape_ref.py, entry by entry: the dual-number kernels of
shape_sens.h ((dR/duhat)^T lambda; d/duhat of compliance, mass and elastic_energy), the uhat branch of the p-norm stress gradient and
the uhat direction of femo_residual_jvp -- on every small case with mesh motion, each with its own clamp (penalty facets at beta = 1e15),
at every vertex and every row.  The reference, its uncertainty and its scale come from tests/golden/shape_sens.npz
(tests/golden/make_shape_goldens.py); nothing is differenced here.

  shape_scaled(value, golden, scale) <= parity_metrics.BOUND_FACTOR * SHAPE_FLOOR[(quantity, case)]

The factor of 50 has the reason parity_metrics.py gives -- the kernels add the same terms over 9-25 points and up to 39 columns in another
order -- and here also the dual part of each operation.  tests/test_shape_ref_cpu.py holds the golden's own uncertainty below a tenth of
each bound.  The finite-difference tests of test_gpu_parity.py (three random vertices, beta = 1e6, re-solves) stay beside this one.

Every value is printed as ``shape <case> <quantity> <value>`` before anything is asserted.

Measured on the MI355X (shape_scaled; bound):
  warped-uhat-penalty      dRdT:uhat                    2.093e-15   7.10e-14
  warped-uhat-penalty      dJ:compliance:uhat           6.727e-16   4.06e-14
  warped-uhat-penalty      dJ:mass:uhat                 1.268e-15   1.07e-13
  warped-uhat-penalty      dJ:elastic_energy:uhat       3.638e-15   8.95e-14
  warped-uhat-penalty      dJ:pnorm_stress:uhat         6.381e-14   7.40e-13
  warped-uhat-penalty      dJ:pnorm_stress:uhat@reg     6.402e-14   7.40e-13
  warped-uhat-penalty      jvp:uhat:dense               1.129e-14   2.57e-13
  warped-uhat-penalty      jvp:uhat:clamp               2.862e-15   2.57e-13
  tri-ewm-uhat-strong      dJ:compliance:uhat           7.968e-16   1.38e-13
  tri-ewm-uhat-strong      dJ:mass:uhat                 1.562e-15   4.48e-13
  tri-ewm-uhat-strong      dJ:elastic_energy:uhat       4.728e-15   1.64e-12
  tri-ewm-uhat-strong      dJ:pnorm_stress:uhat         1.150e-13   1.13e-11
  tri-ewm-uhat-strong      jvp:uhat:dense               2.358e-14   3.26e-12
  tri-ewm-uhat-strong      jvp:uhat:clamp               3.476e-15   3.26e-12
  tee-uhat-penalty         dJ:compliance:uhat           6.018e-16   1.23e-14
  tee-uhat-penalty         dJ:mass:uhat                 7.258e-16   2.56e-14
  tee-uhat-penalty         dJ:elastic_energy:uhat       2.070e-15   7.90e-14
  tee-uhat-penalty         dJ:pnorm_stress:uhat         1.713e-14   5.65e-13
  tee-uhat-penalty         jvp:uhat:dense               3.636e-15   1.18e-13
  tee-uhat-penalty         jvp:uhat:clamp               2.227e-15   1.18e-13
  delaunay-uhat-penalty    dJ:compliance:uhat           7.666e-16   2.92e-13
  delaunay-uhat-penalty    dJ:mass:uhat                 2.371e-15   6.05e-13
  delaunay-uhat-penalty    dJ:elastic_energy:uhat       1.303e-14   1.41e-12
  delaunay-uhat-penalty    dJ:pnorm_stress:uhat         2.260e-13   8.75e-12
  delaunay-uhat-penalty    dJ:pnorm_stress:uhat@sub     3.180e-13   8.75e-12
  delaunay-uhat-penalty    jvp:uhat:dense               5.343e-14   2.70e-12
  delaunay-uhat-penalty    jvp:uhat:clamp               2.620e-15   2.70e-12
  cg1-uhat-strong          dJ:compliance:uhat           6.305e-16   5.60e-14
  cg1-uhat-strong          dJ:mass:uhat                 1.268e-15   1.07e-13
  cg1-uhat-strong          dJ:elastic_energy:uhat       2.944e-15   1.49e-13
  cg1-uhat-strong          dJ:pnorm_stress:uhat         1.706e-13   8.00e-13
  cg1-uhat-strong          jvp:uhat:dense               5.444e-15   1.84e-13
  cg1-uhat-strong          jvp:uhat:clamp               1.598e-15   1.84e-13
  cr1-uhat-penalty         dJ:compliance:uhat           8.373e-16   3.84e-13
  cr1-uhat-penalty         dJ:mass:uhat                 2.509e-15   8.10e-13
  cr1-uhat-penalty         dJ:elastic_energy:uhat       7.253e-15   1.89e-12
  cr1-uhat-penalty         dJ:pnorm_stress:uhat         2.550e-13   1.62e-11
  cr1-uhat-penalty         jvp:uhat:dense               3.596e-14   3.51e-12
  cr1-uhat-penalty         jvp:uhat:clamp               7.948e-15   3.51e-12
  laminate                 dJ:compliance:uhat           6.727e-16   4.06e-14
  laminate                 dJ:mass:uhat                 1.268e-15   1.07e-13
  laminate                 dJ:elastic_energy:uhat       4.079e-15   1.94e-13
  laminate                 dJ:pnorm_stress:uhat         6.381e-14   7.40e-13
  laminate                 jvp:uhat:dense               2.769e-14   7.05e-13
  laminate                 jvp:uhat:clamp               4.376e-15   7.05e-13
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowscaled_cases as rc         # noqa: E402
import shape_ref as sr               # noqa: E402

pytestmark = pytest.mark.gpu

_golden = {}


def _gold():
    if not _golden:
        _golden.update(sr.load_golden())
    return _golden


def device_values(k):
    """quantity -> what the device computes, for the quantities of the case; the context is left as it was built."""
    c, name = k.c, k.name
    c.set_state(k.w)
    c.set_stress_params(sr.STRESS_M, sr.STRESS_RHO)
    v = {}
    for q in sr.quantities(name):
        if q == "dRdT:uhat":
            v[q] = c.dRdarg_T("uhat", k.lam)
        elif q == "dJ:pnorm_stress:uhat@reg":
            c.set_option("stress_regularization", sr.STRESS_REG)
            try:
                v[q] = c.dfunctional("pnorm_stress", "uhat")
            finally:
                c.set_option("stress_regularization", 0.0)
        elif q == "dJ:pnorm_stress:uhat@sub":
            tags = -np.ones(k.m.nel, dtype=np.int32)
            tags[sr.subdomain_cells(k)] = 0
            c.set_cell_tags(tags, 1)
            c.select_subdomain(0)
            try:
                v[q] = c.dfunctional("pnorm_stress", "uhat")
            finally:
                c.select_subdomain(-1)
        elif q.startswith("dJ:"):
            v[q] = c.dfunctional(q.split(":")[1], "uhat")
        elif q.startswith("jvp:"):
            v[q] = c.dRdarg("uhat", sr.directions(k)[q].ravel())
        else:
            raise KeyError(q)
    return v


@pytest.mark.parametrize("name", sr.CASES)
def test_every_entry_within_fifty_floors_of_the_extended_reference(name):
    k = rc.build(name)
    try:
        values = device_values(k)
    finally:
        k.c.close()
    assert set(values) == set(sr.quantities(name))
    over = []
    for q, value in values.items():
        ref, unc, scale = _gold()[(name, q)]
        e, b = sr.shape_scaled(value, ref, scale), sr.bound(q, name)
        print(f"shape {name} {q} {e:.3e}   (bound {b:.2e}, floor {sr.SHAPE_FLOOR[(q, name)]:.2e})")
        if not e <= b:
            over.append((q, e, b))
    if name == sr.SUBDOMAIN:
        # outside the selection the gradient is exact zeros (its scale is zero there: the metric has already demanded it)
        ref, unc, scale = _gold()[(name, "dJ:pnorm_stress:uhat@sub")]
        outside = np.setdiff1d(np.arange(k.m.nn), np.unique(k.m.cells[sr.subdomain_cells(k)]))
        assert outside.size > 0 and np.all(scale[outside] == 0.0)
        assert np.all(values["dJ:pnorm_stress:uhat@sub"].reshape(-1, 3)[outside] == 0.0)
    assert not over, over
