"""The reference of the layup's mass and volume (tests/layup_mass_ref.py) against the oracle's own mass: with an element-wise thickness
h = sum_k t_k and density rho = sum_k rho_k t_k / h the two are the same integral."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from femo_alpha_amd.mesh import quads_to_triangles, wing_skin_mesh               # noqa: E402
from layup_mass_ref import LayupMassRef                                          # noqa: E402
from oracle.rm_shell_oracle import ShellOracle                                   # noqa: E402

MESHES = {"warped": lambda: wing_skin_mesh(4, 8), "tri": lambda: quads_to_triangles(wing_skin_mesh(3, 6))}


@pytest.mark.parametrize("kind", list(MESHES))
@pytest.mark.parametrize("nply", [1, 3, 8])
def test_reference_equals_the_oracle_mass_of_the_smeared_plate(kind, nply):
    m = MESHES[kind]()
    rng = np.random.default_rng(nply)
    uhat = 0.02 * rng.uniform(-1, 1, (m.nn, 3))
    t = 0.05 / nply * (1 + 0.3 * rng.uniform(-1, 1, (m.nel, nply)))
    rho = rng.uniform(1000.0, 2000.0, nply)
    R = LayupMassRef(m, uhat)
    H = t.sum(axis=1)
    o = ShellOracle(m, element_wise_material=True)
    o.set_fields(h=H, rho=(t @ rho) / H, uhat=uhat)
    mass = o.mass()
    assert mass > 0
    assert abs(R.value(t, rho) - mass) <= 1e-13 * mass
    o.set_fields(rho=np.ones(m.nel))
    vol = o.mass()                                                                # int h J dx
    assert abs(R.value(t) - vol) <= 1e-13 * vol
    # the gradient is the value's: linear in t, restricted to the selected cells
    cells = np.arange(0, m.nel, 3)
    g = R.dthickness(nply, rho, cells)
    assert abs(np.sum(g * t) - R.value(t, rho, cells)) <= 1e-13 * mass
    assert np.all(g[np.setdiff1d(np.arange(m.nel), cells)] == 0.0) and np.all(g[cells] > 0.0)
    assert np.array_equal(R.dthickness(nply, None, cells) * rho[None, :], g)      # the volume's gradient: the same measure, unit densities
