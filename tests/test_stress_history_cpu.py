"""CPU-side checks of the space-time stress aggregate of the transient path (femo_newmark_stress_history*): the entries are declared,
listed in the ctypes table, exported by the built library and named in INTEGRATION.md; the operation and the PlateSim / ShellContext
methods exist.  No compute call is made without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["femo_newmark_stress_history", "femo_newmark_stress_history_grad", "femo_newmark_adjoint_seeded"]


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
    from femo_alpha_amd.dynamic_rm_shell.operations import StressHistoryOperation
    from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
    assert callable(StressHistoryOperation.compute) and callable(StressHistoryOperation.compute_derivatives)
    for m in ("newmark_stress_history", "newmark_stress_history_grad", "newmark_adjoint_seeded"):
        assert callable(getattr(ShellContext, m)), m
    for m in ("pnorm_stress_history", "pnorm_stress_history_partials", "pnorm_stress_history_total_gradient"):
        assert callable(getattr(PlateSim, m)), m


def test_plate_sim_still_fails_loudly_without_a_gpu():
    from femo_alpha_amd import _lib
    from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
    from femo_alpha_amd.mesh import plate_mesh
    if _lib.load().femo_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.FemoHipError, match="no CPU fallback"):
        PlateSim(plate_mesh(2.0, 10.0, 2, 4), 1e8, 0.3, 10.0, 0.01, 4)
