"""The ply failure aggregate at wing1m (BASELINE config 3, 1 015 470 DOF) in laminate mode: the per-cell isotropic-equivalent laminate
split into 8 plies, recovery points at the bottom and top of every ply (npt = 16).

    python scripts/bench_ply_failure.py [--reps 10] [--json profiles/ply_failure_wing1m.json]

Host-side times (call to return, host copies included) of the value, dK/dw, dK/dtable and field calls, of
total_gradient("ply_failure", "laminate") beside total_gradient("compliance", "laminate") in the same process -- both do one adjoint
solve and one k_dRdlam_T, so their difference is the new dK/dw path (value pass, k_ply_failure<PF_DW>, k_gather_sum) against
k_dcompliance_du -- and of pnorm_stress (k_pnorm modes 0 / 1) on the same context as the nearest existing kernel.  Kernel times per
launch come from a run of its own under
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_ply_failure.py --reps 3
and the kernel_stats.csv it writes.  Compulsory bytes of the value kernel per cell: the table (16 npt doubles), the state (3 npc + 3 nvc
doubles) and the geometry (3 nvc doubles, nvc + npc indices)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=float(np.median(out)), min_ms=float(np.min(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nply", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, _ = make_workload("wing1m")
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    h, E, nu = float(fields["thickness"][0]), float(fields["E"][0]), float(fields["nu"][0])
    c.set_laminate(lm.isotropic(np.full(m.nel, h), E, nu))
    X = 3e8
    col = lambda v: np.full((m.nel, a.nply), v)
    tab = lm.ply_table(col(E), col(E), col(E / 2 / (1 + nu)), col(nu), col(h / a.nply), col(0.0), lm.tsai_wu(X, X, X, X, X / np.sqrt(3.0)))
    npt = tab.shape[1]
    res = dict(ndof=int(m.ndof), nel=int(m.nel), npt=int(npt))
    res["set_ply_table"] = timed(lambda: c.set_ply_table(tab), 3)
    c.use_direct_solver()
    c.solve_state(True)
    res["forward_solve_with_table"] = timed(lambda: (c.set_field("laminate", c.get_field("laminate")), c.solve_state(True)), a.reps)
    fld = c.ply_failure_field()
    c.set_ply_failure_params(20.0 / fld.max())
    res["max_failure_index"] = float(fld.max())
    res["ply_failure"] = float(c.functional("ply_failure"))
    res["value"] = timed(lambda: c.functional("ply_failure"), a.reps)
    res["field"] = timed(lambda: c.ply_failure_field(), a.reps)
    res["dK_dw"] = timed(lambda: c.dfunctional("ply_failure", "disp_solid"), a.reps)
    res["dK_dtable"] = timed(lambda: c.dfunctional("ply_failure", "ply_table"), a.reps)
    res["pnorm_value"] = timed(lambda: c.functional("pnorm_stress"), a.reps)
    res["pnorm_dw"] = timed(lambda: c.dfunctional("pnorm_stress", "disp_solid"), a.reps)
    for _ in range(2):                                            # alternated
        for fn in ("compliance", "ply_failure"):
            t = timed(lambda: c.total_gradient(fn, "laminate"), a.reps)
            key = f"total_gradient_{fn}_laminate"
            res[key] = t if key not in res or t["median_ms"] < res[key]["median_ms"] else res[key]
    res["total_gradient_difference_ms"] = res["total_gradient_ply_failure_laminate"]["median_ms"] - \
        res["total_gradient_compliance_laminate"]["median_ms"]
    npc, nvc = m.cell_p2.shape[1], m.nvc
    bytes_cell = 8 * (16 * npt + 3 * npc + 3 * nvc + 3 * nvc) + 4 * (npc + nvc)
    res["value_kernel_compulsory_bytes"] = int(bytes_cell * m.nel)
    res["value_kernel_ms_at_hbm_peak"] = bytes_cell * m.nel / (HBM_PEAK_GBS * 1e9) * 1e3
    c.close()
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
