"""Laminate mode against the single-layer law at wing1m (BASELINE config 3, 1 015 470 DOF): forward solve (assembly + factorisation +
PCG refinement), the compliance gradient, and the element operator k_apply4 -- with its share of the fp64 vector peak from the flop
count below.  Both modes solve the same structure: the laminate is the per-cell isotropic-equivalent one (c_drill = E h^3), so the
factor, the iteration counts and the answers are those of the isotropic path and only the kernels differ.

    python scripts/bench_laminate.py [--reps 10] [--json out.json]

Kernel times per launch (k_apply4, k_front_assemble_fc) come from a run of its own under
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_laminate.py --reps 3
and the kernel_stats.csv it writes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6          # bench.py: MI355X fp64 vector peak
# fp64 operations per quadrature point of k_apply4: geometry 176, interpolation 24, constitutive 32, strains 390,
# stresses 21, transposed strains 382 = 1025.  The laminate law replaces the 32 of the single-layer constitutive step by
#   membrane / bending / coupling 6 x 6 symmetric products: 36 FMA = 72, their scaling by the measure: 6,
#   shear 2 x 2: 4 FMA = 8 plus its scaling 2, drilling c_drill * measure * omega: 2, measures (w_S det, w_S det J, w det J / h_K^2): 6
# and drops the thickness / E / nu interpolation (24) it no longer needs (the staged values are read as they are).
FLOPS_ISO = 1025
FLOPS_LAM = 1025 - 32 - 24 + (72 + 6 + 8 + 2 + 2 + 6)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(np.min(out))


def run(mode, reps):
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, _ = make_workload("wing1m")
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    h = float(fields["thickness"][0])
    clt = lm.isotropic(np.full(m.nel, h), float(fields["E"][0]), float(fields["nu"][0])) if mode == "laminate" else None
    if clt is not None:
        c.set_laminate(clt)
    c.use_direct_solver()
    arg = "laminate" if clt is not None else "thickness"

    upload = (lambda: c.set_field("laminate", clt)) if clt is not None else (lambda: c.set_field("thickness", fields["thickness"]))

    def forward_times(n):
        # a new design each time: the field is re-uploaded (untimed; marks the operator changed), then assembly + factorisation + solve
        t = []
        for _ in range(n):
            upload()
            t0 = time.perf_counter()
            c.solve_state(True)
            t.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(t)), float(np.min(t))
    forward_times(2)
    fwd = forward_times(reps)
    up = timed(upload, reps)
    grad = timed(lambda: c.total_gradient("compliance", arg), reps)
    apply_ms = c.bench_kernel("apply", 50)
    npts = c.quadrature()[1]
    flops = (FLOPS_LAM if clt is not None else FLOPS_ISO) * npts * m.nel
    res = dict(mode=mode, ndof=int(m.ndof), nel=int(m.nel), points_per_cell=int(npts), forward_ms_median=fwd[0], forward_ms_min=fwd[1],
               field_upload_ms_median=up[0], compliance_gradient_ms_median=grad[0], compliance_gradient_ms_min=grad[1],
               apply_ms=apply_ms, apply_flops=flops, apply_tflops=flops / apply_ms * 1e-9,
               apply_frac_fp64_vector_peak=flops / apply_ms * 1e-9 / FP64_PEAK_TFLOPS,
               compliance=float(c.functional("compliance")))
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for mode in ("isotropic", "laminate", "isotropic", "laminate"):        # alternated
        r = run(mode, a.reps)
        rows.append(r)
        print(json.dumps(r), flush=True)
    summary = {}
    for mode in ("isotropic", "laminate"):
        rs = [r for r in rows if r["mode"] == mode]
        summary[mode] = {k: float(np.min([r[k] for r in rs])) for k in ("forward_ms_median", "compliance_gradient_ms_median", "apply_ms")}
    ratio = summary["laminate"]["forward_ms_median"] / summary["isotropic"]["forward_ms_median"]
    summary["forward_ratio_laminate_over_isotropic"] = ratio
    print(json.dumps(summary))
    if a.json:
        json.dump(dict(rows=rows, summary=summary), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
