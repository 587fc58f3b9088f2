"""Reverse mode of the ply failure field on the 1 M-DOF wing (the workload of scripts/bench_layup.py: 67 280 cells, 8 plies, recovery
points at the bottom and top of every ply), one GPU, one process:

  (a) the state-mode product (d field / d w)^T cbar -- k_ply_field_vjp and the gather -- beside the aggregate's state gradient as
      femo_dfunctional("ply_failure", "disp_solid") enqueues it (value pass, PF_DW, gather) and beside that value pass alone: device
      events around back-to-back launches (femo_bench_kernel).  Both read the table once, the state, and write and gather one element
      vector per cell;
  (b) field_total_gradients with 4 cotangents with respect to "ply_thickness" (one grouped adjoint solve), beside four single-cotangent
      calls and beside total_gradient("ply_failure", "ply_thickness"): a host clock around calls that end in a device synchronise.

Medians of ``--reps`` calls after a warm-up.  Achieved bytes/s are the kernels' own traffic over the kernel time.  Writes
profiles/ply_field_reverse.txt (``--out``); ``--resource-log`` takes the output of a build of csrc/femo_hip.hip with
``-Rpass-analysis=kernel-resource-usage`` and puts the lines of the new kernels in front (without it an existing section is kept).

    python scripts/bench_ply_field_reverse.py [--reps 21] [--resource-log build.log] [--out profiles/ply_field_reverse.txt]
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLY = dict(E1=1.35e11, E2=1.0e10, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)
STRENGTH = dict(Xt=1.5e9, Xc=1.2e9, Yt=5e7, Yc=2e8, S=7e7)
PF = "ply_failure_field"
RES_HEAD = "resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)"
RES_END = "end of resource usage"


def median_ms(fn, reps):
    fn()                                                       # warm-up: code objects, buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def resource_lines(log):
    """One line per instantiation of k_ply_field_vjp / k_ply_field_jac from the compiler's remarks."""
    rows, cur = [], None
    with open(log) as fh:
        for line in fh:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = {"name": m.group(1)}
                rows.append(cur)
                continue
            m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    out = []
    for r in rows:
        m = re.match(r"_ZN4femo15k_ply_field_(vjp|jac)ILi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)EE", r["name"])
        if not m:
            continue
        kind, npc, nvc, quad, uhat, table = m.groups()
        tf = lambda b: "true" if b == "1" else "false"
        out.append(f"k_ply_field_{kind}<{npc}, {nvc}, {tf(quad)}, {tf(uhat)}, {'TABLE' if table == '1' else 'STATE'}>  VGPRs {r['VGPRs']:>3}  "
                   f"SGPRs {r['TotalSGPRs']:>3}  LDS {r['LDS Size [bytes/block]']:>5} B  scratch {r['ScratchSize [bytes/lane]']} B/lane  "
                   f"{r['Occupancy [waves/SIMD]']} waves/SIMD")
    return out


def kept_resource_lines(path):
    if not os.path.exists(path):
        return []
    with open(path) as fh:
        lines = fh.read().splitlines()
    if RES_HEAD in lines and RES_END in lines:
        return lines[lines.index(RES_HEAD) + 1: lines.index(RES_END)]
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_field_reverse.txt"))
    a = ap.parse_args()
    res = resource_lines(a.resource_log) if a.resource_log else kept_resource_lines(a.out)
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(a.workload)
    nel, nply, surfaces = m.nel, 8, ("bot", "top")
    npt = nply * len(surfaces)
    rng = np.random.default_rng(0)
    t = 1.27e-3 / nply * (1 + 0.2 * rng.uniform(-1, 1, (nel, nply)))
    theta = np.tile([0.0, 45.0, -45.0, 90.0, 90.0, -45.0, 45.0, 0.0], (nel, 1)) + rng.uniform(-5, 5, (nel, nply))
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.use_direct_solver()
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, surfaces)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    ld = 3 * m.npc + 3 * m.nvc
    lines = [RES_HEAD] + res + [RES_END, "",
             f"reverse mode of the ply failure field, {desc}",
             f"{nel} cells, {nply} plies, {npt} recovery points per cell; {a.reps} repetitions, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))

    # ---------------------------------------------------------------- (a) the state-mode product beside the aggregate's
    kr = 200
    k_val, k_dw = c.bench_kernel("ply_value", kr), c.bench_kernel("ply_dw", kr)
    k_vjp, k_tab = c.bench_kernel("ply_field_vjp", kr), c.bench_kernel("ply_field_vjp_table", kr)
    # table and state in, element vector out and in again through the gather, the gathered vector out (+ the cotangent for the field)
    b_state = nel * (16 * npt + ld + 2 * ld) * 8 + m.ndof * 8
    b_vjp = b_state + nel * npt * 8
    b_tab = nel * (16 * npt + ld + npt + 16 * npt) * 8
    say(f"(a) aggregate  value pass (k_ply_failure<PF_VALUE>, combine)      {1e3 * k_val:9.1f} us")
    say(f"(a) aggregate  state gradient as dfunctional enqueues it          {1e3 * k_dw:9.1f} us   (value pass, PF_DW, gather)")
    say(f"(a) aggregate  PF_DW and gather alone (the difference)            {1e3 * (k_dw - k_val):9.1f} us   "
        f"{b_state / 1e6:.1f} MB of their own traffic: {b_state / ((k_dw - k_val) * 1e-3) / 1e12:.2f} TB/s")
    say(f"(a) field      k_ply_field_vjp (state) and gather                 {1e3 * k_vjp:9.1f} us   "
        f"{b_vjp / 1e6:.1f} MB of their own traffic: {b_vjp / (k_vjp * 1e-3) / 1e12:.2f} TB/s")
    say(f"(a) field product / aggregate (PF_DW and gather)                  {k_vjp / (k_dw - k_val):9.2f} x")
    say(f"(a) field      k_ply_field_vjp (table)                            {1e3 * k_tab:9.1f} us   "
        f"{b_tab / 1e6:.1f} MB of its own traffic: {b_tab / (k_tab * 1e-3) / 1e12:.2f} TB/s")
    cb = rng.uniform(-1, 1, (4, nel * npt))
    say("(a) call  dfunctional('ply_failure', 'disp_solid') (gradient out)           %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.dfunctional("ply_failure", "disp_solid"), a.reps))
    say("(a) call  field_output_vjp(field, 'disp_solid') (cotangent in, product out) %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.field_output_vjp(PF, "disp_solid", cb[0]), a.reps))

    # ---------------------------------------------------------------- (b) grouped totals with respect to the ply thicknesses
    g4 = [None]

    def grouped():
        g4[0] = c.field_total_gradients(PF, cb, "ply_thickness")[0]
    t4 = median_ms(grouped, a.reps)
    g1 = [None]

    def singles():
        g1[0] = np.array([c.field_total_gradients(PF, cb[k], "ply_thickness")[0][0] for k in range(4)])
    t1 = median_ms(singles, a.reps)
    tagg = median_ms(lambda: c.total_gradient("ply_failure", "ply_thickness"), a.reps)
    say("(b) field_total_gradients(field, 4 cotangents, 'ply_thickness')   %9.2f ms (%.2f .. %.2f)" % t4)
    say("(b) four calls with one cotangent each                            %9.2f ms (%.2f .. %.2f)" % t1)
    say("(b) total_gradient('ply_failure', 'ply_thickness')                %9.2f ms (%.2f .. %.2f)" % tagg)
    say(f"(b) grouped / four singles {t4[0] / t1[0]:.2f} x; grouped / one aggregate total {t4[0] / tagg[0]:.2f} x; "
        f"agreement of the two routes {np.abs(g4[0] - g1[0]).max() / np.abs(g1[0]).max():.1e} of the largest entry")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
