"""Ply strength index aggregate on the 1 M-DOF wing (the workload of scripts/bench_layup.py: 67 280 cells, 8 plies, 16 recovery
points: bottom and top of every ply), one GPU, one process.  Every pass of "ply_strength_index" is measured alternately, round by
round, with its "ply_failure" counterpart, which reads the same bytes; the new passes add one fp64 square root and one division per
(quadrature point, recovery point):

  (a) device events around back-to-back launches (femo_bench_kernel): the value pass with its combine, the state gradient as
      femo_dfunctional enqueues it (value pass, gradient kernel, gather) and the table product (value pass, table kernel);
  (b) a host clock around calls that end in a device synchronise: total_gradient(., "ply_thickness") of both outputs.

Medians of ``--reps`` rounds after a warm-up.  Writes profiles/ply_strength.txt (``--out``); ``--resource-log`` takes the output of a
build of csrc/femo_hip.hip with ``-Rpass-analysis=kernel-resource-usage`` and puts the lines of the new kernels, and of the
k_ply_failure instantiations the wing runs, in front (without it an existing section is kept).  Lines after the measurements that
start with "forward solve" and what follows them (the comparison of bench.py with the parent commit, written by hand) are kept.

    python scripts/bench_ply_strength.py [--reps 21] [--resource-log build.log] [--out profiles/ply_strength.txt]
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLY = dict(E1=1.35e11, E2=1.0e10, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)
STRENGTH = dict(Xt=1.5e9, Xc=1.2e9, Yt=5e7, Yc=2e8, S=7e7)
RES_HEAD = "resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)"
RES_END = "end of resource usage"
TAIL_HEAD = "forward solve"
MODES = {"0": "VALUE", "1": "FIELD", "2": "DW", "3": "DTABLE"}


def timed_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def resource_lines(log):
    """One line per instantiation of k_ply_strength, per k_ply_failure instantiation of the 9-node quadrilateral, and for the table
    check, from the compiler's remarks."""
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
    tf = lambda b: "true" if b == "1" else "false"
    for r in rows:
        m = re.match(r"_ZN4femo\d+(k_ply_strength|k_ply_failure)ILi(\d)ELi(\d)ELb(\d)ELb(\d)ELi(\d)EE", r["name"])
        if m:
            kern, npc, nvc, quad, uhat, mode = m.groups()
            if kern == "k_ply_failure" and npc != "9":
                continue
            name = f"{kern}<{npc}, {nvc}, {tf(quad)}, {tf(uhat)}, {'PSI' if kern == 'k_ply_strength' else 'PF'}_{MODES[mode]}>"
        elif re.match(r"_ZN4femo\d+k_ply_psd_checkE", r["name"]):
            name = "k_ply_psd_check"
        else:
            continue
        out.append(f"{name}  VGPRs {r['VGPRs']:>3}  AGPRs {r['AGPRs']:>3}  SGPRs {r['TotalSGPRs']:>3}  LDS {r['LDS Size [bytes/block]']:>5} B  "
                   f"scratch {r['ScratchSize [bytes/lane]']} B/lane  {r['Occupancy [waves/SIMD]']} waves/SIMD")
    return out


def kept_lines(path):
    """(resource section, hand-written tail) of an existing file."""
    if not os.path.exists(path):
        return [], []
    with open(path) as fh:
        lines = fh.read().splitlines()
    res = lines[lines.index(RES_HEAD) + 1: lines.index(RES_END)] if RES_HEAD in lines and RES_END in lines else []
    tail = next((lines[i:] for i, s in enumerate(lines) if s.startswith(TAIL_HEAD)), [])
    return res, tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_strength.txt"))
    a = ap.parse_args()
    res, tail = kept_lines(a.out)
    if a.resource_log:
        res = resource_lines(a.resource_log)
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(a.workload)
    nel, nply = m.nel, 8
    rng = np.random.default_rng(0)
    t = 1.27e-3 / nply * (1 + 0.2 * rng.uniform(-1, 1, (nel, nply)))
    theta = np.tile([0.0, 45.0, -45.0, 90.0, 90.0, -45.0, 45.0, 0.0], (nel, 1)) + rng.uniform(-5, 5, (nel, nply))
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.use_direct_solver()
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, ("bot", "top"))
    c.solve_state(True)
    fi, r = c.ply_failure_field(), c.ply_strength_index_field()
    # one exponent for both aggregates, rho times the larger index of order 5: every point contributes to both
    c.set_ply_failure_params(5.0 / max(np.abs(fi).max(), r.max()))
    npt = 2 * nply
    lines = [RES_HEAD] + res + [RES_END, "",
             f"ply strength index aggregate beside ply_failure, {desc}",
             f"{nel} cells, {nply} plies, {npt} recovery points of 16 doubles; largest failure index {np.abs(fi).max():.3e}, largest strength "
             f"index {r.max():.3e}; {a.reps} rounds, each pass alternating with its counterpart, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    fmt = lambda v, u: f"{np.median(v):9.2f} {u} ({np.min(v):.2f} .. {np.max(v):.2f})"

    kr = 50
    pairs = (("value pass (value kernel, combine)", "ply_strength_value", "ply_value"),
             ("state gradient (value pass, DW kernel, gather)", "ply_strength_dw", "ply_dw"),
             ("table product (value pass, DTABLE kernel)", "ply_strength_dtable", "ply_dtable"))
    for what, new, old in pairs:
        for n in (new, old):
            c.bench_kernel(n, kr)                              # warm-up
        T = {new: [], old: []}
        for _ in range(a.reps):
            for n in (new, old):
                T[n].append(1e3 * c.bench_kernel(n, kr))       # us
        say(f"(a) {what}")
        say(f"      ply_strength_index {fmt(T[new], 'us')}   ply_failure {fmt(T[old], 'us')}   ratio {np.median(T[new]) / np.median(T[old]):.2f}")
    calls = {n: (lambda n=n: c.total_gradient(n, "ply_thickness")) for n in ("ply_strength_index", "ply_failure")}
    for fn in calls.values():
        fn()                                                   # warm-up
    T = {n: [] for n in calls}
    for _ in range(a.reps):
        for n, fn in calls.items():
            T[n] += timed_ms(fn, 1)
    say("(b) call  total_gradient(., 'ply_thickness')")
    say(f"      ply_strength_index {fmt(T['ply_strength_index'], 'ms')}   ply_failure {fmt(T['ply_failure'], 'ms')}   "
        f"ratio {np.median(T['ply_strength_index']) / np.median(T['ply_failure']):.2f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + ([""] + tail if tail else [])) + "\n")
    c.close()


if __name__ == "__main__":
    main()
