"""Hashin fibre and matrix aggregates on the 1 M-DOF wing (the workload of scripts/bench_ply_strength.py: 67 280 cells, 8 plies, 16
recovery points: bottom and top of every ply), one GPU, one process.  Every pass of "ply_hashin_fibre" and "ply_hashin_matrix" is
measured alternately, round by round, with its "ply_failure" counterpart.  A Hashin pass reads 10 entries of the ply table and the
strengths of its index (2 for the fibre, 4 for the matrix) where ply_failure reads 16 entries, and evaluates the same number of
exponentials:

  (a) device events around back-to-back launches (femo_bench_kernel): the value pass with its combine, the state gradient as
      femo_dfunctional enqueues it (value pass, gradient kernel, gather) and the table product (value pass, table kernel);
  (b) a host clock around calls that end in a device synchronise: total_gradient(., "ply_thickness") of the three outputs.

Medians of ``--reps`` rounds after a warm-up.  Writes profiles/ply_hashin.txt (``--out``); ``--resource-log`` takes the output of a
build of csrc/femo_hip.hip with ``-Rpass-analysis=kernel-resource-usage`` and puts the lines of the new kernels, and of the
k_ply_failure instantiations the wing runs, in front (without it an existing section is kept).  Lines after the measurements that
start with "forward solve" and what follows them (the comparison of bench.py with the parent commit, written by hand) are kept.

    python scripts/bench_ply_hashin.py [--reps 21] [--resource-log build.log] [--out profiles/ply_hashin.txt]
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ply_strength import PLY, RES_END, RES_HEAD, STRENGTH, kept_lines, timed_ms      # noqa: E402

MODES = {"0": "VALUE", "1": "FIELD", "2": "DW", "3": "DTABLE"}
NAMES = ("ply_hashin_fibre", "ply_hashin_matrix", "ply_failure")


def resource_lines(log):
    """One line per instantiation of k_ply_hashin, per k_ply_failure instantiation of the 9-node quadrilateral, and for the check of
    the strengths, from the compiler's remarks."""
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
        h = re.match(r"_ZN4femo\d+k_ply_hashinILi(\d)ELi(\d)ELb(\d)ELb(\d)ELi(\d)ELi(\d)EE", r["name"])
        f = re.match(r"_ZN4femo\d+k_ply_failureILi(\d)ELi(\d)ELb(\d)ELb(\d)ELi(\d)EE", r["name"])
        if h:
            npc, nvc, quad, uhat, mode, idx = h.groups()
            name = f"k_ply_hashin<{npc}, {nvc}, {tf(quad)}, {tf(uhat)}, PH_{MODES[mode]}, {'PH_FIBRE' if idx == '0' else 'PH_MATRIX'}>"
        elif f and f.group(1) == "9":
            npc, nvc, quad, uhat, mode = f.groups()
            name = f"k_ply_failure<{npc}, {nvc}, {tf(quad)}, {tf(uhat)}, PF_{MODES[mode]}>"
        elif re.match(r"_ZN4femo\d+k_hashin_checkE", r["name"]):
            name = "k_hashin_check"
        else:
            continue
        out.append(f"{name}  VGPRs {r['VGPRs']:>3}  AGPRs {r['AGPRs']:>3}  SGPRs {r['TotalSGPRs']:>3}  LDS {r['LDS Size [bytes/block]']:>5} B  "
                   f"scratch {r['ScratchSize [bytes/lane]']} B/lane  {r['Occupancy [waves/SIMD]']} waves/SIMD")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_hashin.txt"))
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
    ply = dict(PLY, **STRENGTH, ST=0.35 * STRENGTH["Yc"])
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, ("bot", "top"), hashin=ply)
    c.solve_state(True)
    fi = c.ply_failure_field()
    ff, fm = c.ply_hashin_field()
    # one exponent for the three aggregates, rho times the largest index of order 5: every point contributes
    c.set_ply_failure_params(5.0 / max(np.abs(fi).max(), ff.max(), fm.max()))
    npt = 2 * nply
    lines = [RES_HEAD] + res + [RES_END, "",
             f"Hashin fibre and matrix aggregates beside ply_failure, {desc}",
             f"{nel} cells, {nply} plies, {npt} recovery points of 16 doubles and 6 strengths; largest Tsai-Wu index {np.abs(fi).max():.3e}, "
             f"largest fibre index {ff.max():.3e}, largest matrix index {fm.max():.3e} (smallest {fm.min():.3e}); {a.reps} rounds, the passes of the "
             f"three outputs alternating, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    fmt = lambda v, u: f"{np.median(v):9.2f} {u} ({np.min(v):.2f} .. {np.max(v):.2f})"

    def report(T, unit):
        for n in NAMES:
            ratio = "" if n == "ply_failure" else f"   ratio {np.median(T[n]) / np.median(T['ply_failure']):.2f}"
            say(f"      {n:<18} {fmt(T[n], unit)}{ratio}")

    kr = 50
    passes = (("value pass (value kernel, combine)", "value", "ply_value"),
              ("state gradient (value pass, DW kernel, gather)", "dw", "ply_dw"),
              ("table product (value pass, DTABLE kernel)", "dtable", "ply_dtable"))
    for what, suffix, old in passes:
        kern = {"ply_hashin_fibre": "ply_hashin_fibre_" + suffix, "ply_hashin_matrix": "ply_hashin_matrix_" + suffix, "ply_failure": old}
        for n in NAMES:
            c.bench_kernel(kern[n], kr)                        # warm-up
        T = {n: [] for n in NAMES}
        for _ in range(a.reps):
            for n in NAMES:
                T[n].append(1e3 * c.bench_kernel(kern[n], kr))  # us
        say(f"(a) {what}")
        report(T, "us")
    calls = {n: (lambda n=n: c.total_gradient(n, "ply_thickness")) for n in NAMES}
    for fn in calls.values():
        fn()                                                   # warm-up
    T = {n: [] for n in NAMES}
    for _ in range(a.reps):
        for n, fn in calls.items():
            T[n] += timed_ms(fn, 1)
    say("(b) call  total_gradient(., 'ply_thickness')")
    report(T, "ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + ([""] + tail if tail else [])) + "\n")
    c.close()


if __name__ == "__main__":
    main()
