"""What the reference surface of a layup (femo_set_layup_reference) costs, on the 1 M-DOF wing layup of scripts/bench_layup.py
(67 280 cells x 8 plies, 16 recovery points), one GPU.

Two quantities: the laminate-and-table build (k_layup_build, device events around 200 back-to-back launches, femo_bench_kernel) and
total_gradient("ply_failure", "ply_thickness") (a host clock around the call, which ends in a device synchronise; the median of
``--reps`` calls after a warm-up).  Three legs, each a process of its own:

  parent / mid   a checkout of the parent commit (``--parent DIR``, built beforehand), which knows the mid-surface only;
  this / mid     this tree, the default reference surface;
  this / top+c   this tree, reference "top" and a per-cell offset of the order of H: the one extra 8-byte read per cell.

The legs run alternately, ``--rounds`` times over, so that drift of the machine shows in every leg alike.  "mid" on this tree has to
lie within the spread of the parent's own rounds.  The forward solve of bench.py does not touch these kernels: with ``--bench-pairs N``
bench.py runs N times in either tree, alternately, and the pairs are recorded.  ``--resource-log`` takes the output of a build of
csrc/femo_hip.hip with ``-Rpass-analysis=kernel-resource-usage`` (and ``--parent-resource-log`` the parent's) and records the
registers, scratch and occupancy of the layup kernels.  Writes profiles/layup_reference.txt (``--out``).

    python scripts/bench_layup_reference.py --parent ../parent [--rounds 3] [--reps 21] [--bench-pairs 3]
    python scripts/bench_layup_reference.py --leg top            # one leg in this tree: prints one JSON line
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLY = dict(E1=1.35e11, E2=1.0e10, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)
STRENGTH = dict(Xt=1.5e9, Xc=1.2e9, Yt=5e7, Yc=2e8, S=7e7)
KERNELS = re.compile(r"k_layup_(build|jvp|vjp)")


def leg(root, which, reps, workload):
    """One leg inside the tree ``root``: {"build_us", "total_ms": [median, min, max]}."""
    sys.path.insert(0, root)
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(workload)
    nel, nply, surfaces = m.nel, 8, ("bot", "top")
    rng = np.random.default_rng(0)
    t = 1.27e-3 / nply * (1 + 0.2 * rng.uniform(-1, 1, (nel, nply)))
    theta = np.tile([0.0, 45.0, -45.0, 90.0, 90.0, -45.0, 45.0, 0.0], (nel, 1)) + rng.uniform(-5, 5, (nel, nply))
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.use_direct_solver()
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, surfaces)
    if which == "top":
        c.set_layup_reference("top", 1.27e-3 * rng.uniform(-1, 1, nel))
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    c.total_gradient("ply_failure", "ply_thickness")                              # warm-up: code objects, buffers, the factor
    builds, ts = [], []
    for _ in range(3):
        builds.append(1e3 * c.bench_kernel("layup_build", 200))
    for _ in range(reps):
        t0 = time.perf_counter()
        c.total_gradient("ply_failure", "ply_thickness")
        ts.append(1e3 * (time.perf_counter() - t0))
    c.close()
    return {"desc": desc, "cells": nel, "build_us": float(np.median(builds)), "total_ms": [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]}


def child(root, *args):
    """A fresh process in ``root``; its last output line is the JSON result."""
    out = subprocess.run([sys.executable, *args], cwd=root, capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise RuntimeError(f"{' '.join(args)} in {root} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def resource_lines(log):
    rows, cur = [], None
    with open(log) as fh:
        for line in fh:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = {"name": m.group(1)} if KERNELS.search(m.group(1)) else None
                if cur:
                    rows.append(cur)
                continue
            m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    return [f"  {r['name']:<58} VGPRs {r.get('VGPRs', '?'):>4}  SGPRs {r.get('TotalSGPRs', '?'):>4}  scratch {r.get('ScratchSize [bytes/lane]', '?'):>3} B/lane  "
            f"occupancy {r.get('Occupancy [waves/SIMD]', '?')}  LDS {r.get('LDS Size [bytes/block]', '?')} B" for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["mid", "top"], default=None)
    ap.add_argument("--root", default=ROOT, help="the tree a leg runs in")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--bench-pairs", type=int, default=0)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--parent-resource-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layup_reference.txt"))
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(os.path.abspath(a.root), a.leg, a.reps, a.workload)), flush=True)
        return
    if not a.parent:
        ap.error("--parent DIR: a built checkout of the parent commit (or --leg for one leg in this tree)")
    parent = os.path.abspath(a.parent)
    me = os.path.abspath(__file__)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    legs = [("parent / mid", parent, "mid"), ("this   / mid", ROOT, "mid"), ("this   / top+c", ROOT, "top")]
    res = {name: [] for name, _, _ in legs}
    for r in range(a.rounds):
        for name, root, which in legs:
            # the parent tree has no such script: this file runs there too, against that tree's package (--root)
            res[name].append(child(root, me, "--leg", which, "--root", root, "--reps", str(a.reps), "--workload", a.workload))
            if not lines:
                say(f"reference surface of a layup, {res[name][-1]['desc']}")
                say(f"{res[name][-1]['cells']} cells, 8 plies, 16 recovery points per cell; {a.rounds} rounds of the three legs run alternately, a process each")
                say(f"build: k_layup_build, us per launch (200 back-to-back launches, the median of 3);  total: total_gradient('ply_failure', "
                    f"'ply_thickness'), ms, median (min .. max) of {a.reps} calls")
            x = res[name][-1]
            say(f"round {r}  {name:<15} build {x['build_us']:7.1f} us   total {x['total_ms'][0]:7.3f} ms ({x['total_ms'][1]:.3f} .. {x['total_ms'][2]:.3f})")
    for name, _, _ in legs:
        b = [x["build_us"] for x in res[name]]
        t = [x["total_ms"][0] for x in res[name]]
        say(f"over the rounds  {name:<15} build {np.median(b):7.1f} us ({min(b):.1f} .. {max(b):.1f})   total {np.median(t):7.3f} ms ({min(t):.3f} .. {max(t):.3f})")
    say("the offset leg reads 8 B per cell more (0.54 MB) beside the 318.6 MB the build moves")
    for i in range(a.bench_pairs):
        pair = []
        for name, root in (("parent", parent), ("this", ROOT)):
            j = child(root, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline",
                      "--no-keep-numbering-leg")
            pair.append(f"{name} forward {j['forward_ms']:.3f} ms, adjoint {j['adjoint_ms']:.3f} ms, {j['value']:.4e} DOF/s")
        say(f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}, pair {i}:  " + ";  ".join(pair))
    for title, log in (("parent", a.parent_resource_log), ("this", a.resource_log)):
        if log:
            say(f"resource usage of the layup kernels, {title} (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
            for ln in resource_lines(log):
                say(ln)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
