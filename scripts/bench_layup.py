"""The layup design step on the 1 M-DOF wing (67 280 cells, 8 plies, recovery points at the bottom and top of every ply), on one GPU:

  device   the laminate and the ply table built from ply thicknesses and angles (femo_set_layup), the pull-back of a laminate and a table
           cotangent (femo_layup_vjp) and one total_gradients call with respect to "ply_thickness";
  host     the same step the way it was done before layups existed: femo_alpha_amd/laminate.py with Jacobians, set_laminate,
           set_field("ply_table"), the totals with respect to "laminate" and "ply_table" copied out, then contracted.

Kernel times are device events around back-to-back launches (femo_bench_kernel); call times are a host clock around calls that end
in a device synchronise, warmed up, the median of ``--reps`` repetitions.  The achieved bytes/s of the build kernel is its own traffic
-- 2 nply 8 B in, (2 32 + 2 16 npt) 8 B out per cell -- over its kernel time.  Writes profiles/layup_wing1m.txt (``--out``).

    python scripts/bench_layup.py [--reps 7] [--out profiles/layup_wing1m.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLY = dict(E1=1.35e11, E2=1.0e10, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)
STRENGTH = dict(Xt=1.5e9, Xc=1.2e9, Yt=5e7, Yc=2e8, S=7e7)
NAMES = ["compliance", "ply_failure"]


def median_ms(fn, reps):
    fn()                                                       # warm-up: code objects, buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layup_wing1m.txt"))
    a = ap.parse_args()
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(a.workload)
    nel, nply, surfaces = m.nel, 8, ("bot", "top")
    npt = nply * len(surfaces)
    rng = np.random.default_rng(0)
    t = 1.27e-3 / nply * (1 + 0.2 * rng.uniform(-1, 1, (nel, nply)))
    theta = np.tile([0.0, 45.0, -45.0, 90.0, 90.0, -45.0, 45.0, 0.0], (nel, 1)) + rng.uniform(-5, 5, (nel, nply))
    F = lm.tsai_wu(**STRENGTH)
    mat = [np.full((nel, nply), PLY[k]) for k in ("E1", "E2", "G12", "nu12", "G13", "G23")]
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.use_direct_solver()
    lines = [f"layup design step, {desc}", f"{nel} cells, {nply} plies, {npt} recovery points per cell; {a.reps} repetitions, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))

    # ---------------------------------------------------------------- device
    c.set_layup(dict(PLY, F=F), t, theta, surfaces)
    c_drill = float(c.get_field("laminate")[31])
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    k_build = c.bench_kernel("layup_build", 200)
    k_vjp = c.bench_kernel("layup_vjp", 200)
    k_vjp_a = c.bench_kernel("layup_vjp_angle", 200)
    traffic = nel * (2 * nply * 8 + (2 * 32 + 2 * 16 * npt) * 8)
    say(f"device  k_layup_build               {1e3 * k_build:9.1f} us   {traffic / 1e6:.1f} MB of its own traffic: {traffic / (k_build * 1e-3) / 1e9:.0f} GB/s")
    say(f"device  k_layup_vjp (thickness)     {1e3 * k_vjp:9.1f} us")
    say(f"device  k_layup_vjp (angle)         {1e3 * k_vjp_a:9.1f} us")
    lbar, tbar = rng.uniform(-1, 1, (nel, 32)), rng.uniform(-1, 1, (nel, npt, 16))
    say("device  set_field('ply_thickness') (upload, check, build)   %9.2f ms (%.2f .. %.2f)" % median_ms(lambda: c.set_field("ply_thickness", t), a.reps))
    say("device  layup_vjp call (cotangents in, gradient out)        %9.2f ms (%.2f .. %.2f)" % median_ms(lambda: c.layup_vjp("ply_thickness", lbar, tbar), a.reps))
    c.solve_state(True)
    g_dev = [None]

    def dev_totals():
        g_dev[0] = c.total_gradients(NAMES, "ply_thickness")[0]
    say("device  total_gradients(%d functionals, 'ply_thickness')      %9.2f ms (%.2f .. %.2f)" % ((len(NAMES),) + median_ms(dev_totals, a.reps)))

    def dev_step():
        c.set_field("ply_thickness", t)
        c.solve_state(True)
        dev_totals()
    say("device  design step: set, solve, totals                     %9.2f ms (%.2f .. %.2f)" % median_ms(dev_step, max(3, a.reps // 2)))

    # ---------------------------------------------------------------- host: the same step without layups
    c.set_layup(None)
    res = {}

    def host_build():
        res["clt"], res["dclt"] = lm.clt_from_plies(*mat, t, theta, jacobian=True)
        res["tab"], res["dz"] = lm.ply_table(*mat[:4], t, theta, F, surfaces, jacobian=True)
    say("host    clt_from_plies + ply_table with Jacobians           %9.2f ms (%.2f .. %.2f)" % median_ms(host_build, max(3, a.reps // 2)))

    def host_set():
        c.set_laminate(lm.pack(*res["clt"], c_drill))
        c.set_field("ply_table", res["tab"])
    say("host    set_laminate + set_field('ply_table')               %9.2f ms (%.2f .. %.2f)" % median_ms(host_set, max(3, a.reps // 2)))
    c.solve_state(True)
    g_host = [None]

    def host_totals():
        gl = c.total_gradients(NAMES, "laminate")[0].reshape(len(NAMES), nel, 32)
        gt = c.total_gradients(NAMES, "ply_table")[0].reshape(len(NAMES), nel, npt, 16)
        d = res["dclt"]
        dlam = lm.pack(d[0].reshape(-1, 3, 3), d[1].reshape(-1, 3, 3), d[2].reshape(-1, 3, 3), d[3].reshape(-1, 2, 2), 0.0).reshape(nel, nply, 32)
        g_host[0] = np.einsum("iep,pj->iej", gt[..., 9], res["dz"]) + np.einsum("iek,ejk->iej", gl, dlam)
    say("host    totals wrt 'laminate' and 'ply_table', contracted   %9.2f ms (%.2f .. %.2f)" % median_ms(host_totals, max(3, a.reps // 2)))

    def host_step():
        host_build()
        host_set()
        c.solve_state(True)
        host_totals()
    say("host    design step: build, set, solve, totals              %9.2f ms (%.2f .. %.2f)" % median_ms(host_step, 3))
    gd = g_dev[0].reshape(len(NAMES), nel, nply)
    for i, n in enumerate(NAMES):
        say(f"agreement of the two gradients [{n}]: {np.abs(gd[i] - g_host[0][i]).max() / np.abs(g_host[0][i]).max():.1e} of the largest entry")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
