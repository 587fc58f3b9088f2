"""Mass of a laminate and its gradient with respect to the ply thicknesses on the 1 M-DOF wing (67 280 cells, 8 plies), on one GPU,
two routes in one process and one context (element-wise material, layup mode with ply densities):

  device   functional("layup_mass") + dfunctional("layup_mass", "ply_thickness") (femo_alpha_amd/csrc/layup_mass.h);
  host     the route without these outputs: get_field("ply_thickness"), H = sum_k t_k and rho = sum_k rho_k t_k / H on the host,
           set_field("thickness", H) and set_field("density", rho), functional("mass"), dfunctional("mass", "thickness") and
           dfunctional("mass", "density"), chained back to the plies on the host:
           d mass / d t_ek = d mass / d h_e + d mass / d rho_e (rho_k - rho_e) / H_e.

Call times are a host clock around calls that end in a device synchronise (every call copies its result back), warmed up, the median of
``--reps`` repetitions.  Writes profiles/layup_mass.txt (``--out``).

    python scripts/bench_layup_mass.py [--reps 21] [--out profiles/layup_mass.txt]
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


def median_ms(fn, reps):
    for _ in range(2):                                         # warm-up: code objects, buffers
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layup_mass.txt"))
    a = ap.parse_args()
    from bench import make_workload
    from femo_alpha_amd import laminate as lm
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(a.workload)
    nel, nply = m.nel, 8
    rng = np.random.default_rng(0)
    t = 1.27e-3 / nply * (1 + 0.2 * rng.uniform(-1, 1, (nel, nply)))
    theta = np.tile([0.0, 45.0, -45.0, 90.0, 90.0, -45.0, 45.0, 0.0], (nel, 1)) + rng.uniform(-5, 5, (nel, nply))
    rho = 1600.0 * (1 + 0.2 * rng.uniform(-1, 1, nply))
    c = ShellContext(m, element_wise_material=True)            # the host route needs element-wise "thickness" and "density"
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_field("uhat", 1e-3 * rng.uniform(-1, 1, (m.nn, 3)))
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, ("bot", "top"), density=rho)
    lines = [f"laminate mass and its ply-thickness gradient, {desc}", f"{nel} cells, {nply} plies, uhat != 0; {a.reps} repetitions, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    res = {}

    def device_value():
        res["J_dev"] = c.functional("layup_mass")

    def device_grad():
        res["g_dev"] = c.dfunctional("layup_mass", "ply_thickness")

    def device_route():
        device_value()
        device_grad()

    def host_route():
        tt = c.get_field("ply_thickness").reshape(nel, nply)
        H = tt.sum(axis=1)
        rbar = (tt @ rho) / H
        c.set_field("thickness", H)
        c.set_field("density", rbar)
        res["J_host"] = c.functional("mass")
        gh = c.dfunctional("mass", "thickness")
        gr = c.dfunctional("mass", "density")
        res["g_host"] = (gh[:, None] + gr[:, None] * (rho[None, :] - rbar[:, None]) / H[:, None]).ravel()

    say("device  functional('layup_mass')                                %9.3f ms (%.3f .. %.3f)" % median_ms(device_value, a.reps))
    say("device  dfunctional('layup_mass', 'ply_thickness')              %9.3f ms (%.3f .. %.3f)" % median_ms(device_grad, a.reps))
    say("device  both                                                    %9.3f ms (%.3f .. %.3f)" % median_ms(device_route, a.reps))
    say("host    get, smear, set thickness and density, mass, chain      %9.3f ms (%.3f .. %.3f)" % median_ms(host_route, a.reps))
    say("device  both, again after the host route                        %9.3f ms (%.3f .. %.3f)" % median_ms(device_route, a.reps))
    say(f"layup_mass {res['J_dev']:.12e} against mass of the smeared plate {res['J_host']:.12e}: "
        f"{abs(res['J_dev'] - res['J_host']) / abs(res['J_host']):.1e} relative")
    say(f"agreement of the two gradients: {np.abs(res['g_dev'] - res['g_host']).max() / np.abs(res['g_host']).max():.1e} of the largest entry")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
