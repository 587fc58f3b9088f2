"""Two displacement constraints beside compliance and stress on the 1 M-DOF wing, on one GPU, two routes to the same four thickness
gradients in one process and one context (the benchmark's solver settings, state solved once):

  A  total_gradients(["compliance", "pnorm_stress", "max_disp", "max_disp1"], "thickness"): four adjoints through one grouped solve,
     the aggregates' seeds made on the device (femo_alpha_amd/csrc/disp_aggregate.h);
  B  the route without these outputs: total_gradients of the first two, get_state, the KS value and seed of both aggregates in numpy,
     the two seeds through solve_linear_multi, two dRdarg_T.

"max_disp" is the magnitude over the mesh vertices, "max_disp1" the smooth minimum of u_z (direction (0, 0, 1), scaler -1), both at
rho |s| max x = 50.  Call times are a host clock around calls that end in a device synchronise, warmed up, the median of ``--reps``
repetitions; kernel times are device events around back-to-back launches (femo_bench_kernel).  Writes profiles/disp_aggregate.txt.

    python scripts/bench_disp_aggregate.py [--reps 21] [--out profiles/disp_aggregate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    for _ in range(2):                                         # warm-up: code objects, buffers
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def ks(x, rho):
    """(S, p) of the shifted log-sum-exp."""
    xm = x.max()
    S = xm + np.log(np.sum(np.exp(rho * (x - xm)))) / rho
    return S, np.exp(rho * (x - S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disp_aggregate.txt"))
    a = ap.parse_args()
    from bench import make_workload
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, desc = make_workload(a.workload)
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.enable_frontal(m.recommended_leaf_size())
    c.set_solver(preconditioner=2, rtol=1e-10, maxit=50, check_every=1)
    it, rr = c.solve_state(True)
    w = c.get_state()
    nn, nP2 = m.nn, m.nP2
    u = w[: 3 * nn].reshape(nn, 3)
    rho0 = 50.0 / np.linalg.norm(u, axis=1).max()
    rho1 = 50.0 / np.abs(u[:, 2]).max()
    c.set_disp_aggregate(0, rho0, 1.0, None, "vertices")
    c.set_disp_aggregate(1, rho1, -1.0, (0.0, 0.0, 1.0), "vertices")
    c.set_stress_params(1.0 / c.field_output("stress").max(), 10.0)
    lines = [f"max-displacement aggregates beside compliance and stress, {desc}",
             f"{m.ndof} DOFs, {nn} vertices, {nP2} displacement nodes; forward solve {it} iterations, relres {rr:.1e}; "
             f"{a.reps} repetitions, median (min .. max)"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    res = {}

    def route_a():
        res["A"] = c.total_gradients(["compliance", "pnorm_stress", "max_disp", "max_disp1"], "thickness")[0]

    def route_b():
        G = c.total_gradients(["compliance", "pnorm_stress"], "thickness")[0]
        ww = c.get_state()
        uu = ww[: 3 * nn].reshape(nn, 3)
        seeds = np.zeros((2, ww.size))
        r = np.sqrt(np.sum(uu * uu, axis=1))
        S0, p0 = ks(r, rho0)
        seeds[0, : 3 * nn] = (np.where(r > 0, p0 / np.where(r > 0, r, 1.0), 0.0)[:, None] * uu).ravel()
        S1, p1 = ks(-uu[:, 2], rho1)
        seeds[1, 2: 3 * nn: 3] = p1
        res["M_host"] = (S0, -S1)
        lam = c.solve_linear_multi(seeds)[0]
        res["B"] = np.vstack([G, -c.dRdarg_T("thickness", lam[0]), -c.dRdarg_T("thickness", lam[1])])

    def values():
        res["M_dev"] = (c.functional("max_disp"), c.functional("max_disp1"))

    say("A  total_gradients of the four outputs, one grouped call             %9.3f ms (%.3f .. %.3f)" % median_ms(route_a, a.reps))
    say("B  two grouped, state to the host, numpy KS, two solves, two dR^T   %9.3f ms (%.3f .. %.3f)" % median_ms(route_b, a.reps))
    say("A  again after B                                                      %9.3f ms (%.3f .. %.3f)" % median_ms(route_a, a.reps))
    say("   functional('max_disp') + functional('max_disp1')                   %9.3f ms (%.3f .. %.3f)" % median_ms(values, a.reps))
    say("   dfunctional('max_disp', 'disp_solid') with its copy to the host    %9.3f ms (%.3f .. %.3f)"
        % median_ms(lambda: c.dfunctional("max_disp", "disp_solid"), a.reps))
    for nodes, n in (("vertices", nn), ("all", nP2)):
        c.set_disp_aggregate(0, rho0, 1.0, None, nodes)
        kv = c.bench_kernel("disp_agg_value", 200)
        kg = c.bench_kernel("disp_agg_grad", 200)
        say(f"   kernels alone, nodes = {nodes} ({n} selected of {nP2} threads): value pass + combine {1e3 * kv:.1f} us, gradient {1e3 * kg:.1f} us; "
            f"against the 24 bytes per selected node they must read: {24 * n / (1e-3 * kv) / 1e9:.1f} and {24 * n / (1e-3 * kg) / 1e9:.1f} GB/s")
    c.set_disp_aggregate(0, rho0, 1.0, None, "vertices")
    for i, name in enumerate(("max_disp", "max_disp1")):
        say(f"{name}: device {res['M_dev'][i]:.12e}, host {res['M_host'][i]:.12e}, {abs(res['M_dev'][i] - res['M_host'][i]) / abs(res['M_host'][i]):.1e} relative")
    names = ("compliance", "pnorm_stress", "max_disp", "max_disp1")
    agree = lambda i: np.abs(res["A"][i] - res["B"][i]).max() / np.abs(res["B"][i]).max()
    for i, name in enumerate(names):
        say(f"agreement of the two routes' gradients at the timed solver settings (rtol 1e-10) [{name}]: {agree(i):.1e} of the largest entry")
    # the same comparison with the adjoints refined to the rounding floor: what is left is the difference of the routes themselves
    c.set_solver(preconditioner=2, rtol=1e-15, maxit=20, check_every=1)
    c.set_option("strict", 0)
    route_a()
    route_b()
    worst = 0.0
    for i, name in enumerate(names):
        worst = max(worst, agree(i))
        say(f"agreement of the two routes' gradients, adjoints refined to the rounding floor [{name}]: {agree(i):.1e} of the largest entry")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    c.close()
    assert worst <= 1e-10, "the two routes' gradients differ by more than 1e-10 of the largest entry"


if __name__ == "__main__":
    main()
