"""Timings of the max-displacement aggregate (csrc/disp_history.h) at BASELINE config 5 (bench.dynamic_case: 508 734 DOF, 101 time
levels, the bench's PlateSim settings at the product tolerance), in the lpc example's setting (rho = 300, scaler = 1 / max of the tip
history): value, partials and the device-resident total gradient, beside the host route an example takes without them (history
download, numpy KS value and gradient, adjoint_history(G), residual_T_products), and one march as the yardstick.  Host wall-clock
after a device synchronise, median of `reps` after one warm-up; one JSON line (and the file given as argv[1]).

Run it a second time under `rocprofv3 --kernel-trace --stats` for the per-kernel times, then
    python scripts/profile_disp_history.py --merge plain.json kernel_stats.csv profiles/disp_history_plate500k.json
adds the achieved bandwidth of every k_disp_ks_* kernel, as a fraction of 6.3 TB/s (the bytes the kernel must move, from the shapes)."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12          # achievable HBM read rate, bytes/s (MI355X_MICROARCH)


def host_ks(W, rho, s):
    """numpy KS value and gradient over every entry of the (levels, ndof) history: what an example computes on the host."""
    x = np.abs(s) * np.abs(W)
    xm = x.max()
    ks = xm + np.log(np.sum(np.exp(rho * (x - xm)))) / rho
    G = np.sign(s) * np.sign(W) * np.exp(rho * (x - ks))
    return ks / s, G


def kernel_table(path, ndof, levels, grad_levels):
    """{kernel: {calls, avg_ms, total_ms, bytes, fraction_of_hbm}} from a rocprofv3 kernel-stats CSV.  Bytes the kernel must move,
    from the shapes: the partial kernel reads the history once per call; the gradient kernels read and write every level they
    handle (grad_levels in all, over every call and chunk of the run), so their fraction is taken on the total time."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "k_disp_ks" not in name:
                continue
            short = name.replace("void ", "").split("(")[0]
            calls, avg_ns, tot_ns = int(row["Calls"]), float(row["AverageNs"]), float(row["TotalDurationNs"])
            r = dict(calls=calls, avg_ms=avg_ns * 1e-6, total_ms=tot_ns * 1e-6)
            if "partial" in short:
                r["bytes_per_call"] = levels * ndof * 8
                r["fraction_of_hbm"] = r["bytes_per_call"] / HBM / (avg_ns * 1e-9)
            elif "grad" in short:
                r["bytes_total"] = 2 * grad_levels * ndof * 8
                r["fraction_of_hbm"] = r["bytes_total"] / HBM / (tot_ns * 1e-9)
            out[short] = r
    return out


def merge(plain_path, stats_path, out_path):
    """The wall-clock record of an untraced run plus the kernel table of a traced run of the same script."""
    rec = json.load(open(plain_path))
    rec["kernels"] = kernel_table(stats_path, rec["ndof"], rec["time_levels"], rec["grad_levels_per_run"])
    rec["kernel_stats"] = os.path.basename(out_path).replace(".json", "_kernel_stats.csv")
    with open(out_path, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec["kernels"], indent=1))


def main(out_path=None, reps=5):
    import torch
    import bench
    from femo_alpha_amd.dynamic_rm_shell.plate_sim import PlateSim
    mesh, dt, F = bench.dynamic_case()
    ps = PlateSim(mesh, 1e8, 0.3, 10.0, dt, 100, quad_deg=3, leaf_size=mesh.recommended_leaf_size())
    ps.update_t(np.full(mesh.nn, 0.1))
    ps.update_f_history(F)
    ps.solve_dynamic_problem()
    T, ctx = ps.time_levels, ps.ctx
    rho, s = 300.0, 1.0 / np.max(ps.tip_disp_history)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    def host_value():
        return host_ks(ctx.newmark_history(0), rho, s)[0]

    def host_total():
        M, G = host_ks(ctx.newmark_history(0), rho, s)
        ps.adjoint_history(G.T)
        g_t, dF = ps.residual_T_products()
        return -g_t, -dF

    M = ps.max_displacement_history(rho, s)
    out = dict(workload="plate500k_dynamic (BASELINE config 5)", ndof=int(ps.fe_dofs), time_levels=int(T), rho=rho, scaler=s, M=M,
               M_host=float(host_value()), history_bytes=int(T * ps.fe_dofs * 8),
               unit="ms (host wall-clock after a device synchronise, median of 5)")
    out["value"] = timed(lambda: ps.max_displacement_history(rho, s))
    out["partials"] = timed(lambda: ps.max_displacement_history_partials(rho, s))
    out["total_gradient_device"] = timed(lambda: ps.max_displacement_history_total_gradient(rho, s))
    out["host_download"] = timed(lambda: ctx.newmark_history(0))
    out["host_value"] = timed(host_value)
    out["host_total_gradient"] = timed(host_total)
    out["tip_history"] = timed(lambda: ps.tip_displacement_history())
    out["march"] = timed(lambda: ps.solve_dynamic_problem())
    out["grad_levels_per_run"] = 2 * (1 + reps) * T          # partials and device total gradient: every level, every call
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
