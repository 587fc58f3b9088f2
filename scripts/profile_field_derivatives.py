"""Timings of the stress-field derivatives (csrc/stress_grad.h) at BASELINE config 3 (wing1m, 1 015 470 DOF, 5 x 5 points):
the reverse products with respect to every argument, the partial Jacobians and the 4-cotangent total derivative beside
femo_total_gradients with four functionals.  Host wall-clock around each C-ABI call (device-to-host copies included), median of
`reps` after one warm-up; one JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(reps=5):
    from bench import make_workload
    from femo_alpha_amd.backend import ShellContext
    m, fields, marker, _ = make_workload("wing1m")
    c = ShellContext(m)
    for k, v in fields.items():
        c.set_field(k, v)
    c.set_penalty_facets(m.penalty_facets(marker))
    c.use_direct_solver()
    c.solve_state(zero_guess=True)
    rng = np.random.default_rng(0)
    cb = rng.uniform(-1, 1, (4, m.nvc * m.nel))

    def timed(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    out = dict(workload="wing1m", ndof=m.ndof, nel=m.nel, nquad=c.nquad, unit="ms (host wall-clock, median)")
    for arg in ("disp_solid", "thickness", "E", "nu", "uhat"):
        out[f"vjp_{arg}"] = timed(lambda: c.field_output_vjp("stress", arg, cb[0]))
    for arg in ("disp_solid", "thickness", "uhat"):
        out[f"jacobian_{arg}"] = timed(lambda: c.field_output_jacobian("stress", arg))
    out["field_output"] = timed(lambda: c.field_output("stress"))
    out["field_total_gradients_4_thickness"] = timed(lambda: c.field_total_gradients("stress", cb, "thickness"))
    c.set_stress_params(m=1e-6, rho=6.0)
    names = ["compliance", "elastic_energy", "pnorm_stress", "tip_disp"]
    out["total_gradients_4_functionals_thickness"] = timed(lambda: c.total_gradients(names, "thickness"))
    print(json.dumps(out))
    c.close()


if __name__ == "__main__":
    main()
