"""Timings of the forward mode of the static path (csrc/residual_jvp.h) at BASELINE config 3 (wing1m, 1 015 470 DOF, 5 x 5 points):
per argument femo_residual_jvp beside the matching femo_dRdarg_T and one application of the operator in the same process,
femo_total_jvp with 1 and 4 directions against 4 single calls and against femo_total_gradients with four functionals, and the
distance between the forward and the adjoint totals.  Host wall-clock around each C-ABI call (device-to-host copies included),
median of `reps` after one warm-up; one JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
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

    def timed(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    out = dict(workload="wing1m", ndof=m.ndof, nel=m.nel, nquad=c.nquad, unit="ms (host wall-clock, median)")
    x = rng.uniform(-1, 1, m.ndof)
    lam = rng.uniform(-1, 1, m.ndof)
    out["apply_K"] = timed(lambda: c.apply_K(x))
    for arg in ("thickness", "E", "nu", "F_solid", "uhat"):
        v = rng.uniform(-1, 1, c.field_size(arg))
        out[f"residual_jvp_{arg}"] = timed(lambda: c.dRdarg(arg, v))
        out[f"dRdarg_T_{arg}"] = timed(lambda: c.dRdarg_T(arg, lam))
    c.set_stress_params(m=1e-6, rho=6.0)
    names = ["compliance", "elastic_energy", "pnorm_stress", "mass"]
    h = c.get_field("thickness")
    V = h * rng.uniform(0.5, 1.0, (4, h.size))
    out["total_jvp_1_direction"] = timed(lambda: c.total_jvp("thickness", V[0], names))
    out["total_jvp_4_directions"] = timed(lambda: c.total_jvp("thickness", V, names))
    out["total_jvp_4_single_calls"] = timed(lambda: [c.total_jvp("thickness", v, names) for v in V])
    out["total_gradients_4_functionals"] = timed(lambda: c.total_gradients(names, "thickness"))
    dJ = c.total_jvp("thickness", V, names, want_states=False)[1]
    G = c.total_gradients(names, "thickness")[0]
    want = G @ V.T
    out["forward_against_adjoint_totals"] = float(np.abs(dJ / want - 1.0).max())
    print(json.dumps(out))
    c.close()


if __name__ == "__main__":
    main()
