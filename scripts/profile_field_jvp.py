"""Timings of the forward mode of the field outputs (csrc/field_jvp.h) at BASELINE config 3 (wing1m, 1 015 470 DOF, 5 x 5 points),
for ndir = 1 and 4:

  field_output_jvp("stress", "disp_solid")                                   the matrix-free partial
  field_total_jvp(("stress", "stress_mid", "stress_bot"), "thickness")      the forward chain for fields

beside the only route to the same numbers without them ("csr route"): total_jvp for the tangent states, field_output_jacobian for
"disp_solid" and for the argument (CSR, brought to the host), and the two host products -- end to end.  A call the library does not
have is skipped, so the same script times the csr route on an older checkout.  Host wall-clock around each call (copies included),
median of `reps` after one warm-up; one JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("stress", "stress_mid", "stress_bot")


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
    dw = 1e-4 * rng.uniform(-1, 1, (4, m.ndof))
    dh = c.get_field("thickness") * rng.uniform(-1, 1, (4, m.nn))

    def timed(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    def csr_partial(V):
        return c.field_output_jacobian("stress", "disp_solid") @ V.T

    def csr_total(V):
        dW = c.total_jvp("thickness", V)[0]
        return [c.field_output_jacobian(n, "disp_solid") @ dW.T + c.field_output_jacobian(n, "thickness") @ V.T for n in NAMES]

    out = dict(workload="wing1m", ndof=m.ndof, nel=m.nel, nquad=c.nquad, unit="ms (host wall-clock, median)")
    new = hasattr(c, "field_output_jvp")
    for nd in (1, 4):
        out[f"csr_partial_stress_w_{nd}"] = timed(lambda: csr_partial(dw[:nd]))
        out[f"csr_total_3_fields_thickness_{nd}"] = timed(lambda: csr_total(dh[:nd]))
        if new:
            out[f"jvp_partial_stress_w_{nd}"] = timed(lambda: c.field_output_jvp("stress", "disp_solid", dw[:nd]))
            out[f"jvp_total_3_fields_thickness_{nd}"] = timed(lambda: c.field_total_jvp(NAMES, "thickness", dh[:nd]))
    if new:
        got = c.field_total_jvp(NAMES, "thickness", dh[:1])[0]
        want = csr_total(dh[:1])
        out["routes_agree_rel"] = float(max(np.abs(got[n][0] - w[:, 0]).max() / np.abs(w).max() for n, w in zip(NAMES, want)))
    print(json.dumps(out))
    c.close()


if __name__ == "__main__":
    main()
