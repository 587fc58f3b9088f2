"""Writes tests/golden/shape_sens.npz: the extended-precision reference of the derivatives with respect to uhat (tests/shape_ref.py) for
every case and quantity of tests/test_gpu_shape_parity.py -- the reference as a hi / lo pair of float64, its uncertainty and its scale.

numpy.longdouble must be the 80-bit type (x86); generation takes a few minutes.  Inputs are the deterministic ones of
rowscaled_cases.build plus the seeded directions of shape_ref.directions.  With --floors it also prints the SHAPE_FLOOR table
(twice the measured floors) to paste into tests/shape_ref.py.

    python tests/golden/make_shape_goldens.py [--floors]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rowscaled_cases as rc         # noqa: E402
import shape_ref as sr               # noqa: E402


def main():
    if not np.finfo(np.longdouble).eps < 2e-19:
        raise SystemExit("numpy.longdouble is not the 80-bit type here: the reference cannot be generated")
    out, table = {}, []
    for name in sr.CASES:
        k = rc.build(name, device=False)
        if "--floors" in sys.argv:
            for q, v in sr.measure_floors(k).items():
                table.append(f'    ("{q}", "{name}"): {float(f"{2 * v:.3g}")!r},')
        for q, (ref, unc, scale) in sr.reference(k).items():
            hi, lo = sr.split(ref)
            key = f"{name}|{q}|"
            out[key + "hi"], out[key + "lo"] = hi, lo
            out[key + "unc"], out[key + "scale"] = np.asarray(unc, dtype=np.float64), np.asarray(scale, dtype=np.float64)
            print(f"{name} {q}: unc/scale {sr.pm._ratio(unc.ravel(), scale.ravel()):.2e}", flush=True)
    np.savez_compressed(sr.GOLDEN, **out)
    print("wrote", sr.GOLDEN, os.path.getsize(sr.GOLDEN), "bytes")
    if table:
        print("SHAPE_FLOOR = {\n" + "\n".join(table) + "\n}")


if __name__ == "__main__":
    main()
