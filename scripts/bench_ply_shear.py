"""Interlaminar shear failure aggregate on the 1 M-DOF wing (the workload of scripts/bench_layup.py: 67 280 cells, 8 plies), one
GPU, one process.  The layup carries Tsai-Wu strengths (16 recovery points of "ply_failure": bottom and top of every ply) and
transverse shear strengths (8 recovery points of "ply_shear_failure": one per ply):

  (a) device events around back-to-back launches (femo_bench_kernel): the value pass with its combine, the state gradient as
      femo_dfunctional enqueues it (value pass, PS_DW, gather) and the table product (value pass, PS_DTABLE); alongside, in the same
      process and alternating with the new value pass round by round, the value pass of "ply_failure" on the same layup.  Bytes are
      each kernel's own traffic, set against the HBM peak (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy);
  (b) a host clock around calls that end in a device synchronise: the functional, its state gradient, and
      total_gradient("ply_shear_failure", "ply_thickness");
  (c) the host route: the state to the host, then the numpy reference of tests/ply_shear_ref.py.

Medians of ``--reps`` rounds after a warm-up.  Writes profiles/ply_shear.txt (``--out``); ``--resource-log`` takes the output of a
build of csrc/femo_hip.hip with ``-Rpass-analysis=kernel-resource-usage`` and puts the lines of the new kernels in front (without it
an existing section is kept).

    python scripts/bench_ply_shear.py [--reps 21] [--resource-log build.log] [--out profiles/ply_shear.txt]
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLY = dict(E1=1.35e11, E2=1.0e10, G12=5e9, nu12=0.3, G13=5e9, G23=3.5e9)
STRENGTH = dict(Xt=1.5e9, Xc=1.2e9, Yt=5e7, Yc=2e8, S=7e7)
SHEAR = (6e7, 4e7)
HBM_SPEC, HBM_COPY = 8.0, 6.29                                 # TB/s
RES_HEAD = "resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)"
RES_END = "end of resource usage"
MODES = {"0": "PS_VALUE", "1": "PS_FIELD", "2": "PS_DW", "3": "PS_DTABLE"}


def median_ms(fn, reps):
    fn()                                                       # warm-up: code objects, buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def resource_lines(log):
    """One line per instantiation of k_ply_shear and per layup shear kernel from the compiler's remarks."""
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
        m = re.match(r"_ZN4femo11k_ply_shearILi(\d)ELi(\d)ELb(\d)ELb(\d)ELi(\d)EE", r["name"])
        l = re.match(r"_ZN4femo\d+(k_layup_shear_(?:build|vjp))E", r["name"])
        if m:
            npc, nvc, quad, uhat, mode = m.groups()
            name = f"k_ply_shear<{npc}, {nvc}, {tf(quad)}, {tf(uhat)}, {MODES[mode]}>"
        elif l:
            name = l.group(1)
        else:
            continue
        out.append(f"{name}  VGPRs {r['VGPRs']:>3}  SGPRs {r['TotalSGPRs']:>3}  LDS {r['LDS Size [bytes/block]']:>5} B  "
                   f"scratch {r['ScratchSize [bytes/lane]']} B/lane  {r['Occupancy [waves/SIMD]']} waves/SIMD")
    return out


def kept_resource_lines(path):
    if not os.path.exists(path):
        return []
    with open(path) as fh:
        lines = fh.read().splitlines()
    if RES_HEAD in lines and RES_END in lines:
        return lines[lines.index(RES_HEAD) + 1: lines.index(RES_END)]
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--workload", default="wing1m")
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ply_shear.txt"))
    a = ap.parse_args()
    res = resource_lines(a.resource_log) if a.resource_log else kept_resource_lines(a.out)
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
    c.set_layup(dict(PLY, F=lm.tsai_wu(**STRENGTH)), t, theta, ("bot", "top"), shear_strength=SHEAR)
    c.solve_state(True)
    c.set_ply_failure_params(5.0 / np.abs(c.ply_failure_field()).max())
    fld = c.ply_shear_failure_field()
    rho = 5.0 / fld.max()
    c.set_ply_shear_params(rho)
    ld = 3 * m.npc + 3 * m.nvc
    npt, npt_f = nply, 2 * nply
    lines = [RES_HEAD] + res + [RES_END, "",
             f"interlaminar shear failure aggregate, {desc}",
             f"{nel} cells, {nply} plies: {npt} recovery points of 6 doubles (ply_shear_failure) beside {npt_f} of 16 (ply_failure); "
             f"{a.reps} rounds, median (min .. max)",
             f"HBM peak: {HBM_SPEC} TB/s specified, {HBM_COPY} TB/s measured with a float4 copy"]
    say = lambda s: (print(s, flush=True), lines.append(s))

    # ---------------------------------------------------------------- (a) kernels, the two value passes alternating round by round
    kr = 50
    names = ("ply_shear_value", "ply_value", "ply_shear_dw", "ply_shear_dtable")
    for n in names:
        c.bench_kernel(n, kr)                                  # warm-up
    T = {n: [] for n in names}
    for _ in range(a.reps):
        for n in names:
            T[n].append(1e3 * c.bench_kernel(n, kr))           # us
    med = {n: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for n, v in T.items()}
    geo = 3 * m.nvc * 8 + (m.npc + m.nvc) * 4                  # per cell: vertex coordinates (doubles) and node numbers (ints)
    b_val = nel * ((6 * npt + ld) * 8 + geo)                   # table, state and geometry in
    b_valf = nel * ((16 * npt_f + ld) * 8 + geo)
    b_dw = 2 * b_val + nel * 2 * ld * 8 + m.ndof * 8           # the value pass, the same reads again, element vector out and in, gradient out
    b_dt = 2 * b_val + nel * 6 * npt * 8                       # the value pass, the same reads again, the 6 npt row out
    tb = lambda b, us: b / (us * 1e-6) / 1e12
    rep = lambda n, b: (f"{med[n][0]:9.1f} us ({med[n][1]:.1f} .. {med[n][2]:.1f})   {b / 1e6:6.1f} MB of its own traffic: "
                        f"{tb(b, med[n][0]):.2f} TB/s = {100 * tb(b, med[n][0]) / HBM_SPEC:.0f} % of the specified, "
                        f"{100 * tb(b, med[n][0]) / HBM_COPY:.0f} % of the copy peak")
    say(f"(a) ply_shear_failure  value pass (k_ply_shear<PS_VALUE>, combine)        {rep('ply_shear_value', b_val)}")
    say(f"(a) ply_failure        value pass (k_ply_failure<PF_VALUE>, combine)      {rep('ply_value', b_valf)}")
    say(f"(a) new value pass / ply_failure's value pass beside it                   {med['ply_shear_value'][0] / med['ply_value'][0]:9.2f} x")
    say(f"(a) ply_shear_failure  state gradient (value pass, PS_DW, gather)         {rep('ply_shear_dw', b_dw)}")
    say(f"(a) ply_shear_failure  table product (value pass, PS_DTABLE)              {rep('ply_shear_dtable', b_dt)}")

    # ---------------------------------------------------------------- (b) calls
    say("(b) call  functional('ply_shear_failure')                                   %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.functional("ply_shear_failure"), a.reps))
    say("(b) call  dfunctional('ply_shear_failure', 'disp_solid') (gradient out)     %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.dfunctional("ply_shear_failure", "disp_solid"), a.reps))
    say("(b) call  total_gradient('ply_shear_failure', 'ply_thickness')              %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.total_gradient("ply_shear_failure", "ply_thickness"), a.reps))
    say("(b) call  total_gradient('ply_failure', 'ply_thickness') beside it          %9.2f ms (%.2f .. %.2f)"
        % median_ms(lambda: c.total_gradient("ply_failure", "ply_thickness"), a.reps))

    # ---------------------------------------------------------------- (c) the host route
    from oracle.rm_shell_oracle import degree4_rule
    from ply_shear_ref import PlyShearOracle
    o = PlyShearOracle(m, nquad=degree4_rule(m))
    o.set_fields(h=np.full(m.nn, 1.27e-3), E=np.full(m.nn, 1.0), nu=np.full(m.nn, 0.3), rho=np.ones(m.nn), f=np.zeros((m.nn, 3)))
    o.set_ply_shear_table(c.get_field("ply_shear_table"), npt)
    K = c.functional("ply_shear_failure")
    host = [None]

    def host_route():
        host[0] = o.value(c.get_state(), rho)
    th = median_ms(host_route, 3)
    say("(c) host route: state to the host, numpy reference value (3 rounds)         %9.2f ms (%.2f .. %.2f)" % th)
    say(f"(c) device K {K:.12e}, host K {host[0]:.12e}: {abs(K - host[0]) / fld.max():.1e} of the largest index {fld.max():.3e}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
