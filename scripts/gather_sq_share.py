"""Vector-issue share of the gathering launches of one factorisation, from a rocprofv3 --pmc run of scripts/r3_pmc_target.py with
SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES (a run of its own, no tracing beside it).  The target
factorises three times; the last third of every kernel class's dispatches is the last factorisation.
    python3 scripts/gather_sq_share.py <counter_collection.csv>"""
import collections
import csv
import sys

CLASSES = [("k_trailing_mfma<true>", "rank-k, gathering"), ("k_trailing_mfma<false>", "rank-k, plain"),
           ("k_trailing_fine<true>", "fine, gathering"), ("k_trailing_fine<false>", "fine, plain"), ("k_extend_gather", "extend gather")]
COUNTERS = ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_VALU_MFMA_BUSY_CYCLES"]

by = {c: collections.OrderedDict() for c, _ in CLASSES}
for r in csv.DictReader(open(sys.argv[1])):
    for c, _ in CLASSES:
        if c in r["Kernel_Name"]:
            d = by[c].setdefault(int(r["Dispatch_Id"]), {"grid": int(r["Grid_Size"])})
            d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
print(f"{'class':20s} launches " + " ".join(f"{n[3:]:>22s}" for n in COUNTERS) + "   VALU inst / busy cycle   MFMA busy / busy")
for c, label in CLASSES:
    ids = sorted(by[c])
    last = ids[len(ids) - len(ids) // 3:]
    tot = {n: sum(by[c][i].get(n, 0.0) for i in last) for n in COUNTERS}
    busy = max(tot["SQ_BUSY_CYCLES"], 1.0)
    print(f"{label:20s} {len(last):8d} " + " ".join(f"{tot[n]:22.0f}" for n in COUNTERS)
          + f"   {tot['SQ_INSTS_VALU'] / busy:22.3f}   {tot['SQ_VALU_MFMA_BUSY_CYCLES'] / busy:16.3f}")
print("\ngathering rank-k launches of the last factorisation, in dispatch order")
print("  # workgroups x 256     INSTS_VALU   ACTIVE_INST_VALU    BUSY_CYCLES   MFMA_BUSY_CYCLES")
c = CLASSES[0][0]
ids = sorted(by[c])
for k, i in enumerate(ids[len(ids) - len(ids) // 3:]):
    d = by[c][i]
    print(f"{k:3d} {d['grid']:17d} " + " ".join(f"{d.get(n, 0.0):16.0f}" for n in COUNTERS))
