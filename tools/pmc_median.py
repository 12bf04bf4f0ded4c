#!/usr/bin/env python3
"""median over the launches of a rocprofv3 --pmc pass, plain step kernel only:  pmc_median.py <output dir> <label>"""
import collections, csv, glob, json, statistics, sys
if sys.argv[1] == "--full-line":      # pmc_median.py --full-line <bench --full output> <label>: the three per-step times
    d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
    def find(o, key):
        if isinstance(o, dict):
            for k, v in o.items():
                if key in k and isinstance(v, dict) and "ms_per_step" in v:
                    return v["ms_per_step"]
                r = find(v, key)
                if r is not None:
                    return r
    print(sys.argv[3], "headline %.3f" % (d["ms_per_step"] * 1e3), " ".join("%s %.3f" % (k, find(d, k) * 1e3) for k in ("persistent_rollout", "state_emitting_step") if find(d, k)))
    sys.exit(0)
d = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "truss_step_kernel" in r["Kernel_Name"] and "false" in r["Kernel_Name"]:
            d[r["Counter_Name"]].append(float(r["Counter_Value"]))
m = {k: statistics.median(v) for k, v in d.items()}
keys = ("SQ_INSTS_LDS", "SQ_ACTIVE_INST_LDS", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT")
print(f"{sys.argv[2]:28s} " + "  ".join(f"{k}={m.get(k, float('nan')):.0f}" for k in keys))
