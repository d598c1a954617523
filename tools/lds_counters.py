#!/usr/bin/env python3
"""Summary of a rocprofv3 --pmc pass with the LDS counters (SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE
SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES, a pass of its own, no trace domains) of the bench command for the tick
kernel -> profiles/<name>.json.

    python tools/lds_counters.py <counter_collection.csv> <kernel substring> <batch> <waves per controller> <name> [<library>]

Per launch averages, then per wave and tick (a launch fuses 10 ticks), the bank-conflict ratio SQ_LDS_BANK_CONFLICT /
SQ_LDS_IDX_ACTIVE (conflict cycles per cycle the LDS index unit is busy) and the share of the waves' cycles spent waiting
for an LDS instruction (SQ_WAIT_INST_LDS / SQ_WAVE_CYCLES, both summed over waves)."""
import collections
import csv
import hashlib
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
path, kernel, batch, waves_per_ctrl, name = sys.argv[1], sys.argv[2], int(sys.argv[3]), float(sys.argv[4]), sys.argv[5]
lib = sys.argv[6] if len(sys.argv) > 6 else os.path.join(root, "cgmres_cpp_amd", "lib", "libcgmres_hip.so")
ticks_per_launch = 10
acc = collections.defaultdict(lambda: [0, 0.0])
kname = None
for r in csv.DictReader(open(path)):
    if kernel not in r["Kernel_Name"]:
        continue
    kname = r["Kernel_Name"]
    a = acc[r["Counter_Name"]]
    a[0] += 1
    a[1] += float(r["Counter_Value"])
out = {k: v / n for k, (n, v) in acc.items()}
waves = batch * waves_per_ctrl
res = dict(out)
res["kernel"] = kname
res["launches"] = max(n for n, _ in acc.values())
res["per_wave_and_tick"] = {k: out[k] / waves / ticks_per_launch for k in out}
res["lds_bank_conflict_ratio"] = out["SQ_LDS_BANK_CONFLICT"] / out["SQ_LDS_IDX_ACTIVE"]
res["wait_inst_lds_share_of_wave_cycles"] = out["SQ_WAIT_INST_LDS"] / out["SQ_WAVE_CYCLES"]
res["library_sha256_16"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
res["note"] = (f"rocprofv3 --pmc (own pass, no trace domains) of `bench.py --steps 100 --warmup 20 --reps 1 --check-sample 0 "
               f"--no-cpu-baseline --no-ref-mode` at batch {batch}: {res['launches']} launches of 10 ticks averaged")
json.dump(res, open(os.path.join(root, "profiles", name + ".json"), "w"), indent=1)
print(json.dumps({k: res[k] for k in ("per_wave_and_tick", "lds_bank_conflict_ratio", "wait_inst_lds_share_of_wave_cycles")}, indent=1))
