#!/usr/bin/env python3
"""Serial against row form of a caller's operator in the stand-alone Gmres (csrc/user_operator.hip.h), on one GPU.

    python tools/bench_gmres_user.py [--batch 4096] [--k-max 10] [--out profiles/gmres_row_ab.json]

Times cgmres_hip_gmres_user — the WALL time of the blocking call, host-to-device and device-to-host copies of x, b,
params and the status arrays included — for the convection-diffusion stencil of tests/user_models at len = 150 and 300,
tol = 0 (every solve runs all k_max iterations): one warm-up call, then the median of 5.  Both forms run in this one
process, the serial form (the operator contract before the row form existed: Op::Ax on lane 0) first, then the row form
(Op::Ax_row on all lanes).  Prints one JSON line: both times, their ratio, the plan of each solve, the library's hash."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cgmres_cpp_amd as cg  # noqa: E402
from cgmres_cpp_amd import plugin  # noqa: E402

UM = os.path.join(ROOT, "tests", "user_models")
FORMS = (("serial", os.path.join(UM, "gmres_ops.hpp"), "ConvDiffOp{n}", "convdiff{n}"),
         ("row", os.path.join(UM, "gmres_row_ops.hpp"), "ConvDiffRowOp{n}", "convdiff{n}_row"))


def sha16(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--k-max", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"what": "cgmres_hip_gmres_user, convection-diffusion stencil, fp64, tol 0: wall time of the blocking call "
                   "(PCIe copies of x, b, params and status included), one warm-up then the median of the calls; "
                   "serial form first, then the row form, one process",
           "batch": a.batch, "k_max": a.k_max, "calls": a.calls, "library_sha256_16": sha16(cg.lib_path()), "len": {}}
    for n in (150, 300):
        e = np.arange(n)
        i = np.arange(a.batch)[:, None] % 12  # the scenarios of the tests, cycled over the batch
        P = np.concatenate([0.4 + 0.07 * i, 0.35 - 0.02 * i], axis=1)
        Bv, X0 = np.sin(0.3 * e + 0.5 * i) + 0.1 * e, 0.01 * (e - i)
        entry, xs = {}, {}
        for form, hdr, cls, name in FORMS:
            so = plugin.build_operator(hdr, cls.format(n=n), name=name.format(n=n))
            oid = plugin.register_operator(so)
            times = []
            for c in range(a.calls + 1):
                t0 = time.perf_counter()
                x, n_ax, why = cg.gmres_user(oid, X0, Bv, a.k_max, 0.0, P)
                times.append(time.perf_counter() - t0)
            assert np.all(n_ax == a.k_max) and np.all(why == cg.EXIT_NATURAL)
            xs[form] = x
            entry[form] = {"plan": list(cg.operator_plan(oid, a.k_max)), "plugin_sha256_16": sha16(so),
                           "warmup_ms": 1e3 * times[0], "calls_ms": [1e3 * t for t in times[1:]],
                           "median_ms": 1e3 * statistics.median(times[1:])}
        entry["row_over_serial"] = entry["row"]["median_ms"] / entry["serial"]["median_ms"]
        entry["row_not_slower"] = entry["row"]["median_ms"] <= entry["serial"]["median_ms"]
        entry["max_abs_x_row_minus_x_serial"] = float(np.max(np.abs(xs["row"] - xs["serial"])))
        res["len"][str(n)] = entry
    line = json.dumps(res)
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
