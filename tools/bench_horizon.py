#!/usr/bin/env python3
"""What cgmres_hip_horizon_device costs beside one control tick (needs an MI355X).

    python tools/bench_horizon.py [--out profiles/horizon_cost.json] [--direct-lib _ab/direct/lib.so] [--calls 200] [--ticks 200]

The headline handle (pendulum, fp64, 4096 controllers, dv = 50, k_max = 10, the library's choice of mapping) runs `ticks`
fused closed-loop ticks; then, in the same process and all between timer_start / timer_stop (HIP events on the handle's
stream) after a warm-up of each form:
    us_all_outputs    median of `calls` horizon_device calls that fill xtau, ltau, F and fnorm
    us_fnorm_only     median of `calls` calls that fill fnorm alone (x, trig and F go through the context's scratch)
    us_*_back_to_back `calls` calls enqueued behind each other, total / calls (a caller that scores every tick)
    us_per_tick       `ticks` further fused ticks, total / ticks
    fnorm_over_tick   us_fnorm_only / us_per_tick: the figure that matters
The record also holds the sha256 (16 hex digits) of the library and the compiler's resource-usage lines of the kernel
(hipcc -Rpass-analysis=kernel-resource-usage on the instantiation the handle runs: registers, LDS, scratch).
--direct-lib: a library built with -DCGM_HORIZON_DIRECT (tools/ab_build.py build direct:-DCGM_HORIZON_DIRECT), the
straightforward kernel that loads U, ptau, x and trig from global memory in every stage; it is timed the same way in a
child process of its own (CGMRES_HIP_LIB) and recorded under "direct", with the largest difference of the two kernels'
outputs."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cgmres_cpp_amd as cg  # noqa: E402
from cgmres_cpp_amd import build as _build, scenarios  # noqa: E402

MODEL, B, DV, KMAX = "pendulum", 4096, 50, 10
PROBE = """#include "horizon.hip.h"
template __global__ void cgm::horizon_kernel<cgm::PendulumDev<double>, double, %s>(cgm::HorizonParams<double>);
"""


def resource_usage(rows, flags=()):
    """The compiler's remarks for the fp64 pendulum instantiation (rows: the wg contexts' layout)."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "horizon_probe.hip")
        with open(src, "w") as f:
            f.write(PROBE % ("true" if rows else "false"))
        r = subprocess.run([_build.HIPCC] + _build.CFLAGS + list(flags) + ["-c", "-Rpass-analysis=kernel-resource-usage", "-I", _build.CSRC,
                            "-o", os.path.join(d, "probe.o"), src], capture_output=True, text=True, check=True)
    keep = ("Function Name", "SGPRs:", "VGPRs:", "AGPRs:", "ScratchSize", "Occupancy", "LDS Size")
    return [re.sub(r"^.*remark:\s*(.*?)\s*\[-Rpass-analysis.*$", r"\1", l) for l in r.stderr.splitlines()
            if any(k in l for k in keep)]


def measure(calls, ticks, dump=None):
    x0, u0, p = scenarios.batch(cg.PENDULUM, B)
    c = cg.CgmresBatch(MODEL, batch=B, dv=DV, k_max=KMAX)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    xd, ud = c.device_buffer((B, c.dim_x)).upload(x0), c.device_buffer((B, c.dim_u))
    outs = dict(xtau=c.device_buffer((B, DV + 1, c.dim_x)), ltau=c.device_buffer((B, DV + 1, c.dim_x)),
                F=c.device_buffer((B, c.len)), fnorm=c.device_buffer((B,)))
    c.closed_loop_device(xd, ud, ticks)
    c.synchronize()

    def timed(kw, n):
        c.timer_start()
        for _ in range(n):
            c.horizon_device(xd, **kw)
        return 1e3 * c.timer_stop()

    rec = dict(variant_name=c.variant_name, calls=calls, ticks=ticks)
    for name, kw in (("all_outputs", outs), ("fnorm_only", dict(fnorm=outs["fnorm"]))):
        timed(kw, 10)  # warm-up: the code object, and the scratch of this form grows here
        one = sorted(timed(kw, 1) for _ in range(calls))
        rec["us_" + name] = round(one[calls // 2], 2)
        rec["us_" + name + "_min_max"] = [round(one[0], 2), round(one[-1], 2)]
        rec["us_" + name + "_back_to_back"] = round(timed(kw, calls) / calls, 2)
    fn = outs["fnorm"].download()
    if dump:
        c.horizon_device(xd, **outs)
        np.savez(dump, **{k: v.download() for k, v in outs.items()})
    c.timer_start()
    c.closed_loop_device(xd, ud, ticks)
    rec["us_per_tick"] = round(1e3 * c.timer_stop() / ticks, 2)
    rec["fnorm_over_tick"] = round(rec["us_fnorm_only"] / rec["us_per_tick"], 4)
    rec["all_outputs_over_tick"] = round(rec["us_all_outputs"] / rec["us_per_tick"], 4)
    finite = np.isfinite(fn)
    rec["fnorm_finite"], rec["fnorm_median"] = int(finite.sum()), float(np.median(fn[finite]))
    rec["library_sha256_16"] = hashlib.sha256(open(cg.lib_path(), "rb").read()).hexdigest()[:16]
    rows = c.variant != 1
    c.close()
    return rec, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horizon_cost.json"))
    ap.add_argument("--direct-lib")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--child", action="store_true", help="print the record as one JSON line and write no file")
    ap.add_argument("--dump", help="also write the four outputs after the first loop to this .npz")
    a = ap.parse_args()
    rec, rows = measure(a.calls, a.ticks, a.dump)
    if a.child:
        print(json.dumps(rec))
        return
    rec = dict(config=dict(model=MODEL, dtype="f64", batch=B, dv=DV, k_max=KMAX), **rec)
    rec["kernel_resource_usage"] = resource_usage(rows)
    if a.direct_lib:
        with tempfile.TemporaryDirectory() as d:
            mine, theirs = os.path.join(d, "staged.npz"), os.path.join(d, "direct.npz")
            measure(1, a.ticks, mine)  # (a second handle from the same start: the outputs the child's are compared with)
            env = dict(os.environ, CGMRES_HIP_LIB=os.path.abspath(a.direct_lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--ticks", str(a.ticks),
                                "--dump", theirs], env=env, capture_output=True, text=True, check=True)
            rec["direct"] = json.loads(r.stdout.strip().split("\n")[-1])
            rec["direct"]["kernel_resource_usage"] = resource_usage(rows, ("-DCGM_HORIZON_DIRECT",))
            za, zb = np.load(mine), np.load(theirs)
            rec["direct"]["max_abs_difference_to_staged"] = {
                k: float(np.nanmax(np.abs(za[k] - zb[k]))) for k in za.files}
            rec["direct"]["nan_pattern_equal"] = bool(all(np.array_equal(np.isnan(za[k]), np.isnan(zb[k])) for k in za.files))
        rec["staged_over_direct_fnorm_only"] = round(rec["us_fnorm_only"] / rec["direct"]["us_fnorm_only"], 4)
        rec["staged_over_direct_all_outputs"] = round(rec["us_all_outputs"] / rec["direct"]["us_all_outputs"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
