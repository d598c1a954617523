#!/usr/bin/env python3
"""What recording the fused closed loop costs (needs an MI355X).

    python tools/bench_record.py [--out profiles/record_cost.json] [--parent-lib _ab/parent/lib.so] [--calls 20] [--ticks 200]

The headline handle (pendulum, fp64, 4096 controllers, dv = 50, k_max = 10, the library's choice of mapping).  Every leg
takes a fresh handle from the same start, runs 200 warm-up ticks, then `calls` closed-loop calls of `ticks` ticks each
between timer_start / timer_stop (HIP events on the handle's stream); the figure of a leg is the median call, in
microseconds per tick.  One process at a time, one job on the GPU.
    plain               closed_loop_device of this library
    plain_parent        the same on the parent commit's library (--parent-lib: a build of the parent's sources, e.g.
                        `AB_SRC_ROOT=<parent checkout> python tools/ab_build.py build parent:`), in a child process
                        (CGMRES_HIP_LIB).  The two run the same tick code objects: their difference is the noise floor
                        every other line is read against.
    stride{10,5,2,1}_logs_ensemble    closed_loop_device(record=...) with the four logs, t, moments and counts
    stride{10,5,2,1}_ensemble         ... with moments and counts alone
    us_ensemble_call    one cgmres_hip_ensemble_device (both kernels) behind the loop, median of 200 single calls and
                        back to back: the record kernel's own time
Derived: us_per_record_stride10 = (stride-10 leg - plain) * 10, the cost of one record where no launch is added;
stride1_over_plain, the whole price of a record per tick (fusion given up, one record per tick), next to the 7 % DESIGN
§4.1 gives for fusion alone."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cgmres_cpp_amd as cg  # noqa: E402
from cgmres_cpp_amd import scenarios  # noqa: E402

MODEL, B, DV, KMAX, WARMUP = "pendulum", 4096, 50, 10, 200
STRIDES = (10, 5, 2, 1)


def leg(calls, ticks, stride=None, logs=False, ensemble_calls=0):
    x0, u0, p = scenarios.batch(cg.PENDULUM, B)
    c = cg.CgmresBatch(MODEL, batch=B, dv=DV, k_max=KMAX)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    bufs = [c.device_buffer((B, c.dim_x)).upload(x0), c.device_buffer((B, c.dim_u))]
    xd, ud = bufs
    rec = None
    if stride:
        n_rec, nc = ticks // stride, c.dim_x + c.dim_u
        rec = dict(stride=stride, moments=c.device_buffer((n_rec, nc, 4), np.float64),
                   counts=c.device_buffer((n_rec, KMAX + 7), np.int32))
        if logs:
            rec.update(x=c.device_buffer((n_rec, B, c.dim_x)), u=c.device_buffer((n_rec, B, c.dim_u)),
                       n_ax=c.device_buffer((n_rec, B), np.int32), reason=c.device_buffer((n_rec, B), np.int32), t=np.zeros(n_rec))
        bufs += [b for b in rec.values() if isinstance(b, cg.DeviceBuffer)]
    kw = dict(record=rec) if rec else {}
    c.closed_loop_device(xd, ud, WARMUP)
    if rec:
        c.closed_loop_device(xd, ud, ticks, **kw)  # (the scratch of the record grows here)
    c.synchronize()
    ms = []
    for _ in range(calls):
        c.timer_start()
        c.closed_loop_device(xd, ud, ticks, **kw)
        ms.append(c.timer_stop())
    ms.sort()
    out = dict(us_per_tick=round(1e3 * ms[calls // 2] / ticks, 3), us_per_tick_min_max=[round(1e3 * ms[0] / ticks, 3), round(1e3 * ms[-1] / ticks, 3)],
               variant_name=c.variant_name)
    if ensemble_calls:
        md, cd = c.device_buffer((c.dim_x + c.dim_u, 4), np.float64), c.device_buffer((KMAX + 7,), np.int32)
        bufs += [md, cd]
        c.ensemble_device(xd, ud, moments=md, counts=cd)
        one = []
        for _ in range(ensemble_calls):
            c.timer_start()
            c.ensemble_device(xd, ud, moments=md, counts=cd)
            one.append(1e3 * c.timer_stop())
        one.sort()
        c.timer_start()
        for _ in range(ensemble_calls):
            c.ensemble_device(xd, ud, moments=md, counts=cd)
        out["us_ensemble_call"] = round(one[ensemble_calls // 2], 2)
        out["us_ensemble_call_back_to_back"] = round(1e3 * c.timer_stop() / ensemble_calls, 2)
        out["counting_instances"] = int(cd.download()[KMAX + 6])
    for b in bufs:
        b.free()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_cost.json"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--child", action="store_true", help="the plain leg only, as one JSON line (the parent library's leg)")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(leg(a.calls, a.ticks)))
        return
    rec = dict(config=dict(model=MODEL, dtype="f64", batch=B, dv=DV, k_max=KMAX, warmup_ticks=WARMUP, calls=a.calls, ticks_per_call=a.ticks),
               library_sha256_16=hashlib.sha256(open(cg.lib_path(), "rb").read()).hexdigest()[:16], legs={})
    legs = rec["legs"]

    def parent():
        env = dict(os.environ, CGMRES_HIP_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--ticks", str(a.ticks)],
                           env=env, capture_output=True, text=True, check=True)
        return json.loads(r.stdout.strip().split("\n")[-1])
    legs["plain"] = leg(a.calls, a.ticks, ensemble_calls=200)
    if a.parent_lib:
        legs["plain_parent"] = parent()
    for s in STRIDES:
        legs[f"stride{s}_logs_ensemble"] = leg(a.calls, a.ticks, s, True)
        legs[f"stride{s}_ensemble"] = leg(a.calls, a.ticks, s, False)
    legs["plain_again"] = leg(a.calls, a.ticks)  # (the drift of the machine over the run)
    if a.parent_lib:
        legs["plain_parent_again"] = parent()
    plain = legs["plain"]["us_per_tick"]
    floor = [abs(legs[k]["us_per_tick"] - plain) for k in ("plain_parent", "plain_again", "plain_parent_again") if k in legs]
    rec["us_noise_floor_per_tick"] = round(max(floor), 3)
    rec["us_per_record_stride10"] = {k: round((legs[f"stride10_{k}"]["us_per_tick"] - plain) * 10, 2) for k in ("logs_ensemble", "ensemble")}
    rec["us_record_kernels_own_time"] = legs["plain"]["us_ensemble_call_back_to_back"]
    rec["stride_over_plain"] = {k: round(v["us_per_tick"] / plain, 4) for k, v in legs.items() if k.startswith("stride")}
    rec["design_4_1_fusion_gain"] = 0.07
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
