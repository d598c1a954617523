#!/usr/bin/env python3
"""What a closed loop against a plant of its own costs (needs an MI355X).

    python tools/bench_plant.py [--out profiles/plant_cost.json] [--parent-lib _ab/parent/lib.so] [--calls 20] [--ticks 200]

The headline handle (pendulum, fp64, 4096 controllers, dv = 50, k_max = 10, the library's choice of mapping).  Every leg
takes a fresh handle from the same start, runs 200 warm-up ticks of the plain loop, then `calls` closed-loop calls of
`ticks` ticks each between timer_start / timer_stop (HIP events on the handle's stream); the figure of a leg is the median
call, in microseconds per tick.  One process at a time, one job on the GPU.
    plain               closed_loop_device of this library (ten ticks per launch, the plant inside the tick kernel)
    plain_parent        the same on the parent commit's library (--parent-lib: a build of the parent's sources), in a child
                        process (CGMRES_HIP_LIB).  The two run the same tick code objects: their difference is the noise
                        floor every other line is read against, and the check that the plain loop has not moved.
    euler1, rk4_1, rk4_8            closed_loop_device(plant=Plant(...)) with nominal parameters: one tick per launch,
                                    the plant kernel behind every launch
    euler1_theta, rk4_1_theta, rk4_8_theta   the same with per-instance theta (nominal values: the trajectories agree)
    us_plant_step       one cgmres_hip_plant_step_device (RK4, 8 substeps, per-instance theta), back to back: the plant
                        kernel's own time
Derived: plant_over_plain per leg — the 7 % of fusion plus one kernel boundary per tick plus the plant."""
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
PLANTS = (("euler1", "euler", 1), ("rk4_1", "rk4", 1), ("rk4_8", "rk4", 8))


def leg(calls, ticks, integrator=None, substeps=1, theta=False, step_calls=0):
    x0, u0, p = scenarios.batch(cg.PENDULUM, B)
    c = cg.CgmresBatch(MODEL, batch=B, dv=DV, k_max=KMAX)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    bufs = [c.device_buffer((B, c.dim_x)).upload(x0), c.device_buffer((B, c.dim_u))]
    xd, ud = bufs
    kw = {}
    if integrator:
        th = None
        if theta:
            th = c.device_buffer((B, 7)).upload(np.tile(cg.plant_info(MODEL)["nominal"], (B, 1)))
            bufs.append(th)
        kw = dict(plant=cg.Plant(integrator, substeps, th))
    c.closed_loop_device(xd, ud, WARMUP)
    c.synchronize()
    ms = []
    for _ in range(calls):
        c.timer_start()
        c.closed_loop_device(xd, ud, ticks, **kw)
        ms.append(c.timer_stop())
    ms.sort()
    out = dict(us_per_tick=round(1e3 * ms[calls // 2] / ticks, 3), us_per_tick_min_max=[round(1e3 * ms[0] / ticks, 3), round(1e3 * ms[-1] / ticks, 3)],
               variant_name=c.variant_name)
    if step_calls:
        xs = c.device_buffer((B, c.dim_x)).upload(x0)
        bufs.append(xs)
        c.plant_step_device(xs, ud, kw["plant"])
        c.timer_start()
        for _ in range(step_calls):
            c.plant_step_device(xs, ud, kw["plant"])
        out["us_plant_step_back_to_back"] = round(1e3 * c.timer_stop() / step_calls, 2)
    for b in bufs:
        b.free()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_cost.json"))
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
    legs["plain"] = leg(a.calls, a.ticks)
    if a.parent_lib:
        legs["plain_parent"] = parent()
    for name, integrator, substeps in PLANTS:
        legs[name] = leg(a.calls, a.ticks, integrator, substeps)
        legs[name + "_theta"] = leg(a.calls, a.ticks, integrator, substeps, True, step_calls=200 if name == "rk4_8" else 0)
    legs["plain_again"] = leg(a.calls, a.ticks)  # (the drift of the machine over the run)
    if a.parent_lib:
        legs["plain_parent_again"] = parent()
    plain = legs["plain"]["us_per_tick"]
    if a.parent_lib:  # the parent's own run-to-run spread in this job, and how far this library's plain loop is from it
        pp = [legs["plain_parent"]["us_per_tick"], legs["plain_parent_again"]["us_per_tick"]]
        rec["us_parent_run_to_run_spread"] = round(abs(pp[0] - pp[1]), 3)
        rec["us_plain_minus_parent"] = round(min(plain, legs["plain_again"]["us_per_tick"]) - min(pp), 3)
    floor = [abs(legs[k]["us_per_tick"] - plain) for k in ("plain_parent", "plain_again", "plain_parent_again") if k in legs]
    rec["us_noise_floor_per_tick"] = round(max(floor), 3)
    rec["us_plant_kernel_own_time"] = legs["rk4_8_theta"]["us_plant_step_back_to_back"]
    rec["plant_over_plain"] = {k: round(v["us_per_tick"] / plain, 4) for k, v in legs.items() if not k.startswith("plain")}
    rec["design_4_1_fusion_gain"] = 0.07
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
