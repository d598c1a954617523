#!/usr/bin/env python3
"""What previewing a sampled reference signal inside the device loop costs (needs an MI355X).

    python tools/preview_cost.py [--out profiles/preview_cost.json] [--calls 20] [--ticks 200]

The headline handle (pendulum, fp64, 4096 controllers, dv = 50, k_max = 10, the library's choice of mapping), two of them
from the same start, in one process:
    preview     closed_loop_device(preview=Preview(sig)): the rows of every launch written by preview_kernel in front of it
    ptau_seq    closed_loop_device(ptau_seq_dev=rows) over the rows cgmres_hip_preview_device exported for the same ticks
Both run 200 warm-up ticks of the plain loop, then `calls` closed-loop calls of `ticks` ticks each between timer_start /
timer_stop (HIP events on the handle's stream), ALTERNATING preview, ptau_seq, preview, ...  Both handles' clocks run on
from call to call; in front of every call of the ptau_seq leg, outside its timed window, its rows are exported for the
ticks to come, so call for call the two legs run the same horizons and, the loops being bit-identical (checked at the end),
the same solver work.  The yardstick is the ptau_seq leg of the same library in the same job.  Per leg: the
median call in microseconds per tick and the run-to-run spread (min, max, quartiles).  Also recorded: the bytes of
sequence memory the preview saves at this shape, for this run and for a 10 000-tick loop."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cgmres_cpp_amd as cg  # noqa: E402
from cgmres_cpp_amd import scenarios  # noqa: E402

MODEL, B, DV, KMAX, WARMUP = "pendulum", 4096, 50, 10, 200


def handle():
    x0, u0, p = scenarios.batch(cg.PENDULUM, B)
    c = cg.CgmresBatch(MODEL, batch=B, dv=DV, k_max=KMAX)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    xd, ud = c.device_buffer((B, c.dim_x)).upload(x0), c.device_buffer((B, c.dim_u))
    c.closed_loop_device(xd, ud, WARMUP)
    c.synchronize()
    return c, xd, ud, p


def stats(ms, ticks):
    us = np.sort(1e3 * np.asarray(ms) / ticks)
    q = lambda f: round(float(np.quantile(us, f)), 3)  # noqa: E731
    return dict(us_per_tick=q(0.5), us_per_tick_min_max=[q(0.0), q(1.0)], us_per_tick_quartiles=[q(0.25), q(0.75)],
                us_run_to_run_spread=round(float(us[-1] - us[0]), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preview_cost.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    a = ap.parse_args()
    ticks = a.ticks
    ca, xa, ua, p = handle()
    cb, xb, ub, _ = handle()
    t_start = ca.t
    # the pendulum's set point follows a slow sinusoid, one sample per tick, per instance
    j = np.arange((a.calls + 1) * ticks + 64)
    sig = np.ascontiguousarray(p[:, None, :] * (1.0 + 0.05 * np.sin(2 * np.pi * 0.5 * ca.dt * j)[None, :, None]))
    pv = cg.Preview(ca.device_buffer(sig.shape).upload(sig), ca.dt, t_start, "linear")
    rows = cb.device_buffer((ticks, B, cb.dim_p * (DV + 1)))
    pv_b = cg.Preview(cb.device_buffer(sig.shape).upload(sig), cb.dt, t_start, "linear")

    def export():  # the rows of the next `ticks` ticks of the ptau_seq handle, outside the timed window
        cb.preview_device(pv_b, ticks, rows)
        cb.synchronize()
    legs = {"preview": (ca, xa, ua, dict(preview=pv)), "ptau_seq": (cb, xb, ub, dict(ptau_seq_dev=rows))}
    ms = {k: [] for k in legs}
    for k, (c, xd, ud, kw) in legs.items():  # one untimed call of each: the ring, the code objects
        if k == "ptau_seq":
            export()
        c.closed_loop_device(xd, ud, ticks, **kw)
        c.synchronize()
    for _ in range(a.calls):
        for k, (c, xd, ud, kw) in legs.items():
            if k == "ptau_seq":
                export()
            c.timer_start()
            c.closed_loop_device(xd, ud, ticks, **kw)
            ms[k].append(c.timer_stop())
    x_end = xa.download()
    same = bool(np.array_equal(x_end, xb.download()) and np.array_equal(ua.download(), ub.download()))
    es, W = 8, ca.dim_p * (DV + 1)
    rec = dict(config=dict(model=MODEL, dtype="f64", batch=B, dv=DV, k_max=KMAX, warmup_ticks=WARMUP, calls=a.calls, ticks_per_call=ticks,
                           order="alternating: preview, ptau_seq, ..."),
               library_sha256_16=hashlib.sha256(open(cg.lib_path(), "rb").read()).hexdigest()[:16], variant_name=ca.variant_name,
               legs={k: stats(v, ticks) for k, v in ms.items()}, legs_end_bit_identical=same, legs_end_finite=bool(np.all(np.isfinite(x_end))))
    d = rec["legs"]["preview"]["us_per_tick"] - rec["legs"]["ptau_seq"]["us_per_tick"]
    rec["us_preview_minus_ptau_seq_per_tick"] = round(d, 3)
    rec["us_preview_minus_ptau_seq_per_launch"] = round(d * cg.TICKS_PER_LAUNCH, 3)
    rec["bytes"] = dict(sequence_this_run=ticks * B * W * es, sequence_10000_ticks=10000 * B * W * es,
                        signal_this_run=int(sig.nbytes), signal_10000_ticks=10000 * B * ca.dim_p * es,
                        ring=cg.TICKS_PER_LAUNCH * B * W * es)
    try:  # the figure the issue names for comparison: what a stride-10 record costs over its plain loop
        rc = json.load(open(os.path.join(ROOT, "profiles", "record_cost.json")))["legs"]
        rec["us_stride10_record_over_plain_per_tick"] = round(rc["stride10_logs_ensemble"]["us_per_tick"] - rc["plain"]["us_per_tick"], 3)
    except (OSError, KeyError):
        pass
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
