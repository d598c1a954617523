#!/usr/bin/env python3
"""Diagnostic (never part of the product build): the angle increments the row-Newton sweep hands to its rotation, over
closed-loop ticks at the headline size, from a -DCGM_AMAX build of the library (csrc/wg_stamps.hip.h: cgm_amax_record).

    python tools/rot_increments.py [--lib=PATH] [--build] [--batch=4096] [--dv=50] [--kmax=10] [--ticks=250] [--json=FILE]
                                   [--tol=0] [--h=H --zeta=Z ...]   (tuning constants other than the shipped ones)

Prints, for the first Newton iteration of a sweep (the change of x0 under U + h v) and for the later ones (the Newton
correction), the largest increment and the share of wave visits with an increment above 2^-18, 2^-14, 2^-10, 2^-8, 2^-6."""
import ctypes, json, os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cgmres_cpp_amd import build as b

diag = os.path.join(ROOT, "_diag")  # git-ignored
os.makedirs(diag, exist_ok=True)


def opt(name, default, conv=int):
    for a in sys.argv:
        if a.startswith(f"--{name}="):
            return conv(a.split("=", 1)[1])
    return default


lib = os.path.abspath(opt("lib", os.path.join(diag, "libcgmres_hip_amax.so"), str))
if "--build" in sys.argv or not os.path.exists(lib):
    b.build(force="--build" in sys.argv, lib=lib, obj_dir=os.path.join(diag, "amax"), flags=["-DCGM_AMAX"])
b.LIB_PATH = lib
import cgmres_cpp_amd as cg
from cgmres_cpp_amd import scenarios

B, DV, KM, TICKS = opt("batch", 4096), opt("dv", 50), opt("kmax", 10), opt("ticks", 250)
x0, u0, p = scenarios.batch("pendulum", B)
tuning = {k: opt(k, None, float) for k in ("dt", "h", "zeta", "Tf", "alpha") if opt(k, None, float) is not None}
c = cg.CgmresBatch("pendulum", batch=B, dv=DV, k_max=KM, tol=opt("tol", 0.0, float), variant=2, **tuning)
assert c.variant_name == "wg+row-newton", c.variant_name
c.set_ptau_repeat(p); c.init_u0(u0); c.init_u0_newton(u0, x0, p, 10)
xd = c.device_buffer(x0.shape).upload(x0); ud = c.device_buffer(u0.shape)
L = cg.load()
out = (ctypes.c_ulonglong * 16)()
L.cgmres_hip_debug_amax(out)  # (clears what the set-up left)
c.closed_loop_device(xd, ud, TICKS); c.synchronize()
assert L.cgmres_hip_debug_amax(out) == 0
res = dict(batch=B, dv=DV, k_max=KM, ticks=TICKS, tol=c.tol, h=c.h, zeta=c.zeta)
for base, name in ((0, "iteration 0 (change of x0 under U + h v)"), (8, "iterations >= 1 (Newton correction)")):
    w = [int(v) for v in out[base:base + 8]]
    amax = struct.unpack("d", struct.pack("Q", w[0]))[0]
    visits = max(1, w[1])
    row = dict(max=amax, log2_max=(None if amax == 0 else __import__("math").log2(amax)), wave_visits=w[1],
               share_above={k: w[2 + i] / visits for i, k in enumerate(("2^-18", "2^-14", "2^-10", "2^-8", "2^-6"))})
    res[name] = row
    print(name, json.dumps(row))
if opt("json", None, str):
    with open(opt("json", None, str), "w") as fh:
        json.dump(res, fh, indent=1)
