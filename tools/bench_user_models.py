#!/usr/bin/env python3
"""Per-tick time of USER models (plugins) on the lane, wg and wave mappings (needs an MI355X).

    python tools/bench_user_models.py [--ticks 20] [--warmup 10] [--batches 1,64,256,1024,2048,4096] [--models vdp,chain4]
                                      [--mappings lane,wg,wave] [--tols 0,model] [--out FILE]

Cases: VdpModel (tests/user_models/vdp_model.hpp, dv = 30, k_max = 6) and Chain4Model (tests/user_models/chain4_model.hpp,
dv = 25 and 50, k_max = 5), each at tol = 0 (every Arnoldi iteration) and at the model's tol.  One JSON line per
(model, dv, tol, batch, mapping): mean us per tick of closed_loop_device (HIP events around `ticks` fused ticks after
`warmup` ticks), the resolved mapping, the sha256 (16 hex digits) of libcgmres_hip.so and of the plugin.  A mapping that
cannot serve a case prints its error instead of a time."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cgmres_cpp_amd as cg  # noqa: E402
from cgmres_cpp_amd import plugin  # noqa: E402

UM = os.path.join(ROOT, "tests", "user_models")
MODELS = {  # name: (header, class, plugin name, dim_x, dim_u, dim_p, [(dv, k_max)], model tol)
    "vdp": (os.path.join(UM, "vdp_model.hpp"), "VdpModel", "vdp", 2, 3, 2, [(30, 6)], 1e-6),
    "chain4": (os.path.join(UM, "chain4_model.hpp"), "Chain4Model", "chain4_bench", 4, 1, 1, [(25, 5), (50, 5)], 1e-6),
}
MAPPINGS = {1: "lane", 2: "wg", 4: "wave"}


def sha16(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def scenario(name, B, nx, nu, npar):
    rng = np.random.default_rng(5)
    if name == "vdp":
        x0 = np.stack([1.0 + 0.5 * rng.random(B), -0.5 + 0.5 * rng.random(B)], axis=1)
        p = np.stack([0.5 * rng.random(B), 0.1 * rng.random(B)], axis=1)
        u0 = np.tile(np.array([0.1, 1.9, 0.03]), (B, 1))
    else:
        x0 = 0.3 + 0.2 * rng.random((B, nx)) - 0.11 * np.arange(nx)[None, :]
        p = 0.2 + 0.1 * rng.random((B, npar))
        u0 = np.full((B, nu), 0.1)
    return x0, u0, p


def run_case(mid, name, nx, nu, npar, dv, kmax, tol, B, variant, ticks, warmup):
    x0, u0, p = scenario(name, B, nx, nu, npar)
    c = cg.CgmresBatch(mid, batch=B, dv=dv, k_max=kmax, tol=tol, variant=variant)
    try:
        c.set_ptau_repeat(p)
        c.init_u0(u0)
        c.init_u0_newton(u0, x0, p, 10)
        xd, ud = c.device_buffer((B, nx)).upload(x0), c.device_buffer((B, nu))
        c.closed_loop_device(xd, ud, warmup)
        c.synchronize()
        c.timer_start()
        c.closed_loop_device(xd, ud, ticks)
        ms = c.timer_stop()
        u = ud.download()
        n_ax = c.get_status()[0]
        return dict(variant=c.variant, variant_name=c.variant_name, us_per_tick=round(1e3 * ms / ticks, 2),
                    mean_arnoldi=round(float(np.mean(n_ax)), 2), finite=bool(np.all(np.isfinite(u))))
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="1,64,256,1024,2048,4096")
    ap.add_argument("--models", default="vdp,chain4")
    ap.add_argument("--mappings", default="lane,wg,wave")
    ap.add_argument("--tols", default="0,model", help="0 and/or `model` (the model's own tol)")
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = sha16(cg.lib_path())
    out = open(a.out, "w") if a.out else None
    for name in a.models.split(","):
        hdr, cls, pname, nx, nu, npar, shapes, mtol = MODELS[name]
        so = plugin.build(hdr, cls=cls, name=pname)
        mid = plugin.register(so)
        for dv, kmax in shapes:
            for tol in (mtol if t == "model" else float(t) for t in a.tols.split(",")):
                for B in (int(b) for b in a.batches.split(",")):
                    for variant, mapping in ((v, m) for v, m in MAPPINGS.items() if m in a.mappings.split(",")):
                        rec = dict(model=cls, dv=dv, k_max=kmax, tol=tol, batch=B, mapping=mapping, ticks=a.ticks,
                                   library_sha256_16=lib, plugin_sha256_16=sha16(so))
                        try:
                            rec.update(run_case(mid, name, nx, nu, npar, dv, kmax, tol, B, variant, a.ticks, a.warmup))
                        except cg.CgmresHipError as e:
                            rec["error"] = str(e)
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()


if __name__ == "__main__":
    main()
