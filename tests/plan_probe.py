"""The CPU probe of the wg planner as a plain module: tests/plan_probe.hip built with the library's compiler and flags
into the library's build directory and loaded with ctypes, plus the helpers that drive it.  No GPU call is made and
nothing is imported from conftest; tests/test_wg_plan.py and tests/kernel_classes.py share it.  probe_user() is the
same for tests/plan_probe_user.hip (user models: cfg.model_id is the index of an alias of
tests/user_models/shape_models.hpp); plan(), layout() and check_layout() work on either library."""
import ctypes as C
import os

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_SRC = os.path.join(HERE, "plan_probe.hip")
PROBE_SO = os.path.join(B.LIB_DIR, "wg_plan_probe.so")
EINVAL = -1
OUT = ["ipw", "maxm", "plan", "par", "cs_chunks", "nwt", "wave", "variant", "lds_bytes", "lds_bytes_hook", "lds_bytes_tick",
       "fh_hbm", "fh_hbm_hook", "binning"]
ARRAYS = ["U", "Fh", "W", "R", "p", "H", "rho", "g", "hsub", "xs", "xh", "xT", "u0", "flag", "reason", "nax", "ksolve", "binst",
          "binst_end", "scan"]
CONSTS = ["sizeof_T", "ipw", "NSTG", "NU", "tab_bytes", "scan_bytes", "scan2_bytes_3", "scan2_bytes_4", "TAB_PAD", "NWT_TABX",
          "base_array_bytes", "NBASE"]
PLAN_FULL, PLAN_FH_HBM, PLAN_LEAN = 0, 1, 2

USER_PROBE_SRC = os.path.join(HERE, "plan_probe_user.hip")
USER_PROBE_SO = os.path.join(B.LIB_DIR, "wg_plan_probe_user.so")
USER_MODELS_HPP = os.path.join(HERE, "user_models", "shape_models.hpp")

_libs = {}


def _load(src, so):
    """The probe library of `src`, built on first use and rebuilt when its source or a file it includes is newer."""
    if so not in _libs:
        _libs[so] = C.CDLL(B.compile(so, src, ["-shared"]))
        _libs[so].lds_limit.restype = C.c_longlong
    return _libs[so]


def probe():
    """The loaded probe library of the built-in models."""
    return _load(PROBE_SRC, PROBE_SO)


def probe_user():
    """The loaded probe library of the user models of tests/user_models/shape_models.hpp."""
    return _load(USER_PROBE_SRC, USER_PROBE_SO)


def alias_info(lib, alias):
    """dict(dim_x, dim_u, dim_p, NSTG, wave_fits) of alias number `alias` of the user probe"""
    out = (C.c_int * 5)()
    assert lib.alias_info(alias, out) == 0
    return dict(zip(["dim_x", "dim_u", "dim_p", "NSTG", "wave_fits"], out))


def config(model, dtype, dv, k_max, batch, variant, flags, tol, **over):
    cfg = cg.Config(abi_version=cg.ABI_VERSION, model_id=model, dtype=dtype, batch=batch, dv=dv, k_max=k_max, device=0,
                    variant=variant, flags=flags, reserved=0, tol=tol, dt=1e-3, h=1e-3, zeta=1000.0, Tf=1.0, alpha=0.5, stream=None)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def plan(lib, cfg, cus):
    """(dict of the result with variant_name and base_off, None) or (None, error text)"""
    out, name, why = (C.c_longlong * 22)(), C.create_string_buffer(512), C.create_string_buffer(512)
    rc = lib.plan_probe(C.byref(cfg), cus, out, name, why)
    if rc:
        assert rc == EINVAL
        return None, why.value.decode()
    r = dict(zip(OUT, out[:14]))
    r["variant_name"], r["base_off"] = name.value.decode(), list(out[14:22])
    return r, None


def layout(lib, cfg, ipw, tabx, lds_plan):
    out = (C.c_longlong * 32)()
    assert lib.layout_probe(C.byref(cfg), ipw, tabx, lds_plan, out) == 0
    return dict(zip(ARRAYS + CONSTS, out))


def check_layout(probe, cfg, r, lds_bytes=None):
    """The problems of plan `r` (a dict as plan() returns it) as a list of strings; lds_bytes: the tick kernel's allocation
    (default: the plan's own)."""
    lds_bytes = r["lds_bytes"] if lds_bytes is None else lds_bytes
    bad = []
    lean, nwt = r["plan"] == PLAN_LEAN, r["nwt"]
    lay = layout(probe, cfg, r["ipw"], 1 if nwt else 0, r["plan"])
    sz, ipw = lay["sizeof_T"], lay["ipw"]
    # every array starts inside and the last one (binst) ends inside the allocation; the arrays are carved in address order
    for a in ARRAYS:
        if not 0 <= lay[a] <= lds_bytes:
            bad.append(f"{a} at {lay[a]} outside {lds_bytes}")
    if lay["binst_end"] > lds_bytes:
        bad.append(f"binst ends at {lay['binst_end']} > lds_bytes {lds_bytes}")
    if lay["R"] + lay["tab_bytes"] > lay["H"]:
        bad.append("stage table runs into the arrays behind it")
    # costate scratch behind the aligned scan pointer (the row-parallel kernels run no such sweep: to them it is room for base arrays)
    scratch = {0: 0, 1: lay["scan_bytes"], 2: lay["scan2_bytes_%d" % r["cs_chunks"]] if r["par"] == 2 else 0}[r["par"]]
    if lay["scan"] % 16 or lay["scan"] < lay["binst_end"]:
        bad.append("scan pointer")
    if scratch and lay["scan"] + scratch > lds_bytes:
        bad.append(f"costate scratch ends at {lay['scan'] + scratch} > {lds_bytes}")
    limit = probe.lds_limit(1 if lean else 0)
    if lds_bytes > limit:
        bad.append(f"lds_bytes {lds_bytes} > limit {limit}")
    # look-ahead of the costate sweep (WgTraits::lookahead_fits): three stages below the table and below the first output row
    if lay["R"] // (sz * ipw) < 3 * lay["NSTG"] + 2 or lay["W"] // (sz * ipw) < 3 * lay["NU"]:
        bad.append("look-ahead below the stage table / the output row leaves the allocation")
    # row-Newton base arrays: in the stage table, in the costate scratch (both idle during the Arnoldi loop) or behind everything
    if nwt == 1:
        arr, n = lay["base_array_bytes"], lay["NBASE"]
        spans = sorted((o, o + arr) for o in r["base_off"][:n])
        live_end = max(lay["binst_end"], lay["scan"] + scratch)
        for i, (a, b) in enumerate(spans):
            in_tab = lay["R"] <= a and b <= lay["R"] + lay["tab_bytes"]
            in_scan = lay["scan"] <= a and b <= lay["scan"] + scratch
            if not (in_tab or in_scan or a >= live_end) or b > lds_bytes or a % 16:
                bad.append(f"base array [{a}, {b}) overlaps live LDS or leaves the allocation")
            if i and a < spans[i - 1][1]:
                bad.append(f"base arrays overlap at {a}")
    elif any(r["base_off"]):
        bad.append("base_off set without the row-Newton kernel")
    # the white-box hooks: the full / fh_hbm plan of the same sizes, plain stage table
    hook = layout(probe, cfg, r["ipw"], 0, PLAN_FH_HBM if r["fh_hbm_hook"] else PLAN_FULL)
    if hook["binst_end"] > r["lds_bytes_hook"] or r["lds_bytes_hook"] > probe.lds_limit(0):
        bad.append("hook kernel's allocation")
    if (not r["wave"] and r["lds_bytes_tick"] != r["lds_bytes"]) or r["lds_bytes_tick"] > probe.lds_limit(0):
        bad.append("lds_bytes_tick")
    return bad
