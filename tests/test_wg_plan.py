"""CPU tests of the wg planner (csrc/wg_plan.hip.h: plan_wg decides the kernel, the LDS plan and the launch geometry of a
controller batch from the configuration, the CU count and the model's traits) and of the LDS carve-up it sizes (WgLds).

tests/plan_probe.hip is built with the library's compiler and flags into the library's build directory, loaded with
ctypes and run on the CPU.  tests/data/wg_plan_parent.json holds what the library decided before the planner existed
(commit `parent_commit`, recorded on a `cus`-CU MI355X through CgmresBatch(...) with a print in CtxWg::init) over the grid
of tests/wg_plan_grid.py, one result per row of grid() in its order: an index into `results`, whose entries are
`result_fields` (the first an index into `decisions`: `decision_fields`, the first of those an index into `names`),
"lane" (library's choice went to the lane mapping because no wg plan fits), "unsupported" (cgmres_hip_create's
"variant N does not support model ..."), or the text of another refusal.  The `table` fixture expands them to full
rows."""
import ctypes as C
import json
import os
import subprocess

import pytest

import cgmres_cpp_amd as cg
import wg_plan_grid as G
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


@pytest.fixture(scope="module")
def probe():
    _, hdrs = B.sources()
    if not os.path.exists(PROBE_SO) or any(os.path.getmtime(d) > os.path.getmtime(PROBE_SO) for d in hdrs + [PROBE_SRC]):
        os.makedirs(B.LIB_DIR, exist_ok=True)
        r = subprocess.run([B.HIPCC] + B.CFLAGS + ["-shared", "-o", PROBE_SO, PROBE_SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(PROBE_SO)
    lib.lds_limit.restype = C.c_longlong
    return lib


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "data", "wg_plan_parent.json")) as fh:
        t = json.load(fh)
    bytes_f = ["lds_bytes", "lds_bytes_hook", "lds_bytes_tick"]
    assert t["names"] == G.NAMES and ["variant_name"] + t["decision_fields"][1:] == [f for f in G.FIELDS[:-1] if f not in bytes_f]
    assert t["result_fields"][:4] == ["decision"] + bytes_f
    grid = G.grid()
    assert t["grid_digest"] == G.digest() and len(t["rows"]) == len(grid), "the file was recorded over another grid"

    def decode(row, res):
        if res == "unsupported":  # (the text of cgmres_hip_create, not of the wg context)
            return "error: cgmres_hip error -1: variant %d does not support model %d with dv = %d, k_max = %d" % (row[5], row[0], row[2], row[3])
        if isinstance(res, str):
            return res if res == "lane" else "error: cgmres_hip error -1: " + res
        d = dict(zip(t["decision_fields"], t["decisions"][res[0]]), **dict(zip(bytes_f, res[1:4])))
        d["variant_name"] = G.NAMES[d["name"]]
        return [d[f] for f in G.FIELDS[:-1]] + [res[4:12] or [0] * 8]

    t["rows"] = [row + (decode(row, t["results"][i]),) for row, i in zip(grid, t["rows"])]
    return t


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


def test_the_table_holds_the_whole_grid(table):
    have = {r[:8] for r in table["rows"]}
    assert len(have) == len(table["rows"])
    missing = [r for r in G.grid() if r not in have]
    assert not missing, missing[:5]
    assert any(r[:4] == (2, 0, 3, 3) and not isinstance(r[8], str) and r[8][0] == "wg+row-scan" for r in table["rows"])


def test_same_decisions_as_before_the_planner(probe, table):
    """Field for field on every row.  The one exception: a row-scan result's lds_bytes (and lds_bytes_tick, the same
    number) is larger by the NWT_TABX spare scalars per stage of the stage table its kernel lays out and the old byte count
    left out: (dv + TAB_PAD) * NWT_TABX * sizeof(T).
    Refusals: the library used to answer "variant N does not support ..." (explicit variant) or fall back to the lane
    mapping (library's choice) when CtxWg::supported said no — plan_wg's own refusal, with k.ipw == 0, is what
    make_variant maps to exactly these two; every other refusal came from CtxWg::init and keeps its text."""
    bad = []
    for row in table["rows"]:
        cfg, want = config(*row[:8]), row[8]
        got, why = plan(probe, cfg, table["cus"])
        if isinstance(want, str):
            if want == "lane" or "does not support model" in want:
                L = layout(probe, cfg, 16, 0, PLAN_FULL)["NU"] * row[2]  # dim_u * dv
                ok = got is None and why == f"wg mapping: dim_u*dv = {L} / LDS footprint not supported"
                ok = ok and (want == "lane") == (row[5] == 0)
            else:
                ok = got is None and want == "error: cgmres_hip error -1: " + why
        else:
            want = dict(zip(G.FIELDS, want))
            want["base_off"] = want["base_off"][:8]
            if want["variant_name"] == "wg+row-scan":
                lay = layout(probe, cfg, 16, 1, PLAN_FULL)
                extra = (row[2] + lay["TAB_PAD"]) * lay["NWT_TABX"] * lay["sizeof_T"]
                want["lds_bytes"] += extra
                want["lds_bytes_tick"] += extra
            ok = got == want
        if not ok:
            bad.append((row, got, why))
    assert not bad, (len(bad), bad[:3])


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


def test_the_allocation_covers_the_layout(probe, table):
    n, bad = 0, []
    for row in table["rows"]:
        cfg = config(*row[:8])
        r, _ = plan(probe, cfg, table["cus"])
        if r is None:
            continue
        n += 1
        problems = check_layout(probe, cfg, r)
        if problems:
            bad.append((row[:8], problems))
    assert n == sum(1 for row in table["rows"] if not isinstance(row[8], str))
    assert not bad, (len(bad), bad[:3])


def test_the_old_row_scan_byte_count_did_not_cover_the_layout(probe, table):
    """semiactive fp64, dv = 3, k_max = 3: with the recorded lds_bytes the last words of binst lie behind the allocation."""
    rows = [r for r in table["rows"] if r[:4] == (2, 0, 3, 3) and not isinstance(r[8], str) and r[8][0] == "wg+row-scan"]
    assert rows
    for row in rows:
        cfg, old = config(*row[:8]), dict(zip(G.FIELDS, row[8]))
        r, _ = plan(probe, cfg, table["cus"])
        lay = layout(probe, cfg, 16, 1, PLAN_FULL)
        assert lay["binst_end"] - old["lds_bytes"] == 8
        assert any("binst ends" in p for p in check_layout(probe, cfg, r, lds_bytes=old["lds_bytes"]))
        assert not check_layout(probe, cfg, r)


def test_the_planner_is_pure(probe, table):
    """Deterministic; device, stream and the scalars h, dt, zeta, Tf, alpha do not enter; tol only enters `binning`."""
    rows = table["rows"][::7]
    for row in rows:
        base = plan(probe, config(*row[:8]), table["cus"])
        assert plan(probe, config(*row[:8]), table["cus"]) == base
        other = config(*row[:8], device=3, stream=0x1000, h=0.5, dt=0.25, zeta=1.0, Tf=7.0, alpha=3.0, model_id=row[0])
        assert plan(probe, other, table["cus"]) == base
        for tol in (0.0, 1e-3):
            got = plan(probe, config(*row[:7], tol), table["cus"])
            if base[0] is None:
                assert got == base
            else:
                assert {k: v for k, v in got[0].items() if k != "binning"} == {k: v for k, v in base[0].items() if k != "binning"}
                if tol == 0.0:
                    assert got[0]["binning"] == 0
