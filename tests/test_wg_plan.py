"""CPU tests of the wg planner (csrc/wg_plan.hip.h: plan_wg decides the kernel, the LDS plan and the launch geometry of a
controller batch from the configuration, the CU count and the model's traits) and of the LDS carve-up it sizes (WgLds).

tests/plan_probe.py builds tests/plan_probe.hip with the library's compiler and flags into the library's build
directory, loads it with ctypes and runs it on the CPU (tests/kernel_classes.py uses the same module).
tests/data/wg_plan_parent.json holds what the library decided before the planner existed (commit `parent_commit`,
recorded on a `cus`-CU MI355X through CgmresBatch(...) with a print in CtxWg::init) over the grid of
tests/wg_plan_grid.py, one result per row of grid() in its order: an index into `results`, whose entries are
`result_fields` (the first an index into `decisions`: `decision_fields`, the first of those an index into `names`),
"lane" (library's choice went to the lane mapping because no wg plan fits), "unsupported" (cgmres_hip_create's
"variant N does not support model ..."), or the text of another refusal.  The `table` fixture expands them to full
rows."""
import json
import os

import pytest

import plan_probe
import wg_plan_grid as G
from plan_probe import PLAN_FH_HBM, PLAN_FULL, PLAN_LEAN, check_layout, config, layout, plan

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def probe():
    return plan_probe.probe()


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


def test_the_planner_sees_no_kernel_code():
    """The planner's translation unit (tests/plan_probe.hip) depends on no project header that holds a kernel: the
    compiler's own dependency listing of it names the layout headers and the model traits only."""
    from cgmres_cpp_amd import build as B
    plan_probe.probe()
    root = os.path.dirname(HERE)
    deps = {os.path.realpath(d) for d in B.read_deps(plan_probe.PROBE_SO)}
    own = sorted(d for d in deps if d.startswith(root + os.sep) and os.path.isfile(d))
    assert any(d.endswith("wg_plan.hip.h") for d in own) and any(d.endswith("wg_layout.hip.h") for d in own), own
    with_kernel = [os.path.relpath(d, root) for d in own if "__global__" in open(d).read()]
    assert not with_kernel, with_kernel
