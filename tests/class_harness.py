"""What tests/test_gpu_kernel_classes.py and tests/test_gpu_user_kernel_classes.py share: the rule that decides whether a
kernel passed (compare_forced, compare_loop: pure functions on arrays, run on the CPU by tests/test_class_harness.py), the
driver that takes a handle through the teacher-forced ticks or the device loop, and the two parametrised test bodies.
Nothing of cgmres_cpp_amd is imported here: a test module hands its handles in through its Side.

One reference format, that of user_oracle.run_full: arrays [B, ticks, ...] named t, U, d, x (what a tick started from),
u, U1, d1, k, reason (what it left).  A reference has one tick more than the device loop runs: the loop's u, counts and
state are compared with its second-to-last tick, x and t with what its last tick started from."""
import math
from typing import Any, Callable, NamedTuple, Optional

import numpy as np
import pytest

TICKS, LOOP_TICKS = 4, 12
B16, B8 = 20, 11  # controllers for a 16-instance kernel (one full workgroup and one with 4 of 16 rows) and an 8-instance one
EXIT_NATURAL = 0  # cgmres_cpp_amd.EXIT_NATURAL (asserted by the loop test)


class Bounds(NamedTuple):
    f32: bool
    u: float              # forced: on u (fp64 relative to max(1, |u_ref|), fp32 absolute)
    U1: Optional[float]   # forced, fp32 only: on U', absolute
    d: float              # forced: on dUdt', relative to max(1, |dUdt_ref|)
    loop: float           # loop: on u and x (fp32: and U), absolute
    loop_d: Optional[float]  # loop, fp32 only: on dUdt, relative


F64 = Bounds(False, 1e-9, None, 1e-7, 1e-7, None)  # SURVEY.md 8(c); the loop bound of test_gpu_gs_ring.py


def f32_bounds(spread=None):
    """fp32 against the fp32 oracle: 1e-4 on u and U', 5e-3 relative on dUdt', or 8 x the spread (u, U', dUdt') a case
    records for the tolerance mode; the loop bounds of test_gpu_closed_loop.test_closed_loop_device_vs_oracle."""
    su, sU, sd = spread or (None, None, None)
    return Bounds(True, 8 * su if su else 1e-4, 8 * sU if sU else 1e-4, 8 * sd if sd else 5e-3, 1e-4, 2e-3)


def absmax(a):
    return float(np.max(np.abs(a)))


def relmax(a, ref):
    return absmax(a - ref) / max(1.0, absmax(ref))


def worse(a, b):
    return max(a, b) if a == a and b == b else math.inf  # (max() drops a NaN)


def compare_forced(got, ref, bounds, k_max, tol):
    """(problems, worst |du| / bound, worst |ddUdt'| / bound) of teacher-forced ticks: got["u"], ["U1"], ["d1"], ["k"],
    ["reason"] of the first B instances and the first ticks of `ref`.  fp64: counts and reasons equal, with tol = 0 exactly
    k_max iterations; fp32: 1 <= count <= k_max."""
    B, ticks = got["k"].shape
    bad, wu, wd = [], 0.0, 0.0
    for n in range(ticks):
        for i in range(B):
            k, reason = int(got["k"][i, n]), int(got["reason"][i, n])
            if bounds.f32:
                ru = worse(absmax(got["u"][i, n] - ref["u"][i, n]) / bounds.u, absmax(got["U1"][i, n] - ref["U1"][i, n]) / bounds.U1)
                if not 1 <= k <= k_max:
                    bad.append(("count", n, i, k))
            else:
                ru = relmax(got["u"][i, n], ref["u"][i, n]) / bounds.u
                if k != ref["k"][i, n] or reason != ref["reason"][i, n]:
                    bad.append(("count / reason", n, i, k, int(ref["k"][i, n]), reason, int(ref["reason"][i, n])))
                if tol == 0.0 and k != k_max:
                    bad.append(("fixed-k count", n, i, k))
            rd = relmax(got["d1"][i, n], ref["d1"][i, n]) / bounds.d
            if not ru <= 1.0:
                bad.append(("u or U' / bound" if bounds.f32 else "u / bound", n, i, ru))
            if not rd <= 1.0:
                bad.append(("dUdt' / bound", n, i, rd))
            wu, wd = worse(wu, ru), worse(wd, rd)
    return bad, wu, wd


def compare_loop(got, ref, bounds, k_max, tol):
    """(problems, worst |du|, |dx| / bound, worst |ddUdt| / bound) after a device loop of one tick less than `ref` has:
    got["x"], ["u"], ["U"], ["d"] [B, ...], ["k"], ["reason"] [B] and ["t"].  fp64: u and x, the last tick's counts and
    reasons equal, with tol = 0 k_max natural exits; fp32: U and dUdt too, per instance, and at most B // 2 count flips."""
    B, last = len(got["k"]), ref["k"].shape[1] - 2
    k, reason = got["k"], got["reason"]
    bad = []
    if not all(np.all(np.isfinite(got[q])) for q in ("x", "u", "U", "d")):
        bad.append(("not finite",))
    if bounds.f32:
        flips, wu, wd = 0, 0.0, 0.0
        for i in range(B):
            if abs(got["t"] - ref["t"][i, last + 1]) > 1e-6:
                bad.append(("t", got["t"], ref["t"][i, last + 1]))
            ru = 0.0
            for a, b in ((got["u"][i], ref["u"][i, last]), (got["x"][i], ref["x"][i, last + 1]), (got["U"][i], ref["U1"][i, last])):
                ru = worse(ru, absmax(a - b) / bounds.loop)
            rd = relmax(got["d"][i], ref["d1"][i, last]) / bounds.loop_d
            if not ru <= 1.0:
                bad.append(("loop u, x or U / 1e-4", i, ru))
            if not rd <= 1.0:
                bad.append(("loop dUdt / 2e-3", i, rd))
            flips += int(k[i] != ref["k"][i, last])
            wu, wd = worse(wu, ru), worse(wd, rd)
        if flips > B // 2:
            bad.append(("count flips", flips))
        return bad, wu, wd
    if tol == 0.0 and not (np.all(k == k_max) and np.all(reason == EXIT_NATURAL)):
        bad.append(("fixed-k count", k.tolist(), reason.tolist()))
    wu = worse(absmax(got["u"] - ref["u"][:B, last]), absmax(got["x"] - ref["x"][:B, last + 1])) / bounds.loop
    if not wu <= 1.0:
        bad.append(("loop u or x / 1e-7", wu))
    if not (np.array_equal(k, ref["k"][:B, last]) and np.array_equal(reason, ref["reason"][:B, last])):
        bad.append(("loop count / reason", k.tolist(), ref["k"][:B, last].tolist(), reason.tolist(), ref["reason"][:B, last].tolist()))
    return bad, wu, 0.0


class Side(NamedTuple):
    """what a test module knows: its table, and how to make its references, handles and scenario"""
    table: Any
    what: str          # "kernel class" / "user kernel class", the head of every printed figure line
    fixture: str       # the oracle fixture of the module
    reference: Callable  # (oracle, case, tol) -> the oracle's free run of the B16 instances for LOOP_TICKS + 1 ticks
    batch_of: Callable   # (case, tol, variant=None, ...) -> (handle, B); variant None: the case's own, its name asserted
    scenario: Callable   # (oracle, case, B) -> x0, u0, p of the first B instances
    bounds: Callable     # (case, tol) -> Bounds
    loop_line: str     # the figures of the loop's printed line


def forced_problems(side, oracle, case, tol, **handle):
    """compare_forced of TICKS ticks through control(): controller state and x taken from the reference every tick"""
    ref = side.reference(oracle, case, tol)
    c, B = side.batch_of(case, tol, **handle)
    c.set_ptau_repeat(side.scenario(oracle, case, B)[2])
    ticks = []
    for n in range(TICKS):
        c.set_state(float(ref["t"][0, n]), ref["U"][:B, n], ref["d"][:B, n])
        u = c.control(ref["x"][:B, n])
        k, reason = c.get_status()
        _, U1, d1 = c.get_state()
        ticks.append([np.array(v, dtype=np.float64) for v in (u, U1, d1)] + [np.array(k), np.array(reason)])
    c.close()
    got = {q: np.stack(v, axis=1) for q, v in zip(("u", "U1", "d1", "k", "reason"), zip(*ticks))}
    return compare_forced(got, ref, side.bounds(case, tol), case.k_max, tol)


def loop_problems(side, oracle, case, tol, **handle):
    """compare_loop of LOOP_TICKS ticks of closed_loop_device from the seeded start"""
    ref = side.reference(oracle, case, tol)
    bounds = side.bounds(case, tol)
    c, B = side.batch_of(case, tol, **handle)
    x0, u0, p = side.scenario(oracle, case, B)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p if c.dim_p else None, 10)
    xd = c.device_buffer((B, c.dim_x)).upload(x0.astype(np.float32 if bounds.f32 else np.float64))
    ud = c.device_buffer((B, c.dim_u))
    c.closed_loop_device(xd, ud, LOOP_TICKS)
    c.synchronize()
    t, U, d = c.get_state()
    k, reason = c.get_status()
    got = dict(x=xd.download().astype(np.float64), u=ud.download().astype(np.float64), t=t, U=U.astype(np.float64),
               d=d.astype(np.float64), k=k, reason=reason)
    xd.free(), ud.free(), c.close()
    return compare_loop(got, ref, bounds, case.k_max, tol)


def verdict(side, oracle, case, tol, problems_of):
    """for the failure message of an fp64 case: what the lane mapping makes of the same shape"""
    if side.bounds(case, tol).f32:
        return "fp32"
    if side.table.kind(case.cls) == "lane":
        return "this IS the lane mapping"
    lane_bad = problems_of(side, oracle, case, tol, variant=1)[0]
    if lane_bad:
        return "the lane mapping fails too (%r ...): the shape is ill-conditioned, mend the admission rule and replace the case" % (lane_bad[:2],)
    return "the lane mapping passes: a finding about this kernel"


def class_tests(side, cg):
    """the two parametrised tests of a module, over every case of its table"""
    t = side.table
    cases = pytest.mark.parametrize("case", t.RECORDS, ids=[t.case_id(c) for c in t.RECORDS])

    def check(request, case, problems_of, line):
        oracle = request.getfixturevalue(side.fixture)
        for tol in (1e-6, 0.0) if case.fixed_k_ok else (1e-6,):
            bad, wu, wd = problems_of(side, oracle, case, tol)
            print(f"{side.what} {t.class_name(case.cls)} case {t.case_id(case)} tol {tol:g} " + line.format(wu=wu, wd=wd))
            assert not bad, (t.case_id(case), tol, len(bad), bad[:4], verdict(side, oracle, case, tol, problems_of))

    @cases
    def test_teacher_forced_ticks_vs_oracle(request, case):
        check(request, case, forced_problems, "forced: |du|/bound {wu:.3g} |ddUdt|/bound {wd:.3g}")

    @cases
    def test_device_loop_across_a_launch_boundary_vs_oracle(request, case):
        assert LOOP_TICKS > cg.TICKS_PER_LAUNCH and cg.EXIT_NATURAL == EXIT_NATURAL
        check(request, case, loop_problems, side.loop_line)

    return test_teacher_forced_ticks_vs_oracle, test_device_loop_across_a_launch_boundary_vs_oracle
