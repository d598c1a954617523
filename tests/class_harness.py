"""What tests/test_gpu_kernel_classes.py and tests/test_gpu_user_kernel_classes.py share: the rule that decides whether a
kernel passed (compare_forced, compare_loop, compare_loop_inputs: pure functions on arrays, run on the CPU by
tests/test_class_harness.py), the driver that takes a handle through the teacher-forced ticks or the device loop, and the
parametrised test bodies.  Nothing of cgmres_cpp_amd is imported here: a test module hands its handles in through its Side.

One reference format, that of user_oracle.run_full: arrays [B, ticks, ...] named t, U, d, x (what a tick started from),
u, U1, d1, k, reason (what it left).  A reference has one tick more than the device loop runs: the loop's u, counts and
state are compared with its second-to-last tick, x and t with what its last tick started from.

The per-tick inputs of the fused loop (a moving reference, a process disturbance d, a measurement noise v) have their
own seeded sequences (loop_inputs), their own reference (oracle_loop_inputs: the oracle driven tick by tick with the three
statements of include/cgmres_hip.h), rule (compare_loop_inputs) and driver (loop_inputs_problems), in two legs:
"ptau" (the moving reference alone: cgmres_hip_closed_loop_device_ptau) and "all" (all three:
cgmres_hip_closed_loop_device_ex).  tests/test_gpu_kernel_classes.py runs both over every case of the built-in table,
tests/test_gpu_wave.py the "all" leg at the row-boundary horizons of the wave mapping."""
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


LEGS = ("ptau", "all")
INPUT_SIGMA, INPUT_SEED = 1e-3, 7  # the generator and sigma of test_gpu_loop_inputs.noise


def loop_inputs(model_dims, dv, p, dtype):
    """(seq, d, v) for the B16 instances and LOOP_TICKS ticks of a model with model_dims = (dim_x, dim_p) and per-instance
    parameters p [B16, dim_p]; an 8-instance kernel takes the first B8 rows, so a reference is shared per shape.
    d, v [LOOP_TICKS, B16, dim_x]: one seeded generator, d drawn first.  seq [LOOP_TICKS, B16, dv + 1, dim_p], None where
    dim_p = 0: the ramp of test_closed_loop_device_with_moving_reference (component 0 moves with the tick and along the
    horizon, at a slope that depends on the instance; the others stay).  All cast to `dtype` once: with float32 the
    device and the oracle both read the cast values."""
    dim_x, dim_p = model_dims
    rng = np.random.default_rng(INPUT_SEED)
    d = rng.normal(0.0, INPUT_SIGMA, (LOOP_TICKS, B16, dim_x)).astype(dtype)
    v = rng.normal(0.0, INPUT_SIGMA, (LOOP_TICKS, B16, dim_x)).astype(dtype)
    if not dim_p:
        return None, d, v
    p = np.asarray(p, dtype=np.float64).reshape(B16, dim_p)
    k, i, s = np.arange(LOOP_TICKS)[:, None, None], np.arange(B16)[None, :, None], np.arange(dv + 1)[None, None, :]
    seq = np.empty((LOOP_TICKS, B16, dv + 1, dim_p))
    seq[...] = p[None, :, None, :]
    seq[..., 0] = p[None, :, None, 0] * (1.0 + 0.004 * k) + 0.0007 * s * (1 + 0.1 * (i % 5))
    return seq.astype(dtype), d, v


def leg_of(leg, seq, d, v):
    """what a leg hands to the loop of loop_inputs' three sequences"""
    assert leg in LEGS, leg
    return (seq, None, None) if leg == "ptau" else (seq, d, v)


def device_rows(a, B):
    """the first B instances of a sequence of loop_inputs as the loop takes it: contiguous [LOOP_TICKS, B, width]"""
    return np.ascontiguousarray(a[:, :B]).reshape(LOOP_TICKS, B, -1)


def oracle_loop_inputs(orc, model, dtype, dv, k_max, tol, x0, u0, p, seq=None, d=None, v=None, follow_up_ptau=None,
                       which="oracle"):
    """The reference of compare_loop_inputs: per instance of x0 the oracle (dtype "f64" / "f32") from the seeded start,
    LOOP_TICKS ticks of
        y = x + v_k;   set_ptau(seq[k]), u = control(y);   x = (x + plant(x, u) dt) + d_k
    (fp32: the plant step and the sums in float32, as the device takes them), then one plain tick u_next = control(x)
    with the ptau left at seq[-1] (follow_up_ptau: the per-instance parameters to repeat over the horizon before it
    instead, which is what a handle that did not keep the last horizon would do).  dict of u, x, u_next [B, ...], k,
    reason [B] of the last tick of the loop, full [B] (every tick of the loop ran k_max iterations) and t.  which: the
    oracle library (orc.Controller), for the admission tool's second build."""
    npdt = np.float32 if dtype == "f32" else np.float64
    out = {q: [] for q in ("u", "x", "u_next", "k", "reason", "full")}
    for i in range(len(x0)):
        r = orc.Controller(model, dv, k_max, tol, dtype, which=which)
        orc.start_controller(r, x0[i], u0[i], p[i])
        x = np.array(x0[i], dtype=npdt)
        full = True
        for k in range(LOOP_TICKS):
            if seq is not None:
                r.set_ptau(seq[k, i])
            y = x if v is None else (x + v[k, i].astype(npdt)).astype(npdt)
            u = r.control(y)
            full = full and r.last_solve()[0] == k_max
            x = (x + r.plant(x, u).astype(npdt) * npdt(r.dt)).astype(npdt)
            if d is not None:
                x = (x + d[k, i].astype(npdt)).astype(npdt)
        count, _, reason = r.last_solve()
        if follow_up_ptau is not None and r.dim_p:
            r.set_ptau_repeat(follow_up_ptau[i])
        for q, a in zip(out, (u, x.astype(np.float64), r.control(x), count, reason, full)):
            out[q].append(a)
    out = {q: np.array(a) for q, a in out.items()}
    out["t"] = LOOP_TICKS * r.dt
    return out


def compare_loop_inputs(got, ref, bounds, k_max, tol):
    """(problems, worst |du|, |dx| / bound, worst follow-up |du| / bound) of a device loop under per-tick inputs against
    oracle_loop_inputs: got["x"], ["u"], ["u_next"] [B, ...], ["k"], ["reason"] [B] and ["t"], the first B instances of
    `ref`.  fp64: u, x and the follow-up tick's u within bounds.loop, the last tick's counts and reasons equal, with
    tol = 0 k_max natural exits, |t - LOOP_TICKS dt| <= 1e-12; fp32: u, x and the follow-up u within bounds.loop,
    t within 1e-6 (U and dUdt are not compared: under this noise the two oracle builds differ by more than compare_loop's
    bound on dUdt).  Both: everything finite."""
    B = len(got["k"])
    k, reason = got["k"], got["reason"]
    bad = []
    if not all(np.all(np.isfinite(got[q])) for q in ("x", "u", "u_next")):
        bad.append(("not finite",))
    if not abs(got["t"] - ref["t"]) <= (1e-6 if bounds.f32 else 1e-12):
        bad.append(("t", got["t"], ref["t"]))
    wu = worse(absmax(got["u"] - ref["u"][:B]), absmax(got["x"] - ref["x"][:B])) / bounds.loop
    wn = worse(0.0, absmax(got["u_next"] - ref["u_next"][:B])) / bounds.loop
    if not wu <= 1.0:
        bad.append(("inputs loop u or x / bound", wu))
    if not wn <= 1.0:
        bad.append(("follow-up u / bound", wn))
    if not bounds.f32:
        if tol == 0.0 and not (np.all(k == k_max) and np.all(reason == EXIT_NATURAL)):
            bad.append(("fixed-k count", k.tolist(), reason.tolist()))
        if not (np.array_equal(k, ref["k"][:B]) and np.array_equal(reason, ref["reason"][:B])):
            bad.append(("loop count / reason", k.tolist(), ref["k"][:B].tolist(), reason.tolist(), ref["reason"][:B].tolist()))
    return bad, wu, wn


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
    inputs_reference: Optional[Callable] = None  # (oracle, case, tol, leg) -> oracle_loop_inputs of the B16 instances


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


def loop_inputs_problems(side, oracle, case, tol, leg, **handle):
    """compare_loop_inputs of one closed_loop_device call of LOOP_TICKS ticks from the seeded start with the leg's
    sequences as per-instance device buffers, and of one plain control() of the x it left: the handle must have kept the
    last tick's horizon and dropped d and v."""
    ref = side.inputs_reference(oracle, case, tol, leg)
    bounds = side.bounds(case, tol)
    npdt = np.float32 if bounds.f32 else np.float64
    c, B = side.batch_of(case, tol, **handle)
    x0, u0, p = side.scenario(oracle, case, B)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p if c.dim_p else None, 10)
    seq, d, v = leg_of(leg, *loop_inputs((c.dim_x, c.dim_p), case.dv, side.scenario(oracle, case, B16)[2], npdt))
    assert seq is not None or d is not None, "the leg gives this model no input"
    bufs = []

    def dev(a):
        if a is None:
            return None
        a = device_rows(a, B)
        bufs.append(c.device_buffer(a.shape).upload(a))
        return bufs[-1]
    xd = c.device_buffer((B, c.dim_x)).upload(x0.astype(npdt))
    ud = c.device_buffer((B, c.dim_u))
    bufs += [xd, ud]
    c.closed_loop_device(xd, ud, LOOP_TICKS, dev(seq), True, dist_seq_dev=dev(d), meas_seq_dev=dev(v))
    c.synchronize()
    k, reason = c.get_status()
    x = xd.download()
    got = dict(x=x.astype(np.float64), u=ud.download().astype(np.float64), t=c.get_state()[0], k=k, reason=reason)
    got["u_next"] = c.control(x).astype(np.float64)
    for b in bufs:
        b.free()
    c.close()
    return compare_loop_inputs(got, ref, bounds, case.k_max, tol)


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


def class_inputs_tests(side, cg):
    """the two parametrised tests of the loop's per-tick inputs, over every case of the table that has the leg's inputs
    (t.leg_applies); a case the table's admission rule leaves out of a leg (t.leg_skip: a reason) is skipped with it"""
    t = side.table

    def cases(leg):
        rows = [c for c in t.RECORDS if t.leg_applies(c, leg)]
        return pytest.mark.parametrize("case", rows, ids=[t.case_id(c) for c in rows])

    def check(request, case, leg):
        assert LOOP_TICKS > cg.TICKS_PER_LAUNCH and cg.EXIT_NATURAL == EXIT_NATURAL
        why = t.leg_skip(case, leg)
        if why:
            pytest.skip(why)
        oracle = request.getfixturevalue(side.fixture)

        def problems_of(*a, **handle):
            return loop_inputs_problems(*a, leg, **handle)
        for tol in (1e-6, 0.0) if case.fixed_k_ok else (1e-6,):
            bad, wu, wn = problems_of(side, oracle, case, tol)
            print(f"{side.what} {t.class_name(case.cls)} case {t.case_id(case)} tol {tol:g} inputs {leg}: "
                  f"|du|,|dx|/bound {wu:.3g} follow-up |du|/bound {wn:.3g}")
            assert not bad, (t.case_id(case), leg, tol, len(bad), bad[:4], verdict(side, oracle, case, tol, problems_of))

    @cases("ptau")
    def test_device_loop_with_a_moving_reference_vs_oracle(request, case):
        check(request, case, "ptau")

    @cases("all")
    def test_device_loop_with_disturbance_noise_and_moving_reference_vs_oracle(request, case):
        check(request, case, "all")

    return test_device_loop_with_a_moving_reference_vs_oracle, test_device_loop_with_disturbance_noise_and_moving_reference_vs_oracle
