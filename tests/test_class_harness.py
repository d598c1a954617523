"""The rule that decides whether a kernel class passed (tests/class_harness.py: compare_forced, compare_loop) on
hand-made arrays: no GPU, no oracle.  A synthetic fp64 reference of B = 3 instances, 2 ticks, L = 4, k_max = 3.

Behind them the per-tick inputs of the fused loop: the seeded sequences (loop_inputs) as plain arrays, and
compare_loop_inputs on the oracle itself (no GPU): a second oracle run with one planted fault stands in for the device."""
import math

import numpy as np
import pytest

import class_harness as harness
from class_harness import B8, B16, F64, LOOP_TICKS, compare_forced, compare_loop, compare_loop_inputs, f32_bounds, loop_inputs

B, TICKS, L, NU, NX, KMAX = 3, 2, 4, 2, 2, 3


def reference():
    g = np.random.default_rng(7)
    ref = {q: g.uniform(0.5, 2.0, (B, TICKS, n)) for q, n in (("U", L), ("d", L), ("x", NX), ("U1", L), ("d1", L))}
    ref["u"] = ref["U1"][:, :, :NU].copy()
    ref["t"] = np.tile(0.001 * np.arange(TICKS), (B, 1))
    ref["k"] = np.full((B, TICKS), KMAX)
    ref["reason"] = np.zeros((B, TICKS), dtype=int)
    return ref


def forced_of(ref):
    """what a kernel equal to the reference leaves after the teacher-forced ticks"""
    return {q: ref[q].copy() for q in ("u", "U1", "d1", "k", "reason")}


def loop_of(ref):
    """what a kernel equal to the reference leaves after a device loop of TICKS - 1 ticks"""
    n = TICKS - 1
    return dict(x=ref["x"][:, n].copy(), u=ref["u"][:, n - 1].copy(), U=ref["U1"][:, n - 1].copy(), d=ref["d1"][:, n - 1].copy(),
                k=ref["k"][:, n - 1].copy(), reason=ref["reason"][:, n - 1].copy(), t=float(ref["t"][0, n]))


# (compare, result of an exact kernel, index of [instance 1, the compared tick] in a result array)
FORCED = (compare_forced, forced_of, (1, 1))
LOOP = (compare_loop, loop_of, (1,))
BOTH = pytest.mark.parametrize("compare,result,at", [FORCED, LOOP], ids=["forced", "loop"])


def where(compare, at):
    """how a problem of `compare` names the place: (tick, instance) of the forced ticks, nothing per instance in the loop"""
    return (at[1], at[0]) if compare is compare_forced else ()


@BOTH
def test_a_result_equal_to_the_reference_has_no_problem(compare, result, at):
    ref = reference()
    for tol in (1e-6, 0.0):
        assert compare(result(ref), ref, F64, KMAX, tol) == ([], 0.0, 0.0)


@BOTH
def test_u_off_by_twice_its_bound_is_the_u_problem(compare, result, at):
    ref = reference()
    got = result(ref)
    scale = max(1.0, float(np.max(np.abs(got["u"][at])))) if compare is compare_forced else 1.0
    got["u"][at][0] += 2 * (F64.u if compare is compare_forced else F64.loop) * scale
    bad, wu, wd = compare(got, ref, F64, KMAX, 1e-6)
    assert len(bad) == 1 and bad[0][0] == ("u / bound" if compare is compare_forced else "loop u or x / 1e-7")
    assert bad[0][1:-1] == where(compare, at) and bad[0][-1] == pytest.approx(2.0, rel=1e-3)
    assert wu == pytest.approx(2.0, rel=1e-3) and wd == 0.0


def test_dudt_off_by_twice_its_bound_is_the_dudt_problem():
    """(the fp64 loop bounds u and x only: the forced ticks and the fp32 loop bound dUdt)"""
    ref = reference()
    got = forced_of(ref)
    got["d1"][1, 1, 2] += 2 * F64.d * max(1.0, float(np.max(np.abs(ref["d1"][1, 1]))))
    bad, wu, wd = compare_forced(got, ref, F64, KMAX, 1e-6)
    assert [b[:3] for b in bad] == [("dUdt' / bound", 1, 1)] and wd == pytest.approx(2.0, rel=1e-3) and wu == 0.0
    got = loop_of(ref)
    got["d"][1, 2] += 2 * 2e-3 * max(1.0, float(np.max(np.abs(ref["d1"][1, 0]))))
    bad, wu, wd = compare_loop(got, ref, f32_bounds(), KMAX, 1e-6)
    assert [b[:2] for b in bad] == [("loop dUdt / 2e-3", 1)] and wd == pytest.approx(2.0, rel=1e-3) and wu == 0.0


@BOTH
def test_one_count_differing_by_one_is_the_count_problem(compare, result, at):
    ref = reference()
    got = result(ref)
    got["k"][at] -= 1
    bad, wu, wd = compare(got, ref, F64, KMAX, 1e-6)
    assert len(bad) == 1 and bad[0][0] == ("count / reason" if compare is compare_forced else "loop count / reason")
    assert (wu, wd) == (0.0, 0.0)
    if compare is compare_forced:
        assert bad[0][1:5] == (1, 1, KMAX - 1, KMAX)


@BOTH
def test_with_tol_0_a_count_below_k_max_is_the_fixed_k_problem(compare, result, at):
    """(the reference has the same short count, so that nothing else differs)"""
    ref = reference()
    ref["k"][1, :] = KMAX - 1
    bad = compare(result(ref), ref, F64, KMAX, 0.0)[0]
    assert [b[0] for b in bad] == ["fixed-k count"] * (TICKS if compare is compare_forced else 1)
    assert compare(result(ref), ref, F64, KMAX, 1e-6)[0] == []


@BOTH
def test_a_nan_in_u_is_a_problem_and_an_infinite_worst_figure(compare, result, at):
    ref = reference()
    got = result(ref)
    got["u"][at][0] = math.nan
    bad, wu, wd = compare(got, ref, F64, KMAX, 1e-6)
    assert bad and wu == math.inf
    # ... also where the NaN comes first and a finite figure behind it
    got = result(ref)
    got["u"][0][..., 0] = math.nan
    assert compare(got, ref, F64, KMAX, 1e-6)[1] == math.inf


@BOTH
def test_fp32_six_spreads_pass_nine_fail_and_a_count_of_zero_fails(compare, result, at):
    """A recorded spread of u widens the forced bound on u to 8 x it; the loop's fp32 bounds are fixed (1e-4)."""
    ref = reference()
    spread = 3e-5  # above 1e-4 / 8, as a recorded spread is
    bounds = f32_bounds((spread, None, None))
    unit = spread if compare is compare_forced else bounds.loop / 8
    for factor, passes in ((6, True), (9, False)):
        got = result(ref)
        got["u"][at][0] += factor * unit
        bad, wu, wd = compare(got, ref, bounds, KMAX, 1e-6)
        assert (bad == []) == passes and wu == pytest.approx(factor / 8, rel=1e-3), (factor, bad)
    if compare is compare_forced:
        got = result(ref)
        got["k"][at] = 0
        assert compare(got, ref, bounds, KMAX, 1e-6)[0] == [("count", 1, 1, 0)]
        got["k"][at] = 1  # (fp32 counts are not compared with the reference's)
        assert compare(got, ref, bounds, KMAX, 1e-6)[0] == []
    else:  # the loop tolerates B // 2 = 1 count flip, not 2
        got = result(ref)
        got["k"][0] = 0
        assert compare(got, ref, bounds, KMAX, 1e-6)[0] == []
        got["k"][1] = 0
        assert compare(got, ref, bounds, KMAX, 1e-6)[0] == [("count flips", 2)]


# ---- the per-tick inputs of the fused loop ---------------------------------------------------------------------------
def test_loop_inputs_shapes_and_determinism():
    p = np.stack([np.linspace(0.4, 1.2, B16), np.zeros(B16)], axis=1)
    seq, d, v = loop_inputs((4, 2), 7, p, np.float64)
    assert seq.shape == (LOOP_TICKS, B16, 8, 2) and d.shape == v.shape == (LOOP_TICKS, B16, 4)
    assert all(a.dtype == np.float64 for a in (seq, d, v))
    for a, b in zip((seq, d, v), loop_inputs((4, 2), 7, p, np.float64)):
        assert np.array_equal(a, b)
    # d first, then v, from the one generator and sigma of test_gpu_loop_inputs.noise
    rng = np.random.default_rng(7)
    assert np.array_equal(d, rng.normal(0.0, 1e-3, (LOOP_TICKS, B16, 4))) and np.array_equal(v, rng.normal(0.0, 1e-3, (LOOP_TICKS, B16, 4)))
    assert not np.array_equal(d, v) and 5e-4 < d.std() < 2e-3
    # the ramp: component 0 moves with the tick, along the horizon and with the instance; component 1 stays
    k, i, s = 10, 13, 5
    assert seq[k, i, s, 0] == p[i, 0] * (1.0 + 0.004 * k) + 0.0007 * s * (1 + 0.1 * (i % 5))
    assert np.array_equal(seq[..., 1], np.broadcast_to(p[None, :, None, 1], seq.shape[:3]))
    assert len({seq[k, i, s, 0] for k in range(LOOP_TICKS)}) == LOOP_TICKS and seq[0, 1, 3, 0] != seq[0, 2, 3, 0]
    # a model without parameters has no moving reference, and the same d and v
    seq0, d0, v0 = loop_inputs((4, 0), 7, np.zeros((B16, 0)), np.float64)
    assert seq0 is None and np.array_equal(d0, d) and np.array_equal(v0, v)
    assert harness.leg_of("ptau", seq, d, v) == (seq, None, None) and harness.leg_of("all", seq, d, v) == (seq, d, v)


def test_an_8_instance_kernel_gets_the_first_11_rows_of_the_20():
    p = np.stack([np.linspace(0.4, 1.2, B16), np.zeros(B16)], axis=1)
    for a in loop_inputs((4, 2), 3, p, np.float64):
        rows = harness.device_rows(a, B8)
        assert rows.shape == (LOOP_TICKS, B8, a[0, 0].size) and rows.flags["C_CONTIGUOUS"]
        for k in (0, 10, LOOP_TICKS - 1):
            for i in (0, 7, B8 - 1):
                assert np.array_equal(rows[k, i], a[k, i].ravel())  # (seq: stage-major, as set_ptau takes a horizon)
        assert np.array_equal(harness.device_rows(a, B16)[:, :B8], rows)


def test_loop_inputs_in_float32_are_the_float64_ones_cast_once():
    p = np.stack([np.linspace(0.4, 1.2, B16), np.zeros(B16)], axis=1)
    for a, b in zip(loop_inputs((4, 2), 5, p, np.float32), loop_inputs((4, 2), 5, p, np.float64)):
        assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32)) and not np.array_equal(a.astype(np.float64), b)


# (model, dv, k_max): the smallest admitted pendulum and row-Newton shapes, msd and the semi-active damper (no parameters)
FAULT_SHAPES = [(0, 3, 3), (0, 53, 9), (1, 2, 5), (2, 2, 3)]
FAULTS = ("a", "b", "c", "d", "e", "f")
_runs = {}


def oracle_run(orc, model, dv, k_max, fault=None):
    """oracle_loop_inputs of the "all" leg, fp64, tol = 1e-6, with one planted fault (None: none); cached"""
    key = (model, dv, k_max, fault)
    if key not in _runs:
        x0, u0, p = orc.batch_scenario(model, B16)
        dims = orc.Controller(model, dv, k_max)
        seq, d, v = loop_inputs((dims.dim_x, dims.dim_p), dv, p, np.float64)
        second = 10  # the first tick of the second launch (10 ticks per launch)
        follow = None
        if fault == "a":
            d = d.copy()
            d[second] = d[0]
        elif fault == "b":
            v = v.copy()
            v[second] = v[0]
        elif fault == "c":
            seq = seq.copy()
            seq[second] = seq[0]
        elif fault == "d":
            v = np.roll(v, -1, axis=1)  # instance i reads the row of instance i + 1
        elif fault == "e":
            d = d.copy()
            d[LOOP_TICKS - 1] = 0.0
        elif fault == "f":
            follow = p  # the follow-up tick on the handle's original ptau instead of seq[11]
        _runs[key] = harness.oracle_loop_inputs(orc, model, "f64", dv, k_max, 1e-6, x0, u0, p, seq, d, v, follow_up_ptau=follow)
    return _runs[key]


@pytest.mark.parametrize("model,dv,k_max", FAULT_SHAPES)
def test_the_oracle_under_the_same_inputs_passes_compare_loop_inputs(orc, model, dv, k_max):
    ref = oracle_run(orc, model, dv, k_max)
    for B in (B16, B8):
        got = {q: (a if q == "t" else a[:B].copy()) for q, a in oracle_run(orc, model, dv, k_max).items()}
        assert compare_loop_inputs(got, ref, F64, k_max, 1e-6) == ([], 0.0, 0.0)
    got["x"][3, 0] = math.nan
    bad, wu, wn = compare_loop_inputs(got, ref, F64, k_max, 1e-6)
    assert ("not finite",) in bad and wu == math.inf
    got = dict(oracle_run(orc, model, dv, k_max), t=ref["t"] + 1e-3)  # one tick too many or too few
    assert [b[0] for b in compare_loop_inputs(got, ref, F64, k_max, 1e-6)[0]] == ["t"]


# (c) and (f) get the moving reference wrong: they apply where the model has parameters (not the semi-active damper)
@pytest.mark.parametrize("model,dv,k_max,fault", [s + (f,) for s in FAULT_SHAPES for f in FAULTS if not (f in "cf" and s[0] == 2)])
def test_a_planted_input_fault_is_reported_at_the_fp64_bounds(orc, model, dv, k_max, fault):
    """A "device" that is the oracle with one wrong index in how it consumes the inputs:
      (a) d of tick 10 (the first tick of the second launch) taken from tick 0      (d) v of instance i taken from instance i + 1
      (b) v of tick 10 taken from tick 0                                            (e) d not applied on the last tick
      (c) the reference horizon of tick 10 taken from tick 0                        (f) the follow-up tick on the handle's original ptau
    Each must show in u_11, x_12 or the follow-up u at the 1e-7 bound; the smallest effect, (b) on the pendulum at
    dv 3, is 4.8e-6 = 48 bounds.  (c) and (f) need a model with parameters.

    What this says about fp32, whose bound is 1e-4: (a) and (e) (2e-3 and more) and a persistent fault of kind (d) (2e-4
    and more) are visible there; a single tick's v or seq taken from another tick (5e-6 .. 7e-4) is not, on the pendulum
    at all.  The fp32 classes lean on their fp64 twins of the same templates for those."""
    ref, got = oracle_run(orc, model, dv, k_max), oracle_run(orc, model, dv, k_max, fault)
    bad, wu, wn = compare_loop_inputs(got, ref, F64, k_max, 1e-6)
    names = [b[0] for b in bad]
    print(f"model {model} dv {dv} k_max {k_max} fault ({fault}): |du|,|dx|/bound {wu:.3g} follow-up |du|/bound {wn:.3g} {names}")
    if fault == "f":
        assert names == ["follow-up u / bound"] and wu == 0.0 and wn > 10.0
    else:
        assert "inputs loop u or x / bound" in names and wu > 10.0
