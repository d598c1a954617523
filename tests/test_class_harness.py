"""The rule that decides whether a kernel class passed (tests/class_harness.py: compare_forced, compare_loop) on
hand-made arrays: no GPU, no oracle.  A synthetic fp64 reference of B = 3 instances, 2 ticks, L = 4, k_max = 3."""
import math

import numpy as np
import pytest

from class_harness import F64, compare_forced, compare_loop, f32_bounds

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
