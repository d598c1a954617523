"""Every kernel the wg planner can choose (tests/kernel_classes.py: one tick_wg_kernel instantiation in one LDS plan and
chunk count is a class) against the oracle, at the one or two members of each class that CASES lists.

Batch: 20 controllers for a 16-instance kernel (one full workgroup and one with 4 of 16 rows), 11 for an 8-instance
one; the seeded start of orc.batch_scenario.  Per case, with tol = 1e-6 and, where the case's fixed_k_ok says so, tol = 0:

  * 4 teacher-forced ticks through control(): controller state and x taken from the oracle every tick, as
    test_gpu_parity.test_seeded_batch_vs_oracle does.  fp64: |du| <= 1e-9 * max(1, |u_ref|), |ddUdt'| <=
    1e-7 * max(1, |dUdt_ref|), Arnoldi count and exit reason equal, and with tol = 0 exactly k_max iterations everywhere.
    fp32 against the fp32 oracle: 1e-4 on u and U', 5e-3 relative on dUdt' — or 8 x the spread the case records — and
    1 <= n_ax <= k_max.
  * 12 ticks of closed_loop_device from the same start (one launch boundary: the class's hand-over through HBM) against
    the oracle's free run.  fp64: the bounds of test_gpu_gs_ring.py (x and u within 1e-7, the last tick's counts and
    reasons equal); fp32: the bounds of test_gpu_closed_loop.test_closed_loop_device_vs_oracle.
  * the same 12 ticks under the loop's per-tick inputs, which every instantiation of tick_wg_kernel consumes in its own
    code (the parameter table in LDS or, on the lean plan, in HBM; y_0 = x_0 + v_0 of every launch; the plant block's u
    from registers, LDS or HBM; 8 or 16 instances per workgroup), as per-instance device buffers of seeded sequences
    (class_harness.loop_inputs), in two legs: "ptau", a reference that moves with the tick and along the horizon
    (closed_loop_device_ptau; pendulum and msd), and "all", that with a process disturbance d and a measurement noise v
    (closed_loop_device_ex).  Behind the loop one plain control() of the x it left: the handle keeps the last tick's
    horizon and drops d and v.  Against the oracle driven tick by tick with the three statements of
    include/cgmres_hip.h (inputs_reference).  fp64: u, x and the follow-up u within 1e-7, the last tick's counts and
    reasons equal, with tol = 0 k_max natural exits, |t - 12 dt| <= 1e-12; fp32: u, x and the follow-up u within 1e-4
    (U and dUdt are not compared: under this noise the two oracle builds differ by up to 4.7e-3 relative on dUdt).
    The "all" leg skips msd in fp32, where the two oracle builds themselves end 4.6e-5 to 2.4e-4 apart
    (kernel_classes.leg_skip and the figures above it; tools/kernel_case_admission.py --inputs measures them).  What a
    wrong index costs, and what fp32 can and cannot see of it: tests/test_class_harness.py, planted faults.

An fp64 case that exceeds a bound is run again on variant 1, the lane mapping, which keeps the reference's statement
order: where that fails as well the shape is ill-conditioned and tools/kernel_case_admission.py let it through (mend its
rule, replace the case); where the lane mapping passes, the kernel is wrong.  The failure message says which.

The comparisons, the drivers and the test bodies are those of tests/class_harness.py, the first two bodies shared with
tests/test_gpu_user_kernel_classes.py (whose oracle is an executable with fixed forms: no sequences there).  Each check prints its worst |du| and |ddUdt| as a fraction of the bound before it
asserts."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
import class_harness as harness
import kernel_classes as kc
from class_harness import B8, B16, LOOP_TICKS

pytestmark = pytest.mark.gpu

_refs = {}


def reference(orc, case, tol):
    """The oracle's own closed loop of the B16 seeded instances for LOOP_TICKS + 1 ticks, recorded tick by tick in the
    format of class_harness: what goes into each tick (t, U, d, x) and what comes out (u, U1, d1, k, reason).  The first
    TICKS of them are the teacher-forced reference, tick LOOP_TICKS - 1 and the x behind it the device loop's (fp32:
    the plant step in the controller's precision, as the device does x + f * dt in T).  Computed once per shape and
    tolerance, never modified."""
    key = (case.model, case.dtype, case.dv, case.k_max, tol)
    if key not in _refs:
        f32 = case.dtype == 1
        x0, u0, p = orc.batch_scenario(case.model, B16)
        ctrls = []
        for i in range(B16):
            r = orc.Controller(case.model, case.dv, case.k_max, tol, kc.DTYPE_NAMES[case.dtype])
            orc.start_controller(r, x0[i], u0[i], p[i])
            ctrls.append(r)
        x = x0.astype(np.float32).astype(np.float64) if f32 else x0.copy()
        rec = {q: [] for q in ("t", "U", "d", "x", "u", "U1", "d1", "k", "reason")}
        for _ in range(LOOP_TICKS + 1):
            t, U, d = zip(*[r.get_state() for r in ctrls])
            u = np.array([r.control(x[i]) for i, r in enumerate(ctrls)])
            _, U1, d1 = zip(*[r.get_state() for r in ctrls])
            solve = np.array([r.last_solve() for r in ctrls])
            for q, v in zip(rec, (t, U, d, x, u, U1, d1, solve[:, 0], solve[:, 2])):
                rec[q].append(np.array(v))
            for i, r in enumerate(ctrls):
                if f32:
                    x[i] = (x[i].astype(np.float32) + r.plant(x[i], u[i]).astype(np.float32) * np.float32(r.dt)).astype(np.float32)
                else:
                    x[i] = x[i] + r.plant(x[i], u[i]) * r.dt
        _refs[key] = {q: np.stack(v, axis=1) for q, v in rec.items()}
    return _refs[key]


def inputs_reference(orc, case, tol, leg):
    """harness.oracle_loop_inputs of the B16 seeded instances under the leg's sequences of harness.loop_inputs (fp32:
    cast to float32 once, the oracle reads the cast values).  Computed once per shape, tolerance and leg, never modified."""
    key = (case.model, case.dtype, case.dv, case.k_max, tol, leg)
    if key not in _refs:
        x0, u0, p = orc.batch_scenario(case.model, B16)
        dims = orc.Controller(case.model, case.dv, case.k_max)
        npdt = np.float32 if case.dtype == 1 else np.float64
        seq, d, v = harness.leg_of(leg, *harness.loop_inputs((dims.dim_x, dims.dim_p), case.dv, p, npdt))
        _refs[key] = harness.oracle_loop_inputs(orc, case.model, kc.DTYPE_NAMES[case.dtype], case.dv, case.k_max, tol,
                                                x0, u0, p, seq, d, v)
    return _refs[key]


def batch_of(case, tol, variant=None):
    B = B16 if kc.ipw(case.cls) == 16 else B8
    kw = dict(batch=B, dv=case.dv, k_max=case.k_max, tol=tol, dtype=kc.DTYPE_NAMES[case.dtype])
    if variant is not None:
        return cg.CgmresBatch(case.model, variant=variant, **kw), B
    c = cg.CgmresBatch(case.model, variant=case.variant, flags=case.flags, **kw)
    assert c.variant_name == case.variant_name, (kc.case_id(case), c.variant_name, case.variant_name)
    return c, B


def scenario(orc, case, B):
    return tuple(a[:B] for a in orc.batch_scenario(case.model, B16))


def bounds(case, tol):
    """fp32: the spread the case records for the tolerance mode, if any"""
    if case.dtype == 0:
        return harness.F64
    return harness.f32_bounds((case.fp32_spread or (None, None))[0 if tol else 1])


SIDE = harness.Side(kc, "kernel class", "orc", reference, batch_of, scenario, bounds,
                    "loop: |du|,|dx|/bound {wu:.3g} |ddUdt|/bound {wd:.3g}", inputs_reference)
test_teacher_forced_ticks_vs_oracle, test_device_loop_across_a_launch_boundary_vs_oracle = harness.class_tests(SIDE, cg)
(test_device_loop_with_a_moving_reference_vs_oracle,
 test_device_loop_with_disturbance_noise_and_moving_reference_vs_oracle) = harness.class_inputs_tests(SIDE, cg)
