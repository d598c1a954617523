"""Every kernel a PLUGIN model can be given — plan_wg<UserDev<Model>, double> (csrc/wg_plan.hip.h) through the CPU probe
tests/plan_probe_user.hip, plus the wave and the lane mapping — and the shapes at which each one is held to the oracle's
generic controller on the GPU (tests/test_gpu_user_kernel_classes.py).  A plain module: no GPU call, nothing from
conftest.  The method is that of tests/kernel_classes.py; the models are the five aliases of
tests/user_models/shape_models.hpp:

    Shape110  (1, 1, 0)  smallest shape, no parameters, odd NBW_RAW (UserDev's second pad)
    Shape321  (3, 2, 1)  odd dim_x with even dim_u: both pads of UserDev, serial costate only on wg, 3 x 3 maps on wave
    Shape262  (2, 6, 2)  the wave limit on dim_u; long vectors (MAXM = 20) from dv 27; fh_hbm
    Shape431  (4, 3, 1)  largest kPar2 shape, 32 stage coefficients, long vectors from dv 54
    Shape521  (5, 2, 1)  beyond kPar2 and beyond the wave mapping

A CLASS is (alias, ipw, maxm, par, plan, cs_chunks) with the planner's own fields (par: 0 serial, 1 chunk-parallel with
LDS scratch, 2 two-pass; plan: 0 full, 1 fh_hbm; cs_chunks: 3 or 4 with the two-pass sweep, else 0).  Two more per
alias, written with ipw 1 and ipw 0 and zeros behind: the wave kernel (where WaveOps::FITS holds) and the lane kernel.

grid(): 5 aliases, dv 1..107, k_max 1..20, batch 16, tol 1e-6, variants 2, 3 and 4, at most one kernel-selecting flag.
The lane class's members are every (dv, k_max) of the grid on variant 1.

CASES, chosen by tools/user_case_admission.py --select from the ADMITTED members (measured on the reference side, the
fp64 rule of tools/kernel_case_admission.py unchanged: the tool's docstring has it):

    wg classes   A and B by class_ledger.order_a / order_b (A: smallest dv with k_max >= 3; B: largest lds_bytes)
    wave class   A, B' (largest dv, there the largest k_max: dv 63, k_max 10) and N: the admitted dv nearest to 17 with
                 k_max 5 (dv 17 puts one stage past a 16-lane DPP row; Chain4 covers the other row edges)
    lane class   A only

DEVICE_MISSES as in tests/kernel_classes.py (empty: nothing has been moved there).  tests/test_user_kernel_ledger.py is
the CPU side."""
from collections import namedtuple
from operator import itemgetter

import plan_probe
from class_ledger import CASE_COLUMNS, MEMBER_COLUMNS, order_a, order_b

ALIASES = ("Shape110", "Shape321", "Shape262", "Shape431", "Shape521")
FLAG_BITS = {"SERIAL_COSTATE": 1, "IPW8": 2, "TWO_PASS_COSTATE": 8}
FLAGS = (0, 1, 2, 8)
VARIANTS = (2, 3, 4)
DV, KMAX = range(1, 108), range(1, 21)
BATCH, TOL = 16, 1e-6
CUS = 256  # enters the library's own choice (variant 0) and `binning` only: neither is part of a class
WAVE_NEAR_DV, WAVE_NEAR_K = 17, 5

# class -> {(dv, k_max): what was seen}
DEVICE_MISSES = {}
# (alias, dv, k_max) at which the planner refuses an explicit variant 2 (32 stage coefficients against rows of 15 controls:
# WgTraits::lookahead_fits); the GPU test asks for it on the device and expects an error, not a fault
REFUSED_WG = (3, 5, 5)


# one row of CASES; one configuration of grid() (or of the lane kernel) with what the planner makes of it
Case = namedtuple("Case", "alias " + CASE_COLUMNS + " member")
Member = namedtuple("Member", "alias " + MEMBER_COLUMNS)


def cfg(alias, dv, k_max, variant, flags, batch=BATCH, tol=TOL):
    return plan_probe.config(alias, 0, dv, k_max, batch, variant, flags, tol)


def resolve(lib, alias, dv, k_max, variant, flags, batch=BATCH, tol=TOL, cus=CUS):
    """The planner's result for one configuration (variant 2, 3, 4 or 0, with its alias), or None where it refuses."""
    r, _ = plan_probe.plan(lib, cfg(alias, dv, k_max, variant, flags, batch, tol), cus)
    if r is not None:
        r["alias"] = alias
    return r


def class_of(r):
    if r["wave"]:
        return wave_class(r["alias"])
    return (r["alias"], r["ipw"], r["maxm"], r["par"], r["plan"], r["cs_chunks"])


def wave_class(alias):
    return (alias, 1, 0, 0, 0, 0)


def lane_class(alias):
    return (alias, 0, 0, 0, 0, 0)


# the fields of a class, by name
alias_of, ipw, maxm, par, plan, cs_chunks = (itemgetter(i) for i in range(6))


def kind(c):
    return {0: "lane", 1: "wave"}.get(ipw(c), "wg")


def class_name(c):
    if kind(c) != "wg":
        return "%s-%s" % (ALIASES[c[0]], kind(c))
    return "%s-ipw%d-maxm%d-par%d-plan%d-chunks%d" % ((ALIASES[c[0]],) + tuple(c[1:]))


def grid():
    return [(a, dv, k, v, f) for a in range(len(ALIASES)) for dv in DV for k in KMAX for v in VARIANTS for f in FLAGS]


def members(lib):
    """class -> its members"""
    out = {}
    for row in grid():
        r = resolve(lib, *row)
        if r is not None:
            out.setdefault(class_of(r), []).append(Member(*row, r["lds_bytes_tick"], r["variant_name"]))
    for a in range(len(ALIASES)):
        out[lane_class(a)] = [Member(a, dv, k, 1, 0, 0, "lane") for dv in DV for k in KMAX]
    return out


def order_wave_b(rows):
    """largest dv, there the largest k_max; the plain configuration first"""
    return sorted(rows, key=lambda r: (-r.dv, -r.k_max, r.flags))


def order_wave_near(rows):
    """k_max 5, by the distance of dv from 17 (the shorter horizon first at equal distance)"""
    return sorted((r for r in rows if r.k_max == WAVE_NEAR_K), key=lambda r: (abs(r.dv - WAVE_NEAR_DV), r.dv, r.flags))


def orders(c):
    """the selections of class c: (letter, ordering) pairs"""
    if kind(c) == "lane":
        return (("A", order_a),)
    if kind(c) == "wave":
        return (("A", order_a), ("B", order_wave_b), ("N", order_wave_near))
    return (("A", order_a), ("B", order_b))


def key(r):
    """the configuration of a case or a member"""
    return (r.alias, r.dv, r.k_max, r.variant, r.flags)


def case_id(r):
    return "%s-dv%d-k%d-v%d-f%d" % ((ALIASES[r.alias],) + key(r)[1:])


def dims(lib, alias):
    return plan_probe.alias_info(lib, alias)


# (alias, dv, k_max, variant, flags, class, variant_name, fixed_k_ok, member)
# member: which selection(s) of its class the case is ("A", "B", "AB", "N", ...); the debug-LDS flavour of the GPU test
# runs the wg cases with a B.  The comment above each case: the number of members of its class and its lds_bytes
# (horizons that were passed over because they were not admitted are listed in front of the case that took their
# place), then what the two oracle builds disagree by over the 20 instances, tol = 1e-6 | tol = 0: the spread of u and of
# dUdt' over 6 teacher-forced ticks relative to max(1, |.|) and whether every count and exit reason agreed; "loop": |du|,
# |dx| after 12 free-running ticks and whether the last tick's counts and reasons agreed; "early exits": some tick of the
# free run ended before k_max iterations.
# BEGIN CASES (tools/user_case_admission.py --select writes this block)
CASES = [
    # dv 1 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 0.0e+00 0.0e+00 COUNTS DIFFER, loop 1.1e-16 COUNTS DIFFER, early exits | 0.0e+00 0.0e+00 COUNTS DIFFER, loop 1.1e-16 COUNTS DIFFER, early exits)
    # Shape110-lane: A of 2140, lds_bytes 0: 2.1e-16 1.2e-13 agree, loop 1.3e-15 agree, early exits | 0.0e+00 0.0e+00 agree, loop 1.1e-16 agree, early exits
    (0, 2, 3, 1, 0, (0, 0, 0, 0, 0, 0), 'lane', False, 'A'),
    # Shape110-wave: A of 2400, lds_bytes 16: 1.1e-16 1.1e-13 agree, loop 1.3e-15 agree, early exits | 2.0e-16 1.0e-13 agree, loop 2.2e-16 agree
    (0, 4, 3, 4, 0, (0, 1, 0, 0, 0, 0), 'wave', True, 'A'),
    # Shape110-wave: B of 2400, lds_bytes 16: 2.1e-16 1.4e-13 agree, loop 6.7e-16 agree, early exits | 2.5e-14 4.4e-11 agree, loop 2.2e-16 agree
    (0, 63, 10, 4, 0, (0, 1, 0, 0, 0, 0), 'wave', True, 'B'),
    # Shape110-wave: N of 2400, lds_bytes 16: 1.9e-16 1.1e-13 agree, loop 8.0e-15 agree, early exits | 7.3e-15 2.1e-11 agree, loop 2.2e-16 agree
    (0, 17, 5, 4, 0, (0, 1, 0, 0, 0, 0), 'wave', True, 'N'),
    # Shape110-ipw8-maxm10-par0-plan0-chunks0: A of 2080, lds_bytes 4016: 1.1e-16 1.1e-13 agree, loop 1.3e-15 agree, early exits | 2.0e-16 1.0e-13 agree, loop 2.2e-16 agree
    (0, 4, 3, 2, 2, (0, 8, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape110-ipw8-maxm10-par0-plan0-chunks0: B of 2080, lds_bytes 67376: 1.8e-16 1.5e-13 agree, loop 2.2e-16 agree, early exits | 3.6e-13 4.9e-10 agree, loop 4.4e-16 agree
    (0, 107, 20, 2, 2, (0, 8, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape110-ipw16-maxm10-par0-plan0-chunks0: A of 6240, lds_bytes 8016: 1.1e-16 1.1e-13 agree, loop 1.3e-15 agree, early exits | 2.0e-16 1.0e-13 agree, loop 2.2e-16 agree
    (0, 4, 3, 2, 0, (0, 16, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape110-ipw16-maxm10-par0-plan0-chunks0: B of 6240, lds_bytes 134736: 1.8e-16 1.5e-13 agree, loop 2.2e-16 agree, early exits | 3.6e-13 4.9e-10 agree, loop 4.4e-16 agree
    (0, 107, 20, 2, 0, (0, 16, 10, 0, 0, 0), 'wg', True, 'B'),
    # dv 1 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 7.8e-03 7.6e+00 COUNTS DIFFER, loop 7.1e-05 COUNTS DIFFER, early exits | 0.0e+00 0.0e+00 COUNTS DIFFER, loop 4.4e-16 COUNTS DIFFER, early exits)
    # Shape321-lane: A of 2140, lds_bytes 0: 2.8e-15 4.4e-13 agree, loop 6.7e-16 agree, early exits | 3.1e-15 4.7e-13 agree, loop 6.7e-16 agree
    (1, 2, 3, 1, 0, (1, 0, 0, 0, 0, 0), 'lane', True, 'A'),
    # Shape321-wave: A of 2160, lds_bytes 16: 6.3e-15 1.5e-12 agree, loop 8.9e-16 agree, early exits | 6.6e-15 1.5e-12 agree, loop 8.9e-16 agree
    (1, 10, 3, 4, 0, (1, 1, 0, 0, 0, 0), 'wave', True, 'A'),
    # Shape321-wave: B of 2160, lds_bytes 16: 2.4e-14 5.0e-12 agree, loop 4.4e-16 agree, early exits | 4.9e-13 7.2e-11 agree, loop 8.0e-15 agree
    (1, 63, 10, 4, 0, (1, 1, 0, 0, 0, 0), 'wave', True, 'B'),
    # Shape321-wave: N of 2160, lds_bytes 16: 8.3e-15 1.5e-12 agree, loop 4.4e-16 agree, early exits | 9.0e-15 1.6e-12 agree, loop 4.4e-16 agree
    (1, 17, 5, 4, 0, (1, 1, 0, 0, 0, 0), 'wave', True, 'N'),
    # Shape321-ipw8-maxm10-par0-plan0-chunks0: A of 3745, lds_bytes 20144: 6.3e-15 1.5e-12 agree, loop 8.9e-16 agree, early exits | 6.6e-15 1.5e-12 agree, loop 8.9e-16 agree
    (1, 10, 3, 2, 2, (1, 8, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape321-ipw8-maxm10-par0-plan0-chunks0: B of 3745, lds_bytes 158512: 1.5e-14 4.7e-12 agree, loop 1.1e-15 agree, early exits | 6.8e-12 8.4e-10 agree, loop 4.6e-14 agree
    (1, 80, 20, 2, 0, (1, 8, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape321-ipw8-maxm20-par0-plan0-chunks0: A of 668, lds_bytes 142896: 2.9e-14 4.9e-12 agree, loop 6.7e-16 agree, early exits | 2.9e-14 4.9e-12 agree, loop 8.9e-16 agree
    (1, 81, 3, 2, 0, (1, 8, 20, 0, 0, 0), 'wg', True, 'A'),
    # Shape321-ipw8-maxm20-par0-plan0-chunks0: B of 668, lds_bytes 162736: 1.5e-14 1.8e-12 agree, loop 6.7e-16 agree | 1.5e-14 1.8e-12 agree, loop 6.7e-16 agree
    (1, 93, 1, 2, 0, (1, 8, 20, 0, 0, 0), 'wg', True, 'B'),
    # Shape321-ipw16-maxm10-par0-plan0-chunks0: A of 1935, lds_bytes 40272: 6.3e-15 1.5e-12 agree, loop 8.9e-16 agree, early exits | 6.6e-15 1.5e-12 agree, loop 8.9e-16 agree
    (1, 10, 3, 2, 0, (1, 16, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape321-ipw16-maxm10-par0-plan0-chunks0: B of 1935, lds_bytes 162640: 2.0e-14 3.2e-12 agree, loop 6.7e-16 agree, early exits | 2.0e-14 3.2e-12 agree, loop 5.6e-16 agree
    (1, 44, 7, 2, 0, (1, 16, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape262-lane: A of 2140, lds_bytes 0: 5.6e-16 2.8e-13 agree, loop 2.8e-16 agree | 5.6e-16 2.8e-13 agree, loop 2.8e-16 agree
    (2, 1, 3, 1, 0, (2, 0, 0, 0, 0, 0), 'lane', True, 'A'),
    # Shape262-wave: A of 2040, lds_bytes 16: 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree | 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree
    (2, 3, 3, 4, 0, (2, 1, 0, 0, 0, 0), 'wave', True, 'A'),
    # Shape262-wave: B of 2040, lds_bytes 16: 5.0e-15 4.0e-12 agree, loop 3.9e-16 agree, early exits | 5.0e-15 4.0e-12 agree, loop 4.4e-16 agree
    (2, 53, 10, 4, 0, (2, 1, 0, 0, 0, 0), 'wave', True, 'B'),
    # Shape262-wave: N of 2040, lds_bytes 16: 3.1e-15 1.8e-12 agree, loop 2.8e-16 agree | 3.1e-15 1.8e-12 agree, loop 2.8e-16 agree
    (2, 17, 5, 4, 0, (2, 1, 0, 0, 0, 0), 'wave', True, 'N'),
    # Shape262-ipw8-maxm10-par0-plan0-chunks0: A of 486, lds_bytes 9968: 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree | 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree
    (2, 3, 3, 2, 2, (2, 8, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape262-ipw8-maxm10-par0-plan0-chunks0: B of 486, lds_bytes 83312: 2.6e-15 2.2e-12 agree, loop 3.3e-16 agree, early exits | 1.6e-14 1.1e-11 agree, loop 6.1e-16 agree
    (2, 26, 20, 2, 0, (2, 8, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape262-ipw8-maxm20-par0-plan0-chunks0: A of 1632, lds_bytes 68336: 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree | 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree
    (2, 27, 3, 2, 2, (2, 8, 20, 0, 0, 0), 'wg', True, 'A'),
    # Shape262-ipw8-maxm20-par0-plan0-chunks0: B of 1632, lds_bytes 148976: 5.0e-15 4.0e-12 agree, loop 3.9e-16 agree, early exits | 2.8e-13 1.2e-10 agree, loop 1.3e-15 agree
    (2, 53, 20, 2, 0, (2, 8, 20, 0, 0, 0), 'wg', True, 'B'),
    # Shape262-ipw16-maxm10-par0-plan0-chunks0: A of 560, lds_bytes 19920: 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree | 1.1e-15 6.1e-13 agree, loop 3.3e-16 agree
    (2, 3, 3, 2, 0, (2, 16, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape262-ipw16-maxm10-par0-plan0-chunks0: B of 560, lds_bytes 161744: 3.5e-15 2.2e-12 agree, loop 2.8e-16 agree, early exits | 9.3e-15 7.1e-12 agree, loop 4.4e-16 agree
    (2, 25, 20, 2, 0, (2, 16, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape262-ipw16-maxm10-par1-plan0-chunks0: A of 403, lds_bytes 33504: 9.4e-16 6.4e-13 agree, loop 5.0e-16 agree | 9.4e-16 6.4e-13 agree, loop 5.0e-16 agree
    (2, 4, 3, 2, 0, (2, 16, 10, 1, 0, 0), 'wg+parallel-costate', True, 'A'),
    # Shape262-ipw16-maxm10-par1-plan0-chunks0: B of 403, lds_bytes 162784: 2.6e-15 1.9e-12 agree, loop 3.3e-16 agree, early exits | 2.6e-15 1.9e-12 agree, loop 3.9e-16 agree
    (2, 22, 16, 2, 0, (2, 16, 10, 1, 0, 0), 'wg+parallel-costate', True, 'B'),
    # Shape262-ipw16-maxm10-par2-plan0-chunks3: A of 40, lds_bytes 35808: 2.2e-15 1.0e-12 agree, loop 5.0e-16 agree | 2.2e-15 1.0e-12 agree, loop 5.0e-16 agree
    (2, 6, 3, 2, 8, (2, 16, 10, 2, 0, 3), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm10-par2-plan0-chunks3: B of 40, lds_bytes 75488: 2.1e-15 1.0e-12 agree, loop 2.8e-16 agree, early exits | 1.1e-14 4.2e-12 agree, loop 5.6e-16 agree
    (2, 7, 20, 2, 8, (2, 16, 10, 2, 0, 3), 'wg+two-pass-costate', True, 'B'),
    # Shape262-ipw16-maxm10-par2-plan0-chunks4: A of 431, lds_bytes 46560: 2.3e-15 1.3e-12 agree, loop 3.9e-16 agree | 2.3e-15 1.3e-12 agree, loop 3.9e-16 agree
    (2, 8, 3, 2, 8, (2, 16, 10, 2, 0, 4), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm10-par2-plan0-chunks4: B of 431, lds_bytes 162784: 2.6e-15 2.2e-12 agree, loop 3.3e-16 agree, early exits | 2.6e-15 2.2e-12 agree, loop 3.9e-16 agree
    (2, 26, 18, 2, 0, (2, 16, 10, 2, 0, 4), 'wg+two-pass-costate', True, 'B'),
    # Shape262-ipw16-maxm20-par0-plan0-chunks0: A of 77, lds_bytes 136656: 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree | 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree
    (2, 27, 3, 2, 1, (2, 16, 20, 0, 0, 0), 'wg', True, 'A'),
    # Shape262-ipw16-maxm20-par0-plan0-chunks0: B of 77, lds_bytes 162512: 5.0e-15 2.3e-12 agree, loop 2.8e-16 agree, early exits | 5.0e-15 2.3e-12 agree, loop 3.3e-16 agree
    (2, 31, 8, 2, 0, (2, 16, 20, 0, 0, 0), 'wg', True, 'B'),
    # Shape262-ipw16-maxm20-par0-plan1-chunks0: A of 121, lds_bytes 144464: 3.2e-15 2.3e-12 agree, loop 3.3e-16 agree, early exits | 3.2e-15 2.3e-12 agree, loop 3.3e-16 agree
    (2, 27, 18, 2, 1, (2, 16, 20, 0, 1, 0), 'wg', True, 'A'),
    # Shape262-ipw16-maxm20-par0-plan1-chunks0: B of 121, lds_bytes 162640: 4.0e-15 2.7e-12 agree, loop 4.4e-16 agree, early exits | 4.1e-15 2.7e-12 agree, loop 3.9e-16 agree
    (2, 34, 14, 2, 0, (2, 16, 20, 0, 1, 0), 'wg', True, 'B'),
    # Shape262-ipw16-maxm20-par2-plan0-chunks3: A of 6, lds_bytes 162272: 2.7e-15 3.0e-12 agree, loop 3.3e-16 agree, early exits | 2.8e-15 3.0e-12 agree, loop 4.4e-16 agree
    (2, 30, 10, 2, 0, (2, 16, 20, 2, 0, 3), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm20-par2-plan0-chunks3: B of 6, lds_bytes 162272: 5.4e-15 2.3e-12 agree, loop 3.9e-16 agree | 5.4e-15 2.3e-12 agree, loop 3.9e-16 agree
    (2, 32, 3, 2, 0, (2, 16, 20, 2, 0, 3), 'wg+two-pass-costate', True, 'B'),
    # Shape262-ipw16-maxm20-par2-plan0-chunks4: A of 118, lds_bytes 138976: 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree | 3.2e-15 2.2e-12 agree, loop 3.9e-16 agree
    (2, 27, 3, 2, 0, (2, 16, 20, 2, 0, 4), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm20-par2-plan0-chunks4: B of 118, lds_bytes 162528: 3.5e-15 2.4e-12 agree, loop 3.9e-16 agree, early exits | 3.5e-15 2.4e-12 agree, loop 2.8e-16 agree
    (2, 29, 12, 2, 0, (2, 16, 20, 2, 0, 4), 'wg+two-pass-costate', True, 'B'),
    # Shape262-ipw16-maxm20-par2-plan1-chunks3: A of 8, lds_bytes 162144: 5.0e-15 2.3e-12 agree, loop 2.8e-16 agree, early exits | 5.0e-15 2.3e-12 agree, loop 3.3e-16 agree
    (2, 31, 18, 2, 0, (2, 16, 20, 2, 1, 3), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm20-par2-plan1-chunks3: B of 8, lds_bytes 162400: 5.5e-15 3.0e-12 agree, loop 3.1e-16 agree, early exits | 5.5e-15 3.1e-12 agree, loop 3.3e-16 agree
    (2, 33, 15, 2, 0, (2, 16, 20, 2, 1, 3), 'wg+two-pass-costate', True, 'B'),
    # Shape262-ipw16-maxm20-par2-plan1-chunks4: A of 198, lds_bytes 146784: 3.2e-15 2.3e-12 agree, loop 3.3e-16 agree, early exits | 3.2e-15 2.3e-12 agree, loop 3.3e-16 agree
    (2, 27, 18, 2, 0, (2, 16, 20, 2, 1, 4), 'wg+two-pass-costate', True, 'A'),
    # Shape262-ipw16-maxm20-par2-plan1-chunks4: B of 198, lds_bytes 162656: 3.2e-15 2.4e-12 agree, loop 3.9e-16 agree, early exits | 3.2e-15 2.4e-12 agree, loop 3.3e-16 agree
    (2, 35, 11, 2, 0, (2, 16, 20, 2, 1, 4), 'wg+two-pass-costate', True, 'B'),
    # dv 1 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 3.5e-15 4.1e-13 agree, loop 8.3e-05 COUNTS DIFFER | 7.0e-06 7.0e-03 COUNTS DIFFER, loop 5.6e-16 agree)
    # Shape431-lane: A of 2140, lds_bytes 0: 3.7e-15 6.5e-13 agree, loop 5.6e-16 agree | 3.7e-15 6.5e-13 agree, loop 5.6e-16 agree
    (3, 2, 3, 1, 0, (3, 0, 0, 0, 0, 0), 'lane', True, 'A'),
    # Shape431-wave: A of 1932, lds_bytes 16: 1.2e-14 2.3e-12 agree, loop 1.0e-15 agree | 1.2e-14 2.3e-12 agree, loop 5.6e-16 agree
    (3, 11, 3, 4, 0, (3, 1, 0, 0, 0, 0), 'wave', True, 'A'),
    # Shape431-wave: B of 1932, lds_bytes 16: 2.1e-14 5.3e-12 agree, loop 5.6e-16 agree, early exits | 2.1e-14 5.3e-12 agree, loop 1.1e-15 agree
    (3, 59, 5, 4, 0, (3, 1, 0, 0, 0, 0), 'wave', True, 'B'),
    # Shape431-wave: N of 1932, lds_bytes 16: 9.4e-15 2.6e-12 agree, loop 5.8e-16 agree, early exits | 9.5e-15 2.6e-12 agree, loop 5.6e-16 agree
    (3, 17, 5, 4, 0, (3, 1, 0, 0, 0, 0), 'wave', True, 'N'),
    # Shape431-ipw8-maxm10-par0-plan0-chunks0: A of 2464, lds_bytes 32624: 1.2e-14 2.3e-12 agree, loop 1.0e-15 agree | 1.2e-14 2.3e-12 agree, loop 5.6e-16 agree
    (3, 11, 3, 2, 2, (3, 8, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape431-ipw8-maxm10-par0-plan0-chunks0: B of 2464, lds_bytes 161392: 2.3e-14 5.0e-12 agree, loop 6.4e-16 agree, early exits | 6.8e-13 9.6e-11 agree, loop 4.3e-15 agree
    (3, 53, 19, 2, 0, (3, 8, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape431-ipw8-maxm20-par0-plan0-chunks0: A of 288, lds_bytes 148336: 3.5e-14 5.9e-12 agree, loop 7.8e-16 agree | 3.5e-14 5.9e-12 agree, loop 8.9e-16 agree
    (3, 54, 3, 2, 0, (3, 8, 20, 0, 0, 0), 'wg', True, 'A'),
    # Shape431-ipw8-maxm20-par0-plan0-chunks0: B of 288, lds_bytes 162800: 1.7e-14 5.7e-12 agree, loop 4.4e-16 agree, early exits | 3.7e-13 6.0e-11 agree, loop 3.7e-15 agree
    (3, 56, 14, 2, 0, (3, 8, 20, 0, 0, 0), 'wg', True, 'B'),
    # Shape431-ipw16-maxm10-par0-plan0-chunks0: A of 346, lds_bytes 65232: 1.2e-14 2.3e-12 agree, loop 1.0e-15 agree | 1.2e-14 2.3e-12 agree, loop 5.6e-16 agree
    (3, 11, 3, 2, 1, (3, 16, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape431-ipw16-maxm10-par0-plan0-chunks0: B of 346, lds_bytes 162000: 2.4e-14 4.2e-12 agree, loop 7.8e-16 agree | 2.4e-14 4.2e-12 agree, loop 7.8e-16 agree
    (3, 29, 3, 2, 0, (3, 16, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape431-ipw16-maxm10-par1-plan0-chunks0: A of 202, lds_bytes 85728: 1.2e-14 2.3e-12 agree, loop 1.0e-15 agree | 1.2e-14 2.3e-12 agree, loop 5.6e-16 agree
    (3, 11, 3, 2, 0, (3, 16, 10, 1, 0, 0), 'wg+parallel-costate', True, 'A'),
    # Shape431-ipw16-maxm10-par1-plan0-chunks0: B of 202, lds_bytes 162272: 1.0e-14 1.6e-12 agree, loop 5.6e-16 agree | 1.0e-14 1.6e-12 agree, loop 5.6e-16 agree
    (3, 23, 1, 2, 0, (3, 16, 10, 1, 0, 0), 'wg+parallel-costate', True, 'B'),
    # Shape431-ipw16-maxm10-par2-plan0-chunks3: AB of 20, lds_bytes 162784: 1.6e-14 3.3e-12 agree, loop 6.7e-16 agree, early exits | 8.7e-14 3.4e-11 agree, loop 2.4e-15 agree
    (3, 22, 20, 2, 0, (3, 16, 10, 2, 0, 3), 'wg+two-pass-costate', True, 'AB'),
    # Shape431-ipw16-maxm10-par2-plan0-chunks4: A of 404, lds_bytes 71392: 1.2e-14 2.3e-12 agree, loop 1.0e-15 agree | 1.2e-14 2.3e-12 agree, loop 5.6e-16 agree
    (3, 11, 3, 2, 8, (3, 16, 10, 2, 0, 4), 'wg+two-pass-costate', True, 'A'),
    # Shape431-ipw16-maxm10-par2-plan0-chunks4: B of 404, lds_bytes 162528: 1.6e-14 3.3e-12 agree, loop 4.4e-16 agree, early exits | 1.3e-13 2.2e-11 agree, loop 1.5e-15 agree
    (3, 25, 13, 2, 0, (3, 16, 10, 2, 0, 4), 'wg+two-pass-costate', True, 'B'),
    # dv 1 k_max 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20 not admitted (k_max 3: 1.2e-02 2.9e+01 COUNTS DIFFER, loop 4.1e-04 COUNTS DIFFER, early exits | 0.0e+00 0.0e+00 COUNTS DIFFER, loop 1.1e-15 COUNTS DIFFER, early exits)
    # Shape521-lane: A of 2140, lds_bytes 0: 1.4e-14 1.3e-12 agree, loop 1.1e-15 agree, early exits | 1.4e-14 1.3e-12 agree, loop 1.3e-15 agree
    (4, 2, 3, 1, 0, (4, 0, 0, 0, 0, 0), 'lane', True, 'A'),
    # Shape521-ipw8-maxm10-par0-plan0-chunks0: A of 2119, lds_bytes 69424: 2.7e-14 4.4e-12 agree, loop 1.8e-15 agree, early exits | 2.7e-14 4.4e-12 agree, loop 1.8e-15 agree
    (4, 21, 3, 2, 2, (4, 8, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape521-ipw8-maxm10-par0-plan0-chunks0: B of 2119, lds_bytes 162736: 4.0e-14 6.4e-12 agree, loop 1.8e-15 agree, early exits | 4.0e-14 6.4e-12 agree, loop 1.9e-15 agree
    (4, 50, 7, 2, 0, (4, 8, 10, 0, 0, 0), 'wg', True, 'B'),
    # Shape521-ipw16-maxm10-par0-plan0-chunks0: A of 141, lds_bytes 138832: 2.7e-14 4.4e-12 agree, loop 1.8e-15 agree, early exits | 2.7e-14 4.4e-12 agree, loop 1.8e-15 agree
    (4, 21, 3, 2, 0, (4, 16, 10, 0, 0, 0), 'wg', True, 'A'),
    # Shape521-ipw16-maxm10-par0-plan0-chunks0: B of 141, lds_bytes 162384: 3.3e-14 5.6e-12 agree, loop 1.8e-15 agree, early exits | 3.3e-14 5.6e-12 agree, loop 2.7e-15 agree
    (4, 24, 7, 2, 0, (4, 16, 10, 0, 0, 0), 'wg', True, 'B'),
]
# END CASES
CASES_DIGEST = 'a45431abacdde86f'
RECORDS = [Case(*c) for c in CASES]
