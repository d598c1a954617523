"""Every kernel a plugin model can be given (tests/user_kernel_classes.py: one tick_wg_kernel instantiation of
UserDev<Model> in one LDS plan and chunk count is a class, the wave and the lane kernel one more each) against the
oracle's generic controller on the same header (tests/user_models/user_oracle.cpp), at the members of each class that
CASES lists.  The models are the five aliases of tests/user_models/shape_models.hpp.

Batch: 20 controllers for a 16-instance kernel (one full workgroup and one with 4 of 16 rows), 11 for an 8-instance
one, 20 for wave and lane; the scenario of user_oracle.cpp.  Per case, with tol = 1e-6 and, where the case's fixed_k_ok
says so, tol = 0:

  * 4 teacher-forced ticks through control(): controller state and x taken from the plain oracle every tick.
    |du| <= 1e-9 * max(1, |u_ref|), |ddUdt'| <= 1e-7 * max(1, |dUdt_ref|), Arnoldi count and exit reason
    equal, and with tol = 0 exactly k_max iterations everywhere.
  * 12 ticks of closed_loop_device from the seeded start (one launch boundary; the plant is Model::dxdt with stage-0 p)
    against the oracle's free run: u and x within 1e-7, the last tick's counts and reasons equal, everything finite
    (the bounds of test_gpu_gs_ring.py).

A case that exceeds a bound is run again on variant 1, the lane mapping, which calls the user's functions as they are
in the reference's statement order: where that fails as well the shape is ill-conditioned and
tools/user_case_admission.py let it through (mend its rule, replace the case); where the lane mapping passes, the kernel
is wrong.  The failure message says which.

The white-box hooks (F_func, prepare, Ax_func) once per alias and distinct hook kernel (instances per workgroup, short
or long vectors, full or fh_hbm plan) at that class's member A, with the bounds of test_gpu_parity.test_hooks_vs_golden.
The member B of every wg class of Shape431 and Shape262 (tightest allocation, deepest look-ahead) once more on a
-DCGM_DEBUG_LDS build of the plugin, which checks every address of the costate sweep against the allocation.  And the refusals on the device.

The comparison, the driver and the two test bodies shared with tests/test_gpu_kernel_classes.py are those of
tests/class_harness.py.  Each check prints its worst figure as a fraction of its bound before it asserts."""
import ctypes
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
import class_harness as harness
import user_kernel_classes as uk
import user_oracle
from cgmres_cpp_amd import plugin
from class_harness import B8, B16, LOOP_TICKS, forced_problems, relmax

pytestmark = pytest.mark.gpu

HEADER = os.path.join(user_oracle.ROOT, "tests", "user_models", "shape_models.hpp")
HOOK_F, HOOK_B, HOOK_AX = 1e-11, 1e-7, 1e-7
DIMS = {"Shape110": (1, 1, 0), "Shape321": (3, 2, 1), "Shape262": (2, 6, 2), "Shape431": (4, 3, 1), "Shape521": (5, 2, 1)}
# the aliases with a -DCGM_DEBUG_LDS flavour: the two with the most kernel classes (every sweep form, both vector
# lengths, fh_hbm); the other three have the serial sweep only, whose look-ahead check_layout covers on the CPU
DBG_ALIASES = ("Shape431", "Shape262")
DBG_CASES = [c for c in uk.RECORDS if uk.kind(c.cls) == "wg" and "B" in c.member and uk.ALIASES[c.alias] in DBG_ALIASES]


def hook_cases():
    """member A of the first class (in class order: the serial sweep first) of every (alias, ipw, maxm, plan)"""
    out = {}
    for c in sorted(uk.RECORDS, key=lambda c: c.cls):
        if uk.kind(c.cls) == "wg" and "A" in c.member:
            out.setdefault(hook_kernel(c.cls), c)
    return list(out.values())


def hook_kernel(cls):
    return (uk.alias_of(cls), uk.ipw(cls), uk.maxm(cls), uk.plan(cls))


HOOK_CASES = hook_cases()

_mids, _exes, _refs = {}, {}, {}


def model_id(alias, debug=False):
    """the registered plugin of the alias; built on demand where __graft_entry__.build() has not left it"""
    key = (alias, debug)
    if key not in _mids:
        if not os.path.exists(plugin._build.HIPCC) and not os.path.exists(plugin.plugin_path(plugin_name(alias, debug))):
            pytest.skip("neither the plugin nor hipcc is available")
        so = plugin.build(HEADER, cls=uk.ALIASES[alias], name=plugin_name(alias, debug), extra_flags=("-DCGM_DEBUG_LDS",) if debug else ())
        _mids[key] = (plugin.register(so), so)
    return _mids[key]


def plugin_name(alias, debug):
    return uk.ALIASES[alias].lower() + ("_dbg" if debug else "")


def oracle_exe(alias, tmp_path_factory):
    """the prebuilt plain-flavour executable when it is there, g++ otherwise"""
    if alias not in _exes:
        cls = uk.ALIASES[alias]
        exe = user_oracle.prebuilt(cls)
        if not os.path.exists(exe):
            if not user_oracle.have_gxx():
                pytest.skip("neither the oracle executable nor g++ is available")
            exe = user_oracle.build(HEADER, cls, tmp_path_factory.mktemp("user_oracle") / f"user_oracle_{cls}")
        _exes[alias] = exe
    return _exes[alias]


@pytest.fixture
def oracle(tmp_path_factory):
    def reference(alias, dv, km, tol):
        """The oracle's free run of the B16 instances for LOOP_TICKS + 1 ticks, recorded tick by tick (what goes into each
        tick, what comes out): the first TICKS of them are the teacher-forced reference, tick LOOP_TICKS - 1 and the x
        behind it the device loop's.  Computed once per shape and tolerance, never modified."""
        key = (alias, dv, km, tol)
        if key not in _refs:
            nx, nu, _ = DIMS[uk.ALIASES[alias]]
            _refs[key] = user_oracle.run_full(oracle_exe(alias, tmp_path_factory), nx, nu, B16, LOOP_TICKS + 1, dv, km, tol)[0]
        return _refs[key]

    reference.exe = lambda alias: oracle_exe(alias, tmp_path_factory)
    return reference


def batch_of(case, tol, variant=None, debug=False):
    B = B8 if uk.ipw(case.cls) == 8 else B16
    mid = model_id(case.alias, debug)[0]
    if variant is not None:
        return cg.CgmresBatch(mid, batch=B, dv=case.dv, k_max=case.k_max, tol=tol, variant=variant), B
    c = cg.CgmresBatch(mid, batch=B, dv=case.dv, k_max=case.k_max, tol=tol, variant=case.variant, flags=case.flags)
    assert c.variant_name == case.variant_name, (uk.case_id(case), c.variant_name, case.variant_name)
    return c, B


def scenario_of(case, B):
    return user_oracle.scenario(B, *DIMS[uk.ALIASES[case.alias]])


SIDE = harness.Side(uk, "user kernel class", "oracle", lambda oracle, case, tol: oracle(case.alias, case.dv, case.k_max, tol), batch_of,
                    lambda oracle, case, B: scenario_of(case, B), lambda case, tol: harness.F64, "loop: |du|,|dx|/bound {wu:.3g}")
test_teacher_forced_ticks_vs_oracle, test_device_loop_across_a_launch_boundary_vs_oracle = harness.class_tests(SIDE, cg)


@pytest.mark.parametrize("case", DBG_CASES, ids=[uk.case_id(c) for c in DBG_CASES])
def test_member_b_on_the_debug_lds_build_stays_inside_its_allocation(oracle, case):
    """The teacher-forced ticks with tol = 1e-6 on the -DCGM_DEBUG_LDS flavour of the plugin: the same bounds, and no
    address of the costate sweep outside the workgroup's allocation."""
    so = model_id(case.alias, debug=True)[1]
    bad, wu, wd = forced_problems(SIDE, oracle, case, 1e-6, debug=True)
    oob = ctypes.CDLL(so).cgmres_hip_plugin_debug_lds_oob()
    print(f"user kernel class {uk.class_name(case.cls)} case {uk.case_id(case)} tol 1e-06 debug-lds: |du|/bound {wu:.3g} |ddUdt|/bound {wd:.3g} oob {oob:#x}")
    assert not bad, (uk.case_id(case), len(bad), bad[:4])
    assert oob == 0, hex(oob)


@pytest.mark.parametrize("case", HOOK_CASES, ids=["%s-ipw%d-maxm%d-plan%d" % ((uk.ALIASES[c.alias],) + hook_kernel(c.cls)[1:]) for c in HOOK_CASES])
def test_hooks_vs_oracle(oracle, case):
    """F_func, the pre-solve part of control (prepare: b) and Ax_func of a user model's handle, after the Newton start,
    one control() and the plant step, against the same statements of the oracle (user_oracle.cpp's "hooks" form)."""
    a, dv, km = case.alias, case.dv, case.k_max
    nx, nu, _ = DIMS[uk.ALIASES[a]]
    ref = user_oracle.run_hooks(oracle.exe(a), nx, nu, B16, dv, km, 1e-6)
    c, B = batch_of(case, 1e-6)
    c.set_ptau_repeat(scenario_of(case, B)[2])
    c.set_state(ref["t"], ref["U"][:B], ref["d"][:B])
    got = (c.F_func(ref["U"][:B], ref["x"][:B], ref["t"]), c.prepare(ref["x"][:B]), c.Ax_func(ref["v"][:B]))
    c.close()
    worst = [max(relmax(g[i], ref[k][i]) for i in range(B)) / bound
             for g, k, bound in zip(got, ("F", "b", "Ax"), (HOOK_F, HOOK_B, HOOK_AX))]
    print(f"user kernel class {uk.class_name(case.cls)} case {uk.case_id(case)} hooks: F/bound {worst[0]:.3g} b/bound {worst[1]:.3g} Ax/bound {worst[2]:.3g}")
    assert all(w <= 1.0 for w in worst), (uk.case_id(case), worst)


def test_refusals_leave_the_plugin_usable(oracle):
    """An explicit variant 3 (the lean plan: a state equation that reads p is refused there) and an explicit variant 2 at
    sizes the planner refuses (uk.REFUSED_WG, asserted on the CPU in tests/test_user_kernel_ledger.py) raise
    CgmresHipError; after each, a valid handle of the same plugin still runs a tick inside the bounds."""
    a, dv, km = uk.REFUSED_WG
    mid = model_id(a)[0]
    case = next(c for c in uk.RECORDS if c.alias == a and uk.kind(c.cls) == "wg" and "A" in c.member)

    def one_tick():
        ref = oracle(a, case.dv, case.k_max, 1e-6)
        c, B = batch_of(case, 1e-6)
        c.set_ptau_repeat(scenario_of(case, B)[2])
        c.set_state(float(ref["t"][0, 1]), ref["U"][:B, 1], ref["d"][:B, 1])
        u = c.control(ref["x"][:B, 1])
        c.close()
        assert max(relmax(u[i], ref["u"][i, 1]) for i in range(B)) <= harness.F64.u

    with pytest.raises(cg.CgmresHipError):
        cg.CgmresBatch(mid, batch=B16, dv=case.dv, k_max=case.k_max, variant=3)
    one_tick()
    with pytest.raises(cg.CgmresHipError):
        cg.CgmresBatch(mid, batch=B16, dv=dv, k_max=km, variant=2)
    one_tick()
