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

Each check prints its worst figure as a fraction of its bound before it asserts."""
import ctypes
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
import user_kernel_classes as uk
import user_oracle
from cgmres_cpp_amd import plugin

pytestmark = pytest.mark.gpu

HEADER = os.path.join(user_oracle.ROOT, "tests", "user_models", "shape_models.hpp")
B16, B8 = 20, 11
TICKS, LOOP_TICKS = 4, 12
U_TOL, DUDT_REL, LOOP_TOL = 1e-9, 1e-7, 1e-7
HOOK_F, HOOK_B, HOOK_AX = 1e-11, 1e-7, 1e-7
DIMS = {"Shape110": (1, 1, 0), "Shape321": (3, 2, 1), "Shape262": (2, 6, 2), "Shape431": (4, 3, 1), "Shape521": (5, 2, 1)}
IDS = [uk.case_id(c) for c in uk.CASES]
# the aliases with a -DCGM_DEBUG_LDS flavour: the two with the most kernel classes (every sweep form, both vector
# lengths, fh_hbm); the other three have the serial sweep only, whose look-ahead check_layout covers on the CPU
DBG_ALIASES = ("Shape431", "Shape262")
DBG_CASES = [c for c in uk.CASES if uk.kind(c[5]) == "wg" and "B" in c[8] and uk.ALIASES[c[0]] in DBG_ALIASES]


def hook_cases():
    """member A of the first class (in class order: the serial sweep first) of every (alias, ipw, maxm, plan)"""
    out = {}
    for c in sorted(uk.CASES, key=lambda c: c[5]):
        if uk.kind(c[5]) == "wg" and "A" in c[8]:
            out.setdefault((c[5][0], c[5][1], c[5][2], c[5][4]), c)
    return list(out.values())


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


def tols(case):
    return (1e-6, 0.0) if case[7] else (1e-6,)


def batch_of(case, tol, variant=None, debug=False):
    a, dv, km, v, f, cls, name = case[:7]
    B = B8 if cls[1] == 8 else B16
    mid = model_id(a, debug)[0]
    if variant is not None:
        return cg.CgmresBatch(mid, batch=B, dv=dv, k_max=km, tol=tol, variant=variant), B
    c = cg.CgmresBatch(mid, batch=B, dv=dv, k_max=km, tol=tol, variant=v, flags=f)
    assert c.variant_name == name, (uk.case_id(case), c.variant_name, name)
    return c, B


def scenario_of(case, B):
    return user_oracle.scenario(B, *DIMS[uk.ALIASES[case[0]]])


def relmax(a, ref):
    return float(np.max(np.abs(a - ref))) / max(1.0, float(np.max(np.abs(ref))))


def forced_problems(oracle, case, tol, variant=None, debug=False):
    """(problems, worst |du| / bound, worst |ddUdt'| / bound) of the teacher-forced ticks"""
    a, dv, km = case[:3]
    ref = oracle(a, dv, km, tol)
    c, B = batch_of(case, tol, variant, debug)
    c.set_ptau_repeat(scenario_of(case, B)[2])
    bad, wu, wd = [], 0.0, 0.0
    for n in range(TICKS):
        c.set_state(float(ref["t"][0, n]), ref["U"][:B, n], ref["d"][:B, n])
        u = c.control(ref["x"][:B, n])
        n_ax, reason = c.get_status()
        _, _, d1 = c.get_state()
        for i in range(B):
            ru = relmax(u[i], ref["u"][i, n]) / U_TOL
            rd = relmax(d1[i], ref["d1"][i, n]) / DUDT_REL
            if n_ax[i] != ref["k"][i, n] or reason[i] != ref["reason"][i, n]:
                bad.append(("count / reason", n, i, int(n_ax[i]), int(ref["k"][i, n]), int(reason[i]), int(ref["reason"][i, n])))
            if tol == 0.0 and n_ax[i] != km:
                bad.append(("fixed-k count", n, i, int(n_ax[i])))
            if not ru <= 1.0:
                bad.append(("u / bound", n, i, ru))
            if not rd <= 1.0:
                bad.append(("dUdt' / bound", n, i, rd))
            wu, wd = max(wu, ru) if ru == ru else np.inf, max(wd, rd) if rd == rd else np.inf
    c.close()
    return bad, wu, wd


def loop_problems(oracle, case, tol, variant=None, debug=False):
    a, dv, km = case[:3]
    ref = oracle(a, dv, km, tol)
    c, B = batch_of(case, tol, variant, debug)
    x0, u0, p = scenario_of(case, B)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p if c.dim_p else None, 10)
    xd = c.device_buffer((B, c.dim_x)).upload(x0)
    ud = c.device_buffer((B, c.dim_u))
    c.closed_loop_device(xd, ud, LOOP_TICKS)
    c.synchronize()
    x, u = xd.download(), ud.download()
    _, U, dU = c.get_state()
    n_ax, reason = c.get_status()
    xd.free(), ud.free(), c.close()
    n = LOOP_TICKS
    bad = []
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(U)) and np.all(np.isfinite(dU))):
        bad.append(("not finite",))
    if tol == 0.0 and not (np.all(n_ax == km) and np.all(reason == cg.EXIT_NATURAL)):
        bad.append(("fixed-k count", n_ax.tolist(), reason.tolist()))
    wu = max(float(np.max(np.abs(u - ref["u"][:B, n - 1]))), float(np.max(np.abs(x - ref["x"][:B, n])))) / LOOP_TOL
    if not wu <= 1.0:
        bad.append(("loop u or x / 1e-7", wu))
    if not (np.array_equal(n_ax, ref["k"][:B, n - 1]) and np.array_equal(reason, ref["reason"][:B, n - 1])):
        bad.append(("loop count / reason", n_ax.tolist(), ref["k"][:B, n - 1].tolist(), reason.tolist(), ref["reason"][:B, n - 1].tolist()))
    return bad, wu, 0.0


def verdict(oracle, case, tol, problems_of):
    """for the failure message: what the lane mapping makes of the same shape"""
    if uk.kind(case[5]) == "lane":
        return "this IS the lane mapping"
    lane_bad = problems_of(oracle, case, tol, variant=1)[0]
    if lane_bad:
        return "the lane mapping fails too (%r ...): the shape is ill-conditioned, mend the admission rule and replace the case" % (lane_bad[:2],)
    return "the lane mapping passes: a finding about this kernel"


@pytest.mark.parametrize("case", uk.CASES, ids=IDS)
def test_teacher_forced_ticks_vs_oracle(oracle, case):
    for tol in tols(case):
        bad, wu, wd = forced_problems(oracle, case, tol)
        print(f"user kernel class {uk.class_name(case[5])} case {uk.case_id(case)} tol {tol:g} forced: |du|/bound {wu:.3g} |ddUdt|/bound {wd:.3g}")
        assert not bad, (uk.case_id(case), tol, len(bad), bad[:4], verdict(oracle, case, tol, forced_problems))


@pytest.mark.parametrize("case", uk.CASES, ids=IDS)
def test_device_loop_across_a_launch_boundary_vs_oracle(oracle, case):
    assert LOOP_TICKS > cg.TICKS_PER_LAUNCH
    for tol in tols(case):
        bad, wu, _ = loop_problems(oracle, case, tol)
        print(f"user kernel class {uk.class_name(case[5])} case {uk.case_id(case)} tol {tol:g} loop: |du|,|dx|/bound {wu:.3g}")
        assert not bad, (uk.case_id(case), tol, len(bad), bad[:4], verdict(oracle, case, tol, loop_problems))


@pytest.mark.parametrize("case", DBG_CASES, ids=[uk.case_id(c) for c in DBG_CASES])
def test_member_b_on_the_debug_lds_build_stays_inside_its_allocation(oracle, case):
    """The teacher-forced ticks with tol = 1e-6 on the -DCGM_DEBUG_LDS flavour of the plugin: the same bounds, and no
    address of the costate sweep outside the workgroup's allocation."""
    so = model_id(case[0], debug=True)[1]
    bad, wu, wd = forced_problems(oracle, case, 1e-6, debug=True)
    oob = ctypes.CDLL(so).cgmres_hip_plugin_debug_lds_oob()
    print(f"user kernel class {uk.class_name(case[5])} case {uk.case_id(case)} tol 1e-06 debug-lds: |du|/bound {wu:.3g} |ddUdt|/bound {wd:.3g} oob {oob:#x}")
    assert not bad, (uk.case_id(case), len(bad), bad[:4])
    assert oob == 0, hex(oob)


@pytest.mark.parametrize("case", HOOK_CASES, ids=["%s-ipw%d-maxm%d-plan%d" % (uk.ALIASES[c[5][0]], c[5][1], c[5][2], c[5][4]) for c in HOOK_CASES])
def test_hooks_vs_oracle(oracle, case):
    """F_func, the pre-solve part of control (prepare: b) and Ax_func of a user model's handle, after the Newton start,
    one control() and the plant step, against the same statements of the oracle (user_oracle.cpp's "hooks" form)."""
    a, dv, km = case[:3]
    nx, nu, _ = DIMS[uk.ALIASES[a]]
    ref = user_oracle.run_hooks(oracle.exe(a), nx, nu, B16, dv, km, 1e-6)
    c, B = batch_of(case, 1e-6)
    c.set_ptau_repeat(scenario_of(case, B)[2])
    c.set_state(ref["t"], ref["U"][:B], ref["d"][:B])
    got = (c.F_func(ref["U"][:B], ref["x"][:B], ref["t"]), c.prepare(ref["x"][:B]), c.Ax_func(ref["v"][:B]))
    c.close()
    worst = [max(relmax(g[i], ref[k][i]) for i in range(B)) / bound
             for g, k, bound in zip(got, ("F", "b", "Ax"), (HOOK_F, HOOK_B, HOOK_AX))]
    print(f"user kernel class {uk.class_name(case[5])} case {uk.case_id(case)} hooks: F/bound {worst[0]:.3g} b/bound {worst[1]:.3g} Ax/bound {worst[2]:.3g}")
    assert all(w <= 1.0 for w in worst), (uk.case_id(case), worst)


def test_refusals_leave_the_plugin_usable(oracle):
    """An explicit variant 3 (the lean plan: a state equation that reads p is refused there) and an explicit variant 2 at
    sizes the planner refuses (uk.REFUSED_WG, asserted on the CPU in tests/test_user_kernel_ledger.py) raise
    CgmresHipError; after each, a valid handle of the same plugin still runs a tick inside the bounds."""
    a, dv, km = uk.REFUSED_WG
    mid = model_id(a)[0]
    case = next(c for c in uk.CASES if c[0] == a and uk.kind(c[5]) == "wg" and "A" in c[8])

    def one_tick():
        ref = oracle(a, case[1], case[2], 1e-6)
        c, B = batch_of(case, 1e-6)
        c.set_ptau_repeat(scenario_of(case, B)[2])
        c.set_state(float(ref["t"][0, 1]), ref["U"][:B, 1], ref["d"][:B, 1])
        u = c.control(ref["x"][:B, 1])
        c.close()
        assert max(relmax(u[i], ref["u"][i, 1]) for i in range(B)) <= U_TOL

    with pytest.raises(cg.CgmresHipError):
        cg.CgmresBatch(mid, batch=B16, dv=case[1], k_max=case[2], variant=3)
    one_tick()
    with pytest.raises(cg.CgmresHipError):
        cg.CgmresBatch(mid, batch=B16, dv=dv, k_max=km, variant=2)
    one_tick()
