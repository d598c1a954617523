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
    the oracle's free run.  fp64: the helper and bounds of test_gpu_gs_ring.py (x and u within 1e-7, the last tick's
    counts and reasons equal); fp32: the bounds of test_gpu_closed_loop.test_closed_loop_device_vs_oracle.

An fp64 case that exceeds a bound is run again on variant 1, the lane mapping, which keeps the reference's statement
order: where that fails as well the shape is ill-conditioned and tools/kernel_case_admission.py let it through (mend its
rule, replace the case); where the lane mapping passes, the kernel is wrong.  The failure message says which.

Each check prints its worst |du| and |ddUdt| as a fraction of the bound before it asserts."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
import kernel_classes as kc
from test_gpu_closed_loop import OracleLoop
from test_gpu_gs_ring import _oracle_free_run

pytestmark = pytest.mark.gpu

B16, B8 = 20, 11
TICKS, LOOP_TICKS = 4, 12
U_TOL, DUDT_REL = 1e-9, 1e-7
F32_U, F32_D = 1e-4, 5e-3
IDS = [kc.case_id(c) for c in kc.CASES]

_forced, _loops = {}, {}


def tols(case):
    return (1e-6, 0.0) if case[8] else (1e-6,)


def forced_reference(orc, model, dtype, dv, km, tol):
    """The oracle's own closed loop of the B16 seeded instances, recorded tick by tick: what goes in (t, U, dUdt, x) and
    what comes out (u, U', dUdt', count, reason).  Computed once per shape and tolerance, never modified."""
    key = (model, dtype, dv, km, tol)
    if key not in _forced:
        f32 = dtype == 1
        x0, u0, p = orc.batch_scenario(model, B16)
        refs = []
        for i in range(B16):
            r = orc.Controller(model, dv, km, tol, kc.DTYPE_NAMES[dtype])
            orc.start_controller(r, x0[i], u0[i], p[i])
            refs.append(r)
        x = x0.astype(np.float32).astype(np.float64) if f32 else x0.copy()
        ticks = []
        for _ in range(TICKS):
            t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
            rec = dict(t=t_o[0], U=np.array(U_o), d=np.array(d_o), x=x.copy())
            u = np.array([r.control(x[i]) for i, r in enumerate(refs)])
            _, U1, d1 = zip(*[r.get_state() for r in refs])
            solve = np.array([r.last_solve() for r in refs])
            rec.update(u=u, U1=np.array(U1), d1=np.array(d1), n_ax=solve[:, 0], reason=solve[:, 2])
            for i, r in enumerate(refs):
                if f32:
                    x[i] = (x[i].astype(np.float32) + r.plant(x[i], u[i]).astype(np.float32) * np.float32(r.dt)).astype(np.float32)
                else:
                    x[i] = x[i] + r.plant(x[i], u[i]) * r.dt
            ticks.append(rec)
        _forced[key] = (p, ticks)
    return _forced[key]


def loop_reference(orc, model, dtype, dv, km, tol):
    key = (model, dtype, dv, km, tol)
    if key not in _loops:
        x0, u0, p = orc.batch_scenario(model, B16)
        if dtype == 0:
            _loops[key] = (x0, u0, p, _oracle_free_run(orc, dv, km, tol, x0, u0, p, LOOP_TICKS, model=model))
        else:
            _loops[key] = (x0, u0, p, OracleLoop(orc, model, dv, km, tol, "f32", x0, u0, p, list(range(B16)), {LOOP_TICKS}).snap[LOOP_TICKS])
    return _loops[key]


def batch_of(case, tol, variant=None):
    m, d, dv, km, v, f, cls, name = case[:8]
    B = B16 if cls[2] == 16 else B8
    if variant is not None:
        return cg.CgmresBatch(m, batch=B, dv=dv, k_max=km, tol=tol, dtype=kc.DTYPE_NAMES[d], variant=variant), B
    c = cg.CgmresBatch(m, batch=B, dv=dv, k_max=km, tol=tol, dtype=kc.DTYPE_NAMES[d], variant=v, flags=f)
    assert c.variant_name == name, (kc.case_id(case), c.variant_name, name)
    return c, B


def relmax(a, ref):
    return float(np.max(np.abs(a - ref))) / max(1.0, float(np.max(np.abs(ref))))


def forced_problems(orc, case, tol, variant=None):
    """(problems, worst |du| / bound, worst |ddUdt'| / bound) of the teacher-forced ticks"""
    m, d, dv, km = case[:4]
    f32 = d == 1
    p, ticks = forced_reference(orc, m, d, dv, km, tol)
    c, B = batch_of(case, tol, variant)
    c.set_ptau_repeat(p[:B])
    spread = (case[9] or (None, None))[0 if tol else 1] or (None, None, None)
    bad, wu, wd = [], 0.0, 0.0
    for n, rec in enumerate(ticks):
        c.set_state(rec["t"], rec["U"][:B], rec["d"][:B])
        u = c.control(rec["x"][:B]).astype(np.float64)
        n_ax, reason = c.get_status()
        _, U1, d1 = c.get_state()
        U1, d1 = U1.astype(np.float64), d1.astype(np.float64)
        for i in range(B):
            if f32:
                eu, eU = float(np.max(np.abs(u[i] - rec["u"][i]))), float(np.max(np.abs(U1[i] - rec["U1"][i])))
                ru, rU = eu / (8 * spread[0] if spread[0] else F32_U), eU / (8 * spread[1] if spread[1] else F32_U)
                rd = relmax(d1[i], rec["d1"][i]) / (8 * spread[2] if spread[2] else F32_D)
                ru = max(ru, rU)
                if not 1 <= n_ax[i] <= km:
                    bad.append(("count", n, i, int(n_ax[i])))
            else:
                ru = relmax(u[i], rec["u"][i]) / U_TOL
                rd = relmax(d1[i], rec["d1"][i]) / DUDT_REL
                if n_ax[i] != rec["n_ax"][i] or reason[i] != rec["reason"][i]:
                    bad.append(("count / reason", n, i, int(n_ax[i]), int(rec["n_ax"][i]), int(reason[i]), int(rec["reason"][i])))
                if tol == 0.0 and n_ax[i] != km:
                    bad.append(("fixed-k count", n, i, int(n_ax[i])))
            if not ru <= 1.0:
                bad.append(("u or U' / bound", n, i, ru))
            if not rd <= 1.0:
                bad.append(("dUdt' / bound", n, i, rd))
            wu, wd = max(wu, ru), max(wd, rd)
    c.close()
    return bad, wu, wd


def loop_problems(orc, case, tol, variant=None):
    m, d, dv, km = case[:4]
    f32 = d == 1
    x0, u0, p, ref = loop_reference(orc, m, d, dv, km, tol)
    c, B = batch_of(case, tol, variant)
    npdt = np.float32 if f32 else np.float64
    c.set_ptau_repeat(p[:B]), c.init_u0(u0[:B]), c.init_u0_newton(u0[:B], x0[:B], p[:B] if c.dim_p else None, 10)
    xd = c.device_buffer((B, c.dim_x)).upload(x0[:B].astype(npdt))
    ud = c.device_buffer((B, c.dim_u))
    c.closed_loop_device(xd, ud, LOOP_TICKS)
    c.synchronize()
    x, u = xd.download().astype(np.float64), ud.download().astype(np.float64)
    t, U, dU = c.get_state()
    n_ax, reason = c.get_status()
    xd.free(), ud.free(), c.close()
    bad = []
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(U)) and np.all(np.isfinite(dU))):
        bad.append(("not finite",))
    if tol == 0.0 and not f32 and not (np.all(n_ax == km) and np.all(reason == cg.EXIT_NATURAL)):
        bad.append(("fixed-k count", n_ax.tolist(), reason.tolist()))
    if f32:
        flips, wu, wd = 0, 0.0, 0.0
        for i in range(B):
            t_o, U_o, d_o = ref["state"][i]
            if abs(t - t_o) > 1e-6:
                bad.append(("t", t, t_o))
            ru = max(float(np.max(np.abs(u[i] - ref["u"][i]))), float(np.max(np.abs(x[i] - ref["x"][i]))),
                     float(np.max(np.abs(U[i].astype(np.float64) - U_o)))) / 1e-4
            rd = relmax(dU[i].astype(np.float64), d_o) / 2e-3
            if not ru <= 1.0:
                bad.append(("loop u, x or U / 1e-4", i, ru))
            if not rd <= 1.0:
                bad.append(("loop dUdt / 2e-3", i, rd))
            flips += int(n_ax[i] != ref["solve"][i][0])
            wu, wd = max(wu, ru), max(wd, rd)
        if flips > B // 2:
            bad.append(("count flips", flips))
        return bad, wu, wd
    xo, uo, ko, ro = ref
    wu = max(float(np.max(np.abs(u - uo[:B]))), float(np.max(np.abs(x - xo[:B])))) / 1e-7
    if not wu <= 1.0:
        bad.append(("loop u or x / 1e-7", wu))
    if not (np.array_equal(n_ax, ko[:B, -1]) and np.array_equal(reason, ro[:B, -1])):
        bad.append(("loop count / reason", n_ax.tolist(), ko[:B, -1].tolist(), reason.tolist(), ro[:B, -1].tolist()))
    return bad, wu, 0.0


def verdict(orc, case, tol, problems_of, bad):
    """for the failure message of an fp64 case: what the lane mapping makes of the same shape"""
    if case[1] == 1:
        return "fp32"
    lane_bad = problems_of(orc, case, tol, variant=1)[0]
    if lane_bad:
        return "the lane mapping fails too (%r ...): the shape is ill-conditioned, mend the admission rule and replace the case" % (lane_bad[:2],)
    return "the lane mapping passes: a finding about this kernel"


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_teacher_forced_ticks_vs_oracle(orc, case):
    for tol in tols(case):
        bad, wu, wd = forced_problems(orc, case, tol)
        print(f"kernel class {kc.class_name(case[6])} case {kc.case_id(case)} tol {tol:g} forced: |du|/bound {wu:.3g} |ddUdt|/bound {wd:.3g}")
        assert not bad, (kc.case_id(case), tol, len(bad), bad[:4], verdict(orc, case, tol, forced_problems, bad))


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_device_loop_across_a_launch_boundary_vs_oracle(orc, case):
    assert LOOP_TICKS > cg.TICKS_PER_LAUNCH
    for tol in tols(case):
        bad, wu, wd = loop_problems(orc, case, tol)
        print(f"kernel class {kc.class_name(case[6])} case {kc.case_id(case)} tol {tol:g} loop: |du|,|dx|/bound {wu:.3g} |ddUdt|/bound {wd:.3g}")
        assert not bad, (kc.case_id(case), tol, len(bad), bad[:4], verdict(orc, case, tol, loop_problems, bad))
