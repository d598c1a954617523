"""GPU parity at tuning constants other than the shipped ones.  dt, h, zeta, Tf and alpha are run-time fields of
cgmres_hip_config, but every built-in model ships dt = 1e-3, h = 2e-3, zeta = 1000, alpha = 0.5 — so the rest of the
suite only ever runs 1 - zeta*h = -1, 1/h = 500 and dtau <= 0.02, and a kernel that hard-coded, sign-flipped or
mis-scaled one of them would pass it.  Here every mapping runs the three sets of tests/tuning_cases.py against the
oracle created with the same constants (orc_create_tuned; tests/test_oracle_vs_ref.py holds that oracle to the
reference compiled with them), from states the oracle reached by running 0, 40, 190 and 400 ticks from t = 0: early
exits at the start, all k_max iterations later, and — pendulum under `long` — horizon trajectories inside, across and
beyond the range of the rotation form of the trig update (tests/test_tuning_scenarios.py establishes all of that on
the CPU).

Tolerances are the project's (|du| <= 1e-9, |dUdt| <= 1e-7 relative, Arnoldi counts equal; the combined
bound on u of test_gpu_wave._teacher_forced), each times max(1, 2e-3 / h): the error is the 1/h amplification of
rounding in (F - Fh)/h, and the bounds were set at h = 2e-3.  That is 2 for `fast` and 1 for the other sets.  The
Arnoldi count of a (tick, instance) pair whose exit the oracle decided within 0.1 % of tol is not compared; at most
2 % of a test's pairs may be such."""
import ctypes as C

import numpy as np
import pytest

import cgmres_cpp_amd as cg
import tuning_cases as tc
from gpu_helpers import DUDT_REL, U_TOL, VARIANTS, new_batch

pytestmark = pytest.mark.gpu

FIELDS = ("dt", "h", "zeta", "Tf", "alpha")
CASES = [(m, name, dv, km) for dv, km in tc.SIZES for name in tc.SETS for m in tc.MODELS]
IDS = [f"{tc.MODEL_NAMES[m]}-{name}-dv{dv}k{km}" for m, name, dv, km in CASES]


def tuned_batch(model, name, dv, kmax, variant, dtype="f64"):
    """A handle of tc.BATCH controllers under tc.SETS[name]; the constants read back from get_config must be the set."""
    try:
        c = new_batch(model, batch=tc.BATCH, dv=dv, k_max=kmax, tol=tc.TOL, dtype=dtype, variant=variant, **tc.SETS[name])
    except cg.CgmresHipError as e:
        if variant == 3 and "wg-lean mapping" in str(e):
            pytest.skip("lean LDS plan does not cover these sizes")
        raise
    cfg = cg.Config()
    assert cg.load().cgmres_hip_get_config(c._h, cfg) == 0
    assert tuple(getattr(cfg, k) for k in FIELDS) == tuple(tc.SETS[name][k] for k in FIELDS)
    assert (c.dt, c.h, c.zeta, c.Tf, c.alpha) == tuple(tc.SETS[name][k] for k in FIELDS)
    assert c.variant == (2 if variant == "2s" else variant)
    return c


def within_cap(skipped, pairs):
    assert skipped <= tc.MARGINAL_CAP * pairs, (skipped, pairs)


def teacher_forced(c, refs, x, name, ticks=tc.TICKS_AFTER):
    """Every tick: controller state and x taken from the oracle; u, U', dUdt', the Arnoldi count and the exit reason
    compared per instance (test_gpu_wave._teacher_forced, with U' and the h scale of the bounds)."""
    k = tc.tol_scale(name)
    skipped = 0
    for tick in range(ticks):
        t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
        c.set_state(t_o[0], np.array(U_o), np.array(d_o))
        u = c.control(x)
        n_ax, reason = c.get_status()
        t1, U1, d1 = c.get_state()
        assert abs(t1 - (t_o[0] + tc.SETS[name]["dt"])) < 1e-12, (t1, t_o[0])
        for i, r in enumerate(refs):
            ur = r.control(x[i])
            _, U_ref, d_ref = r.get_state()
            d_bound = DUDT_REL * max(1.0, float(np.max(np.abs(d_ref))))
            # u = U' = U + dUdt*dt (cgmres.hpp:102-109): the bound on u that goes with the bound on dUdt
            bound = U_TOL * max(1.0, float(np.max(np.abs(ur)))) + r.dt * d_bound
            assert np.max(np.abs(u[i] - ur)) <= k * bound, (tick, i, u[i], ur)
            U_bound = U_TOL * max(1.0, float(np.max(np.abs(U_ref)))) + r.dt * d_bound
            assert np.max(np.abs(U1[i] - U_ref)) <= k * U_bound, (tick, i, float(np.max(np.abs(U1[i] - U_ref))))
            assert np.max(np.abs(d1[i] - d_ref)) <= k * d_bound, (tick, i, float(np.max(np.abs(d1[i] - d_ref))), d_bound)
            k_o, _, reason_o = r.last_solve()
            if tc.is_marginal(r):
                skipped += 1
            else:
                assert n_ax[i] == k_o and reason[i] == reason_o, (tick, i, n_ax[i], k_o, reason[i], reason_o)
            x[i] = x[i] + r.plant(x[i], ur) * r.dt
    within_cap(skipped, ticks * len(refs))


@pytest.mark.parametrize("W", tc.CHECKPOINTS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("model,name,dv,kmax", CASES, ids=IDS)
def test_teacher_forced_ticks_vs_tuned_oracle(orc, model, name, dv, kmax, variant, W):
    c = tuned_batch(model, name, dv, kmax, variant)
    if (dv, kmax, variant) == (50, 10, 2):  # which kernel is being held
        assert c.variant_name == ("wg+row-newton", "wg+two-pass-costate", "wg+row-scan")[model]
    run = tc.free_run(orc, model, name, dv, kmax)
    refs, x = run.restore(orc, model, dv, kmax, name, W)
    c.set_ptau_repeat(run.p)
    teacher_forced(c, refs, x, name)
    c.close()


@pytest.mark.parametrize("variant", [2, 1, 4])
@pytest.mark.parametrize("model,name,dv,kmax", CASES, ids=IDS)
def test_hooks_vs_tuned_oracle(orc, model, name, dv, kmax, variant):
    """F_func, the pre-solve part of control (b), Ax_func and gmres as separate records at W = 40: b = (F (1 - zeta h) -
    Fh) / h pins 1 - zeta*h and 1/h apart from the solve, F_func(t) pins dtau(t)."""
    W = 40
    c = tuned_batch(model, name, dv, kmax, variant)
    run = tc.free_run(orc, model, name, dv, kmax)
    refs, x = run.restore(orc, model, dv, kmax, name, W)
    c.set_ptau_repeat(run.p)
    s = run.snap[W]
    k = tc.tol_scale(name)
    c.set_state(s["t"], s["U"], s["dUdt"])
    rel = lambda ref: max(1.0, float(np.max(np.abs(ref))))
    F0 = c.F_func(s["U"], x, s["t"])
    b = c.prepare(x)
    v = np.random.default_rng(7).standard_normal((tc.BATCH, c.len))
    ax = c.Ax_func(v)
    b_o = np.array([r.prepare(x[i]) for i, r in enumerate(refs)])
    sol = c.gmres(s["dUdt"], b_o)
    n_ax, reason = c.get_status()
    skipped = 0
    for i, r in enumerate(refs):
        F_o = r.F(s["U"][i], x[i], s["t"])
        assert np.max(np.abs(F0[i] - F_o)) <= 1e-11 * rel(F_o), (i, float(np.max(np.abs(F0[i] - F_o))))
        assert np.max(np.abs(b[i] - b_o[i])) <= k * 1e-7 * rel(b_o[i]), (i, float(np.max(np.abs(b[i] - b_o[i]))))
        ax_o = r.Ax(v[i])
        assert np.max(np.abs(ax[i] - ax_o)) <= k * 1e-7 * rel(ax_o), (i, float(np.max(np.abs(ax[i] - ax_o))))
        sol_o = r.gmres(s["dUdt"][i], b_o[i])
        assert np.max(np.abs(sol[i] - sol_o)) <= k * DUDT_REL * rel(sol_o), (i, float(np.max(np.abs(sol[i] - sol_o))))
        if tc.is_marginal(r):
            skipped += 1
        else:
            assert n_ax[i] == r.last_solve()[0] and reason[i] == r.last_solve()[2], (i, n_ax[i], r.last_solve())
    within_cap(skipped, tc.BATCH)
    # the residual scale must have been worth pinning: F(t) != 0 and b is not -(F + Fh)/h of the shipped 1 - zeta*h = -1
    assert float(np.max(np.abs(b_o))) > 1e-3
    c.close()


def _start(c, run):
    c.set_ptau_repeat(run.p)
    c.init_u0(run.u0)
    c.init_u0_newton(run.u0, run.x0, run.p if c.dim_p else None, 10)


@pytest.mark.parametrize("n", tc.LOOP_TICKS)
@pytest.mark.parametrize("variant", [2, 3, 4, 1])
@pytest.mark.parametrize("name", ["fast", "long"])
@pytest.mark.parametrize("model", [0, 1])
def test_closed_loop_device_vs_tuned_oracle(orc, model, name, variant, n):
    """The fused device loop from the seeded start: `fast` has dt != shipped (plant step, U += dUdt*dt, t = n*dt),
    `long` the open horizon.  The assertions of test_gpu_closed_loop.test_closed_loop_device_vs_oracle."""
    dv, kmax = 50, 10
    run = tc.free_run(orc, model, name, dv, kmax)
    c = tuned_batch(model, name, dv, kmax, variant)
    _start(c, run)
    xd = c.device_buffer((tc.BATCH, c.dim_x)).upload(run.x0)
    ud = c.device_buffer((tc.BATCH, c.dim_u))
    c.closed_loop_device(xd, ud, n)
    c.synchronize()
    x, u = xd.download(), ud.download()
    t, U, d = c.get_state()
    n_ax, reason = c.get_status()
    xd.free(), ud.free(), c.close()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(U)) and np.all(np.isfinite(d))
    s = run.snap[n]
    k = tc.tol_scale(name)
    assert abs(t - s["t"]) <= 1e-12 and abs(t - n * tc.SETS[name]["dt"]) <= 1e-12, (t, s["t"])
    skipped = 0
    for i in range(tc.BATCH):
        assert np.max(np.abs(u[i] - s["u"][i])) <= k * 1e-9, (i, u[i], s["u"][i])
        assert np.max(np.abs(x[i] - s["x"][i])) <= k * 1e-9, (i, x[i], s["x"][i])
        assert np.max(np.abs(U[i] - s["U"][i])) <= k * 1e-9, i
        scale = max(1.0, float(np.max(np.abs(s["dUdt"][i]))))
        assert np.max(np.abs(d[i] - s["dUdt"][i])) <= k * 1e-7 * scale, (i, float(np.max(np.abs(d[i] - s["dUdt"][i]))))
        if run.marginal[n - 1, i]:
            skipped += 1
        else:
            assert n_ax[i] == s["n_ax"][i] and reason[i] == s["reason"][i], (i, n_ax[i], s["n_ax"][i])
    within_cap(skipped, tc.BATCH)


@pytest.mark.parametrize("variant", [2, 3, 4, 1])
def test_closed_loop_device_with_moving_reference_under_fast(orc, variant):
    """cgmres_hip_closed_loop_device_ptau for the pendulum under `fast`: a per-instance parameter horizon before every
    tick (test_gpu_closed_loop.test_closed_loop_device_with_moving_reference), 23 ticks = two launch boundaries + a
    tail; the target ramps along the horizon and from tick to tick."""
    model, name, dv, kmax, n, B = 0, "fast", 50, 10, 23, tc.BATCH
    x0, u0, p = orc.batch_scenario(model, B)
    c = tuned_batch(model, name, dv, kmax, variant)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    stage = np.arange(dv + 1)
    seq = np.empty((n, B, dv + 1, c.dim_p))
    for j in range(n):
        for i in range(B):
            seq[j, i, :, 0] = p[i, 0] * (1.0 + 0.004 * j) + 0.0007 * stage * (1 + 0.1 * (i % 5))
            seq[j, i, :, 1] = p[i, 1]
    seq = seq.reshape(n, B, c.dim_p * (dv + 1))
    sd = c.device_buffer(seq.shape).upload(seq)
    xd = c.device_buffer((B, c.dim_x)).upload(x0)
    ud = c.device_buffer((B, c.dim_u))
    c.closed_loop_device(xd, ud, n, sd, True)
    c.synchronize()
    x, u = xd.download(), ud.download()
    n_ax, _ = c.get_status()
    assert abs(c.t - n * tc.SETS[name]["dt"]) <= 1e-12
    u_next = c.control(x)  # the handle keeps the last tick's horizon
    k = tc.tol_scale(name)
    skipped = 0
    for i in range(B):
        r = orc.Controller(model, dv, kmax, tc.TOL, tuning=tc.SETS[name])
        orc.start_controller(r, x0[i], u0[i], p[i])
        xi = x0[i].copy()
        for j in range(n):
            r.set_ptau(seq[j, i])
            ui = r.control(xi)
            xi = xi + r.plant(xi, ui) * r.dt
        assert np.max(np.abs(u[i] - ui)) <= k * 1e-9 and np.max(np.abs(x[i] - xi)) <= k * 1e-9, (i, u[i], ui)
        if tc.is_marginal(r):
            skipped += 1
        else:
            assert n_ax[i] == r.last_solve()[0], (i, n_ax[i], r.last_solve())
        assert np.max(np.abs(u_next[i] - r.control(xi))) <= k * 1e-9, i
    within_cap(skipped, B)
    sd.free(), xd.free(), ud.free(), c.close()


# fp32 cases whose admissible rounding spread exceeds the 1e-4 of test_fp32_vs_fp32_reference (a bound set on the
# pendulum, |u| ~ 3; the two-mass system has |u| ~ 10 and a longer vector).  Measured on the CPU: the fp32 tuned oracle
# compiled with and without -ffp-contract=fast, both stepped from the same records (the checkpoint states of
# tc.free_run(..., "f32"), 3 teacher-forced ticks of the 20 instances), max |difference| of u and of U'.  Those two
# builds are the same statements in the same order and already differ by this much, so it is rounding, not a
# constant; the bound of such a case is 8 x the measured spread (the margin allows for the device's other association
# order).  Seen on the device before this table: 1.0e-4 .. 2.5e-4 on these cases, all mappings, lane included.
#   (model, set, dv, k_max, W): (spread of u, spread of U')     None: that quantity keeps 1e-4
FP32_SPREAD = {
    (1, "long", 50, 10, 0): (1.73e-4, 2.96e-4),
    (1, "long", 50, 10, 40): (7.96e-4, 7.96e-4),
    (1, "mid", 50, 10, 0): (1.15e-3, 2.57e-3),
    (1, "mid", 50, 10, 40): (None, 1.78e-4),
    (0, "long", 12, 4, 40): (2.00e-4, 2.00e-4),
    (1, "long", 12, 4, 0): (3.07e-5, 3.07e-5),
    (1, "mid", 12, 4, 0): (1.64e-4, 1.64e-4),
    (1, "mid", 12, 4, 40): (4.44e-4, 4.44e-4),
}


@pytest.mark.parametrize("W", [0, 40])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("model,name,dv,kmax", [c for c in CASES if c[1] != "fast"],
                         ids=[i for c, i in zip(CASES, IDS) if c[1] != "fast"])
def test_fp32_teacher_forced_vs_fp32_tuned_oracle(orc, model, name, dv, kmax, variant, W):
    """fp32 kernels against the fp32 oracle under `long` and `mid` (h >= 2e-3: fp32 forward differences carry eps/h
    relative noise), teacher-forced.  The bounds of test_gpu_parity.test_fp32_vs_fp32_reference: 1e-4 on u and U',
    5e-3 relative on dUdt', the count not compared; FP32_SPREAD lists the cases whose bound on u / U' is 8 x the
    measured rounding spread instead."""
    su, sU = FP32_SPREAD.get((model, name, dv, kmax, W), (None, None))
    c = tuned_batch(model, name, dv, kmax, variant, dtype="f32")
    run = tc.free_run(orc, model, name, dv, kmax, "f32")
    refs, x = run.restore(orc, model, dv, kmax, name, W, "f32")
    c.set_ptau_repeat(run.p)
    k = tc.tol_scale(name)
    for tick in range(tc.TICKS_AFTER):
        t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
        c.set_state(t_o[0], np.array(U_o), np.array(d_o))
        u = c.control(x).astype(np.float64)
        n_ax, _ = c.get_status()
        _, U1, d1 = c.get_state()
        for i, r in enumerate(refs):
            ur = r.control(x[i])
            _, U_ref, d_ref = r.get_state()
            print("fp32 figures", model, name, dv, kmax, variant, W, tick, i, float(np.max(np.abs(u[i] - ur))),
                  float(np.max(np.abs(U1[i].astype(np.float64) - U_ref))),
                  float(np.max(np.abs(d1[i].astype(np.float64) - d_ref))) / max(1.0, float(np.max(np.abs(d_ref)))))
            assert np.max(np.abs(u[i] - ur)) <= (8 * su if su else k * 1e-4), (tick, i, u[i], ur)
            assert np.max(np.abs(U1[i].astype(np.float64) - U_ref)) <= (8 * sU if sU else k * 1e-4), (tick, i)
            err = float(np.max(np.abs(d1[i].astype(np.float64) - d_ref)))
            assert err <= k * 5e-3 * max(1.0, float(np.max(np.abs(d_ref)))), (tick, i, err, float(np.max(np.abs(d_ref))))
            assert 1 <= int(n_ax[i]) <= kmax
            x[i] = (x[i].astype(np.float32) + r.plant(x[i], ur).astype(np.float32) * np.float32(r.dt)).astype(np.float32)
    c.close()


BAD = [(f, v) for f in FIELDS for v in (float("nan"), float("inf"), float("-inf"))] + \
      [("h", 0.0), ("h", -1e-3), ("dt", 0.0), ("dt", -5e-4)]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_create_rejects_unusable_tuning(field, value):
    """h <= 0, dt <= 0 and a NaN / Inf in any of the five constants: cgmres_hip_create returns CGMRES_HIP_EINVAL (-1)
    and no handle — for every mapping, before any device work."""
    L = cg.load()
    for variant in (0, 1, 2, 3, 4):
        cfg = cg.Config()
        assert L.cgmres_hip_default_config(0, cfg) == 0
        cfg.batch, cfg.dv, cfg.k_max, cfg.variant = 4, 12, 4, variant
        for k, v in tc.SETS["mid"].items():
            setattr(cfg, k, v)
        setattr(cfg, field, value)
        h = C.c_void_p()
        assert L.cgmres_hip_create(cfg, C.byref(h)) == -1, (field, value, variant)
        assert not h.value and L.cgmres_hip_last_error()
    with pytest.raises(cg.CgmresHipError, match="error -1"):
        cg.CgmresBatch("pendulum", batch=4, dv=12, k_max=4, **dict(tc.SETS["mid"], **{field: value}))
    # ... and the same constants without the bad one are accepted
    cg.CgmresBatch("pendulum", batch=4, dv=12, k_max=4, **tc.SETS["mid"]).close()
