"""CPU: what tests/test_gpu_tuning.py relies on about the scenarios of tests/tuning_cases.py, established with the
oracle alone (itself held to the reference under these constants by tests/test_oracle_vs_ref.py)."""
import numpy as np
import pytest

import tuning_cases as tc

CASES = [(m, name, dv, km) for dv, km in tc.SIZES for name in tc.SETS for m in tc.MODELS]
IDS = [f"{tc.MODEL_NAMES[m]}-{name}-dv{dv}k{km}" for m, name, dv, km in CASES]


def test_the_sets_leave_every_shipped_constant(orc):
    for model in tc.MODELS:
        s = orc.Controller(model, 8, 3)
        for name, tun in tc.SETS.items():
            c = orc.Controller(model, 8, 3, tuning=tun)
            assert (c.dt, c.h, c.zeta, c.Tf, c.alpha) == tuple(tun[k] for k in orc.TUNING_FIELDS)
            assert 1.0 - c.zeta * c.h != 1.0 - s.zeta * s.h and c.h != s.h and c.alpha != s.alpha
            assert c.Tf != s.Tf or name == "mid"   # (mid keeps the Tf = 1 of two of the models)
        assert tc.SETS["fast"]["dt"] != s.dt
    assert sorted(1.0 - t["zeta"] * t["h"] for t in tc.SETS.values()) == pytest.approx([-0.5, -0.2, 0.5], abs=1e-12)
    assert [tc.tol_scale(n) for n in ("fast", "long", "mid")] == [2.0, 1.0, 1.0]


@pytest.mark.parametrize("model,name,dv,kmax", CASES, ids=IDS)
def test_free_run_is_finite_and_its_exits_are_decided(orc, model, name, dv, kmax):
    r = tc.free_run(orc, model, name, dv, kmax)
    assert sorted(r.snap) == sorted(set(tc.CHECKPOINTS) | set(tc.LOOP_TICKS))
    for W, s in r.snap.items():
        for k in ("U", "dUdt", "x", "u"):
            assert np.all(np.isfinite(s[k])), (W, k)
        assert abs(s["t"] - W * tc.SETS[name]["dt"]) < 1e-12
    # only the two ordinary exits of gmres.hpp occur (no breakdown, no ||r0|| < tol)
    assert set(np.unique(r.reason)) <= {orc.EXIT_NATURAL, orc.EXIT_CONVERGED}
    # late ticks run all k_max iterations ...
    late = slice(tc.CHECKPOINTS[-1], tc.CHECKPOINTS[-1] + tc.TICKS_AFTER)
    assert np.all(r.reason[late] == orc.EXIT_NATURAL) and np.all(r.n_ax[late] == kmax)
    # ... and at k_max = 10 the first ones leave early, every instance of the first tick (k_max = 4 is too few
    # iterations to converge from the second tick on under any of the sets: those sizes check NATURAL exits only)
    if kmax == 10:
        early = slice(0, tc.TICKS_AFTER)
        assert np.all(r.reason[0] == orc.EXIT_CONVERGED)
        assert np.all(r.n_ax[0] <= kmax) and np.all(r.n_ax[0] >= 1)
        if model != 1:   # (the two-mass system converges on the first tick only)
            assert (r.reason[early] == orc.EXIT_CONVERGED).sum() > tc.BATCH
    # exits decided within 0.1 % of tol: the GPU tests may leave the Arnoldi count of such a pair uncompared
    assert r.marginal.mean() <= tc.MARGINAL_CAP, r.marginal.mean()


def test_pendulum_horizon_straddles_the_rotation_range_under_long(orc):
    """(50, 10): under `long` the per-stage angle increments pass the 0.04 rad of the rotation form between W = 40 and
    W = 400 — at W = 190 some instances of the first workgroup are beyond it and some are not, at W = 400 all are;
    under `fast` none ever is."""
    dv, kmax = 50, 10
    inc = {(name, W): tc.pendulum_stage_increments(orc, tc.free_run(orc, 0, name, dv, kmax).snap[W], name, dv, kmax)
           for name in ("long", "fast") for W in tc.CHECKPOINTS}
    assert np.all(inc["long", 40] < tc.ROT_RANGE)
    mixed = inc["long", 190]
    assert 4 <= (mixed[:16] > tc.ROT_RANGE).sum() <= 12 and 2 <= (mixed[16:] > tc.ROT_RANGE).sum() <= 3, mixed
    assert np.all(inc["long", 400] > 2 * tc.ROT_RANGE)
    for W in tc.CHECKPOINTS:
        assert np.all(inc["fast", W] < 0.6 * tc.ROT_RANGE), (W, inc["fast", W].max())


def test_marginal_exit_detector(orc):
    """is_marginal against a direct construction: with tol set to |rho_e| of a known column (times 1 +- 0.05 %) the exit
    is marginal, with tol moved by 1 % it is not."""
    c = orc.Controller(0, 50, 10, 0.0, tuning=tc.SETS["mid"])
    x0, u0, p = orc.batch_scenario(0, 1)
    orc.start_controller(c, x0[0], u0[0], p[0])
    c.control(x0[0])
    rho = np.abs(c.krylov()[2])         # tol = 0: all k_max columns run, rho[k_max] is the last estimate
    k_ax, _, why = c.last_solve()
    assert k_ax == 10 and why == orc.EXIT_NATURAL and rho[10] > 0
    for factor, want in ((1.0005, True), (0.9995, True), (1.01, False), (0.99, False)):
        tol = float(rho[10]) * factor   # just above the last estimate: CONVERGED in the last column; just below: NATURAL
        d = orc.Controller(0, 50, 10, tol, tuning=tc.SETS["mid"])
        orc.start_controller(d, x0[0], u0[0], p[0])
        d.control(x0[0])
        assert d.last_solve()[0] == 10
        assert tc.is_marginal(d, tol) == want, (factor, d.last_solve())
