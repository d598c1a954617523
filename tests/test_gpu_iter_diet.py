"""GPU checks of what the row-Newton Arnoldi iteration no longer issues (csrc/tick_wg.hip.h, csrc/models.hip.h):

  * abs_t is fabs (a source modifier) instead of a compare and a select — used by the rotation guard and the convergence
    test of the Newton iteration and by the breakdown / tolerance tests of every solver;
  * a Gram-Schmidt round copies a parked basis row out of the accumulator file once, not twice;
  * the first stage of the two local folds of the Newton sweep (from a zero start) is written out.

None of them changes an arithmetic operation or its order, so what is held here is what held before, at the batch B = 20
throughout: one full workgroup and one with four valid rows, i.e. one wave whose other rows idle.

Parity: variant 2 against the serial-sweep kernel of the same library (FLAG_SERIAL_STATE_SWEEP) and against the oracle,
dv = 33, 50, 53 (the terminal stage first in its lane, in the middle of it, last with every lane owning stages), k_max = 3
and 10 (dv = 53, k_max = 10 is beyond the row-Newton kernel's LDS plan: variant 2 is the serial-sweep kernel there), 12
free-running ticks (two launches) at the 1e-7 of test_gpu_gs_ring.py, with and without FLAG_WAVE_FRESH_TRIG
(both sides of the guard's branch).  NaN: one instance of a wave starts from a NaN state.  Exits: ||r0|| < tol,
convergence in the first column and the |h(k+1,k)| < eps breakdown, after test_gpu_parity.py's test_status_exit_paths."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from gpu_helpers import _oracle_free_run

pytestmark = pytest.mark.gpu

NAME = "wg+row-newton"
B = 20
TICKS = 12  # one launch fuses at most 10 ticks: the 11th starts a second launch
FREE_TOL = 1e-7  # test_gpu_gs_ring.py / test_gpu_row_newton.py: free-running x and u against the oracle
U_TOL = 1e-9  # one tick from the same state

_oracle_runs = {}


def _oracle(orc, dv, km):
    """The free-running oracle of the seeded batch, once per shape (shared by the two trig forms; not modified)."""
    if (dv, km) not in _oracle_runs:
        x0, u0, p = orc.batch_scenario(0, B)
        _oracle_runs[(dv, km)] = (x0, u0, p) + _oracle_free_run(orc, dv, km, 0.0, x0, u0, p, TICKS)
    return _oracle_runs[(dv, km)]


def _free_run(dv, km, flags, x0, u0, p, x_start=None):
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=0.0, variant=2, flags=flags)
    name = c.variant_name
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    xd, ud = c.device_buffer((B, 4)).upload(x0 if x_start is None else x_start), c.device_buffer((B, 3))
    c.closed_loop_device(xd, ud, TICKS)
    c.synchronize()
    x, u = xd.download(), ud.download()
    n_ax, reason = c.get_status()
    c.close()
    return name, x, u, n_ax, reason


@pytest.mark.parametrize("flags,trig", [(0, "rotation"), (cg.FLAG_WAVE_FRESH_TRIG, "fresh-trig")])
@pytest.mark.parametrize("km", [3, 10])
@pytest.mark.parametrize("dv", [33, 50, 53])
def test_free_running_ticks_vs_serial_sweep_kernel_and_oracle(orc, dv, km, flags, trig):
    """12 device-resident ticks on the row-Newton kernel, on the serial-sweep kernel of the same library and on the
    oracle, from the same start: Arnoldi counts and exit reasons of the last tick equal, x and u within 1e-7 of the
    oracle and of each other.  (Asserted: 1e-7; the figures are printed.)"""
    x0, u0, p, xo, uo, ko, ro = _oracle(orc, dv, km)
    name, x, u, n_ax, reason = _free_run(dv, km, flags, x0, u0, p)
    # (dv = 53 with k_max = 10: the base trajectory of the Newton sweep does not fit LDS next to a basis of that length
    # and the planner, csrc/wg_plan.hip.h, answers variant 2 with the serial-sweep kernel itself; with k_max = 3 it fits)
    assert name == (NAME if (dv, km) != (53, 10) else "wg+parallel-costate"), (dv, km, name)
    name_s, xs, us, n_s, reason_s = _free_run(dv, km, cg.FLAG_SERIAL_STATE_SWEEP, x0, u0, p)
    assert name_s != NAME, (dv, km, name_s)
    e_o = max(float(np.max(np.abs(u - uo))), float(np.max(np.abs(x - xo))))
    e_s = max(float(np.max(np.abs(u - us))), float(np.max(np.abs(x - xs))))
    print(f"dv {dv} k_max {km} {trig}: vs oracle {e_o:.3e}, vs {name_s} {e_s:.3e}")
    assert np.array_equal(n_ax, ko[:, -1]) and np.array_equal(reason, ro[:, -1]), (dv, km, n_ax, ko[:, -1], reason)
    assert np.array_equal(n_ax, n_s) and np.array_equal(reason, reason_s), (dv, km, n_ax, n_s)
    assert e_o <= FREE_TOL and e_s <= FREE_TOL, (dv, km, trig, e_o, e_s)


@pytest.mark.parametrize("planted", [6, 17])
def test_nan_state_of_one_instance_leaves_its_wave_mates_alone(orc, planted):
    """One instance of a wave — of the full workgroup (6), of the wave whose other rows idle (17) — starts the closed loop
    from a NaN state; its controller was initialised from the clean one.  The reference tests for no NaN: every
    comparison is false, all k_max iterations run on NaNs (status 0) and u is NaN — checked below on the oracle.  The
    device stops the instance at the residual test with EXIT_NONFINITE and no Arnoldi step (tick_lane.hip.h:
    poison_nonfinite) and u = NaN.  Its lanes still go through every Newton iteration its wave runs, on NaNs: in the
    rotation guard fmax drops a NaN, in the convergence test a NaN violation is no violation, so its values must
    neither force nor suppress a branch for the three wave mates — those, and every other instance, stay within 1e-7
    of the oracle over the 12 ticks, counts and reasons equal."""
    dv, km = 50, 10
    x0, u0, p, xo, uo, ko, ro = _oracle(orc, dv, km)
    xn = x0.copy()
    xn[planted] = np.nan
    r = orc.Controller(0, dv, km, 0.0)
    orc.start_controller(r, x0[planted], u0[planted], p[planted])
    assert np.all(np.isnan(r.control(xn[planted])))  # the reference's fall-through
    name, x, u, n_ax, reason = _free_run(dv, km, 0, x0, u0, p, x_start=xn)
    assert name == NAME
    others = np.arange(B) != planted
    print(f"planted {planted}: status {reason[planted]} after {n_ax[planted]} iterations; others vs oracle "
          f"|du| {np.max(np.abs(u[others] - uo[others])):.3e} |dx| {np.max(np.abs(x[others] - xo[others])):.3e}")
    assert reason[planted] == cg.EXIT_NONFINITE and n_ax[planted] == 0, (reason[planted], n_ax[planted])
    assert np.all(np.isnan(u[planted])) and np.all(np.isnan(x[planted]))
    assert np.array_equal(n_ax[others], ko[others, -1]) and np.array_equal(reason[others], ro[others, -1])
    assert np.max(np.abs(u[others] - uo[others])) <= FREE_TOL and np.max(np.abs(x[others] - xo[others])) <= FREE_TOL


def test_breakdown_and_tolerance_exits(orc):
    """test_gpu_parity.py's test_status_exit_paths at B = 20 on variant 2 (semi-active damper, dv = 8, k_max = 3), instance by
    instance against the oracle — the tests that take an absolute value: ||r0|| < tol (gmres.hpp:39-41), convergence in
    the first column |rho_e[1]| < tol (:93-95) and the breakdown |h(k+1,k)| < DBL_EPSILON (:63-65)."""
    dv, km = 8, 3
    x0, u0, p = orc.batch_scenario(2, B)

    def both(tol, u_init=None, x0=x0):
        c = cg.CgmresBatch("semiactive", batch=B, dv=dv, k_max=km, tol=tol, variant=2)
        ui = u0 if u_init is None else u_init
        c.init_u0(ui)
        refs = []
        for i in range(B):
            r = orc.Controller(2, dv, km, tol)
            r.init_u0(ui[i])
            refs.append(r)
        if u_init is None:
            c.init_u0_newton(u0, x0, None, 10)
            for i, r in enumerate(refs):
                r.init_u0_newton(u0[i], x0[i], p[i], 10)
        _, U0, d0 = c.get_state()
        u = c.control(x0)
        n_ax, reason = c.get_status()
        _, U1, d1 = c.get_state()
        c.close()
        for i, r in enumerate(refs):
            ur = r.control(x0[i])
            k_o, _, reason_o = r.last_solve()
            assert n_ax[i] == k_o and reason[i] == reason_o, (tol, i, n_ax[i], k_o, reason[i], reason_o)
            if np.all(np.isfinite(ur)):
                assert np.max(np.abs(u[i] - ur)) <= U_TOL * max(1.0, float(np.max(np.abs(ur)))), (tol, i)
        return U0, d0, U1, d1, n_ax, reason, refs

    # (1) huge tol: every instance leaves at the residual test
    U0, d0, U1, d1, n_ax, reason, _ = both(1e30)
    assert np.all(reason == cg.EXIT_SMALL_RESIDUAL) and np.all(n_ax == 0)
    assert np.array_equal(d0, d1) and np.allclose(U1, U0 + d0 * 1e-3)

    # (2) tol between ||r0|| and |rho_e[1]|, from the oracle's own numbers
    r0n, e1 = [], []
    for i in range(B):
        r = orc.Controller(2, dv, 1, 0.0)
        orc.start_controller(r, x0[i], u0[i], p[i])
        b = r.prepare(x0[i])
        r0n.append(float(np.linalg.norm(b - r.Ax(r.get_state()[2]))))
        r.control(x0[i])
        e1.append(abs(float(r.krylov()[2][1])))
    r0n, e1 = np.array(r0n), np.array(e1)
    assert np.all(e1 < r0n)
    tol = float(np.sqrt(np.median(r0n) * np.median(e1)))
    U0, d0, U1, d1, n_ax, reason, refs = both(tol)
    hit = (reason == cg.EXIT_CONVERGED) & (n_ax == 1)
    assert hit.sum() >= B // 2, (hit.sum(), tol)
    for i in np.nonzero(hit)[0]:
        assert refs[i].last_solve()[1] == 0  # the oracle solved a 0 x 0 system
        assert np.array_equal(d0[i], d1[i])  # dUdt untouched
    assert np.allclose(U1[hit], U0[hit] + d0[hit] * 1e-3)

    # (3) breakdown: |U| = 1e17 absorbs h*v at a resting plant, A*v0 = 0 exactly (see test_status_exit_paths)
    big = np.full((B, 3), 1e17)
    U0, d0, U1, d1, n_ax, reason, _ = both(0.0, u_init=big, x0=np.zeros_like(x0))
    assert np.all(reason == cg.EXIT_BREAKDOWN) and np.all(n_ax == 1)
    assert np.array_equal(d0, d1) and np.array_equal(d1, np.zeros_like(d1))
    assert np.array_equal(U1, U0)
