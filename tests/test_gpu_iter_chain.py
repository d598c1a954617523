"""GPU checks of the row-Newton sweep's short, shared rotation (csrc/newton_rot.hip.h, csrc/wg_sweep_rows.hip.h):

  * the Newton iteration turns its trig pairs with the polynomials of |d| <= R = 2^CGM_NEWTON_ROT_LOG2_R — what the
    increments of a mat-vec stay within (profiles/r09_iter_chain_ab.json) — and anything larger takes the fresh
    sin / cos pair through the guard amax <= R;
  * from the second iteration on one pair (sin e, cos e - 1) turns (sd, cd) by -e and (s1, c1) by +e.

Everything at B = 20: one full workgroup and one wave with four valid rows.  dv = 33, 50, 53 (the terminal stage first in
its lane, in the middle, last with every lane owning stages) and k_max = 3, 10; dv = 53 with k_max = 10 is outside the
row-Newton kernel's LDS plan and runs the serial-sweep kernel by the planner's choice, which is asserted.  Checker: the
oracle on the same seeded inputs, and the serial-sweep kernel of the same library (FLAG_SERIAL_STATE_SWEEP).
Tolerances: 1e-7 free-running (test_gpu_gs_ring.py), 1e-9 teacher-forced, 1e-6 relative on the
exported Krylov arrays (test_gpu_row_newton.py: test_exported_krylov_arrays_vs_oracle)."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from gpu_helpers import U_TOL, _oracle_free_run, _refs, _teacher_forced

pytestmark = pytest.mark.gpu

NAME = "wg+row-newton"
B = 20
TICKS = 12  # one launch fuses at most 10 ticks: the 11th starts a second launch
FREE_TOL = 1e-7
SHAPES = [(33, 3), (33, 10), (50, 3), (50, 10), (53, 3), (53, 10)]

_oracle_runs = {}


def _expected_name(dv, km):
    return NAME if (dv, km) != (53, 10) else "wg+parallel-costate"


def _oracle(orc, dv, km, tol):
    """The free-running oracle of the seeded batch, once per shape and tolerance (shared by the trig forms; not modified)."""
    key = (dv, km, tol)
    if key not in _oracle_runs:
        x0, u0, p = orc.batch_scenario(0, B)
        _oracle_runs[key] = (x0, u0, p) + _oracle_free_run(orc, dv, km, tol, x0, u0, p, TICKS)
    return _oracle_runs[key]


def _free_run(dv, km, tol, flags, x0, u0, p, x_start=None):
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=tol, variant=2, flags=flags)
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
@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("dv,km", SHAPES)
def test_free_running_ticks_vs_oracle_and_serial_sweep_kernel(orc, dv, km, tol, flags, trig):
    """12 free-running ticks in two launches, with the rotation and with the fresh sin / cos pair (both sides of the
    guard): Arnoldi counts and exit reasons of the last tick equal the oracle's, x and u within 1e-7 of the oracle and
    of the serial-sweep kernel."""
    x0, u0, p, xo, uo, ko, ro = _oracle(orc, dv, km, tol)
    name, x, u, n_ax, reason = _free_run(dv, km, tol, flags, x0, u0, p)
    assert name == _expected_name(dv, km), (dv, km, name)
    name_s, xs, us, n_s, reason_s = _free_run(dv, km, tol, cg.FLAG_SERIAL_STATE_SWEEP, x0, u0, p)
    assert name_s != NAME, (dv, km, name_s)
    e_o = max(float(np.max(np.abs(u - uo))), float(np.max(np.abs(x - xo))))
    e_s = max(float(np.max(np.abs(u - us))), float(np.max(np.abs(x - xs))))
    print(f"dv {dv} k_max {km} tol {tol} {trig}: vs oracle {e_o:.3e}, vs {name_s} {e_s:.3e}")
    assert np.array_equal(n_ax, ko[:, -1]) and np.array_equal(reason, ro[:, -1]), (dv, km, n_ax, ko[:, -1], reason)
    assert e_o <= FREE_TOL and e_s <= FREE_TOL, (dv, km, tol, trig, e_o, e_s)


@pytest.mark.parametrize("dv,km", SHAPES)
def test_one_teacher_forced_tick(orc, dv, km):
    """One tick from the oracle's controller state with the horizon part open: u within 1e-9 (with the bound on dUdt
    that goes with it), counts and exit reasons equal."""
    x0, u0, p = orc.batch_scenario(0, B)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=1e-6, variant=2)
    assert c.variant_name == _expected_name(dv, km)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    refs = _refs(orc, 0, dv, km, 1e-6, x0, u0, p)
    for r in refs:
        _, U_o, d_o = r.get_state()
        r.set_state(0.7, U_o, d_o)
    worst = _teacher_forced(orc, c, refs, x0, 1, u_tol=U_TOL)
    print(f"dv {dv} k_max {km}: |du| {worst:.3e}")
    c.close()


@pytest.mark.parametrize("tol", [1e-6, 0.0])
def test_exported_krylov_arrays(orc, tol):
    """H, g and rho of get_krylov after one tick within 1e-6 relative of the oracle's, leading columns (the later ones
    are built on a converged residual), both column schedules."""
    dv, km = 50, 10
    x0, u0, p = orc.batch_scenario(0, B)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=tol, variant=2)
    assert c.variant_name == NAME
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    refs = _refs(orc, 0, dv, km, tol, x0, u0, p)
    for r in refs:
        _, U_o, d_o = r.get_state()
        r.set_state(0.4, U_o, d_o)
    t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
    c.set_state(t_o[0], np.array(U_o), np.array(d_o))
    c.control(x0)
    n_ax, _ = c.get_status()
    _, H, rho, g = c.get_krylov(with_V=True)
    k1 = km + 1
    worst_rho = 0.0
    for i, r in enumerate(refs):
        r.control(x0[i])
        k_o, _, _ = r.last_solve()
        assert n_ax[i] == k_o
        _, Ho, rhoo, go = r.krylov()
        Hd, gd = np.asarray(H[i]).reshape(k1, k1), np.asarray(g[i]).reshape(km, 3)
        cols = min(k_o, 4)
        for col in range(cols):
            ref_col = Ho[col][: col + 1]
            assert np.max(np.abs(np.abs(Hd[col][: col + 1]) - np.abs(ref_col))) <= 1e-6 * max(1.0, float(np.max(np.abs(ref_col)))), (i, col)
            assert np.max(np.abs(np.abs(gd[col]) - np.abs(go[col]))) <= 1e-6 * max(1.0, float(np.max(np.abs(go[col])))), (i, col)
        # rho: the solution y of the triangular system in its leading entries, the last residual estimate behind them
        n = k_o + 1
        ref_rho, got = np.asarray(rhoo)[:n], np.asarray(rho[i])[:n]
        e_rho = float(np.max(np.abs(np.abs(got) - np.abs(ref_rho))))
        worst_rho = max(worst_rho, e_rho)
        assert e_rho <= 1e-6 * max(1.0, float(np.max(np.abs(ref_rho)))), (i, e_rho)
    print(f"tol {tol}: |rho| differs by at most {worst_rho:.3e}")
    c.close()


def _one_tick_vs_oracle(orc, model, name, dv, km, tol, u_init, xx, pp, newton):
    c = cg.CgmresBatch(name, batch=B, dv=dv, k_max=km, tol=tol, variant=2)
    vname = c.variant_name
    if pp is not None and model == 0:
        c.set_ptau_repeat(pp)
    c.init_u0(u_init)
    if newton:
        c.init_u0_newton(u_init, xx, pp if model == 0 else None, 10)
    _, U0, d0 = c.get_state()
    u = c.control(xx)
    n_ax, reason = c.get_status()
    _, U1, d1 = c.get_state()
    c.close()
    for i in range(B):
        r = orc.Controller(model, dv, km, tol)
        if r.dim_p:
            r.set_ptau_repeat(pp[i])
        r.init_u0(u_init[i])
        if newton:
            r.init_u0_newton(u_init[i], xx[i], pp[i], 10)
        ur = r.control(xx[i])
        k_o, _, reason_o = r.last_solve()
        assert n_ax[i] == k_o and reason[i] == reason_o, (tol, i, n_ax[i], k_o, reason[i], reason_o)
        if np.all(np.isfinite(ur)):
            assert np.max(np.abs(u[i] - ur)) <= U_TOL * max(1.0, float(np.max(np.abs(ur)))), (tol, i)
    return vname, U0, d0, U1, d1, n_ax, reason


def test_small_residual_and_first_column_exits(orc):
    """On the row-Newton kernel: ||r0|| < tol (gmres.hpp:39-41) under a huge tolerance, and convergence in the first
    column (:93-95) under a tolerance between ||r0|| and |rho_e[1]| taken from the oracle's own numbers."""
    dv, km = 50, 10
    x0, u0, p = orc.batch_scenario(0, B)
    name, U0, d0, U1, d1, n_ax, reason = _one_tick_vs_oracle(orc, 0, "pendulum", dv, km, 1e30, u0, x0, p, True)
    assert name == NAME
    assert np.all(reason == cg.EXIT_SMALL_RESIDUAL) and np.all(n_ax == 0)
    assert np.array_equal(d0, d1)
    r0n, e1 = [], []
    for i in range(B):
        r = orc.Controller(0, dv, 1, 0.0)
        orc.start_controller(r, x0[i], u0[i], p[i])
        b = r.prepare(x0[i])
        r0n.append(float(np.linalg.norm(b - r.Ax(r.get_state()[2]))))
        r.control(x0[i])
        e1.append(abs(float(r.krylov()[2][1])))
    r0n, e1 = np.array(r0n), np.array(e1)
    tol = float(np.sqrt(np.median(r0n) * np.median(e1)))
    name, U0, d0, U1, d1, n_ax, reason = _one_tick_vs_oracle(orc, 0, "pendulum", dv, km, tol, u0, x0, p, True)
    assert name == NAME
    hit = (reason == cg.EXIT_CONVERGED) & (n_ax == 1)
    print(f"tol {tol:.3e}: {hit.sum()} of {B} instances converge in the first column")
    assert hit.sum() >= 1, (tol, n_ax, reason)
    for i in np.nonzero(hit)[0]:
        assert np.array_equal(d0[i], d1[i])  # a 0 x 0 system: dUdt untouched


def test_breakdown_exit(orc):
    """|h(k+1,k)| < DBL_EPSILON (gmres.hpp:63-65) after test_gpu_parity.py's test_status_exit_paths: |U| = 1e17 absorbs
    h*v at a resting plant, A*v0 = 0 exactly (semi-active damper, dv = 8, k_max = 3: the pendulum's costate recurrence
    overflows under controls of that size, in the reference as well — test_gpu_row_newton.py)."""
    x0, _, p = orc.batch_scenario(2, B)
    big = np.full((B, 3), 1e17)
    _, U0, d0, U1, d1, n_ax, reason = _one_tick_vs_oracle(orc, 2, "semiactive", 8, 3, 0.0, big, np.zeros_like(x0), p, False)
    assert np.all(reason == cg.EXIT_BREAKDOWN) and np.all(n_ax == 1)
    assert np.array_equal(d0, d1) and np.array_equal(d1, np.zeros_like(d1)) and np.array_equal(U1, U0)


@pytest.mark.parametrize("planted", [6, 17])
def test_nan_instance_leaves_its_wave_mates_alone(orc, planted):
    """One instance of a wave — of the full workgroup (6), of the wave with four valid rows (17) — starts from a NaN
    state: EXIT_NONFINITE with no Arnoldi step and u = NaN for it; every other instance, its three wave mates included,
    within 1e-7 of the oracle with equal counts and reasons.  Its lanes go through every Newton iteration of their wave
    on NaNs: in the guard fmax drops a NaN, so they neither force the fresh pair on the mates nor keep it from them."""
    dv, km = 50, 10
    x0, u0, p, xo, uo, ko, ro = _oracle(orc, dv, km, 0.0)
    xn = x0.copy()
    xn[planted] = np.nan
    name, x, u, n_ax, reason = _free_run(dv, km, 0.0, 0, x0, u0, p, x_start=xn)
    assert name == NAME
    others = np.arange(B) != planted
    assert reason[planted] == cg.EXIT_NONFINITE and n_ax[planted] == 0, (reason[planted], n_ax[planted])
    assert np.all(np.isnan(u[planted])) and np.all(np.isnan(x[planted]))
    assert np.array_equal(n_ax[others], ko[others, -1]) and np.array_equal(reason[others], ro[others, -1])
    assert np.max(np.abs(u[others] - uo[others])) <= FREE_TOL and np.max(np.abs(x[others] - xo[others])) <= FREE_TOL


def test_scaled_dudt_through_set_state(orc):
    """dUdt scaled by 1e3 through set_state, one teacher-forced tick at the tolerances above.  (The Arnoldi directions
    are normalised, so this scales the preamble's A*dUdt — serial sweeps — and the right-hand side, not the increments
    of the Newton sweep; the next test is the one that passes the guard.)"""
    dv, km = 50, 10
    x0, u0, p = orc.batch_scenario(0, B)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=1e-6, variant=2)
    assert c.variant_name == NAME
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    refs = _refs(orc, 0, dv, km, 1e-6, x0, u0, p)
    for i, r in enumerate(refs):
        r.control(x0[i])  # one tick gives a non-zero dUdt
        _, U_o, d_o = r.get_state()
        r.set_state(0.7, U_o, np.asarray(d_o) * 1e3)
    _teacher_forced(orc, c, refs, x0, 1, u_tol=U_TOL)
    c.close()


# h large enough for U + h v, |v| = 1, to move the trajectory by more than R = 2^-13 per stage (the shipped h = 2e-3
# gives increments up to 9e-6, and they are linear in h): with zeta = 1 / h, the other constants the shipped ones
BIG_H = dict(dt=1e-3, h=0.5, zeta=2.0, Tf=1.0, alpha=0.5)


def test_increments_beyond_the_range_take_the_fresh_pair_without_the_flag(orc):
    """Under h = 0.5 the increments of the Newton sweep exceed R, so waves take the fresh sin / cos pair through the
    guard itself, no debug flag set: two teacher-forced ticks with the horizon open against the oracle created with the
    same constants, at the tolerances above."""
    dv, km = 50, 10
    x0, u0, p = orc.batch_scenario(0, B)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=1e-6, variant=2, **BIG_H)
    assert c.variant_name == NAME
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    refs = []
    for i in range(B):
        r = orc.Controller(0, dv, km, 1e-6, tuning=BIG_H)
        orc.start_controller(r, x0[i], u0[i], p[i])
        _, U_o, d_o = r.get_state()
        r.set_state(0.7, U_o, d_o)
        refs.append(r)
    worst = _teacher_forced(orc, c, refs, x0, 2, u_tol=U_TOL)
    print(f"h = {BIG_H['h']}: |du| {worst:.3e}")
    c.close()
