"""GPU checks of the row-Newton kernel where the horizon ends inside a lane (csrc/wg_sweep_rows.hip.h, csrc/wg_gmres.hip.h):

  * stages beyond the horizon are identities by DATA — zero step sizes, and a base trajectory whose x1 repeats the
    terminal value, so that the residuals of the Newton sweep vanish there — where per-stage selects used to clear them;
  * all 16 lanes of a row store h(i,k), h(k+1,k) and the Arnoldi count;
  * hn and 1/hn of a new basis row come from one reciprocal square root.

Everything at B = 20: one full workgroup and one wave with four valid rows.  dv = 33 (seven lanes of a row own no stage)
and 48, 49, 50, 51: the terminal stage in each of the four slots of its lane.  k_max = 3 and 10; the planner gives the
row-Newton kernel for every one of these shapes, which is asserted.  Helpers: tests/test_gpu_iter_chain.py (the oracle's
free run is shared with that file through its cache).  Tolerances: 1e-7 free-running, 1e-9 teacher-forced, 1e-6 relative
on the exported Krylov arrays — those of test_gpu_iter_chain.py."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from gpu_helpers import U_TOL, _refs, _teacher_forced
from test_gpu_iter_chain import B, FREE_TOL, NAME, _free_run, _oracle

pytestmark = pytest.mark.gpu

DVS = [33, 48, 49, 50, 51]
KMS = [3, 10]


@pytest.mark.parametrize("flags,trig", [(0, "rotation"), (cg.FLAG_WAVE_FRESH_TRIG, "fresh-trig")])
@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("km", KMS)
@pytest.mark.parametrize("dv", DVS)
def test_free_running_ticks_vs_oracle_and_serial_sweep_kernel(orc, dv, km, tol, flags, trig):
    """12 free-running ticks in two launches: Arnoldi counts and exit reasons of the last tick equal the oracle's, x and u
    within 1e-7 of the oracle and of the serial-sweep kernel (FLAG_SERIAL_STATE_SWEEP)."""
    x0, u0, p, xo, uo, ko, ro = _oracle(orc, dv, km, tol)
    name, x, u, n_ax, reason = _free_run(dv, km, tol, flags, x0, u0, p)
    assert name == NAME, (dv, km, name)
    name_s, xs, us, n_s, reason_s = _free_run(dv, km, tol, cg.FLAG_SERIAL_STATE_SWEEP, x0, u0, p)
    assert name_s != NAME, (dv, km, name_s)
    e_o = max(float(np.max(np.abs(u - uo))), float(np.max(np.abs(x - xo))))
    e_s = max(float(np.max(np.abs(u - us))), float(np.max(np.abs(x - xs))))
    print(f"dv {dv} k_max {km} tol {tol} {trig}: vs oracle {e_o:.3e}, vs {name_s} {e_s:.3e}")
    assert np.array_equal(n_ax, ko[:, -1]) and np.array_equal(reason, ro[:, -1]), (dv, km, n_ax, ko[:, -1], reason)
    assert np.array_equal(n_ax, n_s) and np.array_equal(reason, reason_s), (dv, km, n_ax, n_s, reason, reason_s)
    assert e_o <= FREE_TOL and e_s <= FREE_TOL, (dv, km, tol, trig, e_o, e_s)


@pytest.mark.parametrize("km", KMS)
@pytest.mark.parametrize("dv", DVS)
def test_one_teacher_forced_tick(orc, dv, km):
    """One tick from the oracle's controller state with the horizon part open: u within 1e-9 (with the bound on dUdt
    that goes with it), counts and exit reasons equal."""
    x0, u0, p = orc.batch_scenario(0, B)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=1e-6, variant=2)
    assert c.variant_name == NAME
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    refs = _refs(orc, 0, dv, km, 1e-6, x0, u0, p)
    for r in refs:
        _, U_o, d_o = r.get_state()
        r.set_state(0.7, U_o, d_o)
    worst = _teacher_forced(orc, c, refs, x0, 1, u_tol=U_TOL)
    print(f"dv {dv} k_max {km}: |du| {worst:.3e}")
    c.close()


@pytest.mark.parametrize("tol", [1e-6, 0.0])
def test_exported_krylov_arrays_and_basis_rows(orc, tol):
    """dv = 50, k_max = 10, one tick: H, g, rho and the rows of V (get_krylov(with_V=True)) within 1e-6 relative of the
    oracle's, leading columns (the later ones are built on a converged residual), for both column schedules (tol > 0:
    every column rotated in its iteration; tol = 0: all columns behind the loop).  H holds what all 16 lanes of a row
    stored, V the rows normalised with the reciprocal square root."""
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
    V, H, rho, g = c.get_krylov(with_V=True)
    k1 = km + 1
    worst = dict(H=0.0, g=0.0, rho=0.0, V=0.0)
    rel = lambda got, ref: float(np.max(np.abs(np.abs(got) - np.abs(ref)))) / max(1.0, float(np.max(np.abs(ref))))
    for i, r in enumerate(refs):
        r.control(x0[i])
        k_o, _, _ = r.last_solve()
        assert n_ax[i] == k_o
        Vo, Ho, rhoo, go = r.krylov()
        Hd, gd = np.asarray(H[i]).reshape(k1, k1), np.asarray(g[i]).reshape(km, 3)
        cols = min(k_o, 4)
        for col in range(cols):
            worst["H"] = max(worst["H"], rel(Hd[col][: col + 1], Ho[col][: col + 1]))
            worst["g"] = max(worst["g"], rel(gd[col], go[col]))
        n = k_o + 1
        worst["rho"] = max(worst["rho"], rel(np.asarray(rho[i])[:n], np.asarray(rhoo)[:n]))
        nv = min(cols + 1, k1)
        Vd = np.asarray(V[i]).reshape(k1, -1)
        worst["V"] = max(worst["V"], rel(Vd[:nv], np.asarray(Vo)[:nv]))
        assert np.max(np.abs(Vd[:nv] @ Vd[:nv].T - np.eye(nv))) < 1e-8, i
    print(f"tol {tol}: relative differences " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert all(v <= 1e-6 for v in worst.values()), worst
    c.close()


def test_controls_of_1e17_on_this_kernel(orc):
    """test_gpu_row_newton.py's breakdown inputs, |U| = 1e17 at a resting plant, once on this kernel (dv = 50, k_max =
    10).  Controls of that size overflow the pendulum's costate recurrence, in the reference as well (see there), so
    the breakdown exit itself is out of reach here.  Held per instance: where the oracle's u is non-finite — the
    reference has no test for it and iterates on — the kernel reports EXIT_NONFINITE with a non-finite u; where it is
    finite, the kernel has the oracle's Arnoldi count, exit reason and u."""
    dv, km = 50, 10
    x0, _, p = orc.batch_scenario(0, B)
    big, rest = np.full((B, 3), 1e17), np.zeros_like(x0)
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=0.0, variant=2)
    assert c.variant_name == NAME
    c.set_ptau_repeat(p), c.init_u0(big)
    u = c.control(rest)
    n_ax, reason = c.get_status()
    c.close()
    overflowed = 0
    for i in range(B):
        r = orc.Controller(0, dv, km, 0.0)
        r.set_ptau_repeat(p[i])
        r.init_u0(big[i])
        ur = r.control(rest[i])
        k_o, _, reason_o = r.last_solve()
        if np.all(np.isfinite(ur)):
            assert n_ax[i] == k_o and reason[i] == reason_o, (i, n_ax[i], k_o, reason[i], reason_o)
            assert np.max(np.abs(u[i] - ur)) <= U_TOL * max(1.0, float(np.max(np.abs(ur)))), i
        else:
            overflowed += 1
            assert reason[i] == cg.EXIT_NONFINITE and not np.any(np.isfinite(u[i])), (i, n_ax[i], reason[i], u[i])
    print(f"|U| = 1e17: {overflowed} of {B} instances overflow in the oracle; counts {sorted(set(n_ax.tolist()))}")
