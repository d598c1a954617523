"""GPU parity of the row-Newton kernel's Gram-Schmidt ring (csrc/wg_gmres.hip.h, gmres(): the first NKEEP = 2 basis rows
stay in registers, the older ones pass through a ring of NBUF = 3 row buffers — one loop of NBUF rounds per trip with a
clamped, unconditional refill after every round, a peeled tail of fewer than NBUF rounds, and the same loop in the
x += V y update) at every basis length at which the loop takes another path:

    k_max   1, 2   no ring row (k <= NKEEP)
            3, 5   ring rows, none refilled (k <= NKEEP + NBUF): tail only (k = 3, 4), first full trip (k = 5)
            6      first refill that is consumed; tail of 1
            7      tail of 2
            12     the longest basis the ring serves (KRING): three full trips, tails of 0, 1 and 2 on the way

Pendulum, fp64, dv = 33 (the shortest horizon of this kernel) and 50 (the headline), B = 16 (one full workgroup) and
40 (a last workgroup with 8 of 16 rows valid), fixed-k (tol = 0: Hessenberg QR after the loop) and tol = 1e-6 (rows of
one wave leave the loop at different iterations).  Checker: the oracle (oracle/liboracle.so), same seeded inputs;
tolerances are those of test_gpu_row_newton.py (SURVEY.md §8(c) teacher-forced, 1e-7 free-running)."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from gpu_helpers import U_TOL, _oracle_free_run, _refs

pytestmark = pytest.mark.gpu

NAME = "wg+row-newton"
KMAX = [1, 2, 3, 5, 6, 7, 12]
TICKS = 12  # one launch fuses at most 10 ticks: the 11th starts a second launch


def _batch(B, dv, km, tol):
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=tol, variant=2)
    assert c.variant_name == NAME, (dv, km, B, tol, c.variant_name)
    return c


@pytest.mark.parametrize("km", KMAX)
@pytest.mark.parametrize("dv", [33, 50])
def test_free_running_ticks_across_the_launch_boundary_vs_oracle(orc, dv, km):
    """12 device-resident ticks from the scenario's own start against the free-running oracle: x and u within 1e-7, the
    last tick's Arnoldi counts and exit reasons equal.  With tol = 1e-6 and k_max >= 7 the start is one at which the
    oracle's counts differ between the four instances of a wave (checked below on the oracle's own numbers): a row that
    has converged sits out the ring rounds its wave mates still run.  dv = 50, k_max = 6 (tail of one round) has such
    waves at its third tick, which the device runs on the way.  Shorter bases cannot show that from any start of this
    scenario: from the fourth tick on the oracle needs six or more iterations everywhere, i.e. all k_max of them.
    (Asserted: 1e-7, the bound of test_gpu_row_newton.py's free-running test; the figures are printed.)"""
    for B in (16, 40):
        x0, u0, p = orc.batch_scenario(0, B)
        for tol in (0.0, 1e-6):
            xo, uo, ko, ro = _oracle_free_run(orc, dv, km, tol, x0, u0, p, TICKS)
            if tol > 0 and (km >= 7 or (dv, km) == (50, 6)):
                waves = ko.reshape(B // 4, 4, TICKS)  # a wave holds four consecutive instances
                mixed = waves.max(axis=1) != waves.min(axis=1)  # [wave, tick]
                if km >= 7:  # on the compared last tick as well
                    assert mixed[:, -1].sum() >= 2, (dv, km, B, ko[:, -1])
                else:
                    assert mixed.any(axis=1).sum() >= 1, (dv, km, B)
            c = _batch(B, dv, km, tol)
            c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
            xd, ud = c.device_buffer((B, 4)).upload(x0), c.device_buffer((B, 3))
            c.closed_loop_device(xd, ud, TICKS)
            c.synchronize()
            x, u = xd.download(), ud.download()
            n_ax, reason = c.get_status()
            c.close()
            print(f"dv {dv} k_max {km} B {B} tol {tol}: |du| {np.max(np.abs(u - uo)):.3e} |dx| {np.max(np.abs(x - xo)):.3e}")
            assert np.array_equal(n_ax, ko[:, -1]) and np.array_equal(reason, ro[:, -1]), (dv, km, B, tol, n_ax, ko[:, -1])
            assert np.max(np.abs(u - uo)) <= 1e-7 and np.max(np.abs(x - xo)) <= 1e-7, (dv, km, B, tol)


@pytest.mark.parametrize("tol", [1e-6, 0.0])
@pytest.mark.parametrize("km", KMAX)
def test_exported_krylov_arrays_vs_oracle(orc, km, tol):
    """get_krylov after one tick, both horizons, against the oracle's private members at the tolerances of
    test_gpu_row_newton.py (1e-6 on the basis, the Hessenberg columns and the reflectors, signs aside; 1e-8 on
    orthonormality).  k_max <= 7: ALL columns of H and g the solve produced, ALL k_max + 1 basis rows, and orthonormality
    over ALL produced rows — every ring round, refill and tail round of the loop leaves its h(i,k) and its row here.
    The oracle of the same k_max no longer holds row k_max (it is the accumulator of x += V y, cgmres_oracle.hpp:207-211 /
    matrix.hpp:82-91): that row comes from a second oracle with one more column from the same start, whose first k_max
    iterations are the same arithmetic.  Bounds from the reference's own error: its basis from this start is orthonormal
    to 4.4e-13 over up to 4 rows, 4.9e-9 over 5 to 7 rows — and only to 1.2e-5 (dv = 33) / 2.0e-5 (dv = 50) over 8 rows,
    the modified Gram-Schmidt defect eps * kappa of a sequence whose eighth vector is built on a nearly converged
    residual.  Two roundings of such a sequence differ by as much, so the orthonormality bound, and the bound on the
    difference of row k_max, is the tolerance of test_gpu_row_newton.py (1e-8, 1e-6) or twice the batch's worst defect
    of the ORACLE over the same rows, whichever is larger: 1e-8 and 1e-6 up to k_max = 6, ~2.4e-5 / 4e-5 at k_max = 7.
    k_max = 12: from this start the oracle's own basis is orthogonal only to 1.4e-2 ... 7.0e-2 (modified Gram-Schmidt on a
    residual that has converged by the eighth vector), so the late rows are rounding on either side: the leading four
    columns and five rows as in test_gpu_row_newton.py, and unit length for every produced row."""
    B = 16
    x0, u0, p = orc.batch_scenario(0, B)
    k1 = km + 1
    worst = dict(H=0.0, g=0.0, V=0.0, ortho=0.0)
    for dv in (33, 50):
        c = _batch(B, dv, km, tol)
        c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
        refs = _refs(orc, 0, dv, km, tol, x0, u0, p)
        for r in refs:
            _, U_o, d_o = r.get_state()
            r.set_state(0.4, U_o, d_o)
        t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
        c.set_state(t_o[0], np.array(U_o), np.array(d_o))
        c.control(x0)
        n_ax, reason = c.get_status()
        V, H, rho, g = c.get_krylov(with_V=True)
        c.close()
        checks = []
        wide, o_defect = [], 0.0  # k_max <= 7: the oracle with one more column (holds row k_max) and its own defect
        if km <= 7:
            for i in range(B):
                r = orc.Controller(0, dv, km + 1, 0.0)
                orc.start_controller(r, x0[i], u0[i], p[i])
                r.set_state(t_o[i], U_o[i], d_o[i])
                r.control(x0[i])
                Vw = np.asarray(r.krylov()[0])[:k1]
                wide.append(Vw)
                o_defect = max(o_defect, float(np.max(np.abs(Vw @ Vw.T - np.eye(k1)))))
        on_tol, last_tol = max(1e-8, 2 * o_defect), max(1e-6, 2 * o_defect)
        for i, r in enumerate(refs):
            r.control(x0[i])
            k_o, ks_o, reason_o = r.last_solve()
            assert n_ax[i] == k_o and reason[i] == reason_o, (dv, i, n_ax[i], k_o)
            assert reason_o in (0, 1)
            if km <= 7:
                assert k_o == km  # (checked on the oracle: no instance converges before k_max from this start)
            Vo, Ho, rhoo, go = r.krylov()
            Hd = np.asarray(H[i]).reshape(k1, k1)
            gd = np.asarray(g[i]).reshape(km, 3)
            Vd = np.asarray(V[i]).reshape(k1, -1)
            rows = k_o + 1  # iteration k normalises and stores row k + 1 before its convergence test (gmres.hpp:67, 93)
            cols = k_o if km <= 7 else min(k_o, 4)
            n_vs = min(cols + 1, km)  # rows compared with the oracle
            n_on = rows if km <= 7 else cols + 1  # rows held to mutual orthogonality
            for col in range(cols):
                ref_col = Ho[col][: col + 1]
                scale = max(1.0, float(np.max(np.abs(ref_col))))
                eH = float(np.max(np.abs(np.abs(Hd[col][: col + 1]) - np.abs(ref_col)))) / scale
                eg = float(np.max(np.abs(np.abs(gd[col]) - np.abs(go[col])))) / max(1.0, float(np.max(np.abs(go[col]))))
                worst["H"], worst["g"] = max(worst["H"], eH), max(worst["g"], eg)
                checks.append((eH <= 1e-6 and eg <= 1e-6, ("H/g", dv, i, col, eH, eg)))
            eV = float(np.max(np.abs(np.abs(Vd[:n_vs]) - np.abs(np.asarray(Vo)[:n_vs]))))
            eo = float(np.max(np.abs(Vd[:n_on] @ Vd[:n_on].T - np.eye(n_on))))
            eu = float(np.max(np.abs(np.sum(Vd[:rows] * Vd[:rows], axis=1) - 1.0)))
            worst["V"], worst["ortho"] = max(worst["V"], eV), max(worst["ortho"], eo)
            checks.append((eV <= 1e-6, ("V", dv, i, eV)))
            checks.append((eo < on_tol, ("orthonormality", dv, i, n_on, eo, on_tol)))
            if km <= 7:
                assert np.max(np.abs(wide[i][:km] - np.asarray(Vo)[:km])) == 0.0  # the two oracles: the same arithmetic
                el = float(np.max(np.abs(np.abs(Vd[km]) - np.abs(wide[i][km]))))
                worst["last row"] = max(worst.get("last row", 0.0), el)
                checks.append((el <= last_tol, ("row k_max", dv, i, el, last_tol)))
            # every produced row is a unit vector (a row that never reached memory would be zero or stale)
            checks.append((eu < 1e-8, ("unit length", dv, i, rows, eu)))
        print(f"k_max {km} tol {tol} dv {dv}: worst so far {worst}; oracle's own defect over {k1} rows {o_defect:.2e}")
        bad = [what for ok, what in checks if not ok]
        assert not bad, bad[:6]


@pytest.mark.parametrize("dv", [33, 50])
def test_rows_that_never_enter_the_loop_leave_their_wave_mates_alone(orc, dv):
    """The breakdown start of test_gpu_wave.py / test_gpu_parity.py (|U| = 1e17 at a resting plant) planted in single rows
    of a k_max = 6 batch whose other rows run all six iterations.  On the horizons of this kernel (>= 33 stages) controls
    of that size overflow the pendulum's costate recurrence — in the reference as well, whose ||r0|| is already NaN and
    which falls through with NaNs — so this start is NOT a breakdown here and the planted rows do not leave mid-loop:
    they are switched off at the residual test with CGMRES_HIP_EXIT_NONFINITE and zero Arnoldi steps, and sit masked
    through every ring round, refill and x update their three wave mates run.  What is checked is that the mates agree
    with the oracle.  (Rows that leave in the middle of the loop: the tol = 1e-6 legs of the free-running test.)"""
    B, km = 40, 6
    x0, u0, p = orc.batch_scenario(0, B)
    planted = (1, 22, 37)  # one row of a wave, in a full workgroup and in the partly filled one
    ui, xx, pp = u0.copy(), x0.copy(), p.copy()
    for i in planted:
        ui[i], xx[i], pp[i] = 1e17, 0.0, 0.0
    c = _batch(B, dv, km, 0.0)
    c.set_ptau_repeat(pp)
    c.init_u0(ui)
    u = c.control(xx)
    n_ax, reason = c.get_status()
    _, U1, d1 = c.get_state()
    c.close()
    for i in range(B):
        r = orc.Controller(0, dv, km, 0.0)
        r.set_ptau_repeat(pp[i])
        r.init_u0(ui[i])
        ur = r.control(xx[i])
        k_o, _, reason_o = r.last_solve()
        if i in planted:
            assert np.all(np.isnan(ur))  # the reference's fall-through
            assert reason[i] == cg.EXIT_NONFINITE and n_ax[i] == 0, (i, reason[i], n_ax[i])
            assert np.all(np.isnan(u[i])) and np.all(np.isnan(d1[i]))
        else:
            assert n_ax[i] == k_o == km and reason[i] == reason_o, (i, n_ax[i], k_o, reason[i], reason_o)
            assert np.max(np.abs(u[i] - ur)) <= U_TOL * max(1.0, float(np.max(np.abs(ur)))), i
