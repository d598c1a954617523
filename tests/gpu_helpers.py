"""Helpers that more than one GPU test module uses, so that no test module imports another: the teacher-forced and the
free-running comparison with the oracle (from test_gpu_wave.py, test_gpu_gs_ring.py, test_gpu_closed_loop.py) and the
variant-parametrised handle of test_gpu_parity.py.  A plain module: nothing from conftest."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg

U_TOL, DUDT_REL = 1e-9, 1e-7  # fp64 teacher-forced |du|, relative |ddUdt|
# 2 = "wg" (default mapping; in fp64 with row-parallel sweeps for the pendulum at 33 <= dv <= 53 — Newton on the trajectory —
#     and for the semi-active damper at dv <= 53 — scans only; tick_wg.hip.h: NWT),
# "2s" = the same with FLAG_SERIAL_STATE_SWEEP (the wg kernel with the serial quad sweep, where that differs),
# 1 = "lane" (reference statement order), 3 = "wg-lean" (two workgroups per CU),
# 4 = "wave" (one wavefront per controller: the latency mapping; pendulum fp64, dv <= 63, k_max <= 10)
SERIAL_STATE = "2s"
VARIANTS = [2, SERIAL_STATE, 1, 3, 4]




def new_batch(*a, **kw):
    """cg.CgmresBatch; a size / model the wave mapping does not serve skips the test case."""
    if kw.get("variant") == SERIAL_STATE:
        model = a[0] if a else kw.get("model")
        dv = kw.get("dv", 0)
        row_kernel = (model in (0, "pendulum") and 33 <= dv <= 53) or (model in (2, "semiactive") and dv <= 53)
        if not row_kernel or kw.get("dtype", "f64") != "f64":
            pytest.skip("FLAG_SERIAL_STATE_SWEEP only changes the fp64 kernels of the pendulum and the semi-active damper "
                        "at dim_u*dv <= 160")
        kw = dict(kw, variant=2, flags=kw.get("flags", 0) | cg.FLAG_SERIAL_STATE_SWEEP)
    try:
        return cg.CgmresBatch(*a, **kw)
    except cg.CgmresHipError as e:
        if kw.get("variant") == 4 and "wave mapping" in str(e):
            pytest.skip("the wave mapping does not cover this model / dtype / size")
        raise


def _refs(orc, model, dv, km, tol, x0, u0, p):
    out = []
    for i in range(len(x0)):
        r = orc.Controller(model, dv, km, tol)
        orc.start_controller(r, x0[i], u0[i], p[i])
        out.append(r)
    return out


def _teacher_forced(orc, c, refs, x0, ticks, u_tol=U_TOL):
    """Every tick: controller state and x taken from the oracle, u / dUdt / counts / exit reasons compared."""
    x = x0.copy()
    worst = 0.0
    for tick in range(ticks):
        t_o, U_o, d_o = zip(*[r.get_state() for r in refs])
        c.set_state(t_o[0], np.array(U_o), np.array(d_o))
        u = c.control(x)
        n_ax, reason = c.get_status()
        _, U1, d1 = c.get_state()
        for i, r in enumerate(refs):
            ur = r.control(x[i])
            worst = max(worst, float(np.max(np.abs(u[i] - ur))))
            # u = U + dUdt*dt (cgmres.hpp:102-109): the bound on u that goes with SURVEY 8(c)'s bound on dUdt — relative to
            # |u| and to dt*|dUdt| where a time jump makes them large (|dUdt| ~ 1e5 on the two-mass system)
            d_ref = r.get_state()[2]
            bound = u_tol * max(1.0, float(np.max(np.abs(ur)))) + r.dt * DUDT_REL * max(1.0, float(np.max(np.abs(d_ref))))
            assert np.max(np.abs(u[i] - ur)) <= bound, (tick, i, u[i], ur)
            k_o, _, reason_o = r.last_solve()
            assert n_ax[i] == k_o and reason[i] == reason_o, (tick, i, n_ax[i], k_o, reason[i], reason_o)
            d_ref = r.get_state()[2]
            assert np.max(np.abs(d1[i] - d_ref)) <= DUDT_REL * max(1.0, float(np.max(np.abs(d_ref)))), (tick, i)
            x[i] = x[i] + r.plant(x[i], ur) * r.dt
    return worst


def _oracle_free_run(orc, dv, km, tol, x0, u0, p, ticks, model=0):
    """x, u after `ticks` closed-loop ticks and the Arnoldi counts / exit reasons of every tick, per instance."""
    xs, us, counts, reasons = [], [], [], []
    for i in range(len(x0)):
        r = orc.Controller(model, dv, km, tol)
        orc.start_controller(r, x0[i], u0[i], p[i])
        x, ks, rs = x0[i].copy(), [], []
        for _ in range(ticks):
            u = r.control(x)
            k_o, _, reason_o = r.last_solve()
            ks.append(k_o), rs.append(reason_o)
            x = x + r.plant(x, u) * r.dt
        xs.append(x), us.append(u), counts.append(ks), reasons.append(rs)
    return np.array(xs), np.array(us), np.array(counts), np.array(reasons)
