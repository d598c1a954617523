"""Scenarios with tuning constants other than the shipped ones (dt, h, zeta, Tf, alpha: the run-time fields of
cgmres_hip_config), shared by tests/test_tuning_scenarios.py (CPU: the properties of the scenarios themselves) and
tests/test_gpu_tuning.py (GPU: every mapping against the oracle with the same constants).

Every built-in model ships dt = 1e-3, h = 2e-3, zeta = 1000 — so 1 - zeta*h = -1 and 1/h = 500 exactly — and
Tf (1 - exp(-alpha t)) / dv <= 0.02.  The sets below move every one of them (oracle/ref_records.py: TUNING_SETS, which
the reference was compiled with for tests/test_oracle_vs_ref.py):

    name   dt     h     zeta   Tf    alpha   1 - zeta*h
    fast   5e-4   1e-3  1500   0.25  4.0     -0.5
    long   1e-3   4e-3   125   1.5   1.0     +0.5
    mid    1e-3   3e-3   400   1.0   3.0     -0.2

The batch is orc.batch_scenario(model, 20): one full 16-instance workgroup plus a ragged four.  The oracle runs it
free from t = 0 (control, then the example's Euler plant step) and its controller state and x are kept at the
checkpoints.  A jump of t on a cold U blows up under a long horizon, so late states are reached by running, not set."""
import numpy as np

from oracle.ref_records import TUNING_SETS

SETS = TUNING_SETS
MODELS = (0, 1, 2)
MODEL_NAMES = {0: "pendulum", 1: "msd", 2: "semiactive"}
# (50, 10): the row-Newton / row-scan kernels, MSD on the fh_hbm long-vector plan, the full wave;
# (12, 4): the short-vector costate forms
SIZES = ((50, 10), (12, 4))
BATCH = 20
TOL = 1e-6
# ticks run before a teacher-forced comparison starts.  190 is where the pendulum under `long` straddles the rotation range
# (12 of the 20 instances beyond it, both kinds inside the first workgroup); by 400 all of them are beyond it
CHECKPOINTS = (0, 40, 190, 400)
LOOP_TICKS = (11, 25)            # lengths of the fused closed loops (one launch boundary + a tail; two + a tail)
TICKS_AFTER = 3                  # ticks compared from each checkpoint
ROT_RANGE = 0.04                 # rad per stage: the range of the rotation form of the trig update (rot_zmax = 1.6e-3)
MARGIN = 1e-3                    # an exit is marginal when |rho_e| is within 0.1 % of tol ...
MARGINAL_CAP = 0.02              # ... and at most 2 % of the (tick, instance) pairs may be


def tol_scale(name):
    """(F - Fh)/h amplifies rounding by 1/h: the project's bounds were set at h = 2e-3 and grow with a smaller h."""
    return max(1.0, 2e-3 / SETS[name]["h"])


def is_marginal(ctrl, tol=TOL):
    """Whether the exit of ctrl's last solve was decided within 0.1 % of tol: |rho_e| at the exit column or at the one
    before it.  The earlier estimate is no longer stored (gmres.hpp:88-90 rotates it in place and the back substitution
    overwrites the leading entries), so it is recovered from the reflector of the exit column:
    rho[k+1] = -(g0 rho_k g2) g1."""
    n_ax, _, reason = ctrl.last_solve()
    _, _, rho, g = ctrl.krylov()
    near = lambda v: abs(abs(v) - tol) <= MARGIN * tol
    if near(rho[n_ax]):
        return True
    if n_ax >= 1:
        den = g[n_ax - 1][0] * g[n_ax - 1][1] * g[n_ax - 1][2]
        if den != 0.0 and near(rho[n_ax] / den):
            return True
    return False


def oracle_batch(orc, model, dv, kmax, name, dtype="f64", batch=BATCH):
    """(controllers started like the example main, x0, u0, p) of the seeded batch under SETS[name]."""
    x0, u0, p = orc.batch_scenario(model, batch)
    ctrls = []
    for i in range(batch):
        c = orc.Controller(model, dv, kmax, TOL, dtype, tuning=SETS[name])
        orc.start_controller(c, x0[i], u0[i], p[i])
        ctrls.append(c)
    return ctrls, x0, u0, p


class FreeRun:
    """The oracle's closed loop of the seeded batch from t = 0.  snap[W] = dict(t, U, dUdt, x) BEFORE tick W (W = 0: the
    start) and u, n_ax, reason of tick W - 1; n_ax / reason / marginal [ticks, BATCH] for every tick run."""

    def __init__(self, orc, model, name, dv, kmax, dtype="f64", ticks=None):
        f32 = dtype == "f32"
        npdt = np.float32 if f32 else np.float64
        ticks = max(CHECKPOINTS) + TICKS_AFTER if ticks is None else ticks
        ctrls, x0, u0, p = oracle_batch(orc, model, dv, kmax, name, dtype)
        self.p, self.x0, self.u0 = p, x0, u0
        xs = [np.array(x, dtype=npdt) for x in x0]
        self.n_ax = np.zeros((ticks, BATCH), dtype=int)
        self.reason = np.zeros((ticks, BATCH), dtype=int)
        self.marginal = np.zeros((ticks, BATCH), dtype=bool)
        self.snap = {}
        u_last = np.zeros((BATCH, ctrls[0].dim_u))
        for tick in range(ticks + 1):
            if tick in CHECKPOINTS or tick in LOOP_TICKS:
                st = [c.get_state() for c in ctrls]
                self.snap[tick] = dict(t=st[0][0], U=np.array([s[1] for s in st]), dUdt=np.array([s[2] for s in st]),
                                       x=np.array(xs, dtype=np.float64), u=u_last.copy(),
                                       n_ax=self.n_ax[tick - 1].copy() if tick else None,
                                       reason=self.reason[tick - 1].copy() if tick else None)
            if tick == ticks:
                break
            for i, c in enumerate(ctrls):
                u = c.control(xs[i])
                k, _, why = c.last_solve()
                self.n_ax[tick, i], self.reason[tick, i], self.marginal[tick, i] = k, why, is_marginal(c)
                # plant step in the controller's precision (the device does x + f*dt in T)
                xs[i] = (xs[i] + c.plant(xs[i], u).astype(npdt) * npdt(c.dt)).astype(npdt)
                u_last[i] = u

    def restore(self, orc, model, dv, kmax, name, W, dtype="f64"):
        """Fresh oracle controllers holding the state of checkpoint W, and a copy of its x."""
        s = self.snap[W]
        ctrls = []
        for i in range(BATCH):
            c = orc.Controller(model, dv, kmax, TOL, dtype, tuning=SETS[name])
            if c.dim_p:
                c.set_ptau_repeat(self.p[i])
            c.set_state(s["t"], s["U"][i], s["dUdt"][i])
            ctrls.append(c)
        return ctrls, s["x"].copy()


_runs = {}


def free_run(orc, model, name, dv, kmax, dtype="f64"):
    """Cached per process: the 400-tick warm-up is CPU work done once per (model, set, size).  fp32 runs stop after the
    W = 40 checkpoint (the fp32 comparison uses W = 0 and 40 only)."""
    key = (model, name, dv, kmax, dtype)
    if key not in _runs:
        _runs[key] = FreeRun(orc, model, name, dv, kmax, dtype, ticks=None if dtype == "f64" else 40 + TICKS_AFTER)
    return _runs[key]


def pendulum_stage_increments(orc, snap, name, dv, kmax):
    """Per instance: the largest angle increment per horizon stage, max over the stages of |d x0|, |d x1| and |d(x0 - x1)|
    (the arguments of the pendulum's sin/cos), on the horizon trajectory of cgmres.hpp:132-140 recomputed in numpy from
    the plant's right-hand side at the checkpoint's (t, U, x)."""
    tun = SETS[name]
    dtau = tun["Tf"] * (1.0 - np.exp(-tun["alpha"] * snap["t"])) / dv
    c = orc.Controller(0, dv, kmax, TOL, tuning=tun)
    out = np.zeros(BATCH)
    for i in range(BATCH):
        x = snap["x"][i].copy()
        for s in range(dv):
            f = c.plant(x, snap["U"][i][3 * s:3 * s + 3])
            step = f * dtau
            out[i] = max(out[i], abs(step[0]), abs(step[1]), abs(step[0] - step[1]))
            x = x + step
    return out
