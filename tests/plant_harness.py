"""Shared by the tests of the plant of a closed loop (cgmres_hip_plant_step_device, cgmres_hip_closed_loop_device_plant):
the numpy plant — forward Euler and classical RK4 on the three parametrised state equations, written here from the
reference's model.hpp files and independently of the device code — the theta draw, and the oracle driven tick by tick
against that plant."""
import math

import numpy as np

from record_harness import DV, KM

PENDULUM, MSD, SEMIACTIVE = 0, 1, 2
# the constants dxdt reads, in the order of theta (include/cgmres_hip.h)
NOMINAL = {PENDULUM: np.array([6.25, 15.6, 39.1111, 0.0407448, 5.65635, 0.905016, 14.1183]),  # As Bs A52 C22 A32a A32 A32b
           MSD: np.ones(6),                                                                  # m1 m2 d1 d2 k1 k2
           SEMIACTIVE: np.array([-1.0, -1.0])}                                               # a b
DIMS = {PENDULUM: (4, 3), MSD: (4, 6), SEMIACTIVE: (2, 3)}


def _sin(a):
    return np.array([math.sin(v) for v in np.atleast_1d(a)])  # (libm, as the oracle: numpy's own sin may differ by an ulp)


def _cos(a):
    return np.array([math.cos(v) for v in np.atleast_1d(a)])


def rhs(model, x, u, th):
    """dxdt of the batch: x [B, nx], u [B, nu], th [B, n_theta] -> [B, nx], float64, the statements of model.hpp."""
    x, u, th = np.atleast_2d(x), np.atleast_2d(u), np.atleast_2d(th)
    f = np.empty_like(x, dtype=np.float64)
    if model == PENDULUM:
        As, Bs, A52, C22, A32a, A32, A32b = th.T
        sd, cd, s1 = _sin(x[:, 0] - x[:, 1]), _cos(x[:, 0] - x[:, 1]), _sin(x[:, 1])
        f[:, 0], f[:, 1] = x[:, 2], x[:, 3]
        f[:, 2] = -As * x[:, 2] + Bs * u[:, 0]
        f[:, 3] = A32 * x[:, 2] * x[:, 2] * sd + A52 * s1 - A32b * cd * u[:, 0] + A32a * cd * x[:, 2] + C22 * (x[:, 2] - x[:, 3])
    elif model == MSD:
        m1, m2, d1, d2, k1, k2 = th.T
        f[:, 0], f[:, 1] = x[:, 2], x[:, 3]
        f[:, 2] = -(k1 * k2) / m1 * x[:, 0] + k2 / m1 * x[:, 1] - (d1 + d2) / m1 * x[:, 2] + d2 / m1 * x[:, 3] + u[:, 0] / m1
        f[:, 3] = k2 / m2 * x[:, 0] - k2 / m2 * x[:, 1] + d2 / m2 * x[:, 2] - d2 / m2 * x[:, 3] + u[:, 1] / m2
    else:
        a, b = th.T
        f[:, 0] = x[:, 1]
        f[:, 1] = a * x[:, 0] + b * u[:, 0] * x[:, 1]
    return f


def shape321_rhs(x, u, p):
    """dxdt of tests/user_models/shape_models.hpp, alias (3, 2, 1): x [B, 3], u [B, 2], p [B, 1]."""
    nx, nu = 3, 2
    f = np.empty_like(x, dtype=np.float64)
    for i in range(nx):
        n = (i + 1) % nx
        fi = -(0.5 + 0.1 * i) * x[:, i] + (0.8 - 0.15 * i) * x[:, n] - (0.3 + 0.05 * i) * x[:, i] * x[:, i] * x[:, n]
        for j in range(nu):
            fi = fi + ((-1.0 if (i + j) % 2 else 1.0) * (0.3 + 0.1 * ((2 * i + 3 * j) % 5))) * u[:, j]
        f[:, i] = fi + (0.2 + 0.1 * i) * p[:, 0]
    return f


def integrate(f, x, integrator, substeps, dt):
    """`substeps` steps of dt/substeps of "euler" | "rk4" on x' = f(x), float64."""
    x = np.array(np.atleast_2d(x), dtype=np.float64)
    hh = dt / substeps
    for _ in range(substeps):
        if integrator == "euler":
            x = x + f(x) * hh
        else:
            k1 = f(x)
            k2 = f(x + k1 * (0.5 * hh))
            k3 = f(x + k2 * (0.5 * hh))
            k4 = f(x + k3 * hh)
            x = x + (((k1 + 2.0 * k2) + 2.0 * k3) + k4) * (hh / 6.0)
    return x


def plant(model, x, u, th, integrator, substeps, dt):
    """Phi(x, u; theta) of the batch (zero-order hold of u and theta)."""
    return integrate(lambda z: rhs(model, z, u, th), x, integrator, substeps, dt)


def theta_draw(model, batch, dtype=np.float64):
    """Per-instance theta, uniform in 0.9 .. 1.1 x nominal, seed 11 (rounded to the handle's dtype)."""
    rng = np.random.default_rng(11)
    return (NOMINAL[model] * rng.uniform(0.9, 1.1, (batch, len(NOMINAL[model])))).astype(dtype)


def oracle_plant_rows(orc, model, x0, u0, p, i, n, th, integrator, substeps, d=None, v=None, seq=None, dv=DV, km=KM, tol=1e-6,
                      dtype="f64"):
    """The three statements of cgmres_hip_closed_loop_device_plant on the oracle for instance i, tick by tick:
    y_k = x_k + v_k, u_k = control(y_k) with ptau_k, x_{k+1} = Phi(x_k, u_k) + d_k.  th [n_theta], d, v [n, nx], seq [n, ...]:
    the rows of THIS instance.  -> (x [n, nx], u [n, nu], n_ax [n], reason [n], controller); in fp32 the state is kept in
    float32 as the device keeps it."""
    npdt = np.float32 if dtype == "f32" else np.float64
    r = orc.Controller(model, dv, km, tol, dtype)
    orc.start_controller(r, x0[i], u0[i], p[i])
    x = np.array(x0[i], dtype=npdt)
    xs, us, ks, why = [], [], [], []
    for k in range(n):
        if seq is not None:
            r.set_ptau(seq[k])
        y = x if v is None else (x + v[k].astype(npdt)).astype(npdt)
        u = r.control(y)
        x = plant(model, x.astype(np.float64), np.asarray(u, dtype=npdt).astype(np.float64), np.asarray(th, dtype=np.float64),
                  integrator, substeps, float(npdt(r.dt)))[0].astype(npdt)
        if d is not None:
            x = (x + d[k].astype(npdt)).astype(npdt)
        xs.append(x.astype(np.float64)), us.append(np.array(u)), ks.append(r.last_solve()[0]), why.append(r.last_solve()[2])
    return np.array(xs), np.array(us), np.array(ks), np.array(why), r
