"""GPU: the preview of a sampled reference signal inside the device loop (cgmres_hip_closed_loop_device_preview,
cgmres_hip_preview_device; csrc/preview.hip.h).

A. the rows the kernel forms against cg.preview_rows, the numpy restatement, fed the handle's own tick times;
B. the loop uses those rows: bit for bit the ptau_seq_dev loop of a twin handle over the exported rows;
C. against the oracle directly (set_ptau(preview_rows) before every control);
D. composition with dist / meas, a record, a plant of its own, the lane mapping;
E. edges: a signal shorter than the loop, n_ticks = 0, dim_p = 0;
F. what is refused;  G. a user model whose state equation reads p.

The bounds of A are derived, not measured: statement for statement the kernel and the restatement differ only by fma
contraction in tau, s and the lerp, which is worth 8 eps (tau_max/ts) max|dsig| + 8 eps max|sig| (eps = 2^-53); an fp32
handle adds one fp32 ulp of the value for the final rounding."""
import ctypes
import ctypes.util
import math
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDP = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
EPS = 2.0 ** -53
N = 23  # two launch boundaries plus a tail: the ring is reused twice


def sample_of(batch, n=14):
    step = max(1, batch // n)
    s = list(range(0, batch, step))[:n]
    for extra in (batch - 1, 15, 16):
        if 0 <= extra < batch and extra not in s:
            s.append(extra)
    return sorted(s)


_expf = None


def expf(x):
    """libm's expf: what std::exp(float) of the handle's host code calls."""
    global _expf
    if _expf is None:
        _expf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").expf
        _expf.restype, _expf.argtypes = ctypes.c_float, [ctypes.c_float]
    return np.float32(_expf(float(x)))


def tick_clock(c, n, t=None):
    """(t_k, dtau_k), k < n, as the handle advances them in its dtype: t += dt (cgmres.hpp:107), get_dtau (:32-34)."""
    ts, ds = [], []
    if c.np_dtype == np.float32:
        f = np.float32
        t = f(c.t if t is None else t)
        for _ in range(n):
            ts.append(t), ds.append(f(f(f(c.Tf) * f(f(1) - expf(f(-f(c.alpha)) * t))) / f(c.dv)))
            t = f(t + f(c.dt))
    else:
        t = float(c.t if t is None else t)
        for _ in range(n):
            ts.append(t), ds.append(c.Tf * (1 - math.exp(-c.alpha * t)) / c.dv)
            t = t + c.dt
    return np.array(ts, dtype=c.np_dtype), np.array(ds, dtype=c.np_dtype)


def start(model, batch, dv, km, variant, orc=None, dtype="f64"):
    from cgmres_cpp_amd import scenarios
    x0, u0, p = (orc.batch_scenario if orc else scenarios.batch)(model, batch)
    c = gh.new_batch(model, batch=batch, dv=dv, k_max=km, tol=1e-6, variant=variant, dtype=dtype)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    return c, x0, u0, p


def signal(p, n_samples, per_instance=True, dtype=np.float64):
    """A slow sinusoid about each instance's set point p [B, dim_p], amplitude and phase per instance."""
    B, j = len(p), np.arange(n_samples)
    b = np.arange(B)[:, None, None]
    sig = p[:, None, :] * (1.0 + 0.05 * np.sin(0.37 * j[None, :, None] + 0.61 * b)) + 0.01 * np.cos(0.23 * j[None, :, None] + b) * np.array([1.0, 0.3])
    sig = np.ascontiguousarray(sig.astype(dtype))
    return sig if per_instance else np.ascontiguousarray(sig[min(3, B - 1)])


class Dev:
    def __init__(self, c):
        self.c, self.bufs = c, []

    def __call__(self, a=None, shape=None, dtype=None):
        b = self.c.device_buffer(a.shape if a is not None else shape, dtype or (self.c.np_dtype if a is None or a.dtype.kind == "f" else a.dtype))
        self.bufs.append(b)
        return b.upload(a) if a is not None else b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def export(c, dev, sig, ts, t0, interp, n):
    rows = dev(shape=(n, c.batch, c.dim_p * (c.dv + 1)))
    c.preview_device(cg.Preview(dev(sig), ts, t0, interp), n, rows)
    return rows


# ---- A. rows against the restatement --------------------------------------------------------------------------------------
CASES_A = [(1, 1, "linear", True, "f64"), (65, 8, "hold", True, "f64"), (83, 50, "linear", True, "f64"), (83, 50, "hold", False, "f64"),
           (65, 8, "linear", False, "f64"), (1, 50, "hold", True, "f64"), (83, 1, "linear", False, "f64"), (83, 50, "linear", True, "f32"),
           (65, 8, "hold", True, "f32")]


@pytest.mark.parametrize("model", [0, 1], ids=["pendulum", "msd"])
@pytest.mark.parametrize("B,dv,interp,per_instance,dtype", CASES_A)
def test_rows_equal_the_restatement(model, B, dv, interp, per_instance, dtype):
    """From t = 2 the horizon is dv * dtau ~ Tf (1 - 1/e) long; 24 samples every 10 ms from t0 ~ 1.99 + 23 ticks: the
    early stages interpolate, the late ones hold the last sample, and with t0 moved ahead of t the front clamps too."""
    c, x0, u0, p = start(model, B, dv, 2, 1, dtype=dtype)
    dev = Dev(c)
    c.set_state(2.0)
    ts, ns = 0.01, 24
    sig = signal(p, ns, per_instance, c.np_dtype)
    t, dtau = tick_clock(c, N)
    assert float(t[0]) == 2.0 and c.t == 2.0
    for t0 in (1.9876543210123, 2.0123456789012):  # behind t: interpolation and the end clamp; ahead of t: the front clamp
        tau = t.astype(np.float64)[:, None] + np.arange(dv + 1)[None, :] * dtau.astype(np.float64)[:, None]
        s = (tau - t0) / ts
        assert np.min(np.abs(s - np.round(s))) > 1e-6, "a knot of the hold rule: choose another t0"  # (inputs only)
        assert (s.min() < 0) == (t0 > 2.0) and (dv < 8 or s.max() > ns - 1)
        rows = dev(shape=(N, B, c.dim_p * (dv + 1)))
        c.preview_device(cg.Preview(dev(sig), ts, t0, interp), N, rows)
        got = rows.download()
        want = cg.preview_rows(sig, ts, t0, interp, t, dtau, dv)
        want = want if per_instance else np.broadcast_to(want[:, None, :], got.shape)
        d = np.max(np.abs(np.diff(sig.astype(np.float64), axis=-2)))
        lim = 8 * EPS * (np.max(np.abs(tau)) / ts) * d + 8 * EPS * np.max(np.abs(sig))
        if dtype == "f32":
            lim = lim + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"B={B} dv={dv} {interp} {dtype} t0={t0}: max error {err.max():.3e}, bound {np.max(lim):.3e}")
        assert got.dtype == c.np_dtype and np.all(err <= lim)
        assert np.max(np.abs(got[0] - got[-1])) > 1e-4  # (the rows move with the tick)
    assert c.t == 2.0  # no state changed
    dev.free(), c.close()


# ---- the loop and its twin ------------------------------------------------------------------------------------------------
def run_loop(c, x0, n, *, preview=None, seq=None, d=None, v=None, stride=None, plant=None):
    """One closed_loop_device call; what the handle and the caller hold afterwards, the logs of a record included."""
    dev = Dev(c)
    xd, ud = dev(x0.astype(c.np_dtype)), dev(shape=(c.batch, c.dim_u))
    rec = None
    if stride:
        n_rec = n // stride
        rec = dict(stride=stride, x=dev(shape=(n_rec, c.batch, c.dim_x)), u=dev(shape=(n_rec, c.batch, c.dim_u)),
                   n_ax=dev(shape=(n_rec, c.batch), dtype=np.int32), reason=dev(shape=(n_rec, c.batch), dtype=np.int32), t=np.zeros(n_rec))
    c.closed_loop_device(xd, ud, n, seq, True, dist_seq_dev=dev(d) if d is not None else None,
                         meas_seq_dev=dev(v) if v is not None else None, record=rec, plant=plant, preview=preview)
    c.synchronize()
    n_ax, reason = c.get_status()
    t, U, dUdt = c.get_state()
    out = dict(x=xd.download(), u=ud.download(), n_ax=n_ax, reason=reason, t=np.array(t), U=U, dUdt=dUdt)
    if rec:
        out.update({"log_" + k: rec[k].download() for k in ("x", "u", "n_ax", "reason")}, log_t=rec["t"])
    out["u_next"] = c.control(out["x"])  # the handle kept the last tick's row as its ptau
    dev.free()
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=False), k
    assert np.all(np.isfinite(a["x"])) and np.all(np.isfinite(a["u"]))


def preview_and_twin(make, sig, ts, t0, interp, n, **extras):
    """The preview loop on one handle; on a twin the ptau_seq_dev loop over the rows preview_device exported."""
    c, x0 = make()
    dev = Dev(c)
    a = run_loop(c, x0, n, preview=cg.Preview(dev(sig), ts, t0, interp), **extras)
    dev.free(), c.close()
    c, x0 = make()
    dev = Dev(c)
    rows = export(c, dev, sig, ts, t0, interp, n)
    c.synchronize()
    assert c.t == 0.0
    b = run_loop(c, x0, n, seq=rows, **extras)
    moved = rows.download()
    dev.free(), c.close()
    assert np.max(np.abs(moved[0] - moved[-1])) > 1e-5  # (a reference that does move)
    return a, b


@pytest.mark.parametrize("variant", [2, 1, 3, 4])
@pytest.mark.parametrize("model", [0, 1], ids=["pendulum", "msd"])
def test_loop_equals_the_ptau_seq_loop_over_the_exported_rows(orc, model, variant):
    """B. ring, strides, cut and the hand-over of the last row, held to a path the suite already holds to the oracle."""
    def make():
        c, x0, u0, p = start(model, 83, 50, 10, variant, orc)
        assert c.variant == variant
        return c, x0
    c_dt = cg.model_info(model)["dt"]
    a, b = preview_and_twin(make, signal(orc.batch_scenario(model, 83)[2], 40), c_dt, 0.0, "linear", N)
    same_bits(a, b)
    assert abs(float(a["t"]) - N * c_dt) < 1e-12


@pytest.mark.parametrize("variant", [2, 1])
def test_loop_against_the_oracle(orc, variant):
    """C. no twin: the oracle is given set_ptau(preview_rows(...)) before every control()."""
    model, B, dv, km = 0, 83, 50, 10
    c, x0, u0, p = start(model, B, dv, km, variant, orc)
    sig, ts = signal(p, 40), c.dt
    t, dtau = tick_clock(c, N)
    rows = cg.preview_rows(sig, ts, 0.0, "linear", t, dtau, dv)
    dev = Dev(c)
    xd, ud = dev(x0), dev(shape=(B, c.dim_u))
    c.closed_loop_device(xd, ud, N, preview=cg.Preview(dev(sig), ts, 0.0, "linear"))
    c.synchronize()
    x, u = xd.download(), ud.download()
    n_ax, _ = c.get_status()
    worst = 0.0
    for i in sample_of(B, 14):
        r = orc.Controller(model, dv, km)
        orc.start_controller(r, x0[i], u0[i], p[i])
        xi = x0[i].copy()
        for k in range(N):
            r.set_ptau(rows[k, i])
            ui = r.control(xi)
            xi = xi + r.plant(xi, ui) * r.dt
        worst = max(worst, float(np.max(np.abs(u[i] - ui))), float(np.max(np.abs(x[i] - xi))))
        assert np.max(np.abs(u[i] - ui)) <= 1e-9 and np.max(np.abs(x[i] - xi)) <= 1e-9, (i, u[i], ui)
        assert n_ax[i] == r.last_solve()[0]
    print(f"variant {variant}: max |x, u - oracle| = {worst:.3e}")
    dev.free(), c.close()


def noise(n, batch, nx):
    rng = np.random.default_rng(7)
    return rng.normal(0.0, 1e-3, (n, batch, nx)), rng.normal(0.0, 1e-3, (n, batch, nx))


@pytest.mark.parametrize("what", ["noise", "record", "plant", "lane-record"])
def test_composition_equals_the_twin(orc, what):
    """D. the same extras on both sides: dist + meas, a record at stride 4 (launches cut at 4; the logs too), a plant of its
    own (one tick per launch), and the lane mapping under a record."""
    variant = 1 if what == "lane-record" else 2

    def make():
        c, x0, u0, p = start(0, 83, 50, 10, variant, orc)
        return c, x0
    d, v = noise(N, 83, 4)
    extras = {"noise": dict(d=d, v=v), "record": dict(stride=4), "plant": dict(plant=cg.Plant("rk4", 2), d=d, v=v),
              "lane-record": dict(stride=4)}[what]
    a, b = preview_and_twin(make, signal(orc.batch_scenario(0, 83)[2], 40), 1e-3, 0.0, "linear", N, **extras)
    same_bits(a, b)
    if "stride" in extras:
        assert a["log_x"].shape[0] == N // 4 and np.max(np.abs(a["log_x"][0] - a["log_x"][-1])) > 0


# ---- E. edges -------------------------------------------------------------------------------------------------------------
def test_signal_shorter_than_the_loop_holds_its_last_sample(orc):
    """8 samples, one per tick, the first 0.4 ms before t = 0 (off the knots of the hold rule): from tick 7 on every stage
    is past the end.  The twin runs the first launch (10 ticks) over the exported rows, then set_ptau_repeat(last sample)
    and the plain loop for the other 13: the same cut, 10 + 10 + 3."""
    c, x0, u0, p = start(0, 83, 50, 10, 2, orc)
    sig = signal(p, 8)
    pv = dict(ts=1e-3, t0=-0.4e-3, interp="hold")
    dev = Dev(c)
    a = run_loop(c, x0, N, preview=cg.Preview(dev(sig), **pv))
    dev.free(), c.close()
    c, x0, u0, p = start(0, 83, 50, 10, 2, orc)
    dev = Dev(c)
    rows = export(c, dev, sig, pv["ts"], pv["t0"], pv["interp"], 10)
    held = rows.download()[7:].reshape(3, 83, 51, 2)
    assert np.array_equal(held, np.broadcast_to(sig[None, :, None, -1, :], held.shape))
    xd, ud = dev(x0), dev(shape=(83, 3))
    c.closed_loop_device(xd, ud, 10, rows, True)
    c.set_ptau_repeat(sig[:, -1])
    c.closed_loop_device(xd, ud, N - 10)
    c.synchronize()
    assert np.array_equal(a["x"], xd.download()) and np.array_equal(a["u"], ud.download())
    t, U, dUdt = c.get_state()
    assert np.array_equal(a["U"], U) and np.array_equal(a["dUdt"], dUdt)
    assert np.array_equal(a["u_next"], c.control(a["x"]))
    dev.free(), c.close()


def test_zero_ticks_do_nothing(orc):
    c, x0, u0, p = start(0, 83, 50, 10, 2, orc)
    fresh, _, _, _ = start(0, 83, 50, 10, 2, orc)
    dev = Dev(c)
    xd, ud = dev(x0), dev(np.full((83, 3), 7.0))
    c.closed_loop_device(xd, ud, 0, preview=cg.Preview(dev(signal(p, 8)), 1e-3))
    c.synchronize()
    assert c.t == 0.0 and np.array_equal(xd.download(), x0) and np.all(ud.download() == 7.0)
    assert np.array_equal(c.control(x0), fresh.control(x0))  # (the handle's ptau is its own still)
    dev.free(), c.close(), fresh.close()


@pytest.mark.parametrize("variant", [2, 1])
def test_a_model_without_parameters_ignores_the_preview(orc, variant):
    """dim_p = 0 (semi-active damper): bit for bit the plain loop; sig_dev may be NULL or anything."""
    outs = []
    for how in ("plain", "null", "given"):
        c, x0, u0, p = start(2, 83, 50, 10, variant, orc)
        assert c.dim_p == 0
        dev = Dev(c)
        pv = {"plain": None, "null": cg.Preview(None, 1e-3), "given": cg.Preview(dev(np.ones((4, 3))), 1e-3, per_instance=False, n_samples=4)}[how]
        if how == "given":
            pv.sig = pv.sig.ptr
        outs.append(run_loop(c, x0, N, preview=pv))
        dev.free(), c.close()
    same_bits(outs[0], outs[1]), same_bits(outs[0], outs[2])


# ---- F. what is refused ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_good(orc):
    B = 20
    c, x0, u0, p = start(0, B, 8, 3, 2, orc)
    fresh, _, _, _ = start(0, B, 8, 3, 2, orc)
    lib, dev = cg.load(), Dev(c)
    xd, ud = dev(x0), dev(np.zeros((B, 3)))
    sg, dd, th = dev(signal(p, 16)), dev(np.zeros((5, B, 4))), dev(np.tile(cg.plant_info(0)["nominal"], (B, 1)))
    xl, rows, seq = dev(shape=(5, B, 4)), dev(shape=(5, B, 18)), dev(shape=(5, B, 18))
    size = ctypes.sizeof(cg.LoopPreview)

    def lv_of(fields):
        return cg.LoopPreview(**dict(dict(struct_size=size, interp=1, sig_per_instance=1, n_samples=16, t0=0.0, ts=1e-3, sig_dev=sg.ptr), **fields))

    def loop(n=5, rec=None, plant=None, li=None, x=xd.ptr, u=ud.ptr, **fields):
        li = li or cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs))
        lv = lv_of(fields)
        cg._check(lib.cgmres_hip_closed_loop_device_preview(c._h, x, u, n, ctypes.byref(li), ctypes.byref(rec) if rec else None,
                                                            ctypes.byref(plant) if plant else None, ctypes.byref(lv)))

    def rows_of(n=5, out=rows.ptr, **fields):
        lv = lv_of(fields)
        cg._check(lib.cgmres_hip_preview_device(c._h, ctypes.byref(lv), n, out))
    for f in (loop, rows_of):
        with pytest.raises(cg.CgmresHipError, match="struct_size .* cgmres_hip_loop_preview"):
            f(struct_size=size - 8)
        with pytest.raises(cg.CgmresHipError, match=r"cgmres_hip_loop_preview.reserved must be 0 \(got 0, 1\)"):
            f(reserved=(ctypes.c_int32 * 2)(0, 1))
        with pytest.raises(cg.CgmresHipError, match="unknown interp 2"):
            f(interp=2)
        with pytest.raises(cg.CgmresHipError, match="sig_per_instance is 2"):
            f(sig_per_instance=2)
        with pytest.raises(cg.CgmresHipError, match="n_samples 0 < 1"):
            f(n_samples=0)
        for bad in (0.0, -1e-3, float("inf"), float("nan")):
            with pytest.raises(cg.CgmresHipError, match="ts must be finite and > 0"):
                f(ts=bad)
        for bad in (float("inf"), float("nan")):
            with pytest.raises(cg.CgmresHipError, match="t0 must be finite"):
                f(t0=bad)
        with pytest.raises(cg.CgmresHipError, match="null sig_dev on a model with dim_p = 2"):
            f(sig_dev=None)
        with pytest.raises(cg.CgmresHipError, match="n_ticks"):
            f(n=-1)
    with pytest.raises(cg.CgmresHipError, match="preview_device: null rows_dev"):
        rows_of(out=None)
    with pytest.raises(cg.CgmresHipError, match="preview_device: null preview"):
        cg._check(lib.cgmres_hip_preview_device(c._h, None, 5, rows.ptr))
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps rows_dev"):
        rows_of(out=sg.ptr + 16)
    li_seq = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs), ptau_per_instance=1, ptau_seq_dev=seq.ptr)
    with pytest.raises(cg.CgmresHipError, match="ptau_seq_dev and a preview are both given"):
        loop(li=li_seq)
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps x_dev"):
        loop(sig_dev=xd.ptr, n_samples=1, sig_per_instance=0)
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps u_dev"):
        loop(sig_dev=ud.ptr + 8, n_samples=1, sig_per_instance=0)
    li_d = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs), dist_per_instance=1, dist_seq_dev=dd.ptr)
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps dist_seq_dev"):
        loop(li=li_d, sig_dev=dd.ptr + 64)
    li_m = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs), meas_per_instance=1, meas_seq_dev=dd.ptr)
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps meas_seq_dev"):
        loop(li=li_m, sig_dev=dd.ptr + 64)
    lp = cg.LoopPlant(struct_size=ctypes.sizeof(cg.LoopPlant), integrator=cg.PLANT_RK4, substeps=2, theta_per_instance=1, theta_dev=th.ptr)
    with pytest.raises(cg.CgmresHipError, match="sig_dev overlaps theta_dev"):
        loop(plant=lp, sig_dev=th.ptr + 8, n_samples=2, sig_per_instance=0)
    rec = cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=1, x_log_dev=xl.ptr)
    with pytest.raises(cg.CgmresHipError, match="x_log_dev overlaps sig_dev"):
        loop(rec=rec, sig_dev=xl.ptr + 16)
    # everything ..._plant refuses
    with pytest.raises(cg.CgmresHipError, match="stride 0 < 1"):
        loop(rec=cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=0, x_log_dev=xl.ptr))
    with pytest.raises(cg.CgmresHipError, match="substeps 0 outside"):
        loop(plant=cg.LoopPlant(struct_size=ctypes.sizeof(cg.LoopPlant), integrator=0, substeps=0))
    with pytest.raises(cg.CgmresHipError, match="null pointer"):
        loop(x=None)
    # the binding checks a typed signal before its address crosses the ABI
    with pytest.raises(ValueError):
        c.preview_device(cg.Preview(dev(np.ones((16, 3))), 1e-3), 5, rows)
    with pytest.raises(ValueError):
        c.preview_device(cg.Preview(dev(np.ones((B + 1, 16, 2))), 1e-3), 5, rows)
    with pytest.raises(TypeError):
        c.preview_device(cg.Preview(dev(np.ones((16, 2), dtype=np.float32), dtype=np.float32), 1e-3), 5, rows)
    with pytest.raises(ValueError):
        c.preview_device(cg.Preview(sg, 1e-3), 4, rows)
    # preview == NULL is the plant entry point
    assert c.t == 0.0
    cg._check(lib.cgmres_hip_closed_loop_device_preview(c._h, xd.ptr, ud.ptr, 0, None, None, None, None))
    c.synchronize()
    assert c.t == 0.0 and np.array_equal(xd.download(), x0)
    got, want = c.control(x0), fresh.control(x0)
    assert np.array_equal(got, want) and np.all(np.isfinite(got))
    for a, b in zip(c.get_state(), fresh.get_state()):
        assert np.array_equal(a, b)
    dev.free(), c.close(), fresh.close()


# ---- G. a user model whose state equation reads p -------------------------------------------------------------------------
def vdp_start(mid, variant, Bn=50):
    rng = np.random.default_rng(11)
    x0 = np.stack([1.0 + 0.5 * rng.random(Bn), -0.5 + 0.5 * rng.random(Bn)], axis=1)
    p = np.stack([0.5 * rng.random(Bn), 0.1 * rng.random(Bn)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (Bn, 1))
    c = cg.CgmresBatch(mid, batch=Bn, variant=variant)
    c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
    return c, x0, p


def vdp_signal(p, ns):
    j = np.arange(ns)[None, :]
    return np.ascontiguousarray(np.stack([p[:, :1] * (1.0 + 0.01 * j) + 0.002 * np.sin(0.3 * j), p[:, 1:2] * np.cos(0.05 * j)], axis=2))


def test_user_model_wg_equals_lane():
    """The bounds of test_user_model_moving_reference_wg_equals_lane: 1e-9 on x, u, the counts and the next tick."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    mid = plugin.register(plugin.build(VDP, cls="VdpModel", name="vdp"))
    outs = {}
    for variant in (2, 1):
        c, x0, p = vdp_start(mid, variant)
        dev = Dev(c)
        o = run_loop(c, x0, N, preview=cg.Preview(dev(vdp_signal(p, 40)), c.dt, 0.0, "linear"))
        outs[variant] = (o["x"], o["u"], o["n_ax"], o["u_next"])
        dev.free(), c.close()
    for a, b in zip(outs[2], outs[1]):
        assert np.max(np.abs(a.astype(float) - b.astype(float))) <= 1e-9
    assert np.all(np.isfinite(outs[2][0])) and np.all(np.isfinite(outs[2][1]))


@pytest.mark.parametrize("variant", [2, 1])
def test_user_model_plant_reads_stage_0_of_the_ticks_row(variant):
    """With Plant the user model's plant is its dxdt(x, u, p), p = stage 0 of that tick's row: bit for bit the twin over the
    exported rows, and not the loop of the handle's constant p."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    mid = plugin.register(plugin.build(VDP, cls="VdpModel", name="vdp"))

    def make():
        c, x0, p = vdp_start(mid, variant)
        make.p = p
        return c, x0
    make()[0].close()
    sig = vdp_signal(make.p, 40)
    sig[:, :, 1] += 0.05 * np.arange(40)[None, :]  # (p[1] drives the state equation: make stage 0 move from tick to tick)
    plant = cg.Plant("rk4", 2)
    a, b = preview_and_twin(make, sig, 0.01, 0.0, "linear", 12, plant=plant)
    same_bits(a, b)
    c, x0 = make()
    const = run_loop(c, x0, 12, plant=plant)
    c.close()
    assert np.max(np.abs(const["x"] - a["x"])) > 1e-6


def test_plugin_built_before_the_preview_is_told_to_rebuild():
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    mid = plugin.register(plugin.build(VDP, cls="VdpModel", name="vdp_nopreview", extra_flags=("-DCGM_PLUGIN_WITHOUT_PREVIEW",)))
    c, x0, p = vdp_start(mid, 0, 4)
    dev = Dev(c)
    xd, ud = dev(x0), dev(np.zeros((4, 3)))
    pv = cg.Preview(dev(vdp_signal(p, 8)), 0.01)
    rows = dev(shape=(3, 4, 2 * (c.dv + 1)))
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.preview_device(pv, 3, rows)
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.closed_loop_device(xd, ud, 3, preview=pv)
    assert c.t == 0.0
    seq = dev(np.tile(np.repeat(p, c.dv + 1, axis=0).reshape(4, -1), (3, 1, 1)))
    c.closed_loop_device(xd, ud, 3, seq, True, record=dict(stride=1, t=np.zeros(3)), plant=cg.Plant())
    c.synchronize()
    assert c.t > 0.0 and np.all(np.isfinite(xd.download()))
    dev.free(), c.close()
