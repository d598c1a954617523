"""The host side of a handle call (csrc/capi.hip ENTER, csrc/ctx_host.hip.h): what a handle refuses and that it is
none the worse for it, the two host-pointer paths of control() against control_device(), and the time of an fp32 handle.
All at dv = 8, k_max = 3."""
import ctypes as C
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin, scenarios

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DV, KMAX = 8, 3


def make(model, batch, variant, dtype="f64"):
    """(controller after the start-up calls of the example mains, its x0)"""
    if model == "vdp":
        b = np.arange(batch, dtype=np.float64)
        x0 = np.stack([1.0 + 0.1 * b, -0.5 + 0.05 * b], axis=1)
        p = np.stack([0.2 * b, 0.05 * (np.arange(batch) % 3)], axis=1)
        u0 = np.tile(np.array([0.1, 1.9, 0.03]), (batch, 1))
        header = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
        model = plugin.register(plugin.build(header, cls="VdpModel", name="vdp"))
    else:
        x0, u0, p = scenarios.batch(model, batch)
    c = cg.CgmresBatch(model, batch=batch, dv=DV, k_max=KMAX, variant=variant, dtype=dtype)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    return c, x0.astype(c.np_dtype)


@pytest.mark.parametrize("model,variant", [("pendulum", 2), ("msd", 1), ("vdp", 0)], ids=["wg", "lane", "user"])
def test_refused_calls_leave_the_handle_good(model, variant):
    """Every call the entry points refuse for a null pointer or a negative count returns EINVAL with its text, and the
    next tick of that handle is, bit for bit, the tick of a handle that never saw such a call."""
    lib = cg.load()
    c, x0 = make(model, 3, variant)
    fresh, _ = make(model, 3, variant)
    assert c.variant == fresh.variant and (variant == 0 or c.variant == variant)
    u = np.empty((3, c.dim_u))
    p0 = np.zeros((3, c.dim_p))
    xd, ud = c.device_buffer(x0.shape).upload(x0), c.device_buffer(u.shape)
    h, hp = c._h, lambda a: a.ctypes.data
    refused = [
        (lambda: lib.cgmres_hip_control(h, None, hp(x0)), "control: null pointer"),
        (lambda: lib.cgmres_hip_control(h, hp(u), None), "control: null pointer"),
        (lambda: lib.cgmres_hip_control_device(h, None, xd.ptr), "control: null pointer"),
        (lambda: lib.cgmres_hip_control_device(h, ud.ptr, None), "control: null pointer"),
        (lambda: lib.cgmres_hip_set_ptau(h, None, 1), "set_ptau: null pointer"),
        (lambda: lib.cgmres_hip_set_ptau_repeat(h, None, 0), "set_ptau: null pointer"),
        (lambda: lib.cgmres_hip_init_u0(h, None, 1), "init_u0: null pointer"),
        (lambda: lib.cgmres_hip_init_u0_newton(h, None, hp(x0), hp(p0), 10), "init_u0_newton: null pointer"),
        (lambda: lib.cgmres_hip_init_u0_newton(h, hp(u), None, hp(p0), 10), "init_u0_newton: null pointer"),
        (lambda: lib.cgmres_hip_init_u0_newton(h, hp(u), hp(x0), None, 10), "init_u0_newton: null pointer"),
        (lambda: lib.cgmres_hip_init_u0_newton(h, hp(u), hp(x0), hp(p0), -1), "init_u0_newton: n_loop < 0"),
        (lambda: lib.cgmres_hip_closed_loop_device(h, None, ud.ptr, 1), "closed_loop: null pointer"),
        (lambda: lib.cgmres_hip_closed_loop_device(h, xd.ptr, None, 1), "closed_loop: null pointer"),
    ]
    assert c.dim_p > 0  # (with dim_p = 0 a null ptau / p0 is no error)
    for call, text in refused:
        assert call() == EINVAL
        assert lib.cgmres_hip_last_error().decode() == text
    assert c.t == 0.0
    got, want = c.control(x0), fresh.control(x0)
    assert np.array_equal(got, want) and np.all(np.isfinite(got))
    for a, b in zip(c.get_state(), fresh.get_state()):
        assert np.array_equal(a, b)
    xd.free(), ud.free(), c.close(), fresh.close()


@pytest.mark.parametrize("batch", [3, 1025], ids=["pinned", "staged"])
@pytest.mark.parametrize("model", ["pendulum", "msd"])
def test_wg_control_through_host_pointers_equals_control_device(model, batch):
    """control() of the wg context goes through host-mapped pinned buffers up to kPinnedIoMaxBatch = 1024 controllers
    and through staged copies above; either way it is the tick control_device() runs on device buffers."""
    host, x0 = make(model, batch, 2)
    dev, _ = make(model, batch, 2)
    xd, ud = dev.device_buffer(x0.shape).upload(x0), dev.device_buffer((batch, dev.dim_u))
    u = host.control(x0)
    dev.control_device(ud, xd)
    dev.synchronize()
    assert np.array_equal(u, ud.download()) and np.all(np.isfinite(u))
    for a, b in zip(host.get_state(), dev.get_state()):
        assert np.array_equal(a, b)
    xd.free(), ud.free(), host.close(), dev.close()


@pytest.mark.parametrize("variant", [2, 1], ids=["wg", "lane"])
def test_time_of_an_fp32_handle_accumulates_in_float(variant):
    c, x0 = make("pendulum", 3, variant, dtype="f32")
    t = np.float32(0)
    for _ in range(5):
        c.control(x0)
        t = np.float32(t + np.float32(c.dt))
    assert c.t == float(t)
    assert c.t != 5 * c.dt  # (the double sum differs: the check above tells the two apart)
    c.close()
