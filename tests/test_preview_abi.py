"""CPU: the ABI of the preview of a sampled reference signal — the two entry points are declared, listed and exported and
refuse a null handle; the ctypes mirror of struct cgmres_hip_loop_preview has the C layout; and cg.preview_rows, the numpy
restatement the GPU tests hold the kernel to, against closed forms."""
import ctypes
import os
import re

import numpy as np
import pytest

import cgmres_cpp_amd as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgmres_hip_closed_loop_device_preview", "cgmres_hip_preview_device")
EPS = 2.0 ** -53


def bound(sig, tau_max, ts):
    """8 eps (tau_max/ts) max|dsig| + 8 eps max|sig|: the freedom of fma contraction in tau, s and the lerp."""
    sig = np.asarray(sig, dtype=np.float64)
    d = np.max(np.abs(np.diff(sig, axis=-2))) if sig.shape[-2] > 1 else 0.0
    return 8 * EPS * (tau_max / ts) * d + 8 * EPS * np.max(np.abs(sig))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    return cg.load()


def test_header_exports_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in cg.SYMBOLS and hasattr(lib, name), name
    assert "#define CGMRES_HIP_ABI_VERSION 3" in hdr and cg.ABI_VERSION == 3
    assert re.search(r"enum \{ CGMRES_HIP_PREVIEW_HOLD = 0, CGMRES_HIP_PREVIEW_LINEAR = 1 \};", code)
    assert (cg.PREVIEW_HOLD, cg.PREVIEW_LINEAR) == (0, 1) and cg.PREVIEW_INTERPS == {"hold": 0, "linear": 1}


def test_loop_preview_struct_layout():
    hdr = open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()
    m = re.search(r"typedef struct cgmres_hip_loop_preview \{(.*?)\} cgmres_hip_loop_preview;", hdr, flags=re.S)
    assert m, "struct cgmres_hip_loop_preview not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|double|const void\*)\s+(\w+)(\[2\])?;", body)
    assert fields == [("int32_t", "struct_size", ""), ("int32_t", "interp", ""), ("int32_t", "sig_per_instance", ""),
                      ("int32_t", "n_samples", ""), ("double", "t0", ""), ("double", "ts", ""), ("const void*", "sig_dev", ""),
                      ("int32_t", "reserved", "[2]")]
    # int32 x4, double x2, a pointer, int32 x2
    assert ctypes.sizeof(cg.LoopPreview) == 48
    assert [name for name, _ in cg.LoopPreview._fields_] == [f[1] for f in fields]
    assert [getattr(cg.LoopPreview, name).offset for name, _ in cg.LoopPreview._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]


def test_null_handle_is_refused(lib):
    lv = cg.LoopPreview(struct_size=ctypes.sizeof(cg.LoopPreview), n_samples=1, ts=1.0)
    assert lib.cgmres_hip_closed_loop_device_preview(None, None, None, 3, None, None, None, ctypes.byref(lv)) == -1
    assert b"null handle" in lib.cgmres_hip_last_error()
    assert lib.cgmres_hip_preview_device(None, ctypes.byref(lv), 3, None) == -1
    assert b"null handle" in lib.cgmres_hip_last_error()
    p = cg.Preview(None, 0.5)
    assert (p.ts, p.t0, p.interp, p.per_instance) == (0.5, 0.0, "linear", None)


@pytest.mark.parametrize("interp", ["hold", "linear"])
def test_at_t_zero_every_stage_is_sample_zero(interp):
    """dtau(0) = 0: every stage has tau = 0, and with t0 = 0 every stage equals sig[0] exactly."""
    rng = np.random.default_rng(1)
    sig = rng.normal(size=(5, 9, 2))
    rows = cg.preview_rows(sig, 0.01, 0.0, interp, [0.0], [0.0], 8)
    assert rows.shape == (1, 5, 18)
    assert np.array_equal(rows[0].reshape(5, 9, 2), np.repeat(sig[:, :1], 9, axis=1))
    one = cg.preview_rows(sig[2], 0.01, 0.0, interp, [0.0], [0.0], 8)  # one signal for every instance: no batch axis
    assert one.shape == (1, 18) and np.array_equal(one, rows[:, 2])


def test_linear_mode_reproduces_an_affine_signal():
    """sig = a + b * time, sampled with dyadic constants so that the samples are exact: linear mode returns a + b * tau."""
    ts, t0, dv, ns = 1.0 / 64, -0.25, 50, 400
    a, b = np.array([1.5, -0.75]), np.array([0.25, 3.0])
    grid = t0 + ts * np.arange(ns)
    sig = a[None, :] + b[None, :] * grid[:, None]
    t = np.array([0.0, 0.013, 1.1, 3.7])
    dtau = np.array([0.0, 1e-4, 8.3e-3, 1.7e-2])
    rows = cg.preview_rows(sig, ts, t0, "linear", t, dtau, dv).reshape(len(t), dv + 1, 2)
    tau = t[:, None] + np.arange(dv + 1)[None, :] * dtau[:, None]
    assert tau.max() < grid[-1]  # (no clamp in this case)
    want = a[None, None, :] + b[None, None, :] * tau[:, :, None]
    worst = np.max(np.abs(rows - want))
    lim = bound(sig, tau.max() - t0, ts)
    print(f"affine: max error {worst:.3e}, bound {lim:.3e}")
    assert worst <= lim


def test_hold_mode_returns_sample_values_only():
    rng = np.random.default_rng(2)
    sig = rng.normal(size=(3, 40, 2))
    t, dtau = np.array([0.0, 0.11, 0.52]), np.array([0.0, 0.004, 0.011])
    rows = cg.preview_rows(sig, 0.02, 0.003, "hold", t, dtau, 12).reshape(3, 3, 13, 2)
    for k in range(3):
        for i in range(13):
            s = min(max((t[k] + i * dtau[k] - 0.003) / 0.02, 0.0), 39.0)
            assert np.array_equal(rows[k, :, i], sig[:, int(np.floor(s))]), (k, i)
    lin = cg.preview_rows(sig, 0.02, 0.003, "linear", t, dtau, 12).reshape(3, 3, 13, 2)
    assert np.max(np.abs(lin - rows)) > 1e-3  # (the two modes differ between knots)


@pytest.mark.parametrize("interp", ["hold", "linear"])
def test_one_and_two_samples(interp):
    t, dtau = np.array([0.0, 0.4, 2.0]), np.array([0.0, 0.05, 0.1])
    one = np.array([[0.7, -1.3]])
    rows = cg.preview_rows(one, 0.5, 0.0, interp, t, dtau, 4).reshape(3, 5, 2)
    assert np.array_equal(rows, np.broadcast_to(one, (3, 5, 2)))
    two = np.array([[1.0, 10.0], [3.0, 14.0]])
    rows = cg.preview_rows(two, 0.5, 0.0, interp, t, dtau, 4).reshape(3, 5, 2)
    tau = t[:, None] + np.arange(5)[None, :] * dtau[:, None]
    s = np.clip(tau / 0.5, 0.0, 1.0)
    if interp == "hold":
        want = two[np.floor(s).astype(int)]
    else:
        want = two[0] + s[:, :, None] * (two[1] - two[0])
    assert np.max(np.abs(rows - want)) <= bound(two, tau.max(), 0.5)
    assert np.array_equal(rows[2], np.broadcast_to(two[1], (5, 2)))  # t = 2.0: past the end, the last sample holds


@pytest.mark.parametrize("interp", ["hold", "linear"])
def test_signal_that_ends_mid_horizon(interp):
    """The last sample is at 0.09; the horizon from t = 0.055 with dtau = 0.01 (s = 5.5, 6.5, ...) passes it at stage 4:
    earlier stages follow the signal, later stages hold the last sample."""
    sig = (np.arange(10.0) ** 2)[:, None] * np.array([1.0, -2.0])[None, :]
    rows = cg.preview_rows(sig, 0.01, 0.0, interp, [0.055], [0.01], 8).reshape(9, 2)
    assert np.array_equal(rows[4:], np.broadcast_to(sig[9], (5, 2)))
    for i in range(4):
        w = (0.055 + i * 0.01) / 0.01 - (5 + i)  # 0.5 up to the decimal constants' rounding
        want = sig[5 + i] if interp == "hold" else sig[5 + i] + w * (sig[6 + i] - sig[5 + i])
        assert abs(w - 0.5) < 1e-12 and np.max(np.abs(rows[i] - want)) <= (0.0 if interp == "hold" else bound(sig, 0.1, 0.01)), i
        assert np.max(np.abs(rows[i] - sig[9])) > 1.0, i


@pytest.mark.parametrize("interp", ["hold", "linear"])
def test_t0_ahead_of_t_clamps_at_the_front(interp):
    sig = np.array([[2.0, 5.0], [4.0, 6.0], [8.0, 7.0]])
    rows = cg.preview_rows(sig, 0.1, 0.25, interp, [0.0], [0.1], 4).reshape(5, 2)  # tau = 0, .1, .2, .3, .4; t0 = .25
    assert np.array_equal(rows[:3], np.broadcast_to(sig[0], (3, 2)))  # before t0 the first sample holds
    if interp == "hold":
        assert np.array_equal(rows[3], sig[0]) and np.array_equal(rows[4], sig[1])
    else:
        want = np.array([sig[0] + 0.5 * (sig[1] - sig[0]), sig[1] + 0.5 * (sig[2] - sig[1])])
        assert np.max(np.abs(rows[3:] - want)) <= 64 * EPS * 8.0  # (0.3 - 0.25 and 0.4 - 0.25 are not exact in binary)


def test_rows_keep_the_signals_dtype():
    sig = np.linspace(0, 1, 12, dtype=np.float32).reshape(6, 2)
    rows = cg.preview_rows(sig, 0.1, 0.0, "linear", np.float32([0.05]), np.float32([0.02]), 3)
    assert rows.dtype == np.float32 and rows.shape == (1, 8)
