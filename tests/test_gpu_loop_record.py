"""GPU: the recorded closed loop (cgmres_hip_closed_loop_device_rec) and the ensemble of a batch
(cgmres_hip_ensemble_device).

Record j of a call holds the reference's own output line (<example>/main.cpp:75-82) for tick k = (j+1)*stride - 1: the
state AFTER the plant step (x_{k+1}, the true state under a disturbance), the input u_k that produced it, the solver
status after tick k and the handle's time when tick k's control() ran.  The record is taken between kernel launches, so
the loop is the loop of a caller who cuts it by hand at every recorded tick — bit for bit (G2) — and the rows are the
oracle's (G1).

Shapes: B = 83 = five full 16-instance workgroups and a ragged three; n = 23 / 53 ticks = launch boundaries and a partial
tail at every stride.  Bounds: x, u against the oracle at 1e-9 (tests/test_gpu_loop_inputs.py derives it); the sums of
the ensemble at (n + 4) 2^-52 sum|term| (tests/record_harness.py: check_ensemble), min / max / counts exact."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin
from record_harness import (B, DV, KM, TOL64, Dev, check_ensemble, final_state, krylov_written, new_batch, noise, oracle_rows, run_caller_cut,
                            run_recorded, same_bits, sample_of)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = ("x", "u", "n_ax", "reason")
END = ("x", "u", "U", "dUdt", "n_ax", "reason", "t")


def ramp(c, p, n):
    """The per-instance moving reference of test_moving_reference_with_disturbance_and_noise."""
    stage = np.arange(c.dv + 1)
    seq = np.empty((n, c.batch, c.dv + 1, c.dim_p))
    for k in range(n):
        for i in range(c.batch):
            seq[k, i, :, 0] = p[i, 0] * (1.0 + 0.004 * k) + 0.0007 * stage * (1 + 0.1 * (i % 5))
            seq[k, i, :, 1] = p[i, 1]
    return seq.reshape(n, c.batch, c.dim_p * (c.dv + 1))


# ---- G1. every tick against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("model,variant", [(0, 2), (1, 2), (2, 2), (0, 3), (0, 4), (0, 1)])
def test_every_recorded_tick_against_the_oracle(orc, model, variant):
    n = 23
    c, x0, u0, p = new_batch(orc, model, tol=1e-6, variant=variant)
    assert c.variant == variant
    d, v = noise(n, B, c.dim_x)
    log, end = run_recorded(c, x0, n, 1, d, v)
    assert log["x"].shape == (n, B, c.dim_x) and log["u"].shape == (n, B, c.dim_u)
    assert np.max(np.abs(log["t"] - np.arange(n) * c.dt)) <= 1e-12
    assert np.array_equal(log["x"][-1], end["x"]) and np.array_equal(log["u"][-1], end["u"])
    sample = sample_of(B)
    assert len(sample) >= 14 and {15, 16, B - 1} <= set(sample)
    worst = 0.0
    for i in sample:
        xo, uo, ko, wo = oracle_rows(orc, model, x0, u0, p, i, n, d[:, i], v[:, i])
        ex, eu = np.max(np.abs(log["x"][:, i] - xo)), np.max(np.abs(log["u"][:, i] - uo))
        worst = max(worst, ex, eu)
        assert ex <= TOL64 and eu <= TOL64, (i, ex, eu)
        assert np.array_equal(log["n_ax"][:, i], ko) and np.array_equal(log["reason"][:, i], wo), i
    print(f"max |gpu - oracle| over every row of {len(sample)} instances: {worst:.3e}")
    c.close()


# ---- G2. bit identity with the loop cut by the caller -----------------------------------------------------------------
@pytest.mark.parametrize("stride,with_ptau", [(1, False), (4, False), (4, True), (10, False), (25, False)])
@pytest.mark.parametrize("variant", [2, 4])
def test_recorded_loop_is_the_loop_cut_by_the_caller(orc, variant, stride, with_ptau):
    n, outs = 53, []
    for run in (run_recorded, run_caller_cut):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        d, v = noise(n, B, c.dim_x)
        seq = ramp(c, p, n) if with_ptau else None
        outs.append(run(c, x0, n, stride, d, v, seq))
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    assert log_a["x"].shape[0] == n // stride
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)


# ---- G3. no record == closed_loop_device_ex ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 4])
def test_null_and_empty_record_are_closed_loop_device_ex(orc, variant):
    n, outs = 23, []
    for how in ("ex", "null", "empty"):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        d, v = noise(n, B, c.dim_x)
        dev = Dev(c)
        xd, ud, dd, vd = dev(x0), dev(np.zeros((B, c.dim_u))), dev(d), dev(v)
        if how == "ex":
            c.closed_loop_device(xd, ud, n, dist_seq_dev=dd, meas_seq_dev=vd)
        else:
            li = c._loop_inputs(n, None, True, dd, vd, True, True)
            rec = cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=3)  # every output NULL
            cg._check(cg.load().cgmres_hip_closed_loop_device_rec(c._h, xd.ptr, ud.ptr, n, ctypes.byref(li),
                                                                  ctypes.byref(rec) if how == "empty" else None))
        outs.append(final_state(c, xd, ud))
        dev.free(), c.close()
    for other in outs[1:]:
        same_bits(outs[0], other, END)


# ---- G4. the ensemble kernel on hand-made data ------------------------------------------------------------------------
def hand_made(batch, nx, nu, dtype):
    rng = np.random.default_rng(11)
    scale = 10.0 ** np.linspace(-3, 3, nx + nu)
    offset = np.array([(-1) ** c * 3.7 * scale[(c + 2) % (nx + nu)] for c in range(nx + nu)])
    rows = (offset + scale * rng.normal(size=(batch, nx + nu))).astype(dtype)
    return np.ascontiguousarray(rows[:, :nx]), np.ascontiguousarray(rows[:, nx:])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 83, 3 * cg.RECORD_BLOCK + 5])
def test_ensemble_of_hand_made_rows(orc, batch, dtype):
    c, x0, u0, p = new_batch(orc, 0, batch=batch, dtype=dtype)
    c.control(x0)  # one tick, so the status is real
    n_ax, reason = c.get_status()
    x, u = hand_made(batch, c.dim_x, c.dim_u, c.np_dtype)
    rows = np.concatenate([x, u], axis=1).astype(np.float64)
    dev = Dev(c)
    xd, ud = dev(x), dev(u)
    for centre in (None, np.median(rows, axis=0)):
        md, cd = dev(shape=(c.dim_x + c.dim_u, 4), dtype=np.float64), dev(shape=(c.k_max + 7,), dtype=np.int32)
        c.ensemble_device(xd, ud, moments=md, counts=cd, centre=dev(centre))
        c.synchronize()
        check_ensemble(md.download(), cd.download(), x, u, n_ax, reason, c.k_max, centre)
    cd = dev(shape=(c.k_max + 7,), dtype=np.int32)  # counts alone
    c.ensemble_device(xd, ud, counts=cd)
    assert cd.download()[c.k_max + 6] == batch and cd.download()[:c.k_max + 1].sum() == batch
    dev.free(), c.close()


# ---- G5 / G6. non-finite rows; determinism ------------------------------------------------------------------------------
def nan_scene(orc, logs=True):
    n, bad = 12, 21
    c, x0, u0, p = new_batch(orc, 0, variant=2)
    d, v = noise(n, B, c.dim_x)
    d[3, bad, 1] = np.nan
    centre = np.concatenate([np.median(x0, axis=0), np.zeros(c.dim_u)])
    log, _ = run_recorded(c, x0, n, 1, d, v, centre=centre, logs=logs)
    c.close()
    return log, centre, n, bad


@pytest.fixture(scope="module")
def nan_log(orc):
    return nan_scene(orc)


def test_non_finite_rows_leave_the_ensemble(nan_log):
    log, centre, n, bad = nan_log
    km = KM
    for j in range(n):
        assert np.all(np.isfinite(log["x"][j, bad])) == (j < 3), j
        assert log["counts"][j, km + 6] == (B if j < 3 else B - 1), j
        assert log["counts"][j, km + 1 + cg.EXIT_NONFINITE] == np.sum(log["reason"][j] == cg.EXIT_NONFINITE), j
        check_ensemble(log["moments"][j], log["counts"][j], log["x"][j], log["u"][j], log["n_ax"][j], log["reason"][j], km, centre)
    flagged = [j for j in range(n) if log["reason"][j, bad] == cg.EXIT_NONFINITE]
    assert flagged and flagged == list(range(flagged[0], n))  # from the record that shows it on
    assert np.all(log["counts"][flagged[0]:, km + 1 + cg.EXIT_NONFINITE] == 1)
    assert np.all(log["counts"][:flagged[0], km + 1 + cg.EXIT_NONFINITE] == 0)


def test_ensemble_bits_are_reproducible(orc, nan_log):
    log = nan_log[0]
    again = nan_scene(orc)[0]
    assert log["moments"].tobytes() == again["moments"].tobytes() and np.array_equal(log["counts"], again["counts"])
    alone = nan_scene(orc, logs=False)[0]  # only the ensemble pointers given
    assert "x" not in alone
    assert log["moments"].tobytes() == alone["moments"].tobytes() and np.array_equal(log["counts"], alone["counts"])


# ---- G7. placement: the log rows follow the instance -----------------------------------------------------------------
def test_rows_follow_the_instance_under_binned_placement(orc):
    model, batch, n, stride = 0, 8300, 25, 5  # the lean plan, 519 workgroups: re-placed before the second and third launch
    d, v = noise(n, batch, 4)
    outs = []
    for flags in (0, cg.FLAG_NO_BINNING):
        c, x0, u0, p = new_batch(orc, model, batch=batch, tol=1e-6, flags=flags)
        assert c.variant == 3
        log, _ = run_recorded(c, x0, n, stride, d, v)
        outs.append(log)
        if flags == 0:
            sample = sample_of(batch)
            assert len(sample) >= 14
            for i in sample:
                xo, uo, ko, wo = oracle_rows(orc, model, x0, u0, p, i, n, d[:, i], v[:, i])
                assert np.max(np.abs(log["x"][-1, i] - xo[-1])) <= TOL64 and np.max(np.abs(log["u"][-1, i] - uo[-1])) <= TOL64, i
                assert log["n_ax"][-1, i] == ko[-1]
            assert np.array_equal(log["counts"][:, :KM + 1], [np.bincount(r, minlength=KM + 1) for r in log["n_ax"]])
        c.close()
    a, b = outs
    assert a["x"].shape == (n // stride, batch, 4)
    # (the noise takes the batch out of the slow phase in which placement is bit-neutral: agreement to rounding only)
    assert np.max(np.abs(a["x"] - b["x"])) <= 1e-12 and np.max(np.abs(a["u"] - b["u"])) <= 1e-12


# ---- G8. fp32 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 3])
def test_fp32_recorded_loop_is_the_loop_cut_by_the_caller(orc, variant):
    batch, dv, km, n, stride = 40, 100, 20, 53, 4
    outs = []
    for run in (run_recorded, run_caller_cut):
        c, x0, u0, p = new_batch(orc, 0, batch=batch, dv=dv, km=km, variant=variant, dtype="f32")
        assert c.variant == variant
        d, v = noise(n, batch, 4, np.float32)
        outs.append(run(c, x0, n, stride, d, v))
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    assert log_a["x"].dtype == np.float32 and log_a["x"].shape == (n // stride, batch, 4)
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)


# ---- G9. user model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 1, 4])
def test_user_model_logs_equal_the_caller_cut_loop(variant):
    """The record kernel is the library's, not the plugin's: the plugin file holds no record kernel (its text is searched),
    the library does, and the plugin is the one build() made — registering it compiles nothing."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    header = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
    path = plugin.build(header, cls="VdpModel", name="vdp")
    stamp = os.path.getmtime(path)
    assert b"record_kernel" not in open(path, "rb").read() and b"record_kernel" in open(cg.lib_path(), "rb").read()
    mid = plugin.register(path)
    batch, n = 20, 12
    b = np.arange(batch, dtype=np.float64)
    x0 = np.stack([1.0 + 0.03 * b, -0.5 + 0.02 * b], axis=1)
    p = np.stack([0.05 * b, 0.05 * (np.arange(batch) % 3)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (batch, 1))
    d, v = noise(n, batch, 2)
    outs = []
    for run in (run_recorded, run_caller_cut):
        c = cg.CgmresBatch(mid, batch=batch, variant=variant)
        assert c.variant == variant
        c.set_ptau_repeat(p)
        c.init_u0(u0)
        c.init_u0_newton(u0, x0, p, 10)
        outs.append(run(c, x0, n, 1, d, v))
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)
    assert np.max(np.abs(log_a["x"][-1] - x0)) > 1e-4  # (the loop ran)
    for j in range(n):
        check_ensemble(log_a["moments"][j], log_a["counts"][j], log_a["x"][j], log_a["u"][j], log_a["n_ax"][j], log_a["reason"][j], c.k_max)
    assert os.path.getmtime(path) == stamp


# ---- G10. the ensemble leaves the handle alone ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 4, 1])
def test_ensemble_leaves_the_handle_alone(orc, variant):
    outs = []
    for with_ensemble in (False, True):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        dev = Dev(c)
        u1 = c.control(x0)
        if with_ensemble:
            md, cd = dev(shape=(c.dim_x + c.dim_u, 4), dtype=np.float64), dev(shape=(c.k_max + 7,), dtype=np.int32)
            c.ensemble_device(dev(x0), dev(u1), moments=md, counts=cd)
            c.synchronize()
            assert cd.download()[c.k_max + 6] == B
        u2 = c.control(x0 + 1e-3)
        t, U, dUdt = c.get_state()
        outs.append((u1, u2, U, dUdt, np.concatenate(krylov_written(c)), c.get_status()[0], c.get_status()[1], np.float64(t)))
        dev.free(), c.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- G11. validation ------------------------------------------------------------------------------------------------------
def test_validation(orc):
    c, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    lib, dev = cg.load(), Dev(c)
    xd, ud = dev(x0), dev(np.zeros((20, 3)))
    dd = dev(np.zeros((5, 20, 4)))
    xl = dev(shape=(5 * 20 * 7,))  # room for the x log and, right behind it, the u log
    kl = dev(shape=(5, 20), dtype=np.int32)
    size, isize = ctypes.sizeof(cg.LoopRecord), ctypes.sizeof(cg.LoopInputs)

    def call(n, x=xd.ptr, u=ud.ptr, seq=None, **fields):
        rec = cg.LoopRecord(**dict(dict(struct_size=size, stride=1, x_log_dev=xl.ptr), **fields))
        li = cg.LoopInputs(struct_size=isize, dist_per_instance=1, dist_seq_dev=seq)
        cg._check(lib.cgmres_hip_closed_loop_device_rec(c._h, x, u, n, ctypes.byref(li), ctypes.byref(rec)))
    with pytest.raises(cg.CgmresHipError, match="struct_size .* cgmres_hip_loop_record"):
        call(5, struct_size=size - 8)
    with pytest.raises(cg.CgmresHipError, match="reserved"):
        call(5, reserved=(ctypes.c_int32 * 2)(0, 1))
    with pytest.raises(cg.CgmresHipError, match="stride 0 < 1"):
        call(5, stride=0)
    with pytest.raises(cg.CgmresHipError, match="n_ticks"):
        call(-1)
    with pytest.raises(cg.CgmresHipError, match="null x_dev"):
        call(5, x=None)
    with pytest.raises(cg.CgmresHipError, match="null u_dev"):
        call(5, u=None)
    with pytest.raises(cg.CgmresHipError, match="x_log_dev overlaps x_dev"):
        call(5, x_log_dev=xd.ptr)
    with pytest.raises(cg.CgmresHipError, match="u_log_dev overlaps u_dev"):
        call(5, u_log_dev=ud.ptr + 8)
    with pytest.raises(cg.CgmresHipError, match="x_log_dev overlaps u_log_dev"):
        call(5, u_log_dev=xl.ptr + 5 * 20 * 4 * 8 - 8)
    with pytest.raises(cg.CgmresHipError, match="n_ax_log_dev overlaps dist_seq_dev"):
        call(5, seq=dd.ptr, n_ax_log_dev=dd.ptr + 16)
    call(5, u_log_dev=xl.ptr + 5 * 20 * 4 * 8)  # (adjacent is not overlapping: the last byte of one, the first of the next)
    c.synchronize()
    # the ensemble entry point
    out_size = ctypes.sizeof(cg.EnsembleOut)

    def ens(x=xd.ptr, u=ud.ptr, **fields):
        out = cg.EnsembleOut(**dict(dict(struct_size=out_size, counts_dev=kl.ptr), **fields))
        cg._check(lib.cgmres_hip_ensemble_device(c._h, x, u, ctypes.byref(out)))
    with pytest.raises(cg.CgmresHipError, match="struct_size .* cgmres_hip_ensemble_out"):
        ens(struct_size=out_size + 8)
    with pytest.raises(cg.CgmresHipError, match="reserved"):
        ens(reserved=3)
    with pytest.raises(cg.CgmresHipError, match="null x_dev"):
        ens(x=None)
    with pytest.raises(cg.CgmresHipError, match="null u_dev"):
        ens(u=None)
    with pytest.raises(cg.CgmresHipError, match="no output wanted"):
        ens(counts_dev=None)
    with pytest.raises(cg.CgmresHipError, match="null out"):
        cg._check(lib.cgmres_hip_ensemble_device(c._h, xd.ptr, ud.ptr, None))
    # n_ticks == 0 touches nothing
    c2, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    d2 = Dev(c2)
    xd2, ud2, log2 = d2(x0), d2(np.zeros((20, 3))), d2(np.full((1, 20, 4), 7.0))
    t = np.full(1, 7.0)
    c2.closed_loop_device(xd2, ud2, 0, record=dict(stride=1, t=np.empty(0)))
    rec = cg.LoopRecord(struct_size=size, stride=1, x_log_dev=log2.ptr, t_host=t.ctypes.data)
    cg._check(lib.cgmres_hip_closed_loop_device_rec(c2._h, xd2.ptr, ud2.ptr, 0, None, ctypes.byref(rec)))
    c2.synchronize()
    assert np.array_equal(xd2.download(), x0) and c2.t == 0.0 and np.all(log2.download() == 7.0) and t[0] == 7.0
    # the binding checks element type and count of a typed buffer before its address crosses the ABI
    with pytest.raises(ValueError):
        c2.closed_loop_device(xd2, ud2, 6, record=dict(stride=2, x=log2))  # 3 records need [3, 20, 4]
    with pytest.raises(TypeError):
        c2.closed_loop_device(xd2, ud2, 1, record=dict(stride=1, n_ax=d2(shape=(1, 20), dtype=np.float64)))
    with pytest.raises(TypeError):
        c2.closed_loop_device(xd2, ud2, 1, record=dict(stride=1, t=np.zeros(1, dtype=np.float32)))
    with pytest.raises(ValueError):
        c2.ensemble_device(xd2, ud2, counts=d2(shape=(c2.k_max + 6,), dtype=np.int32))
    with pytest.raises(cg.CgmresHipError, match="stride"):
        c2.closed_loop_device(xd2, ud2, 6, record=dict(stride=0, x=log2))
    assert c2.t == 0.0
    d2.free(), c2.close()
    dev.free(), c.close()


def test_plugin_built_before_the_record_is_told_to_rebuild():
    """A plugin whose contexts predate the record (imitated with -DCGM_PLUGIN_WITHOUT_RECORD, as the horizon's): the two
    entry points refuse it with the advice to rebuild; everything else of it keeps working."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    header = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
    mid = plugin.register(plugin.build(header, cls="VdpModel", name="vdp_norecord", extra_flags=("-DCGM_PLUGIN_WITHOUT_RECORD",)))
    c = cg.CgmresBatch(mid, batch=4)
    dev = Dev(c)
    xd, ud, cd = dev(np.ones((4, 2))), dev(np.zeros((4, 3))), dev(shape=(c.k_max + 7,), dtype=np.int32)
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.ensemble_device(xd, ud, counts=cd)
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.closed_loop_device(xd, ud, 2, record=dict(stride=1, t=np.zeros(2)))
    assert c.t == 0.0
    c.closed_loop_device(xd, ud, 2)
    c.synchronize()
    assert c.t > 0.0
    dev.free(), c.close()


def test_closed_loop_record_convenience(orc):
    c, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    d, v = noise(12, 20, 4)
    out = c.closed_loop_record(x0, 12, stride=5, dist_seq=d, meas_seq=v)
    assert sorted(out) == ["counts", "moments", "n_ax", "reason", "t", "u", "u_end", "x", "x_end"]
    assert out["x"].shape == (2, 20, 4) and out["moments"].shape == (2, 7, 4) and out["counts"].shape == (2, KM + 7)
    assert np.allclose(out["t"], [4 * c.dt, 9 * c.dt], rtol=0, atol=1e-12) and abs(c.t - 12 * c.dt) <= 1e-12
    c.close()
    c, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    log, end = run_recorded(c, x0, 12, 5, d, v)
    c.close()
    same_bits(out, log, LOGS + ("moments", "counts"))
    assert np.array_equal(out["x_end"], end["x"]) and np.array_equal(out["u_end"], end["u"])


# ---- G12. the C++ overloads ---------------------------------------------------------------------------------------------
def test_cpp_overloads_equal_the_c_calls(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib_dir = os.path.join(ROOT, "cgmres_cpp_amd", "lib")
    exe = tmp_path / "loop_record_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "loop_record_main.cpp"),
                    f"-L{lib_dir}", f"-Wl,-rpath,{lib_dir}", "-lcgmres_hip", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    words = out.split()
    assert words[0] == "max_diff" and float(words[1]) == 0.0, out
    assert float(words[3]) > 1e-4, out  # (the loop ran: the state moved)
    assert float(words[5]) == 20 and abs(float(words[7]) - 0.011) <= 1e-12, out


# ---- G13. the example program's device loop ---------------------------------------------------------------------------
def _read_traj(path):
    return np.array([[float(t) for t in line.split("\t")] for line in open(path) if line.strip()])


def test_example_program_device_loop_reproduces_reference_loop(tmp_path):
    """closed_loop pendulum 1000 --device-loop: the comparison test_example_program_reproduces_reference_loop (test_facade.py)
    applies to the default mode — the reference's own closed loop (golden loop_u / loop_x, shipped sizes), 6 printed decimals."""
    from conftest import GOLDEN_DIR, load_golden
    build_dir = os.path.join(ROOT, "examples", "_build")
    exe = os.path.join(build_dir, "closed_loop")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    g = load_golden(os.path.join(GOLDEN_DIR, "pendulum_dv25_k5_tolref_f64.npz"))
    prefix = str(tmp_path / "pendulum")
    r = subprocess.run([exe, "pendulum", "1000", prefix, "--device-loop"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Elapsed time = " in r.stdout
    u, x = _read_traj(prefix + "_u.txt"), _read_traj(prefix + "_x.txt")
    assert u.shape == (1000, 1 + 3) and x.shape == (1000, 1 + 4)
    np.testing.assert_allclose(u[:, 0], 0.001 * np.arange(1000), atol=1e-9)
    np.testing.assert_allclose(x[:, 0], 0.001 * np.arange(1000), atol=1e-9)
    rows = min(1000, len(g["loop_u"]))
    assert rows >= 100
    assert np.max(np.abs(u[:rows, 1:] - g["loop_u"][:rows])) <= 1.5e-6   # 6 printed decimals
    assert np.max(np.abs(x[:rows, 1:] - g["loop_x"][:rows])) <= 1.5e-6
