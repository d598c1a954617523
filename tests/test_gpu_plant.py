"""GPU: the plant of a closed loop — cgmres_hip_plant_step_device (the kernel alone) and
cgmres_hip_closed_loop_device_plant (the loop: one tick per launch, the plant kernel behind every launch).

K. the kernel alone against the numpy plant (tests/plant_harness.py) in fp64 from the same rounded inputs.  Bound:
   4 * substeps * eps_T * max(1, |x|_inf) per instance — each substep ends in one add into x, so device and reference
   round by at most half an ulp each per substep; the errors of f enter scaled by dt/substeps <= 1e-3, and the factor 4
   covers them and the device's <= 2-ulp trig.
O. the loop against the oracle driven tick by tick with y_k = x_k + v_k, u_k = control(y_k), x_{k+1} = Phi(x_k, u_k) + d_k:
   x, u at 1e-9 (TOL64, the project's bound), equal Arnoldi counts and reasons; fp32 at 1e-4.  RK4/4 against Euler/1 moves x
   by >= 1.4e-5 and the theta draw by >= 3e-4 over the loop: a plant that ignores theta, substeps or the integrator
   fails by four orders of magnitude.
S. the loop against itself, bit for bit.
R. what is refused.
Shapes follow tests/record_harness.py: B = 83, dv = 50, k_max = 10, n = 23, sigma = 1e-3, the seeded generators there."""
import ctypes
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
import plant_harness as ph
from cgmres_cpp_amd import plugin
from record_harness import B, DV, KM, TOL64, Dev, final_state, new_batch, noise, run_recorded, same_bits, sample_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 23
LOGS = ("x", "u", "n_ax", "reason")
END = ("x", "u", "U", "dUdt", "n_ax", "reason", "t")
SHAPES = os.path.join(ROOT, "tests", "user_models", "shape_models.hpp")


def ramp(c, p, n):
    """A per-instance moving reference (the one of tests/test_gpu_loop_record.py)."""
    stage = np.arange(c.dv + 1)
    seq = np.empty((n, c.batch, c.dv + 1, c.dim_p))
    for k in range(n):
        for i in range(c.batch):
            seq[k, i, :, 0] = p[i, 0] * (1.0 + 0.004 * k) + 0.0007 * stage * (1 + 0.1 * (i % 5))
            seq[k, i, :, 1] = p[i, 1]
    return seq.reshape(n, c.batch, c.dim_p * (c.dv + 1))


# ---- K. the kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 83, 3 * 256 + 5])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_plant_step_against_the_numpy_plant(orc, model, dtype, batch):
    c, x0, u0, p = new_batch(orc, model, batch=batch, dtype=dtype)
    T = c.np_dtype
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(11)
    th_inst = ph.theta_draw(model, batch, T)
    x = rng.uniform(-4, 4, (batch, c.dim_x)).astype(T)
    u = rng.uniform(-3, 3, (batch, c.dim_u)).astype(T)
    dev = Dev(c)
    ud, th_b, th_i = dev(u), dev(th_inst[0]), dev(th_inst)
    c.control(x0)  # a controller state worth comparing
    before = (c.get_state(), c.get_status())
    worst = 0.0
    for integrator in ("euler", "rk4"):
        for substeps in (1, 4, 7):
            for mode, th_dev, th in (("absent", None, np.tile(ph.NOMINAL[model].astype(T), (batch, 1))),
                                     ("broadcast", th_b, np.tile(th_inst[0], (batch, 1))), ("per instance", th_i, th_inst)):
                xd = dev(x)
                c.plant_step_device(xd, ud, cg.Plant(integrator, substeps, th_dev))
                got = xd.download().astype(np.float64)
                ref = ph.plant(model, x.astype(np.float64), u.astype(np.float64), th.astype(np.float64), integrator, substeps,
                               float(T(c.dt)))
                unit = 4 * substeps * eps * np.maximum(1.0, np.max(np.abs(ref), axis=1, keepdims=True))
                ratio = float(np.max(np.abs(got - ref) / unit))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (integrator, substeps, mode, ratio)
    print(f"model {model} {dtype} B = {batch}: max |gpu - numpy| / (4 substeps eps max(1, |x|)) = {worst:.3f}")
    assert np.array_equal(ud.download(), u)  # u_dev and the controller state are untouched
    after = (c.get_state(), c.get_status())
    assert before[0][0] == after[0][0] and all(np.array_equal(a, b) for a, b in zip(before[0][1:] + before[1], after[0][1:] + after[1]))
    dev.free(), c.close()


# ---- O. the loop against the oracle -------------------------------------------------------------------------------------
def run_plant_loop(c, x0, n, plant, d=None, v=None, seq=None, stride=0, theta=None):
    """closed_loop_device(plant=...) -> (logs or None, final state); theta: host array uploaded here."""
    dev = Dev(c)
    T = c.np_dtype
    xd, ud = dev(x0.astype(T)), dev(np.zeros((c.batch, c.dim_u), dtype=T))
    if theta is not None:
        plant = cg.Plant(plant.integrator, plant.substeps, dev(np.asarray(theta, dtype=T)))
    rec = None
    if stride:
        n_rec = n // stride
        rec = dict(stride=stride, t=np.full(n_rec, np.nan), x=dev(shape=(n_rec, c.batch, c.dim_x)), u=dev(shape=(n_rec, c.batch, c.dim_u)),
                   n_ax=dev(shape=(n_rec, c.batch), dtype=np.int32), reason=dev(shape=(n_rec, c.batch), dtype=np.int32))
    cast = lambda a: None if a is None else dev(np.asarray(a, dtype=T))
    c.closed_loop_device(xd, ud, n, cast(seq), True, dist_seq_dev=cast(d), meas_seq_dev=cast(v), record=rec, plant=plant)
    end = final_state(c, xd, ud)
    log = None
    if rec:
        log = {k: rec[k].download() for k in LOGS}
        log["t"] = rec["t"]
    dev.free()
    return log, end


@pytest.mark.parametrize("model,variant,flags,name,with_seq,dtype", [
    (0, 2, 0, "wg+row-newton", False, "f64"), (0, 2, 0, "wg+row-newton", True, "f64"),
    (0, 2, cg.FLAG_SERIAL_STATE_SWEEP, None, True, "f64"), (0, 4, 0, "wave", True, "f64"), (0, 1, 0, "lane", True, "f64"),
    (1, 2, 0, None, False, "f64"), (2, 2, 0, None, False, "f64"), (0, 2, 0, None, False, "f32")])
def test_plant_loop_against_the_oracle(orc, model, variant, flags, name, with_seq, dtype):
    c, x0, u0, p = new_batch(orc, model, variant=variant, flags=flags, dtype=dtype)
    assert c.variant == variant and (name is None or c.variant_name == name), c.variant_name
    if flags:
        assert c.variant_name != "wg+row-newton"
    T = c.np_dtype
    d, v = noise(N, B, c.dim_x, T)
    seq = ramp(c, p, N).astype(T) if with_seq else None
    th = ph.theta_draw(model, B, T)
    x0 = x0.astype(T)
    log, end = run_plant_loop(c, x0, N, cg.Plant("rk4", 4), d, v, seq, stride=1, theta=th)
    assert np.array_equal(log["x"][-1], end["x"]) and np.array_equal(log["u"][-1], end["u"])
    assert abs(end["t"] - N * c.dt) <= (1e-6 if dtype == "f32" else 1e-12)
    assert np.max(np.abs(log["t"] - np.arange(N) * c.dt)) <= (1e-6 if dtype == "f32" else 1e-12)
    u_next = c.control(end["x"])  # one more plain tick: plant, sequences and y are gone from the handle
    bound = 1e-4 if dtype == "f32" else TOL64
    sample = sample_of(B)
    assert len(sample) >= 14 and {15, 16, B - 1} <= set(sample)
    worst = 0.0
    for i in sample:
        xo, uo, ko, wo, r = ph.oracle_plant_rows(orc, model, x0.astype(np.float64), u0, p, i, N, th[i], "rk4", 4, d[:, i], v[:, i],
                                                 None if seq is None else seq[:, i], dtype=dtype)
        ex, eu = np.max(np.abs(log["x"][:, i] - xo)), np.max(np.abs(log["u"][:, i] - uo))
        worst = max(worst, ex, eu)
        assert ex <= bound and eu <= bound, (i, ex, eu)
        assert np.all(np.isfinite(xo)) and ko.max() <= KM, (i, ko)
        if dtype == "f64":
            assert np.array_equal(log["n_ax"][:, i], ko) and np.array_equal(log["reason"][:, i], wo), i
        assert np.max(np.abs(u_next[i] - r.control(end["x"][i]))) <= bound, i
    print(f"max |gpu - oracle| over every tick of {len(sample)} instances: {worst:.3e}")
    c.close()


# ---- S. the loop against itself, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 4, 1])
def test_null_plant_is_closed_loop_device_rec(orc, variant):
    outs = []
    for how in ("rec", "plant"):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        d, v = noise(N, B, c.dim_x)
        dev = Dev(c)
        xd, ud, dd, vd = dev(x0), dev(np.zeros((B, c.dim_u))), dev(d), dev(v)
        xl = dev(shape=(N // 4, B, c.dim_x))
        li = c._loop_inputs(N, None, True, dd, vd, True, True)
        rec = cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=4, x_log_dev=xl.ptr)
        if how == "rec":
            cg._check(cg.load().cgmres_hip_closed_loop_device_rec(c._h, xd.ptr, ud.ptr, N, ctypes.byref(li), ctypes.byref(rec)))
        else:
            cg._check(cg.load().cgmres_hip_closed_loop_device_plant(c._h, xd.ptr, ud.ptr, N, ctypes.byref(li), ctypes.byref(rec), None))
        end = final_state(c, xd, ud)
        end["log"] = xl.download()
        outs.append(end)
        dev.free(), c.close()
    same_bits(outs[0], outs[1], END + ("log",))


def caller_loop(c, x0, n, plant, seq=None, theta=None, cut=0):
    """The caller's own loop: control_device + plant_step_device per tick (set_ptau before it where a sequence is given);
    cut > 0: x, u and the status downloaded behind every cut-th tick.  -> (logs, final state)"""
    dev = Dev(c)
    xd, ud = dev(x0), dev(np.zeros((c.batch, c.dim_u)))
    if theta is not None:
        plant = cg.Plant(plant.integrator, plant.substeps, dev(theta))
    log = dict(x=[], u=[], n_ax=[], reason=[])
    for k in range(n):
        if seq is not None:
            c.set_ptau(seq[k])
        c.control_device(ud, xd)
        c.plant_step_device(xd, ud, plant)
        if cut and (k + 1) % cut == 0:
            c.synchronize()
            n_ax, reason = c.get_status()
            log["x"].append(xd.download()), log["u"].append(ud.download()), log["n_ax"].append(n_ax), log["reason"].append(reason)
    end = final_state(c, xd, ud)
    dev.free()
    return {k: np.array(a) for k, a in log.items()}, end


@pytest.mark.parametrize("model,variant", [(0, 2), (0, 4), (0, 1), (1, 2), (2, 2)])
def test_plant_loop_is_the_callers_loop_of_control_and_plant_step(orc, model, variant):
    outs = []
    for how in ("loop", "caller"):
        c, x0, u0, p = new_batch(orc, model, variant=variant)
        th = ph.theta_draw(model, B)
        if how == "loop":
            outs.append(run_plant_loop(c, x0, N, cg.Plant("rk4", 4), stride=4, theta=th))
        else:
            outs.append(caller_loop(c, x0, N, cg.Plant("rk4", 4), theta=th, cut=4))
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    assert log_a["x"].shape == (N // 4, B, ph.DIMS[model][0])
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)
    assert np.max(np.abs(end_a["x"] - x0)) > 1e-4  # (the loop ran)


@pytest.mark.parametrize("variant", [2, 4])
def test_recorded_plant_loop_is_the_plant_loop_cut_by_the_caller(orc, variant):
    """Stride 4, with d, v and a ptau sequence: the recorded loop against the same entry point called once per stride
    window with the sequences offset, in all logs and in the final state."""
    n, stride, outs = N, 4, []
    for how in ("recorded", "cut"):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        d, v = noise(n, B, c.dim_x)
        seq, th = ramp(c, p, n), ph.theta_draw(0, B)
        if how == "recorded":
            outs.append(run_plant_loop(c, x0, n, cg.Plant("rk4", 4), d, v, seq, stride=stride, theta=th))
        else:
            dev = Dev(c)
            xd, ud, thd = dev(x0), dev(np.zeros((B, c.dim_u))), dev(th)
            log = dict(x=[], u=[], n_ax=[], reason=[])
            for k0 in list(range(0, n - n % stride, stride)) + ([n - n % stride] if n % stride else []):
                k1 = min(k0 + stride, n)
                w = Dev(c)
                c.closed_loop_device(xd, ud, k1 - k0, w(seq[k0:k1]), True, dist_seq_dev=w(d[k0:k1]), meas_seq_dev=w(v[k0:k1]),
                                     plant=cg.Plant("rk4", 4, thd))
                c.synchronize()
                w.free()
                if k1 - k0 == stride:
                    n_ax, reason = c.get_status()
                    log["x"].append(xd.download()), log["u"].append(ud.download()), log["n_ax"].append(n_ax), log["reason"].append(reason)
            outs.append(({k: np.array(a) for k, a in log.items()}, final_state(c, xd, ud)))
            dev.free()
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    assert log_a["x"].shape[0] == n // stride
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)


def test_two_plant_loops_from_one_state_agree_bit_for_bit(orc):
    outs = []
    for _ in range(2):
        c, x0, u0, p = new_batch(orc, 0, variant=2)
        d, v = noise(N, B, c.dim_x)
        outs.append(run_plant_loop(c, x0, N, cg.Plant("rk4", 7), d, v, stride=1, theta=ph.theta_draw(0, B)))
        c.close()
    same_bits(outs[0][0], outs[1][0], LOGS)
    same_bits(outs[0][1], outs[1][1], END)


def test_euler_one_step_nominal_plant_loop_against_the_fused_loop(orc):
    """Euler, one substep, nominal theta is the plant of the fused loop: the two loops agree to the project's bound (the
    launches differ — one tick each against ten — so bits are not asked for)."""
    c, x0, u0, p = new_batch(orc, 0, variant=2)
    d, v = noise(N, B, c.dim_x)
    _, a = run_plant_loop(c, x0, N, cg.Plant("euler", 1), d, v)
    c.close()
    c, x0, u0, p = new_batch(orc, 0, variant=2)
    _, b = run_recorded(c, x0, N, 1, d, v)
    c.close()
    assert np.max(np.abs(a["x"] - b["x"])) <= TOL64 and np.max(np.abs(a["u"] - b["u"])) <= TOL64
    assert np.array_equal(a["n_ax"], b["n_ax"]) and a["t"] == b["t"]


# ---- a user model whose dxdt reads p --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 1])
def test_user_model_plant_reads_p_of_stage_0(variant):
    """tests/user_models/shape_models.hpp, alias (3, 2, 1), RK4 with 4 substeps.  Its oracle executable runs a closed loop of
    its own and cannot be driven with an external plant, so the loop is held to the caller-driven loop (bit for bit, with a
    ptau sequence: p is row k's stage 0) and the kernel alone to the numpy plant with the handle's p."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    mid = plugin.register(plugin.build(SHAPES, cls="Shape321", name="shape321"))
    assert cg.plant_info(mid)["n_theta"] == 0
    batch, n, dv = 20, 12, 30
    b = np.arange(batch)[:, None]
    x0, u0, p = 0.3 + 0.05 * b - 0.11 * np.arange(3)[None, :], np.full((batch, 2), 0.1), 0.2 + 0.03 * b + 0.01 * np.arange(1)[None, :]
    stage = np.arange(dv + 1)
    seq = np.stack([p * (1.0 + 0.01 * k) + 0.002 * stage[None, :] for k in range(n)])  # [n, batch, dv+1]; stage 0 differs per tick
    plant = cg.Plant("rk4", 4)

    def fresh():
        c = cg.CgmresBatch(mid, batch=batch, variant=variant)
        assert c.variant == variant and c.dv == dv
        c.set_ptau_repeat(p)
        c.init_u0(u0)
        c.init_u0_newton(u0, x0, p, 10)
        return c
    # the kernel alone: p is stage 0 of the handle's ptau, per instance
    c = fresh()
    c.set_ptau(seq[3])
    dev = Dev(c)
    u = np.random.default_rng(11).uniform(-3, 3, (batch, 2))
    xd, ud = dev(x0), dev(u)
    c.plant_step_device(xd, ud, plant)
    ref = ph.integrate(lambda z: ph.shape321_rhs(z, u, seq[3][:, :1]), x0, "rk4", 4, c.dt)
    unit = 4 * 4 * np.finfo(np.float64).eps * np.maximum(1.0, np.max(np.abs(ref), axis=1, keepdims=True))
    assert np.max(np.abs(xd.download() - ref) / unit) <= 1.0
    assert np.max(np.abs(ref - ph.integrate(lambda z: ph.shape321_rhs(z, u, p), x0, "rk4", 4, c.dt))) > 1e-7  # (p matters)
    with pytest.raises(cg.CgmresHipError, match="no plant parameters"):
        c.plant_step_device(xd, ud, cg.Plant("rk4", 4, dev(np.ones(3))))
    dev.free(), c.close()
    # the loop
    outs = []
    for how in ("loop", "caller"):
        c = fresh()
        outs.append(run_plant_loop(c, x0, n, plant, seq=seq, stride=4) if how == "loop" else caller_loop(c, x0, n, plant, seq=seq, cut=4))
        c.close()
    (log_a, end_a), (log_b, end_b) = outs
    same_bits(log_a, log_b, LOGS)
    same_bits(end_a, end_b, END)
    assert np.max(np.abs(end_a["x"] - x0)) > 1e-4


# ---- R. what is refused ---------------------------------------------------------------------------------------------------
def test_refusals(orc):
    c, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    lib, dev = cg.load(), Dev(c)
    xd, ud = dev(x0), dev(np.zeros((20, 3)))
    dd, th = dev(np.zeros((5, 20, 4))), dev(ph.theta_draw(0, 20))
    xl = dev(shape=(5, 20, 4))
    size = ctypes.sizeof(cg.LoopPlant)

    def call(n=5, rec=None, seq=None, x=xd.ptr, u=ud.ptr, **fields):
        lp = cg.LoopPlant(**dict(dict(struct_size=size, integrator=cg.PLANT_RK4, substeps=4), **fields))
        li = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs), dist_per_instance=1, dist_seq_dev=seq)
        cg._check(lib.cgmres_hip_closed_loop_device_plant(c._h, x, u, n, ctypes.byref(li), ctypes.byref(rec) if rec else None,
                                                          ctypes.byref(lp)))

    def step(**fields):
        lp = cg.LoopPlant(**dict(dict(struct_size=size, integrator=cg.PLANT_RK4, substeps=4), **fields))
        cg._check(lib.cgmres_hip_plant_step_device(c._h, xd.ptr, ud.ptr, ctypes.byref(lp)))
    for f in (call, step):
        with pytest.raises(cg.CgmresHipError, match="struct_size .* cgmres_hip_loop_plant"):
            f(struct_size=size - 8)
        with pytest.raises(cg.CgmresHipError, match="reserved"):
            f(reserved=(ctypes.c_int32 * 2)(0, 1))
        with pytest.raises(cg.CgmresHipError, match="unknown integrator 2"):
            f(integrator=2)
        with pytest.raises(cg.CgmresHipError, match="substeps 0 outside"):
            f(substeps=0)
        with pytest.raises(cg.CgmresHipError, match="substeps 4097 outside"):
            f(substeps=4097)
        with pytest.raises(cg.CgmresHipError, match="theta_per_instance"):
            f(theta_dev=th.ptr, theta_per_instance=2)
        with pytest.raises(cg.CgmresHipError, match="theta_dev overlaps x_dev"):
            f(theta_dev=xd.ptr + 8, theta_per_instance=1)
        with pytest.raises(cg.CgmresHipError, match="theta_dev overlaps u_dev"):
            f(theta_dev=ud.ptr, theta_per_instance=0)
    with pytest.raises(cg.CgmresHipError, match="null plant"):
        cg._check(lib.cgmres_hip_plant_step_device(c._h, xd.ptr, ud.ptr, None))
    with pytest.raises(cg.CgmresHipError, match="theta_dev overlaps dist_seq_dev"):
        call(seq=dd.ptr, theta_dev=dd.ptr + 64, theta_per_instance=1)
    rec = cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=1, x_log_dev=xl.ptr)
    with pytest.raises(cg.CgmresHipError, match="x_log_dev overlaps theta_dev"):
        call(rec=rec, theta_dev=xl.ptr + 16, theta_per_instance=1)
    # everything ..._rec refuses
    with pytest.raises(cg.CgmresHipError, match="n_ticks"):
        call(n=-1)
    with pytest.raises(cg.CgmresHipError, match="stride 0 < 1"):
        call(rec=cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=0, x_log_dev=xl.ptr))
    with pytest.raises(cg.CgmresHipError, match="x_log_dev overlaps x_dev"):
        call(rec=cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=1, x_log_dev=xd.ptr))
    with pytest.raises(cg.CgmresHipError, match="null pointer"):
        call(x=None)
    assert c.t == 0.0
    call(n=0, theta_dev=th.ptr, theta_per_instance=1)  # n_ticks == 0 touches nothing
    c.synchronize()
    assert c.t == 0.0 and np.array_equal(xd.download(), x0)
    # the binding checks a typed theta buffer before its address crosses the ABI
    with pytest.raises(ValueError):
        c.plant_step_device(xd, ud, cg.Plant("rk4", 4, dev(np.ones((20, 6)))))
    with pytest.raises(TypeError):
        c.plant_step_device(xd, ud, cg.Plant("rk4", 4, dev(np.ones(7, dtype=np.float32))))
    dev.free(), c.close()
    # a model without plant parameters
    c, x0, u0, p = new_batch(orc, 2, batch=20, variant=2)
    assert cg.plant_info(2)["n_theta"] == 2
    c.close()


def test_plugin_built_before_the_plant_is_told_to_rebuild():
    """A plugin built before the plant existed (imitated with -DCGM_PLUGIN_WITHOUT_PLANT, as the horizon's and the
    record's): the two entry points refuse it with the advice to rebuild; everything else of it keeps working."""
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    header = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
    mid = plugin.register(plugin.build(header, cls="VdpModel", name="vdp_noplant", extra_flags=("-DCGM_PLUGIN_WITHOUT_PLANT",)))
    c = cg.CgmresBatch(mid, batch=4)
    dev = Dev(c)
    xd, ud = dev(np.ones((4, 2))), dev(np.zeros((4, 3)))
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.plant_step_device(xd, ud, cg.Plant())
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.closed_loop_device(xd, ud, 2, plant=cg.Plant())
    assert c.t == 0.0
    c.closed_loop_device(xd, ud, 2, record=dict(stride=1, t=np.zeros(2)))
    c.synchronize()
    assert c.t > 0.0
    dev.free(), c.close()
