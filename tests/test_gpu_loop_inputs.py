"""GPU: plant disturbances and measurement noise inside the fused closed loop (cgmres_hip_closed_loop_device_ex).

For tick k of one call, with x the TRUE plant state (<example>/main.cpp:63-73 plus two inputs):
    y_k = x_k + v_k,   u_k = control(y_k),   x_{k+1} = (x_k + f(x_k, u_k) dt) + d_k
The yardstick is the oracle driven tick by tick from here with exactly these three statements (Controller.control /
Controller.plant), on a sample that holds both sides of a workgroup edge (15, 16) and the last instance.

Shapes: B = 83 = five full 16-instance workgroups and a ragged three; n = 23 = two launch boundaries and a partial
tail (CGMRES_HIP_TICKS_PER_LAUNCH = 10).  Noise: np.random.default_rng(7), standard deviation 1e-3.
Bounds: x, u at 1e-9 (fp64).  Two oracle runs whose start differs by 1e-13 end within 7e-12 on u under this noise, the
GPU-oracle distance of the project is ~1e-15; a noise of 1e-3 moves x by ~1e-3 and f(y) instead of f(x) by ~1e-6, so a
swapped or dropped input fails by orders of magnitude.  fp32: 1e-4, the project's fp32 closed-loop bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, DV, KM, N = 83, 50, 10, 23
SIGMA = 1e-3
TOL64 = 1e-9


def sample_of(batch, n=14):
    step = max(1, batch // n)
    s = list(range(0, batch, step))[:n]
    for extra in (batch - 1, 15, 16):
        if 0 <= extra < batch and extra not in s:
            s.append(extra)
    return sorted(s)


def noise(n, batch, nx, dtype=np.float64):
    """(d, v), each [n, batch, nx], from the one seeded generator the issue names."""
    rng = np.random.default_rng(7)
    d = rng.normal(0.0, SIGMA, (n, batch, nx)).astype(dtype)
    v = rng.normal(0.0, SIGMA, (n, batch, nx)).astype(dtype)
    return d, v


def new_batch(orc, model, batch=B, dv=DV, km=KM, tol=1e-6, variant=0, dtype="f64", flags=0):
    x0, u0, p = orc.batch_scenario(model, batch)
    c = cg.CgmresBatch(model, batch=batch, dv=dv, k_max=km, tol=tol, variant=variant, dtype=dtype, flags=flags)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    return c, x0, u0, p


def run_device(c, x0, n, d=None, v=None, seq=None, **kw):
    """closed_loop_device with the given sequences -> dict(x, u, n_ax, reason, t); the handle stays open."""
    bufs = []

    def dev(a):
        if a is None:
            return None
        bufs.append(c.device_buffer(a.shape).upload(a))
        return bufs[-1]
    xd = c.device_buffer((c.batch, c.dim_x)).upload(x0.astype(c.np_dtype))
    ud = c.device_buffer((c.batch, c.dim_u)).upload(np.zeros((c.batch, c.dim_u), dtype=c.np_dtype))
    c.closed_loop_device(xd, ud, n, dev(seq), kw.pop("per_instance", True), dist_seq_dev=dev(d), meas_seq_dev=dev(v), **kw)
    c.synchronize()
    n_ax, reason = c.get_status()
    out = dict(x=xd.download().astype(np.float64), u=ud.download().astype(np.float64), n_ax=n_ax, reason=reason, t=c.t)
    for b in bufs + [xd, ud]:
        b.free()
    return out


def oracle_loop(orc, model, x0, u0, p, i, n, d=None, v=None, seq=None, dv=DV, km=KM, tol=1e-6, dtype="f64"):
    """The three statements on the oracle for instance i.  d, v, seq: [n, ...] rows of THIS instance (or None).
    Returns (x_n, u_{n-1}, controller); in fp32 the plant step is taken in float32 as the device takes it."""
    npdt = np.float32 if dtype == "f32" else np.float64
    r = orc.Controller(model, dv, km, tol, dtype)
    orc.start_controller(r, x0[i], u0[i], p[i])
    x = np.array(x0[i], dtype=npdt)
    u = None
    for k in range(n):
        if seq is not None:
            r.set_ptau(seq[k])
        y = x if v is None else (x + v[k].astype(npdt)).astype(npdt)
        u = r.control(y)
        x = (x + r.plant(x, u).astype(npdt) * npdt(r.dt)).astype(npdt)
        if d is not None:
            x = (x + d[k].astype(npdt)).astype(npdt)
    return x.astype(np.float64), u, r


def rows_of(a, i):
    """The per-tick rows of instance i from a per-instance [n, B, nx] or a broadcast [n, nx] sequence."""
    return None if a is None else (a[:, i] if a.ndim == 3 else a)


def check_against_oracle(orc, c, out, model, x0, u0, p, n, d=None, v=None, seq=None, tol=1e-6, sample=None, bound=TOL64,
                         dtype="f64", **okw):
    sample = sample or sample_of(c.batch)
    assert len(sample) >= 14 and {15, 16, c.batch - 1} <= set(sample)
    assert abs(out["t"] - n * c.dt) <= (1e-6 if dtype == "f32" else 1e-12)
    x_n = out["x"].astype(c.np_dtype)
    u_next = c.control(x_n)  # one more plain tick: the sequences are gone from the handle
    worst = 0.0
    for i in sample:
        x_o, u_o, r = oracle_loop(orc, model, x0, u0, p, i, n, rows_of(d, i), rows_of(v, i), rows_of(seq, i), tol=tol,
                                  dtype=dtype, **okw)
        ex, eu = np.max(np.abs(out["x"][i] - x_o)), np.max(np.abs(out["u"][i] - u_o))
        worst = max(worst, ex, eu)
        assert ex <= bound and eu <= bound, (i, ex, eu)
        if dtype == "f64":
            assert out["n_ax"][i] == r.last_solve()[0] and out["reason"][i] == r.last_solve()[2], (i, out["n_ax"][i], r.last_solve())
        assert np.max(np.abs(u_next[i] - r.control(x_n[i]))) <= bound, i
    print(f"max |gpu - oracle| over x, u of {len(sample)} instances: {worst:.3e}")


def intended(name, model, variant):
    """Is `name` the kernel family the (model, variant) case is there to hold?"""
    if variant == 1:
        return name == "lane"
    if variant == 4:
        return name == "wave"
    if variant == 3:
        return name.startswith("wg-lean")
    # variant 2: row-Newton (pendulum), the MAXM = 20 / fh_hbm family (MSD at dv = 50: L = 300), row-scan (semi-active)
    return name == "wg+row-newton" if model == 0 else (name == "wg+row-scan" if model == 2 else
                                                      name in ("wg", "wg+parallel-costate", "wg+two-pass-costate"))


# ---- 1. every mapping and kernel family, d and v together, shipped tol and fixed-k ---------------------------------
@pytest.mark.parametrize("tol", [1e-6, 0.0], ids=["tolref", "fixedk"])
@pytest.mark.parametrize("model,variant", [(0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (0, 4), (1, 4), (2, 4), (0, 1)])
def test_disturbance_and_noise_on_every_mapping(orc, model, variant, tol):
    c, x0, u0, p = new_batch(orc, model, tol=tol, variant=variant)
    assert c.variant == variant and intended(c.variant_name, model, variant), c.variant_name
    d, v = noise(N, B, c.dim_x)
    out = run_device(c, x0, N, d, v)
    if tol == 0.0:
        assert np.all(out["n_ax"] == KM) and np.all(out["reason"] == cg.EXIT_NATURAL)
    check_against_oracle(orc, c, out, model, x0, u0, p, N, d, v, tol=tol)
    c.close()


# ---- 2. d only, v only, mixed broadcast ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["d_only", "v_only", "d_broadcast_v_per_instance"])
@pytest.mark.parametrize("variant", [2, 4])
def test_single_inputs_and_broadcast(orc, variant, which):
    model = 0
    c, x0, u0, p = new_batch(orc, model, variant=variant)
    d, v = noise(N, B, c.dim_x)
    kw = {}
    if which == "d_only":
        v = None
    elif which == "v_only":
        d = None
    else:
        d = np.ascontiguousarray(d[:, 5])  # [n, nx]: one disturbance for every instance
        kw = dict(dist_per_instance=False, meas_per_instance=True)
    out = run_device(c, x0, N, d, v, **kw)
    check_against_oracle(orc, c, out, model, x0, u0, p, N, d, v)
    c.close()


# ---- 3. all three sequences at once --------------------------------------------------------------------------------
def test_moving_reference_with_disturbance_and_noise(orc):
    model = 0
    c, x0, u0, p = new_batch(orc, model, variant=2)
    stage = np.arange(DV + 1)
    seq = np.empty((N, B, DV + 1, c.dim_p))
    for k in range(N):
        for i in range(B):  # the ramp of test_closed_loop_device_with_moving_reference
            seq[k, i, :, 0] = p[i, 0] * (1.0 + 0.004 * k) + 0.0007 * stage * (1 + 0.1 * (i % 5))
            seq[k, i, :, 1] = p[i, 1]
    seq = seq.reshape(N, B, c.dim_p * (DV + 1))
    d, v = noise(N, B, c.dim_x)
    out = run_device(c, x0, N, d, v, seq)
    check_against_oracle(orc, c, out, model, x0, u0, p, N, d, v, seq)  # (the follow-up tick uses the LAST horizon)
    c.close()


# ---- 4. identity: no inputs == the existing entry point, bit for bit -----------------------------------------------
@pytest.mark.parametrize("variant", [2, 4])
def test_ex_without_inputs_is_closed_loop_device(orc, variant):
    import ctypes
    outs = []
    for how in ("plain", "null", "empty"):
        c, x0, u0, p = new_batch(orc, 0, variant=variant)
        xd = c.device_buffer((B, c.dim_x)).upload(x0)
        ud = c.device_buffer((B, c.dim_u)).upload(np.zeros((B, c.dim_u)))
        if how == "plain":
            c.closed_loop_device(xd, ud, N)
        else:
            li = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs))  # every pointer NULL
            cg._check(cg.load().cgmres_hip_closed_loop_device_ex(c._h, xd.ptr, ud.ptr, N, ctypes.byref(li) if how == "empty" else None))
        c.synchronize()
        _, U, dUdt = c.get_state()
        outs.append((xd.download(), ud.download(), U, dUdt, c.get_status()[0], c.t))
        xd.free(), ud.free(), c.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


# ---- 5. binned placement: the sequences follow the INSTANCE, not the slot -----------------------------------------
def test_inputs_follow_the_instance_under_binned_placement(orc):
    model, batch, n = 0, 8300, 25  # the lean plan, 519 workgroups: re-placed before the second and third launch
    d, v = noise(n, batch, 4)
    outs = []
    for flags in (0, cg.FLAG_NO_BINNING):
        c, x0, u0, p = new_batch(orc, model, batch=batch, tol=1e-6, flags=flags)
        assert c.variant == 3
        outs.append(run_device(c, x0, n, d, v))
        if flags == 0:
            sample = sample_of(batch)
            check_against_oracle(orc, c, outs[0], model, x0, u0, p, n, d, v, sample=sample)
        c.close()
    a, b = outs
    # (the noise takes the batch out of the slow phase in which placement is bit-neutral: agreement to rounding only)
    assert np.max(np.abs(a["x"] - b["x"])) <= 1e-12 and np.max(np.abs(a["u"] - b["u"])) <= 1e-12


# ---- 6. fp32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 3])
def test_fp32_pendulum(orc, variant):
    model, batch, dv, km = 0, 40, 100, 20
    c, x0, u0, p = new_batch(orc, model, batch=batch, dv=dv, km=km, variant=variant, dtype="f32")
    assert c.variant == variant
    d, v = noise(N, batch, 4, np.float32)
    out = run_device(c, x0, N, d, v)
    x0f = x0.astype(np.float32)
    check_against_oracle(orc, c, out, model, x0f, u0, p, N, d, v, bound=1e-4, dtype="f32", dv=dv, km=km)
    c.close()


# ---- 7. user model: the fused call against the same loop unrolled by hand on a second handle ----------------------
@pytest.mark.parametrize("variant", [2, 1, 4])
def test_user_model_fused_vs_unrolled(variant):
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    header = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")
    mid = plugin.register(plugin.build(header, cls="VdpModel", name="vdp"))
    batch, n = 20, 12
    b = np.arange(batch, dtype=np.float64)
    x0 = np.stack([1.0 + 0.03 * b, -0.5 + 0.02 * b], axis=1)
    p = np.stack([0.05 * b, 0.05 * (np.arange(batch) % 3)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (batch, 1))
    d, v = noise(n, batch, 2)

    def start():
        c = cg.CgmresBatch(mid, batch=batch, variant=variant)
        assert c.variant == variant
        c.set_ptau_repeat(p)
        c.init_u0(u0)
        c.init_u0_newton(u0, x0, p, 10)
        return c
    c = start()
    out = run_device(c, x0, n, d, v)
    c.close()
    h = start()
    x, lmd = x0.copy(), np.zeros(2)
    for k in range(n):
        u = h.control(x + v[k])
        f = np.stack([cg.model_probe(mid, x[i], u[i], p[i], lmd)[0] for i in range(batch)])  # the DEVICE dxdt, true state
        x = (x + f * h.dt) + d[k]
    n_ax = h.get_status()[0]
    h.close()
    assert np.max(np.abs(out["x"] - x)) <= TOL64 and np.max(np.abs(out["u"] - u)) <= TOL64
    assert np.array_equal(out["n_ax"], n_ax)


# ---- 8. a NaN in d: that instance is flagged, its workgroup mates are untouched ------------------------------------
def test_nan_disturbance_is_flagged_per_instance(orc):
    model, n, bad = 0, 12, 21
    c, x0, u0, p = new_batch(orc, model, variant=2)
    d, v = noise(n, B, c.dim_x)
    d[3, bad, 1] = np.nan
    out = run_device(c, x0, n, d, v)
    c.close()
    nonfinite = out["reason"] == cg.EXIT_NONFINITE
    assert list(np.flatnonzero(nonfinite)) == [bad]
    assert not np.all(np.isfinite(out["x"][bad]))
    others = np.arange(B) != bad
    assert np.all(np.isfinite(out["x"][others])) and np.all(np.isfinite(out["u"][others]))
    for i in (16, 20, 22, 31):  # the rest of its workgroup (instances 16 .. 31)
        x_o, u_o, r = oracle_loop(orc, model, x0, u0, p, i, n, d[:, i], v[:, i])
        assert np.max(np.abs(out["x"][i] - x_o)) <= TOL64 and np.max(np.abs(out["u"][i] - u_o)) <= TOL64, i
        assert out["n_ax"][i] == r.last_solve()[0]


# ---- 9. validation ----------------------------------------------------------------------------------------------------
def test_validation(orc):
    import ctypes
    c, x0, u0, p = new_batch(orc, 0, batch=20, variant=2)
    lib = cg.load()
    xd = c.device_buffer((20, 4)).upload(x0)
    ud = c.device_buffer((20, 3)).upload(np.zeros((20, 3)))
    dd = c.device_buffer((5, 20, 4)).upload(np.zeros((5, 20, 4)))
    size = ctypes.sizeof(cg.LoopInputs)

    def call(n, **fields):
        li = cg.LoopInputs(**dict(dict(struct_size=size, dist_seq_dev=dd.ptr, dist_per_instance=1), **fields))
        cg._check(lib.cgmres_hip_closed_loop_device_ex(c._h, xd.ptr, ud.ptr, n, ctypes.byref(li)))
    with pytest.raises(cg.CgmresHipError, match="struct_size"):
        call(5, struct_size=size - 8)
    with pytest.raises(cg.CgmresHipError, match="per_instance"):
        call(5, meas_per_instance=2)
    with pytest.raises(cg.CgmresHipError, match="overlaps x_dev"):
        call(1, dist_seq_dev=xd.ptr)
    with pytest.raises(cg.CgmresHipError, match="overlaps u_dev"):
        call(1, meas_seq_dev=ud.ptr + 8, meas_per_instance=0)
    with pytest.raises(cg.CgmresHipError, match="n_ticks"):
        call(-1)
    with pytest.raises(cg.CgmresHipError, match="n_ticks"):
        c.closed_loop_device(xd, ud, -1, dist_seq_dev=dd)
    with pytest.raises(ValueError):  # the binding checks the element count of a typed buffer
        c.closed_loop_device(xd, ud, 6, dist_seq_dev=dd)
    call(0)
    c.synchronize()
    assert np.array_equal(xd.download(), x0) and c.t == 0.0
    for b in (xd, ud, dd):
        b.free()
    c.close()


# ---- 10. the C++ overload ---------------------------------------------------------------------------------------------
def test_cpp_overload_equals_the_c_call(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib_dir = os.path.join(ROOT, "cgmres_cpp_amd", "lib")
    exe = tmp_path / "loop_inputs_main"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "loop_inputs_main.cpp"),
                    f"-L{lib_dir}", f"-Wl,-rpath,{lib_dir}", "-lcgmres_hip", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    words = out.split()
    assert words[0] == "max_diff" and float(words[1]) == 0.0, out
    assert float(words[3]) > 1e-4, out  # (the loop ran: the state moved)
