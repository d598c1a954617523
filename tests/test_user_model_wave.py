"""User models on the "wave" mapping (variant 4: one wavefront per controller, csrc/tick_wave.hip.h,
WaveOps<UserDev<Model>>): the state recurrence as a serial sweep inside the wave, the costate recurrence as a scan of
dim_x x dim_x affine maps.  Only an explicit variant = 4 takes it; the library's choice for user models is unchanged.
Helpers and scenarios are those of tests/test_user_model_plugin.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin

from test_user_model_plugin import (B, CHAIN4, HEADER, ROOT, TICKS, _chain4_plugin, _run_chain4, _user_oracle,
                                    load_fixture, scenario)

LIMITS = os.path.join(ROOT, "tests", "user_models", "wave_limit_models.hpp")


@pytest.fixture(scope="module")
def vdp_mid():
    if not os.path.exists(plugin._build.HIPCC):
        pytest.skip("hipcc not available")
    return plugin.register(plugin.build(HEADER, cls="VdpModel", name="vdp"))


def _vdp_batch(mid, batch, x0, u0, p, **kw):
    c = cg.CgmresBatch(mid, batch=batch, **kw)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    return c


def _vdp_plant(x, u, p):
    f = np.stack([x[:, 1], (1.0 - x[:, 0] ** 2) * x[:, 1] - x[:, 0] + u[:, 0] + p[:, 1]], axis=1)
    return x + f * 0.001


@pytest.mark.gpu
def test_wave_user_model_vs_reference_fixture(vdp_mid):
    """(a) VdpModel (its state equation reads p) on the wave mapping, control() every tick against the unmodified
    reference's output at the bound of the wg / lane test."""
    u_ref, x_ref = load_fixture()
    x0, u0, p = scenario()
    c = _vdp_batch(vdp_mid, B, x0, u0, p, variant=4)
    assert c.variant == 4 and c.variant_name == "wave"
    x = x0.copy()
    for t in range(TICKS):
        assert np.max(np.abs(x - x_ref[:, t])) <= 1e-9, t
        u = c.control(x)
        assert np.max(np.abs(u - u_ref[:, t])) <= 1e-9, (t, u, u_ref[:, t])
        x = _vdp_plant(x, u, p)
    c.close()


@pytest.mark.gpu
def test_wave_user_model_fused_device_loop(vdp_mid):
    """(b) The same scenario through closed_loop_device: 24 ticks = launches of 10, 10 and 4 fused ticks, the plant
    step (Model::dxdt with p of stage 0) inside the kernel."""
    u_ref, x_ref = load_fixture()
    x0, u0, p = scenario()
    c = _vdp_batch(vdp_mid, B, x0, u0, p, variant=4)
    assert c.variant_name == "wave"
    xd, ud = c.device_buffer((B, 2)).upload(x0), c.device_buffer((B, 3)).upload(np.zeros((B, 3)))
    c.closed_loop_device(xd, ud, TICKS - 1)
    c.synchronize()
    assert np.max(np.abs(ud.download() - u_ref[:, TICKS - 2])) <= 1e-9
    assert np.max(np.abs(xd.download() - x_ref[:, TICKS - 1])) <= 1e-9
    c.close()


@pytest.mark.gpu
def test_wave_user_model_moving_reference_equals_lane(vdp_mid):
    """(b) A time-varying parameter horizon reloaded at every fused tick (closed_loop_device_ptau), read by the state
    sweeps, the costate coefficients, x + h f and the plant step: wave against lane — x, u, Arnoldi counts and the
    next control()."""
    Bn, n, dv = 50, 23, 30
    rng = np.random.default_rng(11)
    x0 = np.stack([1.0 + 0.5 * rng.random(Bn), -0.5 + 0.5 * rng.random(Bn)], axis=1)
    p = np.stack([0.5 * rng.random(Bn), 0.1 * rng.random(Bn)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (Bn, 1))
    stage = np.arange(dv + 1)
    seq = np.empty((n, Bn, dv + 1, 2))
    for k in range(n):
        seq[k, :, :, 0] = p[:, :1] * (1.0 + 0.01 * k) + 0.002 * stage[None, :]
        seq[k, :, :, 1] = p[:, 1:2] * np.cos(0.05 * k)
    seq = seq.reshape(n, Bn, 2 * (dv + 1))
    outs = {}
    for variant in (4, 1):
        c = _vdp_batch(vdp_mid, Bn, x0, u0, p, variant=variant)
        assert c.variant == variant
        sd = c.device_buffer(seq.shape).upload(seq)
        xd, ud = c.device_buffer((Bn, 2)).upload(x0), c.device_buffer((Bn, 3))
        c.closed_loop_device(xd, ud, n, sd, True)
        c.synchronize()
        outs[variant] = (xd.download(), ud.download(), c.get_status()[0], c.control(xd.download()))
        c.close()
    assert np.array_equal(outs[4][2], outs[1][2])
    for a, b in zip(outs[4], outs[1]):
        assert np.max(np.abs(a.astype(float) - b.astype(float))) <= 1e-9
    assert np.all(np.isfinite(outs[4][0])) and np.all(np.isfinite(outs[4][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("dv", [24, 25, 27, 50, 63])
def test_wave_four_state_model_teacher_forced(tmp_path, dv):
    """(c) dim_x = 4 (a 4 x 4 affine costate scan), against the oracle's generic controller, teacher-forced: every tick
    starts from the oracle's controller and plant state, stays within the single-tick bound and runs the oracle's
    number of Arnoldi iterations.  dv covers every remainder across the 16-lane DPP rows and the 63-lane edge; below
    dv = 24 the wg context of this model cannot be created (WgTraits::lookahead_fits, wg_plan.hip.h), so neither can the wave one."""
    mid = plugin.register(_chain4_plugin("Chain4Model", "chain4_dbg", ("-DCGM_DEBUG_LDS",)))
    Bn, ticks, kmax, tol = 20, 12, 5, 1e-9
    u_ref, x_ref, k_ref, state = _user_oracle(tmp_path, CHAIN4, "Chain4Model", Bn, ticks, dv, kmax, tol, with_state=True)
    v, name = _run_chain4(mid, 4, Bn, ticks, dv, kmax, tol, u_ref, x_ref, k_ref, 1e-9, state_ref=state)
    assert (v, name) == (4, "wave")


@pytest.mark.gpu
def test_wave_stiff_cost_weights_teacher_forced(tmp_path):
    """(c) Cost weights of 1e5 next to Jacobian entries of order 1 (the scaled probe costates of UserDev::stage_coeffs)
    at the 2e-8 bound of the wg / lane test, teacher-forced over 40 ticks with equal Arnoldi counts."""
    mid = plugin.register(_chain4_plugin("Chain4Stiff", "chain4_stiff"))
    Bn, ticks, dv, kmax, tol = 24, 40, 28, 5, 1e-6
    u_ref, x_ref, k_ref, state = _user_oracle(tmp_path, CHAIN4, "Chain4Stiff", Bn, ticks, dv, kmax, tol, with_state=True)
    assert np.max(np.abs(u_ref)) > 100.0
    v, name = _run_chain4(mid, 4, Bn, ticks, dv, kmax, tol, u_ref, x_ref, k_ref, 2e-8, state_ref=state)
    assert (v, name) == (4, "wave")


@pytest.mark.gpu
def test_wave_user_model_batch_in_rounds_equals_lane(vdp_mid):
    """(d) Two controllers per SIMD and three more: the batch runs in rounds.  20 fused ticks of wave against lane."""
    from cgmres_cpp_amd.multi import _cu_count
    Bn = 2 * 4 * _cu_count(0) + 3
    rng = np.random.default_rng(7)
    x0 = np.stack([1.0 + 0.5 * rng.random(Bn), -0.5 + 0.5 * rng.random(Bn)], axis=1)
    p = np.stack([0.5 * rng.random(Bn), 0.1 * rng.random(Bn)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (Bn, 1))
    outs = {}
    for variant in (4, 1):
        c = _vdp_batch(vdp_mid, Bn, x0, u0, p, variant=variant)
        assert c.variant == variant
        xd, ud = c.device_buffer((Bn, 2)).upload(x0), c.device_buffer((Bn, 3))
        c.closed_loop_device(xd, ud, 20)
        c.synchronize()
        outs[variant] = (xd.download(), ud.download(), c.get_status())
        c.close()
    for v in (4, 1):
        assert np.all(np.isfinite(outs[v][0])) and np.all(np.isfinite(outs[v][1]))
    assert np.max(np.abs(outs[4][0] - outs[1][0])) <= 1e-9 and np.max(np.abs(outs[4][1] - outs[1][1])) <= 1e-9
    for a, b in zip(outs[4][2], outs[1][2]):
        assert np.array_equal(a, b)


def _one_wave_tick(mid):
    x0, u0, p = scenario()
    c = _vdp_batch(mid, B, x0, u0, p, variant=4)
    assert c.variant_name == "wave"
    u_ref, _ = load_fixture()
    assert np.max(np.abs(c.control(x0) - u_ref[:, 0])) <= 1e-9
    c.close()


@pytest.mark.gpu
def test_wave_user_model_refusals(vdp_mid):
    """(e) Outside the limits an explicit variant = 4 is refused with CgmresHipError (naming the limit), and the process
    goes on creating and running a valid wave handle.  The library's own choice for the vdp batch stays wg."""
    x0, u0, p = scenario()
    c = cg.CgmresBatch(vdp_mid, batch=B)
    assert c.variant == 2
    c.close()
    with pytest.raises(cg.CgmresHipError, match="dv"):
        cg.CgmresBatch(vdp_mid, batch=B, dv=64, variant=4)
    _one_wave_tick(vdp_mid)
    with pytest.raises(cg.CgmresHipError, match="k_max"):
        cg.CgmresBatch(vdp_mid, batch=B, k_max=11, variant=4)
    _one_wave_tick(vdp_mid)
    # dim_x = 5: the wg context exists at this horizon, the wave mapping is refused by its dim_x limit
    five = plugin.register(plugin.build(LIMITS, cls="Chain5Model", name="wave_chain5"))
    cg.CgmresBatch(five, batch=4, variant=2).close()
    with pytest.raises(cg.CgmresHipError, match="dim_x <= 4"):
        cg.CgmresBatch(five, batch=4, variant=4)
    _one_wave_tick(vdp_mid)
    # dHdx not affine in the costate: lane only (the device check of the plugin)
    naff = plugin.register(plugin.build(LIMITS, cls="NonAffineModel", name="wave_nonaffine"))
    c = cg.CgmresBatch(naff, batch=4)
    assert c.variant == 1
    c.close()
    with pytest.raises(cg.CgmresHipError):
        cg.CgmresBatch(naff, batch=4, variant=4)
    _one_wave_tick(vdp_mid)


@pytest.mark.parametrize("ctor", ["CgmresBatch<VdpModel> c(4, 0, nullptr, 4);", "CgmresBatch<VdpModel> c(4, 0, nullptr);",
                                  "CgmresBatch<VdpModel> c(4);"])
def test_cgmres_batch_variant_argument_compiles(tmp_path, ctor):
    """(f) C++ CgmresBatch<Model> takes the mapping as a trailing defaulted argument; the old forms compile unchanged."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = tmp_path / "ctor.cpp"
    src.write_text('#include "cgmres_batch.hpp"\n#include "vdp_model.hpp"\n'
                   f"void make() {{ {ctor} (void)c.batch(); }}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}/include", f"-I{ROOT}/tests/user_models",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
