"""GPU: cgmres_hip_horizon_device — the predicted state trajectory xtau, the costate trajectory ltau, the optimality
residual F and its norm of every instance, evaluated with the handle's own U, ptau and t on its stream — on every
mapping, both dtypes and user models, against
  * the committed golden fixtures' F0 (tests/golden/*.npz, from the unmodified reference),
  * the oracle's F (oracle/liboracle.so) and
  * tests/horizon_ref.cpp for the two trajectories, which tests/test_horizon_ref.py pins to the oracle bit for bit.
fp64 bar: 1e-11 * max(1, max|reference|), the bar tests/test_gpu_parity.py::test_hooks_vs_golden holds the F hook to.
Worst fp64 deviations observed on an MI355X, relative to max(1, |reference|) (printed at the end of a run with -s):
    F 1.4e-14 (golden, msd dv 50 / 120, t = 0), xtau 1.5e-16, ltau 1.8e-16; user model F 4.4e-16, xtau and ltau 0;
    after a fused loop F 3.1e-16 against the handle's own F_func.  fp32: |device - fp32 reference| is at most 0.016 of
    E = |fp32 reference - fp64 reference| (F, pendulum dv 8), against the 4 allowed."""
import ctypes as C
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin
from conftest import golden_files, golden_ids, load_golden
from gpu_helpers import VARIANTS, _refs, _teacher_forced, new_batch
from horizon_helper import HorizonRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-11
F64_FILES = [p for p in golden_files() if p.endswith("_f64.npz")]
F64_IDS = [i for i in golden_ids() if i.endswith("_f64")]
WORST = {}  # what -> worst |device - reference| / max(1, max|reference|) seen in this run


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return HorizonRef(tmp_path_factory.mktemp("horizon_ref"))


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for k in sorted(WORST):
        print(f"\nhorizon worst {k}: {WORST[k]:.3e}", end="")
    print()


def batch_of(model, variant, **kw):
    """gpu_helpers.new_batch; the lane and the wg mapping serve every model, dtype and size here: no skip on them."""
    try:
        return new_batch(model, variant=variant, **kw)
    except pytest.skip.Exception:
        assert variant not in (1, 2), f"variant {variant} skipped for model {model}, {kw}"
        raise


def close(what, got, want, rel=REL):
    scale = max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(got - want)))
    print(f"{what}: |device - reference| = {err:.3e}, scale {scale:.3e}, ratio to bar {err / (rel * scale):.3f}")
    WORST[what] = max(WORST.get(what, 0.0), err / scale)
    assert np.all(np.isfinite(got)) and err <= rel * scale, (what, err, rel * scale)


def check_fnorm(fnorm, F):
    want = np.sqrt(np.sum(F * F, axis=1))
    assert np.all(np.abs(fnorm - want) <= 1e-12 * np.maximum(want, np.finfo(np.float64).tiny)), (fnorm, want)


def check_against(ref, c, model, x, U, ptau, t, F_want, what):
    """horizon(x) of the handle against F_want [B, L] (golden or oracle) and the helper's trajectories."""
    xtau, ltau, F, fnorm = c.horizon(x)
    xr, lr, Fr = ref.batch(model, "f64", c.dv, c.Tf, c.alpha, t, x, U, ptau)
    close(what + " F", F, F_want)
    close(what + " F (helper)", F, Fr)
    close(what + " xtau", xtau, xr)
    close(what + " ltau", ltau, lr)
    check_fnorm(fnorm, F)
    return xtau, ltau, F, fnorm


# ---- 1. golden fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("path", F64_FILES, ids=F64_IDS)
def test_golden_F0_and_trajectories(path, variant, ref):
    g = load_golden(path)
    case = g["_case"]
    B = 3  # identical instances: their outputs must be bit-equal
    try:
        c = batch_of(case["model"], variant, batch=B, dv=case["dv"], k_max=case["kmax"], tol=case["tol"])
    except cg.CgmresHipError as e:  # sizes beyond half a CU's LDS have no lean plan: no handle, nothing to evaluate
        assert variant == 3 and "wg-lean mapping" in str(e), e
        return
    c.set_ptau(g["ptau"])
    ptau = np.tile(g["ptau"], (B, 1)) if case["dim_p"] else np.zeros((B, 0))
    for tick in g["_ticks"]:
        p = f"tick{tick}_"
        t, U, x = g[p + "t"][0], np.tile(g[p + "U"], (B, 1)), np.tile(g[p + "x"], (B, 1))
        c.set_state(t, U, np.tile(g[p + "dUdt"], (B, 1)))
        out = check_against(ref, c, case["model"], x, U, ptau, t, np.tile(g[p + "F0"], (B, 1)), "golden")
        for a in out:
            assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2]), tick
    c.close()


# ---- 2. seeded batches: two wavefronts with a tail; five 16-instance workgroups with a tail of 6 ---------------------
def seeded_cases():
    cases = []
    for model in (0, 1, 2):
        # dv = 1 has no LDS plan on any wg mapping (cgmres_hip_create refuses variants 2, 3, 4 there): the lane mapping,
        # asked for and as the library's own choice
        cases += [(model, 1, 1, v, 70) for v in (1, 0)]
        cases += [(model, 8, 3, v, 70) for v in VARIANTS]
    cases += [(0, 40, 5, v, 70) for v in (1, 2, 4)]  # the row-Newton context
    cases += [(1, 50, 5, v, 70) for v in (1, 2)]      # L = 300: F_dxh_h in HBM
    cases += [(1, 120, 5, 1, 70)]                     # L = 720: lane only
    cases += [(0, 8, 3, 2, 1)]
    return cases


def start(orc, model, dv, km, variant, B, dtype="f64"):
    x0, u0, p = orc.batch_scenario(model, B)
    c = batch_of(model, variant, batch=B, dv=dv, k_max=km, tol=1e-6, dtype=dtype)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    return c, x0, u0, p


@pytest.mark.parametrize("model,dv,km,variant,B", seeded_cases())
def test_seeded_batch_vs_oracle(orc, ref, model, dv, km, variant, B):
    c, x0, u0, p = start(orc, model, dv, km, variant, B)
    refs = _refs(orc, model, dv, km, 1e-6, x0, u0, p)
    _teacher_forced(orc, c, refs, x0, 3)  # U varies along the horizon, t > 0
    t, U, d = zip(*[r.get_state() for r in refs])
    t, U, d = t[0], np.array(U), np.array(d)
    x = x0 + 0.01 * np.cos(np.arange(x0.size)).reshape(x0.shape)
    c.set_state(t, U, d)
    ptau = np.tile(p, (1, dv + 1))
    assert t > 0 and (dv == 1 or np.max(np.abs(U[:, :c.dim_u] - U[:, -c.dim_u:])) > 0)
    Fo = np.array([r.F(U[i], x[i], t) for i, r in enumerate(refs)])
    check_against(ref, c, model, x, U, ptau, t, Fo, f"seeded dv{dv}")
    # t = 0: dtau = 0, the state never moves and the costate stays the terminal one
    c.set_state(0.0, U, d)
    xtau, ltau, F, fnorm = c.horizon(x)
    assert np.array_equal(xtau, np.repeat(x[:, None, :], dv + 1, axis=1))
    assert np.array_equal(ltau, np.repeat(ltau[:, dv:dv + 1, :], dv + 1, axis=1))
    close("seeded t=0 F", F, np.array([r.F(U[i], x[i], 0.0) for i, r in enumerate(refs)]))
    # a parameter horizon that is a ramp along the stages
    if c.dim_p:
        ramp = ptau + 0.02 * np.repeat(np.arange(dv + 1), c.dim_p)[None, :] * (1 + 0.1 * np.arange(B))[:, None]
        c.set_ptau(ramp)
        c.set_state(t, U, d)
        for i, r in enumerate(refs):
            r.set_ptau(ramp[i])
        Fo = np.array([r.F(U[i], x[i], t) for i, r in enumerate(refs)])
        check_against(ref, c, model, x, U, ramp, t, Fo, f"seeded ramp dv{dv}")
    c.close()


# ---- 3. the call leaves the handle alone ------------------------------------------------------------------------------
def krylov_written(c):
    """What the last solve wrote of get_krylov(), per instance, n = its Arnoldi count: columns 0..n-1 of H down to the
    subdiagonal, rho[0..n], g[0..n-1].  The entries behind them are whatever the kernel's LDS held (two fresh handles that
    never met a horizon call already differ there, in denormal garbage), so they say nothing about this call."""
    n_ax, _ = c.get_status()
    _, H, rho, g = c.get_krylov()
    return [np.concatenate([H[i, col, :col + 2] for col in range(n)] + [rho[i, :n + 1], g[i, :n].ravel()])
            for i, n in enumerate(n_ax)]


@pytest.mark.parametrize("variant,dv", [(1, 40), (2, 40), (2, 25), (4, 40)])
def test_horizon_leaves_the_handle_alone(orc, variant, dv):
    B, km = 20, 5
    pair = [start(orc, 0, dv, km, variant, B) for _ in range(2)]
    (a, x0, _, _), (b, _, _, _) = pair
    xd = a.device_buffer((B, 4))
    outs = [a.device_buffer(s) for s in ((B, dv + 1, 4), (B, dv + 1, 4), (B, 3 * dv), (B,))]
    x = x0.copy()
    for tick in range(5):
        xd.upload(x)
        a.horizon_device(xd, *outs)
        ua, ub = a.control(x), b.control(x)
        assert np.array_equal(ua, ub), tick
        for sa, sb in zip(a.get_state() + a.get_status(), b.get_state() + b.get_status()):
            assert np.array_equal(sa, sb), tick
        for i, (ka, kb) in enumerate(zip(krylov_written(a), krylov_written(b))):
            assert np.array_equal(ka, kb), (tick, i)
        x = x + 1e-3 * np.sin(1.0 + tick + np.arange(x.size)).reshape(x.shape)
    assert a.t == b.t and a.t > 0
    a.close(), b.close()


# ---- 4. optional outputs and bounds -----------------------------------------------------------------------------------
class Guarded:
    """A device array with 64 sentinel elements before and after it."""
    PAD, MARK = 64, -7.25

    def __init__(self, c, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = c.device_buffer((self.n + 2 * self.PAD,)).upload(np.full(self.n + 2 * self.PAD, self.MARK))
        self.ptr = self.buf.ptr + self.PAD * self.buf.dtype.itemsize  # (a raw address: the binding cannot check it)

    def read(self):
        a = self.buf.download()
        assert np.all(a[:self.PAD] == self.MARK) and np.all(a[-self.PAD:] == self.MARK), "sentinel overwritten"
        return a[self.PAD:-self.PAD].reshape(self.shape)


@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("variant", [1, 2])
def test_each_output_alone_and_sentinels(orc, variant, B):
    dv = 20  # five chunks of the pendulum's four stages
    c, x0, _, _ = start(orc, 0, dv, 5, variant, B)
    c.control(x0)  # t > 0, U moves
    xd = c.device_buffer((B, 4)).upload(x0)
    shapes = dict(xtau=(B, dv + 1, 4), ltau=(B, dv + 1, 4), F=(B, 3 * dv), fnorm=(B,))
    every = {k: Guarded(c, s) for k, s in shapes.items()}
    c.horizon_device(xd, **{k: g.ptr for k, g in every.items()})
    want = {k: g.read() for k, g in every.items()}
    assert not np.any(want["F"] == Guarded.MARK) and not np.any(want["xtau"] == Guarded.MARK)
    assert not np.any(want["ltau"] == Guarded.MARK) and not np.any(want["fnorm"] == Guarded.MARK)
    for k, s in shapes.items():
        alone = Guarded(c, s)
        c.horizon_device(xd, **{k: alone.ptr})
        assert np.array_equal(alone.read(), want[k]), k
    assert np.array_equal(c.opt_error(x0), want["fnorm"])
    c.close()


# ---- 5. after a fused loop: stream order, and the kept ptau is the last tick's ---------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
def test_horizon_follows_a_fused_loop_on_the_stream(orc, variant):
    B, dv, N = 70, 25, 13  # 13 ticks: one 10-tick launch and a remainder
    c, x0, _, p = start(orc, 0, dv, 5, variant, B)
    seq = np.tile(p, (1, dv + 1))[None] * (1 + 0.002 * np.arange(N)[:, None, None]) + \
        0.001 * np.arange(2 * (dv + 1))[None, None, :]
    seq_d = c.device_buffer(seq.shape).upload(seq)
    xd = c.device_buffer((B, 4)).upload(x0)
    ud = c.device_buffer((B, 3)).upload(np.zeros((B, 3)))
    F_d, n_d = c.device_buffer((B, 3 * dv)), c.device_buffer((B,))
    c.closed_loop_device(xd, ud, N, seq_d)
    c.horizon_device(xd, F=F_d, fnorm=n_d)  # no synchronise in between
    F, fnorm = F_d.download(), n_d.download()
    t, U, _ = c.get_state()
    x = xd.download()
    assert abs(t - N * c.dt) < 1e-12
    close("after fused loop F", F, c.F_func(U, x, t))  # F_func: the handle's ptau, i.e. the last tick's
    check_fnorm(fnorm, F)
    r = orc.Controller(0, dv, 5, 1e-6)
    r.set_ptau(seq[-1, 7])
    close("after fused loop F (oracle, last tick's ptau)", F[7], r.F(U[7], x[7], t))
    c.close()


# ---- 6. fp32 ----------------------------------------------------------------------------------------------------------
FP32_RATIO = {}


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("model,dv,km", [(0, 8, 3), (1, 50, 5)])
def test_fp32_within_four_times_the_references_own_error(orc, ref, model, dv, km, variant):
    """Bound from the reference side alone: E = max|fp32 reference - fp64 reference| over the case; 4 E allowed (two fp32
    evaluations in different operation order each sit about E from the exact value, and the device's own trig adds to
    that), floor 16 * 2^-23 * scale."""
    B = 70
    c, x0, u0, p = start(orc, model, dv, km, variant, B, dtype="f32")
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    refs = []
    for i in range(B):  # the fp32 oracle's own closed loop for three ticks: its state is what the handle is given
        r = orc.Controller(model, dv, km, 1e-6, "f32")
        orc.start_controller(r, f32(x0[i]), u0[i], p[i])
        xi = f32(x0[i])
        for _ in range(3):
            xi = f32(xi + r.plant(xi, r.control(xi)) * r.dt)
        refs.append(r)
    t, U, d = zip(*[r.get_state() for r in refs])
    t, U, d = t[0], np.array(U), np.array(d)
    x, ptau = f32(x0 + 0.01), f32(np.tile(p, (1, dv + 1)))
    c.set_state(t, U, d)
    xtau, ltau, F, fnorm = c.horizon(x)
    assert xtau.dtype == np.float32 and fnorm.dtype == np.float32
    F32 = np.array([r.F(U[i], x[i], t) for i, r in enumerate(refs)])
    r64 = orc.Controller(model, dv, km, 1e-6)
    F64 = []
    for i in range(B):
        r64.set_ptau(ptau[i])
        F64.append(r64.F(U[i], x[i], t))
    h32 = ref.batch(model, "f32", dv, c.Tf, c.alpha, t, x, U, ptau)
    h64 = ref.batch(model, "f64", dv, c.Tf, c.alpha, t, x, U, ptau)
    for what, got, w32, w64 in (("F", F, F32, np.array(F64)), ("xtau", xtau, h32[0], h64[0]), ("ltau", ltau, h32[1], h64[1])):
        E = float(np.max(np.abs(w32 - w64)))
        scale = max(1.0, float(np.max(np.abs(w64))))
        bound = max(4.0 * E, 16.0 * 2.0 ** -23 * scale)
        err = float(np.max(np.abs(got.astype(np.float64) - w32)))
        ratio = err / max(E, 4.0 * 2.0 ** -23 * scale)
        key = f"fp32 {what} m{model} dv{dv} v{variant}"
        WORST[key + " err/E"] = ratio
        print(f"{key}: E = {E:.3e}, |device - fp32 reference| = {err:.3e}, ratio {ratio:.3f}, bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and err <= bound, (what, err, E, bound)
    want = np.sqrt(np.sum(F.astype(np.float64) ** 2, axis=1))
    # (a sequential fp32 sum of L squares is within L * 2^-24 of the exact one, relative; the square root halves that)
    assert np.all(np.abs(fnorm - want) <= (c.len + 8) * 2.0 ** -24 * want)
    c.close()


# ---- 7. user model ----------------------------------------------------------------------------------------------------
VDP = os.path.join(ROOT, "tests", "user_models", "vdp_model.hpp")


def vdp_start(mid, variant, B=6):
    b = np.arange(B, dtype=np.float64)
    x0 = np.stack([1.0 + 0.1 * b, -0.5 + 0.05 * b], axis=1)
    p = np.stack([0.2 * b, 0.05 * (np.arange(B) % 3)], axis=1)
    u0 = np.tile(np.array([0.1, 1.9, 0.03]), (B, 1))
    c = cg.CgmresBatch(mid, batch=B, variant=variant)
    c.set_ptau_repeat(p)
    c.init_u0(u0)
    c.init_u0_newton(u0, x0, p, 10)
    return c, x0, p


@pytest.mark.parametrize("variant", [1, 2])
def test_user_model_whose_state_equation_reads_p(tmp_path, variant):
    mid = plugin.register(plugin.build(VDP, cls="VdpModel", name="vdp"))
    vdp = HorizonRef(tmp_path, header="tests/user_models/vdp_model.hpp", cls="VdpModel")
    c, x, p = vdp_start(mid, variant)
    assert c.variant == variant
    for _ in range(3):
        c.control(x)
    ptau = np.tile(p, (1, c.dv + 1)) + 0.01 * np.repeat(np.arange(c.dv + 1), 2)[None, :]  # dxdt reads p[1] of every stage
    c.set_ptau(ptau)
    t, U, _ = c.get_state()
    xtau, ltau, F, fnorm = c.horizon(x)
    close("user F", F, c.F_func(U, x, t))
    xr, lr, Fr = vdp.batch(0, "f64", c.dv, c.Tf, c.alpha, t, x, U, ptau)
    close("user F (helper)", F, Fr)
    close("user xtau", xtau, xr)
    close("user ltau", ltau, lr)
    check_fnorm(fnorm, F)
    c.close()


def test_plugin_without_the_horizon_symbol_says_rebuild():
    """What a plugin built before this entry point existed looks like to the library: it registers, its controllers tick,
    and this one call is refused with a text that says what to do."""
    old = plugin.build(VDP, cls="VdpModel", name="vdp_nohorizon", extra_flags=("-DCGM_PLUGIN_WITHOUT_HORIZON",))
    c, x, _ = vdp_start(plugin.register(old), 2)
    u = c.control(x)
    assert np.all(np.isfinite(u))
    with pytest.raises(cg.CgmresHipError, match="rebuild"):
        c.horizon(x)
    c.close()


# ---- 8. refusals on a live handle -------------------------------------------------------------------------------------
def test_refusals(orc):
    B, dv = 4, 8
    c, x0, _, _ = start(orc, 0, dv, 3, 2, B)
    lib = cg.load()
    xd = c.device_buffer((B, 4)).upload(x0)
    fn = c.device_buffer((B,)).upload(np.full(B, -1.0))
    good = dict(struct_size=C.sizeof(cg.Horizon), reserved=0, fnorm_dev=fn.ptr)

    def refused(x, out, text):
        assert lib.cgmres_hip_horizon_device(c._h, x, C.byref(out) if out is not None else None) == -1  # CGMRES_HIP_EINVAL
        assert text in lib.cgmres_hip_last_error().decode(), lib.cgmres_hip_last_error()

    refused(None, cg.Horizon(**good), "null x_dev")
    refused(xd.ptr, None, "null out")
    refused(xd.ptr, cg.Horizon(**dict(good, struct_size=48)), "struct_size 48")
    refused(xd.ptr, cg.Horizon(**dict(good, reserved=1)), "reserved must be 0")
    refused(xd.ptr, cg.Horizon(**dict(good, fnorm_dev=None)), "no output wanted")
    assert np.all(fn.download() == -1.0)  # nothing ran
    with pytest.raises(TypeError):  # the binding checks typed buffers before their address crosses the ABI
        c.horizon_device(xd, fnorm=c.device_buffer((B,), np.float32))
    with pytest.raises(ValueError):
        c.horizon_device(xd, F=c.device_buffer((B, 3 * dv + 1)))
    assert lib.cgmres_hip_horizon_device(c._h, xd.ptr, C.byref(cg.Horizon(**good))) == 0
    assert np.all(fn.download() >= 0.0)
    c.close()
