"""cgmres_cpp_amd — batched C/GMRES control ticks on MI355X (gfx950).

Python mirror of the reference's controller interface (include/cgmres.hpp of blockahead/CGMRES_cpp:
``set_ptau`` / ``set_ptau_repeat`` / ``init_u0`` / ``init_u0_newton`` / ``control``) over the C ABI of
``libcgmres_hip.so`` (include/cgmres_hip.h), batched over independent controller instances.

There is no CPU implementation behind this package: loading fails loudly when the HIP library is
missing, and creating a controller fails when no gfx950 device is usable.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

PENDULUM, MSD, SEMIACTIVE = 0, 1, 2
MODEL_IDS = {"pendulum": PENDULUM, "arm_type_inverted_pendulum": PENDULUM, "msd": MSD,
             "mass_spring_damper": MSD, "semiactive": SEMIACTIVE, "semiactive_damper": SEMIACTIVE}
F64, F32 = 0, 1
EXIT_NATURAL, EXIT_CONVERGED, EXIT_SMALL_RESIDUAL, EXIT_BREAKDOWN, EXIT_NONFINITE = 0, 1, 2, 3, 4
FLAG_SERIAL_COSTATE, FLAG_IPW8, FLAG_NO_BINNING, FLAG_TWO_PASS_COSTATE = 1, 2, 4, 8
FLAG_NO_WAVE, FLAG_WAVE_FRESH_TRIG, FLAG_WAVE_SERIAL_SWEEPS, FLAG_SERIAL_STATE_SWEEP = 16, 32, 64, 128
ABI_VERSION = 3
RECORD_BLOCK = 256  # CGMRES_HIP_RECORD_BLOCK: instances one workgroup of the record kernel covers per grid step
TICKS_PER_LAUNCH = 10  # CGMRES_HIP_TICKS_PER_LAUNCH: closed_loop_device fuses this many ticks per launch (wg mapping)

# every symbol include/cgmres_hip.h declares (tests/test_capi_symbols.py checks header == this == library)
SYMBOLS = [
    "cgmres_hip_model_info", "cgmres_hip_default_config", "cgmres_hip_model_probe", "cgmres_hip_register_model",
    "cgmres_hip_selftest_sincos", "cgmres_hip_register_operator", "cgmres_hip_operator_info", "cgmres_hip_gmres_user",
    "cgmres_hip_operator_plan",
    "cgmres_hip_last_error",
    "cgmres_hip_device_count", "cgmres_hip_create", "cgmres_hip_destroy", "cgmres_hip_get_config", "cgmres_hip_variant_name",
    "cgmres_hip_set_ptau", "cgmres_hip_set_ptau_repeat", "cgmres_hip_init_u0", "cgmres_hip_init_u0_newton",
    "cgmres_hip_control", "cgmres_hip_control_device", "cgmres_hip_closed_loop_device",
    "cgmres_hip_closed_loop_device_ptau", "cgmres_hip_closed_loop_device_ex", "cgmres_hip_synchronize", "cgmres_hip_shard_bounds",
    "cgmres_hip_get_time", "cgmres_hip_get_state", "cgmres_hip_set_state", "cgmres_hip_get_status",
    "cgmres_hip_get_krylov", "cgmres_hip_F_func", "cgmres_hip_prepare", "cgmres_hip_Ax_func", "cgmres_hip_gmres",
    "cgmres_hip_timer_start", "cgmres_hip_timer_stop", "cgmres_hip_malloc", "cgmres_hip_free",
    "cgmres_hip_memcpy_h2d", "cgmres_hip_memcpy_d2h", "cgmres_hip_state_rows", "cgmres_hip_horizon_device",
    "cgmres_hip_ensemble_device", "cgmres_hip_closed_loop_device_rec", "cgmres_hip_record_plan",
    "cgmres_hip_plant_info", "cgmres_hip_plant_step_device", "cgmres_hip_closed_loop_device_plant",
    "cgmres_hip_closed_loop_device_preview", "cgmres_hip_preview_device",
]
PLANT_EULER, PLANT_RK4 = 0, 1  # CGMRES_HIP_PLANT_*
PLANT_INTEGRATORS = {"euler": PLANT_EULER, "rk4": PLANT_RK4}
PREVIEW_HOLD, PREVIEW_LINEAR = 0, 1  # CGMRES_HIP_PREVIEW_*
PREVIEW_INTERPS = {"hold": PREVIEW_HOLD, "linear": PREVIEW_LINEAR}


class Config(C.Structure):
    """struct cgmres_hip_config (include/cgmres_hip.h)."""
    _fields_ = [("abi_version", C.c_int32), ("model_id", C.c_int32), ("dtype", C.c_int32), ("batch", C.c_int32),
                ("dv", C.c_int32), ("k_max", C.c_int32), ("device", C.c_int32), ("variant", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32), ("tol", C.c_double), ("dt", C.c_double), ("h", C.c_double), ("zeta", C.c_double),
                ("Tf", C.c_double), ("alpha", C.c_double), ("stream", C.c_void_p)]


class LoopInputs(C.Structure):
    """struct cgmres_hip_loop_inputs (include/cgmres_hip.h): the per-tick input sequences of closed_loop_device_ex."""
    _fields_ = [("struct_size", C.c_int32), ("ptau_per_instance", C.c_int32), ("dist_per_instance", C.c_int32),
                ("meas_per_instance", C.c_int32), ("ptau_seq_dev", C.c_void_p), ("dist_seq_dev", C.c_void_p),
                ("meas_seq_dev", C.c_void_p)]


class Horizon(C.Structure):
    """struct cgmres_hip_horizon_out (include/cgmres_hip.h): the device arrays cgmres_hip_horizon_device fills."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("xtau_dev", C.c_void_p), ("ltau_dev", C.c_void_p),
                ("F_dev", C.c_void_p), ("fnorm_dev", C.c_void_p)]


class EnsembleOut(C.Structure):
    """struct cgmres_hip_ensemble_out (include/cgmres_hip.h): what cgmres_hip_ensemble_device fills."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("centre_dev", C.c_void_p), ("moments_dev", C.c_void_p),
                ("counts_dev", C.c_void_p)]


class LoopRecord(C.Structure):
    """struct cgmres_hip_loop_record (include/cgmres_hip.h): the logs of cgmres_hip_closed_loop_device_rec."""
    _fields_ = [("struct_size", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32 * 2), ("x_log_dev", C.c_void_p),
                ("u_log_dev", C.c_void_p), ("n_ax_log_dev", C.c_void_p), ("reason_log_dev", C.c_void_p),
                ("t_host", C.c_void_p), ("centre_dev", C.c_void_p), ("moments_log_dev", C.c_void_p),
                ("counts_log_dev", C.c_void_p)]


class LoopPlant(C.Structure):
    """struct cgmres_hip_loop_plant (include/cgmres_hip.h): the plant of cgmres_hip_closed_loop_device_plant."""
    _fields_ = [("struct_size", C.c_int32), ("integrator", C.c_int32), ("substeps", C.c_int32),
                ("theta_per_instance", C.c_int32), ("theta_dev", C.c_void_p), ("reserved", C.c_int32 * 2)]


class Plant:
    """The plant of a closed loop that is not the controller's model stepped by one Euler step: `substeps` steps of
    dt/substeps of integrator "euler" | "rk4" on the model's state equation, with the plant parameters theta
    (plant_info(model): a device buffer [batch, n_theta] or one row [n_theta]; None = nominal).  theta_per_instance: for a
    raw address, whose shape cannot be seen; otherwise decided by the buffer's shape."""

    def __init__(self, integrator="rk4", substeps=4, theta=None, theta_per_instance=None):
        self.integrator, self.substeps, self.theta, self.theta_per_instance = integrator, int(substeps), theta, theta_per_instance


class LoopPreview(C.Structure):
    """struct cgmres_hip_loop_preview (include/cgmres_hip.h): the sampled signal of cgmres_hip_closed_loop_device_preview."""
    _fields_ = [("struct_size", C.c_int32), ("interp", C.c_int32), ("sig_per_instance", C.c_int32), ("n_samples", C.c_int32),
                ("t0", C.c_double), ("ts", C.c_double), ("sig_dev", C.c_void_p), ("reserved", C.c_int32 * 2)]


class Preview:
    """A sampled reference signal the device loop previews into every tick's ptau: sig is a device buffer
    [batch, n_samples, dim_p] or one signal [n_samples, dim_p] for every instance, sample j taken at t0 + j*ts;
    interp "linear" | "hold"; before t0 the first sample holds, past the end the last.  per_instance: for a raw address,
    whose shape cannot be seen (then n_samples must be given too); otherwise decided by the buffer's shape."""

    def __init__(self, sig, ts, t0=0.0, interp="linear", per_instance=None, n_samples=None):
        self.sig, self.ts, self.t0, self.interp, self.per_instance, self.n_samples = sig, float(ts), float(t0), interp, per_instance, n_samples


def preview_rows(sig, ts, t0, interp, t, dtau, dv):
    """The rows a loop with a preview forms, restated in numpy (no GPU): for tick times t [n] and their dtau [n] (the
    handle's own values), ptau rows [n, batch, (dv+1)*dim_p] (sig [batch, n_samples, dim_p]) or [n, (dv+1)*dim_p]
    (sig [n_samples, dim_p]) in sig's dtype.  In double, statement for statement:
        tau = t_k + i*dtau_k;  s = clamp((tau - t0)/ts, 0, n_samples-1)
        hold:   j = min(floor(s), n_samples-1);          p = sig[j]
        linear: j = min(floor(s), max(n_samples-2, 0));  p = sig[j] + (s - j)*(sig[j+1] - sig[j])   (one sample: sig[0])"""
    sig = np.asarray(sig)
    bcast = sig.ndim == 2
    sg = (sig[None] if bcast else sig).astype(np.float64)
    ns, dim_p = sg.shape[1], sg.shape[2]
    t = np.atleast_1d(np.asarray(t)).astype(np.float64)
    dtau = np.atleast_1d(np.asarray(dtau)).astype(np.float64)
    tau = t[:, None] + np.arange(dv + 1, dtype=np.float64)[None, :] * dtau[:, None]  # [n, dv+1]
    s = np.minimum(np.maximum((tau - float(t0)) / float(ts), 0.0), float(ns - 1))
    linear = PREVIEW_INTERPS.get(interp, interp) == PREVIEW_LINEAR
    if linear and ns > 1:
        jf = np.minimum(np.floor(s), float(ns - 2))
        j = jf.astype(np.int64)
        lo, hi = sg[:, j, :], sg[:, j + 1, :]  # [batch, n, dv+1, dim_p]
        p = lo + (s - jf)[None, :, :, None] * (hi - lo)
    else:
        p = sg[:, np.floor(s).astype(np.int64), :]
    rows = np.transpose(p, (1, 0, 2, 3)).reshape(len(t), sg.shape[0], (dv + 1) * dim_p).astype(sig.dtype)
    return rows[:, 0] if bcast else rows


class CgmresHipError(RuntimeError):
    pass


_lib = None


def lib_path():
    """The in-tree library; CGMRES_HIP_LIB overrides it (A/B builds of the kernels, tools/ab_build.py)."""
    return os.environ.get("CGMRES_HIP_LIB") or _build.LIB_PATH


def load():
    """Loads libcgmres_hip.so (never builds implicitly; see cgmres_cpp_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise CgmresHipError(f"{path} is missing: build it with `python -m cgmres_cpp_amd.build` "
                             "(there is no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    lib.cgmres_hip_last_error.restype = C.c_char_p
    lib.cgmres_hip_model_info.argtypes = [i32, C.POINTER(i32), C.POINTER(C.c_double)]
    lib.cgmres_hip_default_config.argtypes = [i32, C.POINTER(Config)]
    lib.cgmres_hip_model_probe.argtypes = [i32, i32] + [C.POINTER(C.c_double)] * 5
    lib.cgmres_hip_selftest_sincos.argtypes = [i32, C.POINTER(C.c_double), i32, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double)]
    lib.cgmres_hip_register_operator.argtypes = [C.c_char_p, C.POINTER(i32)]
    lib.cgmres_hip_operator_info.argtypes = [i32, C.POINTER(i32)]
    lib.cgmres_hip_operator_plan.argtypes = [i32, i32, C.POINTER(i32)]
    lib.cgmres_hip_gmres_user.argtypes = [i32, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp]
    lib.cgmres_hip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.cgmres_hip_destroy.argtypes = [vp]
    lib.cgmres_hip_get_config.argtypes = [vp, C.POINTER(Config)]
    lib.cgmres_hip_variant_name.argtypes = [vp]
    lib.cgmres_hip_variant_name.restype = C.c_char_p
    lib.cgmres_hip_set_ptau.argtypes = [vp, vp, C.c_int]
    lib.cgmres_hip_set_ptau_repeat.argtypes = [vp, vp, C.c_int]
    lib.cgmres_hip_init_u0.argtypes = [vp, vp, C.c_int]
    lib.cgmres_hip_init_u0_newton.argtypes = [vp, vp, vp, vp, i32]
    lib.cgmres_hip_control.argtypes = [vp, vp, vp]
    lib.cgmres_hip_control_device.argtypes = [vp, vp, vp]
    lib.cgmres_hip_closed_loop_device.argtypes = [vp, vp, vp, i32]
    lib.cgmres_hip_closed_loop_device_ptau.argtypes = [vp, vp, vp, i32, vp, C.c_int]
    lib.cgmres_hip_closed_loop_device_ex.argtypes = [vp, vp, vp, i32, C.POINTER(LoopInputs)]
    lib.cgmres_hip_synchronize.argtypes = [vp]
    lib.cgmres_hip_shard_bounds.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.cgmres_hip_get_time.argtypes = [vp, C.POINTER(C.c_double)]
    lib.cgmres_hip_get_state.argtypes = [vp, C.POINTER(C.c_double), vp, vp]
    lib.cgmres_hip_set_state.argtypes = [vp, C.c_double, vp, vp]
    lib.cgmres_hip_get_status.argtypes = [vp, vp, vp]
    lib.cgmres_hip_get_krylov.argtypes = [vp, vp, vp, vp, vp]
    lib.cgmres_hip_F_func.argtypes = [vp, vp, vp, vp, C.c_double]
    lib.cgmres_hip_prepare.argtypes = [vp, vp, vp]
    lib.cgmres_hip_Ax_func.argtypes = [vp, vp, vp]
    lib.cgmres_hip_gmres.argtypes = [vp, vp, vp]
    lib.cgmres_hip_timer_start.argtypes = [vp]
    lib.cgmres_hip_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.cgmres_hip_malloc.argtypes = [vp, C.POINTER(vp), C.c_uint64]
    lib.cgmres_hip_free.argtypes = [vp, vp]
    lib.cgmres_hip_memcpy_h2d.argtypes = [vp, vp, vp, C.c_uint64]
    lib.cgmres_hip_memcpy_d2h.argtypes = [vp, vp, vp, C.c_uint64]
    if hasattr(lib, "cgmres_hip_horizon_device"):  # (absent from A/B builds of older sources, tools/ab_build.py)
        lib.cgmres_hip_horizon_device.argtypes = [vp, vp, C.POINTER(Horizon)]
    if hasattr(lib, "cgmres_hip_closed_loop_device_rec"):  # (absent from A/B builds of older sources, tools/ab_build.py)
        lib.cgmres_hip_ensemble_device.argtypes = [vp, vp, vp, C.POINTER(EnsembleOut)]
        lib.cgmres_hip_closed_loop_device_rec.argtypes = [vp, vp, vp, i32, C.POINTER(LoopInputs), C.POINTER(LoopRecord)]
        lib.cgmres_hip_record_plan.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i32)]
    if hasattr(lib, "cgmres_hip_closed_loop_device_plant"):  # (absent from A/B builds of older sources, tools/ab_build.py)
        lib.cgmres_hip_plant_info.argtypes = [i32, C.POINTER(i32), C.POINTER(C.c_double), i32]
        lib.cgmres_hip_plant_step_device.argtypes = [vp, vp, vp, C.POINTER(LoopPlant)]
        lib.cgmres_hip_closed_loop_device_plant.argtypes = [vp, vp, vp, i32, C.POINTER(LoopInputs), C.POINTER(LoopRecord),
                                                            C.POINTER(LoopPlant)]
    if hasattr(lib, "cgmres_hip_closed_loop_device_preview"):  # (absent from A/B builds of older sources, tools/ab_build.py)
        lib.cgmres_hip_closed_loop_device_preview.argtypes = [vp, vp, vp, i32, C.POINTER(LoopInputs), C.POINTER(LoopRecord),
                                                              C.POINTER(LoopPlant), C.POINTER(LoopPreview)]
        lib.cgmres_hip_preview_device.argtypes = [vp, C.POINTER(LoopPreview), i32, vp]
    if hasattr(lib, "cgmres_hip_state_rows"):  # (absent from A/B builds of older sources, tools/ab_build.py)
        lib.cgmres_hip_state_rows.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise CgmresHipError(f"cgmres_hip error {rc}: {load().cgmres_hip_last_error().decode()}")


def record_plan(n_ticks, stride):
    """cgmres_hip_record_plan: (n_rec, launch_ticks) — the records and the tick counts of the launches of a recorded closed
    loop of n_ticks at `stride` on the mappings that fuse ticks.  No GPU."""
    n_rec, n_l = C.c_int32(), C.c_int32()
    _check(load().cgmres_hip_record_plan(int(n_ticks), int(stride), C.byref(n_rec), None, 0, C.byref(n_l)))
    sizes = (C.c_int32 * max(1, n_l.value))()
    _check(load().cgmres_hip_record_plan(int(n_ticks), int(stride), C.byref(n_rec), sizes, n_l.value, C.byref(n_l)))
    return n_rec.value, list(sizes[:n_l.value])


def device_count():
    return load().cgmres_hip_device_count()


def model_info(model):
    """dict(dim_x, dim_u, dim_p, dv, k_max, dt, h, zeta, Tf, alpha, tol): the Model constants of the registry."""
    model = MODEL_IDS.get(model, model)
    d = (C.c_int32 * 5)()
    t = (C.c_double * 6)()
    _check(load().cgmres_hip_model_info(model, d, t))
    return dict(zip(("dim_x", "dim_u", "dim_p", "dv", "k_max"), list(d)),
                **dict(zip(("dt", "h", "zeta", "Tf", "alpha", "tol"), list(t))))


def plant_info(model):
    """cgmres_hip_plant_info: dict(n_theta, nominal [n_theta]) — the plant parameters of a model, in the order of theta
    (pendulum: As, Bs, A52, C22, A32a, A32, A32b; msd: m1, m2, d1, d2, k1, k2; semiactive: a, b; a user model: none).  No GPU."""
    model = MODEL_IDS.get(model, model)
    n = C.c_int32()
    _check(load().cgmres_hip_plant_info(model, C.byref(n), None, 0))
    nom = (C.c_double * max(1, n.value))()
    _check(load().cgmres_hip_plant_info(model, C.byref(n), nom, n.value))
    return dict(n_theta=n.value, nominal=np.array(nom[:n.value], dtype=np.float64))


def model_probe(model, x, u, p, lmd, device=0):
    """Device evaluation of [dxdt | dPhidx | dHdx | dHdu] at one point (registry fingerprint)."""
    model = MODEL_IDS.get(model, model)
    mi = model_info(model)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, u, p if mi["dim_p"] else np.zeros(1), lmd)]
    out = np.empty(3 * mi["dim_x"] + mi["dim_u"])
    dp = C.POINTER(C.c_double)
    _check(load().cgmres_hip_model_probe(model, device, *[a.ctypes.data_as(dp) for a in arrs],
                                         out.ctypes.data_as(dp)))
    nx = mi["dim_x"]
    return out[:nx], out[nx:2 * nx], out[2 * nx:3 * nx], out[3 * nx:]


def selftest_sincos(a, device=0):
    """(sin, cos) of the fp64 arguments `a` as computed by the device routine of the horizon sweeps."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    s, c = np.empty_like(a), np.empty_like(a)
    dp = C.POINTER(C.c_double)
    _check(load().cgmres_hip_selftest_sincos(device, a.ctypes.data_as(dp), a.size, s.ctypes.data_as(dp),
                                             c.ctypes.data_as(dp)))
    return s, c


def gmres_user(op_id, x0, b, k_max, tol, params=None, device=0):
    """Gmres::gmres(x, b) (reference include/gmres.hpp:28-112) with a registered device operator (plugin.register_operator)
    for a batch of independent systems: x0, b [batch, len]; params [batch, n_params].  Returns (x, n_ax, reason)."""
    d = (C.c_int32 * 2)()
    _check(load().cgmres_hip_operator_info(op_id, d))
    L, npar = d[0], d[1]
    x = np.array(np.asarray(x0, dtype=np.float64).reshape(-1, L))
    bb = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, L))
    B = len(x)
    if len(bb) != B:
        raise ValueError("x0 and b must have the same batch")
    pp = None
    if npar:
        pp = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, npar), (B, npar)))
    n_ax = np.empty(B, dtype=np.int32)
    why = np.empty(B, dtype=np.int32)
    _check(load().cgmres_hip_gmres_user(op_id, device, B, int(k_max), float(tol), pp.ctypes.data if npar else None,
                                        x.ctypes.data, bb.ctypes.data, n_ax.ctypes.data, why.ctypes.data))
    return x, n_ax, why


def operator_plan(op_id, k_max):
    """cgmres_hip_operator_plan: (form, mapping) of a k_max solve with a registered operator — form "serial" (Op::Ax on
    one lane) | "row" (Op::Ax_row on all lanes), mapping "lane" | "wave" (one lane / one wavefront per system).  No GPU."""
    out = (C.c_int32 * 2)()
    _check(load().cgmres_hip_operator_plan(op_id, int(k_max), out))
    return ("serial", "row")[out[0]], ("lane", "wave")[out[1]]


class DeviceBuffer:
    """A raw HBM allocation owned through the C ABI (used where no torch tensor is at hand)."""

    def __init__(self, ctrl, shape, dtype):
        self._ctrl = ctrl
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(load().cgmres_hip_malloc(ctrl._h, C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes
        _check(load().cgmres_hip_memcpy_h2d(self._ctrl._h, self.ptr, a.ctypes.data, self.nbytes))
        return self

    def download(self):
        a = np.empty(self.shape, dtype=self.dtype)
        _check(load().cgmres_hip_memcpy_d2h(self._ctrl._h, a.ctypes.data, self.ptr, self.nbytes))
        return a

    def free(self):
        if self.ptr and self._ctrl._h:
            _check(load().cgmres_hip_free(self._ctrl._h, self.ptr))
        self.ptr = None


def parse_dtype(dtype):
    """F64 / F32 from 'f64' | 'float64' | np.float64 | torch.float64 | F64 (and the fp32 spellings); anything else is a
    TypeError — a silent fp64 default would make the kernels read 8-byte elements from a caller's 4-byte buffers."""
    if isinstance(dtype, (int, np.integer)) and not isinstance(dtype, bool) and int(dtype) in (F64, F32):
        return int(dtype)
    name = dtype if isinstance(dtype, str) else None
    if name is None and dtype is not None:
        s = str(dtype)
        if s.startswith("torch."):
            name = s[6:]
        else:
            try:
                name = np.dtype(dtype).name
            except TypeError:
                name = None
    table = {"f64": F64, "float64": F64, "double": F64, "f32": F32, "float32": F32, "float": F32, "single": F32}
    if name not in table:
        raise TypeError(f"dtype must be fp64 or fp32, got {dtype!r}")
    return table[name]


def _ptr(a, dtype=None, numel=None):
    """Device/host address of a numpy array, a DeviceBuffer, a torch tensor or a raw int.  With dtype/numel the
    element type and element count of typed containers are checked (raw ints cannot be)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    have_dt, have_n = None, None
    if isinstance(a, DeviceBuffer):
        ptr, have_dt, have_n = a.ptr, a.dtype, int(np.prod(a.shape))
    elif isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        ptr, have_dt, have_n = a.ctypes.data, a.dtype, a.size
    elif hasattr(a, "data_ptr"):
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        ptr, have_n = a.data_ptr(), int(a.numel())
        have_dt = np.dtype(str(a.dtype)[6:]) if str(a.dtype).startswith("torch.") else None
    else:
        raise TypeError(type(a))
    if dtype is not None and have_dt is not None and np.dtype(have_dt) != np.dtype(dtype):
        raise TypeError(f"buffer holds {np.dtype(have_dt).name}, the controller computes in {np.dtype(dtype).name}")
    if numel is not None and have_n is not None and have_n != numel:
        raise ValueError(f"buffer holds {have_n} elements, expected {numel}")
    return ptr


class CgmresBatch:
    """`batch` reference controllers (``Cgmres<Model>``, include/cgmres.hpp:9) advancing in lock-step on one GPU.

    Method names, argument meaning and defaults follow the reference class; every vector gains a leading
    batch axis.  ``dv`` / ``k_max`` / ``tol`` and the tuning constants default to the Model's shipped
    ``static constexpr`` values (e.g. arm_type_inverted_pendulum/model.hpp:21-35).
    """

    def __init__(self, model, batch=1, dv=None, k_max=None, tol=None, dtype="f64", device=0, stream=None,
                 variant=0, flags=0, **tuning):
        lib = load()
        self.model = MODEL_IDS.get(model, model)
        cfg = Config()
        _check(lib.cgmres_hip_default_config(self.model, C.byref(cfg)))
        cfg.batch = int(batch)
        cfg.dtype = parse_dtype(dtype)
        if dv is not None:
            cfg.dv = int(dv)
        if k_max is not None:
            cfg.k_max = int(k_max)
        if tol is not None and tol >= 0:
            cfg.tol = float(tol)
        for k, v in tuning.items():
            if k not in ("dt", "h", "zeta", "Tf", "alpha"):
                raise TypeError(f"unknown tuning constant {k}")
            setattr(cfg, k, float(v))
        cfg.device = int(device)
        cfg.variant = int(variant)
        cfg.flags = int(flags)
        cfg.stream = stream
        self._h = None
        h = C.c_void_p()
        _check(lib.cgmres_hip_create(C.byref(cfg), C.byref(h)))
        self._h = h.value
        _check(lib.cgmres_hip_get_config(self._h, C.byref(cfg)))  # resolved variant
        self.cfg = cfg
        self.variant = cfg.variant
        self.variant_name = lib.cgmres_hip_variant_name(self._h).decode()  # "lane" | "wg" | "wg-lean" | "wg+parallel-costate"
        mi = model_info(self.model)
        self.dim_x, self.dim_u, self.dim_p = mi["dim_x"], mi["dim_u"], mi["dim_p"]
        self.batch, self.dv, self.k_max = cfg.batch, cfg.dv, cfg.k_max
        self.len = self.dim_u * self.dv
        self.dt, self.h, self.zeta, self.Tf, self.alpha, self.tol = cfg.dt, cfg.h, cfg.zeta, cfg.Tf, cfg.alpha, cfg.tol
        self.np_dtype = np.float32 if cfg.dtype == F32 else np.float64

    def close(self):
        if self._h:
            load().cgmres_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ----------------------------------------------------------------------------------
    def _host(self, a, shape, allow_broadcast=False):
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        if allow_broadcast and a.size == int(np.prod(shape[1:])):
            return a.reshape(shape[1:]), 0
        if a.size != int(np.prod(shape)):
            raise ValueError(f"expected {shape}, got {a.shape}")
        return a.reshape(shape), 1

    def device_buffer(self, shape, dtype=None):
        return DeviceBuffer(self, shape, dtype or self.np_dtype)

    # -- setup, cgmres.hpp:36-76 ------------------------------------------------------------------
    def set_ptau(self, ptau):
        if self.dim_p == 0:
            return
        a, per = self._host(ptau, (self.batch, self.dim_p * (self.dv + 1)), True)
        _check(load().cgmres_hip_set_ptau(self._h, a.ctypes.data, per))

    def set_ptau_repeat(self, p):
        if self.dim_p == 0:
            return
        a, per = self._host(p, (self.batch, self.dim_p), True)
        _check(load().cgmres_hip_set_ptau_repeat(self._h, a.ctypes.data, per))

    def init_u0(self, u0):
        a, per = self._host(u0, (self.batch, self.dim_u), True)
        _check(load().cgmres_hip_init_u0(self._h, a.ctypes.data, per))

    def init_u0_newton(self, u0, x0, p0=None, n_loop=10):
        """Returns the refined u0 [batch, dim_u] (the reference updates the caller's u0 in place)."""
        u = np.array(np.broadcast_to(np.asarray(u0, dtype=self.np_dtype).reshape(-1, self.dim_u),
                                     (self.batch, self.dim_u)))
        x = np.array(np.broadcast_to(np.asarray(x0, dtype=self.np_dtype).reshape(-1, self.dim_x),
                                     (self.batch, self.dim_x)))
        if self.dim_p:
            p = np.array(np.broadcast_to(np.asarray(p0, dtype=self.np_dtype).reshape(-1, self.dim_p),
                                         (self.batch, self.dim_p)))
            pp = p.ctypes.data
        else:
            pp = None
        _check(load().cgmres_hip_init_u0_newton(self._h, u.ctypes.data, x.ctypes.data, pp, int(n_loop)))
        return u

    # -- the hot path, cgmres.hpp:78-110 ------------------------------------------------------------
    def control(self, x):
        """One tick. x [batch, dim_x] host array -> u [batch, dim_u]."""
        a, _ = self._host(x, (self.batch, self.dim_x))
        u = np.empty((self.batch, self.dim_u), dtype=self.np_dtype)
        _check(load().cgmres_hip_control(self._h, u.ctypes.data, a.ctypes.data))
        return u

    def control_device(self, u_dev, x_dev):
        _check(load().cgmres_hip_control_device(self._h, _ptr(u_dev, self.np_dtype, self.batch * self.dim_u),
                                                _ptr(x_dev, self.np_dtype, self.batch * self.dim_x)))

    def _loop_inputs(self, n_ticks, ptau_seq_dev, per_instance, dist_seq_dev, meas_seq_dev, dist_per_instance, meas_per_instance):
        """struct cgmres_hip_loop_inputs of a call, element counts of typed buffers checked."""
        li = LoopInputs(struct_size=C.sizeof(LoopInputs), ptau_per_instance=1 if per_instance else 0,
                        dist_per_instance=1 if dist_per_instance else 0, meas_per_instance=1 if meas_per_instance else 0)

        def count(per, width):  # (a negative n_ticks is the library's to refuse)
            return int(n_ticks) * (self.batch if per else 1) * width if int(n_ticks) >= 0 else None
        li.ptau_seq_dev = _ptr(ptau_seq_dev, self.np_dtype, count(per_instance, self.dim_p * (self.dv + 1)))
        li.dist_seq_dev = _ptr(dist_seq_dev, self.np_dtype, count(dist_per_instance, self.dim_x))
        li.meas_seq_dev = _ptr(meas_seq_dev, self.np_dtype, count(meas_per_instance, self.dim_x))
        return li

    def closed_loop_device(self, x_dev, u_dev, n_ticks, ptau_seq_dev=None, per_instance=True, *, dist_seq_dev=None,
                           meas_seq_dev=None, dist_per_instance=True, meas_per_instance=True, record=None, plant=None,
                           preview=None):
        """n_ticks of the example main loop on the device.  ptau_seq_dev: optional device array of per-tick parameter
        horizons, [n_ticks, batch, dim_p*(dv+1)] (per_instance) or [n_ticks, dim_p*(dv+1)] — `set_ptau` before every tick.
        dist_seq_dev / meas_seq_dev: optional device arrays [n_ticks, batch, dim_x] (or [n_ticks, dim_x], broadcast) of a
        process disturbance d and a measurement noise v: y_k = x_k + v_k, u_k = control(y_k),
        x_{k+1} = (x_k + f(x_k, u_k)*dt) + d_k; x_dev holds the TRUE state (cgmres_hip_closed_loop_device_ex).
        record: a dict(stride=1, x=, u=, n_ax=, reason=, t=, centre=, moments=, counts=) of device buffers (t: a host float64
        array), every one optional — every stride-th tick is recorded into them (cgmres_hip_closed_loop_device_rec).
        plant: a Plant — x_{k+1} = Phi(x_k, u_k) + d_k with its integrator, substeps and parameters instead of the model's
        Euler step, one tick per launch (cgmres_hip_closed_loop_device_plant).
        preview: a Preview — every tick's ptau is formed on the device from its sampled signal and the handle's own t and
        dtau, instead of ptau_seq_dev (cgmres_hip_closed_loop_device_preview)."""
        xp = _ptr(x_dev, self.np_dtype, self.batch * self.dim_x)
        up = _ptr(u_dev, self.np_dtype, self.batch * self.dim_u)
        if preview is not None:
            li = self._loop_inputs(n_ticks, ptau_seq_dev, per_instance, dist_seq_dev, meas_seq_dev, dist_per_instance,
                                   meas_per_instance)
            lr = self._loop_record(n_ticks, **record) if record is not None else None
            lp = self._loop_plant(plant) if plant is not None else None
            lv = self._loop_preview(preview)
            _check(load().cgmres_hip_closed_loop_device_preview(self._h, xp, up, int(n_ticks), C.byref(li),
                                                                C.byref(lr) if lr is not None else None,
                                                                C.byref(lp) if lp is not None else None, C.byref(lv)))
            return
        if ptau_seq_dev is not None and self.dim_p == 0:
            ptau_seq_dev = None
        if plant is not None:
            li = self._loop_inputs(n_ticks, ptau_seq_dev, per_instance, dist_seq_dev, meas_seq_dev, dist_per_instance,
                                   meas_per_instance)
            lr = self._loop_record(n_ticks, **record) if record is not None else None
            lp = self._loop_plant(plant)
            _check(load().cgmres_hip_closed_loop_device_plant(self._h, xp, up, int(n_ticks), C.byref(li),
                                                              C.byref(lr) if lr is not None else None, C.byref(lp)))
            return
        if record is not None:
            li = self._loop_inputs(n_ticks, ptau_seq_dev, per_instance, dist_seq_dev, meas_seq_dev, dist_per_instance,
                                   meas_per_instance)
            lr = self._loop_record(n_ticks, **record)
            _check(load().cgmres_hip_closed_loop_device_rec(self._h, xp, up, int(n_ticks), C.byref(li), C.byref(lr)))
            return
        if dist_seq_dev is None and meas_seq_dev is None:
            if ptau_seq_dev is None:
                _check(load().cgmres_hip_closed_loop_device(self._h, xp, up, int(n_ticks)))
            else:
                n = int(n_ticks) * (self.batch if per_instance else 1) * self.dim_p * (self.dv + 1)
                _check(load().cgmres_hip_closed_loop_device_ptau(self._h, xp, up, int(n_ticks),
                                                                 _ptr(ptau_seq_dev, self.np_dtype, n), 1 if per_instance else 0))
            return
        li = self._loop_inputs(n_ticks, ptau_seq_dev, per_instance, dist_seq_dev, meas_seq_dev, dist_per_instance,
                               meas_per_instance)
        _check(load().cgmres_hip_closed_loop_device_ex(self._h, xp, up, int(n_ticks), C.byref(li)))

    # -- the preview of a sampled reference signal -------------------------------------------------------
    def _loop_preview(self, preview):
        """struct cgmres_hip_loop_preview of a Preview; a typed sig buffer is checked for element type and count (one signal
        or one per instance, decided by its shape) before its address crosses the ABI."""
        interp = preview.interp
        lv = LoopPreview(struct_size=C.sizeof(LoopPreview), t0=preview.t0, ts=preview.ts,
                         interp=PREVIEW_INTERPS[interp] if isinstance(interp, str) else int(interp))
        sg, dim_p = preview.sig, self.dim_p
        shape = tuple(sg.shape) if hasattr(sg, "shape") else None
        if shape is not None:
            if len(shape) not in (2, 3) or (dim_p and shape[-1] != dim_p) or (len(shape) == 3 and shape[0] != self.batch):
                raise ValueError(f"preview sig must be [n_samples, {dim_p}] or [{self.batch}, n_samples, {dim_p}], got {shape}")
            per, n_samples = len(shape) == 3, shape[-2]
            if preview.per_instance is not None and bool(preview.per_instance) != per:
                raise ValueError(f"preview per_instance={preview.per_instance} contradicts the signal's shape {shape}")
        else:
            if sg is not None and (preview.per_instance is None or preview.n_samples is None):
                raise ValueError("a raw sig address needs per_instance and n_samples")
            per, n_samples = bool(preview.per_instance), preview.n_samples if preview.n_samples is not None else 1
        lv.sig_per_instance, lv.n_samples = 1 if per else 0, int(n_samples)
        lv.sig_dev = _ptr(sg, self.np_dtype, None if shape is None else int(np.prod(shape)))
        return lv

    def preview_device(self, preview, n_ticks, rows):
        """The rows a loop with this Preview would use for its next n_ticks ticks from the handle's current time, into the
        device buffer rows [n_ticks, batch, dim_p*(dv+1)]; on the stream, changes no state (cgmres_hip_preview_device)."""
        lv = self._loop_preview(preview)
        n = int(n_ticks) * self.batch * self.dim_p * (self.dv + 1) if int(n_ticks) >= 0 else None
        _check(load().cgmres_hip_preview_device(self._h, C.byref(lv), int(n_ticks), _ptr(rows, self.np_dtype, n)))

    # -- a plant of its own ----------------------------------------------------------------------------
    def _loop_plant(self, plant):
        """struct cgmres_hip_loop_plant of a Plant; a typed theta buffer is checked for element type and count (one row or
        one row per instance) before its address crosses the ABI."""
        integ = plant.integrator
        lp = LoopPlant(struct_size=C.sizeof(LoopPlant), substeps=int(plant.substeps),
                       integrator=PLANT_INTEGRATORS[integ] if isinstance(integ, str) else int(integ))
        th = plant.theta
        if th is not None:
            n_theta = plant_info(self.model)["n_theta"]
            numel = int(np.prod(th.shape)) if hasattr(th, "shape") else None
            per = numel is not None and numel == self.batch * n_theta and (self.batch > 1 or len(th.shape) > 1)
            if plant.theta_per_instance is not None:
                per = bool(plant.theta_per_instance)
            lp.theta_per_instance = 1 if per else 0
            lp.theta_dev = _ptr(th, self.np_dtype, None if numel is None or n_theta == 0 else (self.batch if per else 1) * n_theta)
        return lp

    def plant_step_device(self, x_dev, u_dev, plant):
        """One plant step on the stream, x_dev <- Phi(x_dev, u_dev) with the Plant's integrator, substeps and theta; no d,
        no v, no controller state changes (cgmres_hip_plant_step_device)."""
        lp = self._loop_plant(plant)
        _check(load().cgmres_hip_plant_step_device(self._h, _ptr(x_dev, self.np_dtype, self.batch * self.dim_x),
                                                   _ptr(u_dev, self.np_dtype, self.batch * self.dim_u), C.byref(lp)))

    # -- the record of a closed loop and the ensemble of a batch ----------------------------------------
    def _loop_record(self, n_ticks, stride=1, x=None, u=None, n_ax=None, reason=None, t=None, centre=None, moments=None,
                     counts=None):
        """struct cgmres_hip_loop_record; typed buffers are checked for element type and count before their address
        crosses the ABI (a stride < 1 or a negative n_ticks is the library's to refuse: nothing is checked then)."""
        ok = int(stride) >= 1 and int(n_ticks) >= 0
        n_rec = int(n_ticks) // int(stride) if ok else None
        nc = self.dim_x + self.dim_u

        def count(width):
            return n_rec * width if ok else None
        if t is not None and not (isinstance(t, np.ndarray) and t.dtype == np.float64):
            raise TypeError("record t must be a host float64 numpy array")
        return LoopRecord(struct_size=C.sizeof(LoopRecord), stride=int(stride),
                          x_log_dev=_ptr(x, self.np_dtype, count(self.batch * self.dim_x)),
                          u_log_dev=_ptr(u, self.np_dtype, count(self.batch * self.dim_u)),
                          n_ax_log_dev=_ptr(n_ax, np.int32, count(self.batch)),
                          reason_log_dev=_ptr(reason, np.int32, count(self.batch)),
                          t_host=_ptr(t, np.float64, count(1)), centre_dev=_ptr(centre, np.float64, nc),
                          moments_log_dev=_ptr(moments, np.float64, count(nc * 4)),
                          counts_log_dev=_ptr(counts, np.int32, count(self.k_max + 7)))

    def ensemble_device(self, x_dev, u_dev, moments=None, counts=None, centre=None):
        """The statistics of one row of the batch on the stream (cgmres_hip_ensemble_device): moments [dim_x+dim_u, 4] =
        {s1, s2, min, max} of double(value) - centre over the instances whose row is finite, counts [k_max+7] = histogram
        of n_ax, instances per exit code, counting instances; float64 / int32 device buffers, centre [dim_x+dim_u] float64."""
        nc = self.dim_x + self.dim_u
        out = EnsembleOut(struct_size=C.sizeof(EnsembleOut), reserved=0, centre_dev=_ptr(centre, np.float64, nc),
                          moments_dev=_ptr(moments, np.float64, nc * 4), counts_dev=_ptr(counts, np.int32, self.k_max + 7))
        _check(load().cgmres_hip_ensemble_device(self._h, _ptr(x_dev, self.np_dtype, self.batch * self.dim_x),
                                                 _ptr(u_dev, self.np_dtype, self.batch * self.dim_u), C.byref(out)))

    def closed_loop_record(self, x, n_ticks, stride=1, centre=None, u=None, ptau_seq=None, per_instance=True, dist_seq=None,
                           meas_seq=None, dist_per_instance=True, meas_per_instance=True, plant=None, preview=None):
        """The convenience form: n_ticks of the device loop from the host state x [batch, dim_x], every stride-th tick
        recorded; the sequences are host arrays.  Allocates, runs, synchronises and returns numpy arrays:
        dict(t [n_rec], x [n_rec, batch, dim_x], u [n_rec, batch, dim_u], n_ax, reason [n_rec, batch],
        moments [n_rec, dim_x+dim_u, 4], counts [n_rec, k_max+7], x_end, u_end).  plant: a Plant whose theta, if any, is a HOST
        array [batch, n_theta] or [n_theta]; preview: a Preview whose sig may be a HOST
        array [batch, n_samples, dim_p] or [n_samples, dim_p]."""
        n_ticks, stride = int(n_ticks), int(stride)
        n_rec, nc, B = n_ticks // stride, self.dim_x + self.dim_u, self.batch
        bufs = []

        def dev(shape, dtype=None, init=None):
            b = self.device_buffer(shape, dtype)
            bufs.append(b)
            return b.upload(init) if init is not None else b

        def seq(a, per, width):
            if a is None:
                return None
            shape = (n_ticks, B, width) if per else (n_ticks, width)
            return dev(shape, init=np.asarray(a, dtype=self.np_dtype).reshape(shape))
        try:
            xd = dev((B, self.dim_x), init=self._host(x, (B, self.dim_x))[0])
            ud = dev((B, self.dim_u), init=np.zeros((B, self.dim_u)) if u is None else self._host(u, (B, self.dim_u))[0])
            t = np.zeros(n_rec)
            rec = dict(stride=stride, x=dev((n_rec, B, self.dim_x)), u=dev((n_rec, B, self.dim_u)),
                       n_ax=dev((n_rec, B), np.int32), reason=dev((n_rec, B), np.int32), t=t,
                       centre=None if centre is None else dev((nc,), np.float64, np.asarray(centre, dtype=np.float64)),
                       moments=dev((n_rec, nc, 4), np.float64), counts=dev((n_rec, self.k_max + 7), np.int32))
            if plant is not None and plant.theta is not None and isinstance(plant.theta, (np.ndarray, list, tuple)):
                th = np.asarray(plant.theta, dtype=self.np_dtype)
                plant = Plant(plant.integrator, plant.substeps, dev(th.shape, init=th), plant.theta_per_instance)
            if preview is not None and isinstance(preview.sig, (np.ndarray, list, tuple)):
                sg = np.asarray(preview.sig, dtype=self.np_dtype)
                preview = Preview(dev(sg.shape, init=sg), preview.ts, preview.t0, preview.interp, preview.per_instance)
            self.closed_loop_device(xd, ud, n_ticks, seq(ptau_seq, per_instance, self.dim_p * (self.dv + 1)) if self.dim_p else None,
                                    per_instance, dist_seq_dev=seq(dist_seq, dist_per_instance, self.dim_x),
                                    meas_seq_dev=seq(meas_seq, meas_per_instance, self.dim_x),
                                    dist_per_instance=dist_per_instance, meas_per_instance=meas_per_instance, record=rec,
                                    plant=plant, preview=preview)
            out = {k: rec[k].download() for k in ("x", "u", "n_ax", "reason", "moments", "counts")}  # (blocks on the stream)
            out.update(t=t, x_end=xd.download(), u_end=ud.download())
            return out
        finally:
            for b in bufs:
                b.free()

    def synchronize(self):
        _check(load().cgmres_hip_synchronize(self._h))

    # -- the predicted horizon and the optimality error, cgmres.hpp:113-162 ---------------------------
    def horizon_device(self, x_dev, xtau=None, ltau=None, F=None, fnorm=None):
        """F_func(ret, U, x, t) with the handle's current U, ptau and t at x_dev [batch, dim_x], on the stream (no copy, no
        synchronise): fills the device arrays given — xtau, ltau [batch, dv+1, dim_x], F [batch, dim_u*dv], fnorm [batch] =
        ||F|| — and leaves the controller state alone (cgmres_hip_horizon_device)."""
        n_traj = self.batch * (self.dv + 1) * self.dim_x
        out = Horizon(struct_size=C.sizeof(Horizon), reserved=0,
                      xtau_dev=_ptr(xtau, self.np_dtype, n_traj), ltau_dev=_ptr(ltau, self.np_dtype, n_traj),
                      F_dev=_ptr(F, self.np_dtype, self.batch * self.len), fnorm_dev=_ptr(fnorm, self.np_dtype, self.batch))
        _check(load().cgmres_hip_horizon_device(self._h, _ptr(x_dev, self.np_dtype, self.batch * self.dim_x), C.byref(out)))

    def _horizon_host(self, x, names):
        xd = None
        if isinstance(x, (DeviceBuffer, int)) or hasattr(x, "data_ptr"):
            x_dev = x
        else:
            x_dev = xd = self.device_buffer((self.batch, self.dim_x)).upload(self._host(x, (self.batch, self.dim_x))[0])
        shapes = {"xtau": (self.batch, self.dv + 1, self.dim_x), "ltau": (self.batch, self.dv + 1, self.dim_x),
                  "F": (self.batch, self.len), "fnorm": (self.batch,)}
        bufs = {k: self.device_buffer(shapes[k]) for k in names}
        try:
            self.horizon_device(x_dev, **bufs)
            return tuple(bufs[k].download() for k in names)  # (memcpy_d2h is stream-ordered and blocks)
        finally:
            for b in list(bufs.values()) + ([xd] if xd is not None else []):
                b.free()

    def horizon(self, x):
        """(xtau, ltau, F, fnorm) as numpy arrays for a host or device x [batch, dim_x]: what the controllers predict the
        plant will do over the horizon, the costates, the optimality residual and its norm."""
        return self._horizon_host(x, ("xtau", "ltau", "F", "fnorm"))

    def opt_error(self, x):
        """||F(U, x, t)|| per instance [batch]: the optimality error, the health figure of C/GMRES."""
        return self._horizon_host(x, ("fnorm",))[0]

    # -- state ------------------------------------------------------------------------------------
    @property
    def t(self):
        t = C.c_double()
        _check(load().cgmres_hip_get_time(self._h, C.byref(t)))
        return t.value

    def get_state(self):
        t = C.c_double()
        U = np.empty((self.batch, self.len), dtype=self.np_dtype)
        d = np.empty((self.batch, self.len), dtype=self.np_dtype)
        _check(load().cgmres_hip_get_state(self._h, C.byref(t), U.ctypes.data, d.ctypes.data))
        return t.value, U, d

    def set_state(self, t, U=None, dUdt=None):
        Ua = self._host(U, (self.batch, self.len))[0] if U is not None else None
        da = self._host(dUdt, (self.batch, self.len))[0] if dUdt is not None else None
        _check(load().cgmres_hip_set_state(self._h, float(t), _ptr(Ua), _ptr(da)))

    def state_rows(self):
        """(U, dUdt, pitch): device addresses of the controller state as the kernels keep it, [batch][pitch] scalars with
        pitch >= dim_u*dv (the words behind dim_u*dv of a row are pads no kernel reads or writes); None for a mapping
        that keeps its state in another form."""
        U, d, pitch = C.c_void_p(), C.c_void_p(), C.c_int32()
        _check(load().cgmres_hip_state_rows(self._h, C.byref(U), C.byref(d), C.byref(pitch)))
        return (U.value, d.value, pitch.value) if U.value else None

    def get_status(self):
        n = np.empty(self.batch, dtype=np.int32)
        r = np.empty(self.batch, dtype=np.int32)
        _check(load().cgmres_hip_get_status(self._h, n.ctypes.data, r.ctypes.data))
        return n, r

    def get_krylov(self, with_V=False):
        k1 = self.k_max + 1
        H = np.empty((self.batch, k1, k1), dtype=self.np_dtype)
        rho = np.empty((self.batch, k1), dtype=self.np_dtype)
        g = np.empty((self.batch, self.k_max, 3), dtype=self.np_dtype)
        V = np.empty((self.batch, k1, self.len), dtype=self.np_dtype) if with_V else None
        _check(load().cgmres_hip_get_krylov(self._h, _ptr(V), H.ctypes.data, rho.ctypes.data, g.ctypes.data))
        return V, H, rho, g

    # -- white-box hooks ----------------------------------------------------------------------------
    def F_func(self, U, x, t):
        Ua = self._host(U, (self.batch, self.len))[0]
        xa = self._host(x, (self.batch, self.dim_x))[0]
        r = np.empty((self.batch, self.len), dtype=self.np_dtype)
        _check(load().cgmres_hip_F_func(self._h, r.ctypes.data, Ua.ctypes.data, xa.ctypes.data, float(t)))
        return r

    def prepare(self, x):
        xa = self._host(x, (self.batch, self.dim_x))[0]
        b = np.empty((self.batch, self.len), dtype=self.np_dtype)
        _check(load().cgmres_hip_prepare(self._h, b.ctypes.data, xa.ctypes.data))
        return b

    def Ax_func(self, v):
        va = self._host(v, (self.batch, self.len))[0]
        o = np.empty((self.batch, self.len), dtype=self.np_dtype)
        _check(load().cgmres_hip_Ax_func(self._h, o.ctypes.data, va.ctypes.data))
        return o

    def gmres(self, x0, b):
        xa = self._host(x0, (self.batch, self.len))[0].copy()
        ba = self._host(b, (self.batch, self.len))[0]
        _check(load().cgmres_hip_gmres(self._h, xa.ctypes.data, ba.ctypes.data))
        return xa

    # -- measurement --------------------------------------------------------------------------------
    def timer_start(self):
        _check(load().cgmres_hip_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        _check(load().cgmres_hip_timer_stop(self._h, C.byref(ms)))
        return ms.value
