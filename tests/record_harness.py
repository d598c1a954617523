"""Shared by the tests of the recorded closed loop (cgmres_hip_closed_loop_device_rec) and of the ensemble kernel
(cgmres_hip_ensemble_device): the batch, noise and oracle helpers of tests/test_gpu_loop_inputs.py (copied: a test file is
not a library), the recorded run, the same loop cut by the caller, and the reference of the ensemble."""
import math

import numpy as np

import cgmres_cpp_amd as cg

B, DV, KM = 83, 50, 10
SIGMA = 1e-3
TOL64 = 1e-9  # the x, u bound of tests/test_gpu_loop_inputs.py, derived there


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


def oracle_rows(orc, model, x0, u0, p, i, n, d=None, v=None, dv=DV, km=KM, tol=1e-6):
    """The three statements of cgmres_hip_closed_loop_device_ex on the oracle for instance i, tick by tick (fp64):
    (x [n, nx] = x_{k+1}, u [n, nu] = u_k, n_ax [n], reason [n]).  d, v: [n, nx] rows of THIS instance (or None)."""
    r = orc.Controller(model, dv, km, tol, "f64")
    orc.start_controller(r, x0[i], u0[i], p[i])
    x = np.array(x0[i], dtype=np.float64)
    xs, us, ks, why = [], [], [], []
    for k in range(n):
        y = x if v is None else x + v[k]
        u = r.control(y)
        x = x + r.plant(x, u) * r.dt
        if d is not None:
            x = x + d[k]
        xs.append(x.copy()), us.append(np.array(u)), ks.append(r.last_solve()[0]), why.append(r.last_solve()[2])
    return np.array(xs), np.array(us), np.array(ks), np.array(why)


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self, c):
        self.c, self.bufs = c, []

    def __call__(self, a=None, shape=None, dtype=None):
        if a is None and shape is None:
            return None
        if a is not None:
            a = np.ascontiguousarray(a)
            b = self.c.device_buffer(a.shape, a.dtype).upload(a)
        else:
            b = self.c.device_buffer(shape, dtype)
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def final_state(c, xd, ud):
    """What two bit-identical loops must agree on: x, u, U, dUdt, n_ax, reason, t."""
    c.synchronize()
    t, U, dUdt = c.get_state()
    n_ax, reason = c.get_status()
    return dict(x=xd.download(), u=ud.download(), U=U, dUdt=dUdt, n_ax=n_ax, reason=reason, t=np.float64(t))


def run_recorded(c, x0, n, stride, d=None, v=None, seq=None, centre=None, logs=True, ensemble=True):
    """One call of closed_loop_device(record=...) -> (logs dict incl. t, final state dict)."""
    dev = Dev(c)
    n_rec, nc = n // stride, c.dim_x + c.dim_u
    xd, ud = dev(x0.astype(c.np_dtype)), dev(np.zeros((c.batch, c.dim_u), dtype=c.np_dtype))
    t = np.full(n_rec, np.nan)
    rec = dict(stride=stride, t=t, centre=dev(None if centre is None else np.asarray(centre, dtype=np.float64)))
    if logs:
        rec.update(x=dev(shape=(n_rec, c.batch, c.dim_x)), u=dev(shape=(n_rec, c.batch, c.dim_u)),
                   n_ax=dev(shape=(n_rec, c.batch), dtype=np.int32), reason=dev(shape=(n_rec, c.batch), dtype=np.int32))
    if ensemble:
        rec.update(moments=dev(shape=(n_rec, nc, 4), dtype=np.float64), counts=dev(shape=(n_rec, c.k_max + 7), dtype=np.int32))
    c.closed_loop_device(xd, ud, n, dev(seq), True, dist_seq_dev=dev(d), meas_seq_dev=dev(v), record=rec)
    end = final_state(c, xd, ud)
    out = {k: rec[k].download() for k in ("x", "u", "n_ax", "reason", "moments", "counts") if k in rec}
    out["t"] = t
    dev.free()
    return out, end


def run_caller_cut(c, x0, n, stride, d=None, v=None, seq=None):
    """The same loop cut by the caller: closed_loop_device (..._ex) once per stride window with the sequences offset, x, u
    and the status downloaded in between, then the tail.  -> (logs dict, final state dict)"""
    dev = Dev(c)
    xd, ud = dev(x0.astype(c.np_dtype)), dev(np.zeros((c.batch, c.dim_u), dtype=c.np_dtype))
    out = dict(x=[], u=[], n_ax=[], reason=[])

    def window(k0, k1):
        w = Dev(c)
        sl = [None if a is None else w(a[k0:k1]) for a in (seq, d, v)]
        c.closed_loop_device(xd, ud, k1 - k0, sl[0], True, dist_seq_dev=sl[1], meas_seq_dev=sl[2])
        c.synchronize()
        w.free()
    for j in range(n // stride):
        window(j * stride, (j + 1) * stride)
        n_ax, reason = c.get_status()
        out["x"].append(xd.download()), out["u"].append(ud.download()), out["n_ax"].append(n_ax), out["reason"].append(reason)
    if n % stride:
        window(n - n % stride, n)
    end = final_state(c, xd, ud)
    dev.free()
    shapes = dict(x=(0, c.batch, c.dim_x), u=(0, c.batch, c.dim_u), n_ax=(0, c.batch), reason=(0, c.batch))
    return {k: np.array(a) if a else np.empty(shapes[k]) for k, a in out.items()}, end


def krylov_written(c):
    """What the last solve wrote of get_krylov(), per instance, n = its Arnoldi count: columns 0..n-1 of H down to the
    subdiagonal, rho[0..n], g[0..n-1] (tests/test_gpu_horizon.py: the entries behind them are whatever the kernel's LDS
    held; two fresh handles already differ there)."""
    n_ax, _ = c.get_status()
    _, H, rho, g = c.get_krylov()
    return [np.concatenate([H[i, col, :col + 2] for col in range(n)] + [rho[i, :n + 1], g[i, :n].ravel()])
            for i, n in enumerate(n_ax)]


def same_bits(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- the reference of the ensemble --------------------------------------------------------------------------------------
def ensemble_ref(x, u, n_ax, reason, k_max, centre=None):
    """(moments [nc, 4], terms [nc, 2], counts [k_max+7], n): math.fsum over double(value) - centre and over its square, over
    the rows that are finite throughout; terms = sum |term| of the two sums (what the error bound scales with)."""
    rows = np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)], axis=1)
    nc = rows.shape[1]
    centre = np.zeros(nc) if centre is None else np.asarray(centre, dtype=np.float64)
    ok = np.all(np.isfinite(rows), axis=1)
    good = rows[ok]
    mom, terms = np.zeros((nc, 4)), np.zeros((nc, 2))
    for c in range(nc):
        z = [float(val) - float(centre[c]) for val in good[:, c]]
        zz = [a * a for a in z]
        mom[c] = [math.fsum(z), math.fsum(zz), np.min(good[:, c]) if len(good) else np.inf, np.max(good[:, c]) if len(good) else -np.inf]
        terms[c] = [math.fsum(abs(a) for a in z), math.fsum(zz)]
    counts = np.concatenate([np.bincount(n_ax, minlength=k_max + 1)[:k_max + 1], np.bincount(reason, minlength=5)[:5],
                             [int(ok.sum())]]).astype(np.int32)
    return mom, terms, counts, int(ok.sum())


def check_ensemble(moments, counts, x, u, n_ax, reason, k_max, centre=None):
    """The bound of the issue: |s - ref| <= (n + 4) 2^-52 sum |term| for both sums — the any-order bound of recursive
    summation plus the roundings of forming a term, so it holds for every reduction tree; min, max and counts exact."""
    mom, terms, cnt, n = ensemble_ref(x, u, n_ax, reason, k_max, centre)
    assert np.array_equal(counts, cnt), (counts, cnt)
    assert np.array_equal(moments[:, 2:], mom[:, 2:]), (moments[:, 2:], mom[:, 2:])
    err = np.abs(moments[:, :2] - mom[:, :2])
    bound = (n + 4) * 2.0 ** -52 * terms
    print(f"ensemble of {n} rows: max |s - ref| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), (err, bound)
