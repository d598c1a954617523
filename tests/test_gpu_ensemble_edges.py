"""GPU: the four things csrc/record.hip.h promises of the ensemble kernel that no other test asserts —
  * a row with more than kRecordGroup = 8 components is walked in groups (MSD: nc = 10 = one full group and one with two
    live and six clamped components; Shape262: nc = 8 = exactly one full group; pendulum: nc = 7, the control);
  * a batch beyond kRecordMaxGrid * kRecordBlock = 16384 instances is strided by the grid (16645 = a second step with one
    full workgroup, one of five live lanes and 62 wholly past the batch);
  * the histogram is filled and stored in passes of 256 bins (k_max = 300: the exit codes and the finite count sit in the
    second pass);
  * finiteness of the whole row is decided before anything is added (NaN, +Inf, -Inf; in x, in u, in the second group,
    in the last row, in the row that would hold a min and a max, in every row).
The reference is record_harness.check_ensemble: math.fsum for the sums within (n + 4) 2^-52 sum|term| — a bound that
holds for every reduction tree — and exact min, max and counts.  Rows are hand-made: a scale and an offset of its own per
component, so that a swapped component shows.  The status comes from one real control()."""
import os

import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin
from record_harness import Dev, check_ensemble, ensemble_ref, new_batch, run_recorded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = cg.RECORD_BLOCK
PENDULUM, MSD, SHAPE262 = 0, 1, "Shape262"
NC = {PENDULUM: 7, MSD: 10, SHAPE262: 8}
STEPPED = 64 * W + W + 5  # 16645: two grid steps


def handle(orc, model, batch, dtype="f64", dv=5, km=3, variant=0, tol=1e-6):
    """A handle after one real control(): (c, n_ax, reason)."""
    if model == SHAPE262:
        if not os.path.exists(plugin._build.HIPCC) and not os.path.exists(plugin.plugin_path("shape262")):
            pytest.skip("neither the plugin nor hipcc is available")
        mid = plugin.register(plugin.build(os.path.join(ROOT, "tests", "user_models", "shape_models.hpp"), cls="Shape262",
                                           name="shape262"))
        c = cg.CgmresBatch(mid, batch=batch, dv=dv, k_max=km, tol=tol, variant=variant)
        b = (np.arange(batch) % 20)[:, None]
        x0 = 0.3 + 0.05 * b - 0.11 * np.arange(c.dim_x)[None, :]
        u0, p = np.full((batch, c.dim_u), 0.1), 0.2 + 0.03 * b + 0.01 * np.arange(c.dim_p)[None, :]
        c.set_ptau_repeat(p)
        c.init_u0(u0)
        c.init_u0_newton(u0, x0, p, 10)
    else:
        c, x0, u0, p = new_batch(orc, model, batch=batch, dv=dv, km=km, tol=tol, variant=variant, dtype=dtype)
    assert c.dim_x + c.dim_u == NC[model]
    c.control(x0)
    n_ax, reason = c.get_status()
    return c, n_ax, reason


def rows_of(c, seed=11):
    """Hand-made rows [batch, nc] in the handle's type: component k is offset_k + scale_k * N(0, 1), scales over six decades."""
    nc = c.dim_x + c.dim_u
    rng = np.random.default_rng(seed)
    scale = 10.0 ** np.linspace(-3, 3, nc)
    offset = np.array([(-1) ** k * 3.7 * scale[(k + 2) % nc] for k in range(nc)])
    return (offset + scale * rng.normal(size=(c.batch, nc))).astype(c.np_dtype)


def ensemble(c, rows, centre=None, moments=True, counts=True):
    """One cgmres_hip_ensemble_device call on `rows` -> (moments or None, counts or None)."""
    dev = Dev(c)
    nx = c.dim_x
    xd, ud = dev(rows[:, :nx]), dev(rows[:, nx:])
    # (filled with a pattern no result equals: an entry the kernels leave alone shows)
    md = dev(np.full((rows.shape[1], 4), -7.25)) if moments else None
    cd = dev(np.full(c.k_max + 7, -3, dtype=np.int32)) if counts else None
    c.ensemble_device(xd, ud, moments=md, counts=cd, centre=dev(centre))
    c.synchronize()
    out = (md.download() if moments else None, cd.download() if counts else None)
    dev.free()
    return out


def check(c, rows, n_ax, reason, centres=("zero", "median"), what=""):
    """Both centres against the reference; -> the (moments, counts) of the last centre."""
    nx = c.dim_x
    r64 = rows.astype(np.float64)
    finite = r64[np.all(np.isfinite(r64), axis=1)]
    out = None
    for how in centres:
        centre = None if how == "zero" or not len(finite) else np.median(finite, axis=0)
        out = ensemble(c, rows, centre)
        mom, terms, _, n = ensemble_ref(rows[:, :nx], rows[:, nx:], n_ax, reason, c.k_max, centre)
        ratio = np.max(np.abs(out[0][:, :2] - mom[:, :2]) / np.maximum((n + 4) * 2.0 ** -52 * terms, 1e-300))
        print(f"{what} centre {how}: worst |s - ref| / bound = {ratio:.3e}; ", end="")
        check_ensemble(out[0], out[1], rows[:, :nx], rows[:, nx:], n_ax, reason, c.k_max, centre)
    return out


# ---- A1. component groups -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 65, 83, W + 5])
@pytest.mark.parametrize("model,dtype", [(MSD, "f64"), (MSD, "f32"), (SHAPE262, "f64"), (PENDULUM, "f64"), (PENDULUM, "f32")])
def test_rows_of_more_than_one_component_group(orc, model, dtype, batch):
    c, n_ax, reason = handle(orc, model, batch, dtype)
    rows = rows_of(c)
    nx = c.dim_x
    m_both, c_both = check(c, rows, n_ax, reason, what=f"{model} {dtype} batch {batch}")
    # moments alone (no histogram) and counts alone (ngroups = 1 without part_m): the same numbers
    centre = np.median(rows.astype(np.float64), axis=0)
    m_alone = ensemble(c, rows, centre, counts=False)[0]
    c_alone = ensemble(c, rows, centre, moments=False)[1]
    assert m_alone.tobytes() == m_both.tobytes() and np.array_equal(c_alone, c_both)
    check_ensemble(m_alone, c_alone, rows[:, :nx], rows[:, nx:], n_ax, reason, c.k_max, centre)
    c.close()


# ---- A2. grid steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dtype", [(MSD, "f64"), (PENDULUM, "f32")])
def test_a_batch_beyond_the_grid_is_strided(orc, model, dtype):
    B = STEPPED
    assert B > 64 * W and (B - 64 * W) // W == 1 and B % W == 5
    c, x0, u0, p = new_batch(orc, model, batch=B, dv=5, km=3, dtype=dtype)
    # the logs of one recorded tick at this batch: every row is the downloaded state
    log, end = run_recorded(c, x0, 1, 1)
    assert log["x"].shape == (1, B, c.dim_x) and log["u"].shape == (1, B, c.dim_u)
    assert np.array_equal(log["x"][0], end["x"], equal_nan=True) and np.array_equal(log["u"][0], end["u"], equal_nan=True)
    assert np.array_equal(log["n_ax"][0], end["n_ax"]) and np.array_equal(log["reason"][0], end["reason"])
    print(f"{model} {dtype} recorded tick: ", end="")
    check_ensemble(log["moments"][0], log["counts"][0], log["x"][0], log["u"][0], log["n_ax"][0], log["reason"][0], c.k_max)
    c.control(x0)
    n_ax, reason = c.get_status()
    rows = rows_of(c)
    check(c, rows, n_ax, reason, what=f"{model} {dtype} batch {B} clean")
    # the row every masked lane loads: instance B - 1, non-finite
    rows[B - 1, c.dim_x + c.dim_u - 1] = np.nan
    m, cnt = check(c, rows, n_ax, reason, what=f"{model} {dtype} batch {B} NaN in row B-1")
    assert cnt[c.k_max + 6] == B - 1 and np.all(np.isfinite(m))
    c.close()


# ---- A3. histogram passes -----------------------------------------------------------------------------------------------
def test_a_histogram_of_more_than_one_pass(orc):
    """k_max + 7 = 307 bins > 256: the lane mapping takes pendulum dv = 10, k_max = 300 (30 * 301 < 65536)."""
    batch, km = 20, 300
    c, n_ax, reason = handle(orc, PENDULUM, batch, "f64", dv=10, km=km, variant=1)
    assert c.variant == 1 and c.k_max == km and c.k_max + 7 > W
    rows = rows_of(c)
    rows[7, 2] = np.inf
    m, cnt = check(c, rows, n_ax, reason, what=f"k_max {km}")
    assert cnt.shape == (km + 7,) and cnt[km + 6] == batch - 1 and cnt[km + 1:km + 6].sum() == batch
    assert cnt[:km + 1].sum() == batch and np.all(cnt >= 0)
    c_alone = ensemble(c, rows, moments=False)[1]
    assert np.array_equal(c_alone, cnt)
    c.close()


# ---- A4. non-finite placements ------------------------------------------------------------------------------------------
def scene(name, rows, nx):
    """rows with the non-finite values of scene `name` placed; -> instances that must leave the ensemble."""
    B, nc = rows.shape
    if name == "nan_last_u_of_last_row":
        rows[B - 1, nc - 1] = np.nan
        return [B - 1]
    if name == "inf_first_x_of_first_row":
        rows[0, 0] = np.inf
        return [0]
    if name == "minus_inf_in_second_group":
        assert nc == 10
        rows[40, 9] = -np.inf
        return [40]
    if name == "rejected_row_holds_min_and_max":
        rows[17, 0] = rows[:, 0].min() - 5.0
        rows[17, 1] = rows[:, 1].max() + 5.0
        rows[17, nx] = np.nan
        return [17]
    assert name == "every_row"
    bad = (np.nan, np.inf, -np.inf)
    for i in range(B):
        rows[i, i % nc] = bad[i % 3]
    return list(range(B))


SCENES = [(MSD, "f64", s) for s in ("nan_last_u_of_last_row", "inf_first_x_of_first_row", "minus_inf_in_second_group",
                                   "rejected_row_holds_min_and_max", "every_row")] + \
         [(PENDULUM, "f32", s) for s in ("nan_last_u_of_last_row", "inf_first_x_of_first_row", "rejected_row_holds_min_and_max",
                                         "every_row")]


@pytest.mark.parametrize("model,dtype,name", SCENES)
def test_non_finite_placements(orc, model, dtype, name):
    B = 83
    c, n_ax, reason = handle(orc, model, B, dtype)
    km, nx = c.k_max, c.dim_x
    rows = rows_of(c)
    _, c_clean = ensemble(c, rows)
    assert c_clean[km + 6] == B
    out = scene(name, rows, nx)
    m, cnt = check(c, rows, n_ax, reason, what=f"{model} {dtype} {name}")
    assert cnt[km + 6] == B - len(out)
    assert np.array_equal(cnt[:km + 6], c_clean[:km + 6])  # the n_ax and exit histograms count every instance
    if name == "rejected_row_holds_min_and_max":
        assert m[0, 2] > float(rows[17, 0]) and m[1, 3] < float(rows[17, 1])
    if name == "every_row":
        assert np.all(m[:, :2] == 0.0) and np.all(m[:, 2] == np.inf) and np.all(m[:, 3] == -np.inf)
    else:
        assert np.all(np.isfinite(m))
    if name == "nan_last_u_of_last_row":  # the first scene, twice: identical bits
        m2, cnt2 = ensemble(c, rows, np.median(rows[:B - 1].astype(np.float64), axis=0))
        assert m2.tobytes() == m.tobytes() and np.array_equal(cnt2, cnt)
    c.close()
