"""The stand-alone Gmres (csrc/user_operator.hip.h) past its first pass: the counts and exit codes of every solve, and the
one-lane-per-system kernel gmres_op_kernel with more than one workgroup, a ragged `ldb` tail, lanes of one wavefront that
leave the Arnoldi loop at different k, early and non-finite exits beside working neighbours, and a grown workspace reused
by a smaller solve.

The golden files hold x only, so n_ax and reason are held to tests/gmres_numpy_ref.py — a plain numpy GMRES written from
the reference's statements.  The CPU tests of this file (no `gpu` mark) pin that solver to the golden files
(max |x_numpy - fixture| <= 1e-12 max|fixture|; a bound on the reference alone, no device tolerance) and assert that
every count the GPU tests require exactly is DECIDED: the residual-to-tol ratio of the reference is further than 1e-6
from 1 at the exit column and the column before it (measured: >= 1.4e-2 over the existing cases, >= 6e-4 over the 131
lane solves), while the device differs from the reference at rounding level.  No instance is left out.

The exact counts of the wave kernel (every entry of CASES x (k_max, tol), both forms) are asserted where the ranges
used to be: test_device_gmres_with_a_user_operator_vs_the_reference (tests/test_user_gmres.py) and
test_row_operator_vs_the_reference (tests/test_user_gmres_row.py).

Lane kernel: ConvDiffOp300 / ConvDiffRowOp300 at k_max = 60 (by GmresWaveLds::count both forms leave the wave mapping
at k_max = 56), tol = 1e-6, scenario("convdiff300", i) for i < 131 = two full wavefronts and three lanes of a third;
the reference leaves after 13 to 37 products across the batch.  x within the project's 1e-9 max|ref|."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from cgmres_cpp_amd import plugin
import gmres_numpy_ref as gr
from test_user_gmres import CASES, N_INST, OPS, TOLS, fixture, scenario
from test_user_gmres_row import row_op, wave_lds_count, LDS_LIMIT

FORMS = ("serial", "row")
KMAX, TOL, NB = gr.LANE_KMAX, gr.LANE_TOL, gr.LANE_BATCH


# ---- CPU: the reference of the counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_numpy_gmres_reproduces_the_golden_files(name):
    """max |x_numpy - fixture| <= 1e-12 max|fixture| per (k_max, tol) case (observed: at most 3.9e-15 max|fixture|)."""
    rows = fixture(name)
    n = N_INST[name]
    for c, (kmax, tol) in enumerate(zip(CASES[name][3], TOLS)):
        x, n_ax, why, _ = gr.case_ref(name, c)
        ref = rows[n * c:n * c + n, 3:]
        err, scale = np.max(np.abs(x - ref)), np.max(np.abs(ref))
        print(f"{name} k_max {kmax} tol {tol}: |x_numpy - fixture|inf / max|fixture| {err / scale:.3e} (bound 1e-12), "
              f"n_ax {n_ax.min()}..{n_ax.max()}")
        assert err <= 1e-12 * scale, (name, kmax, tol, err)
        assert np.all((n_ax >= 1) & (n_ax <= kmax))


@pytest.mark.parametrize("name", list(CASES))
def test_every_count_of_the_existing_cases_is_decided(name):
    for c in range(3):
        m = gr.case_ref(name, c)[3]
        print(f"{name} case {c}: smallest |ratio - 1| = {m.min():.3e}")
        assert np.all(m > gr.MARGIN), (name, c, m)


def test_the_shared_exit_case_has_both_exits_at_the_last_column():
    """convdiff300, k_max 30, tol 1e-6: instances that end at n_ax = 30 with reason 0 and with reason 1."""
    _, n_ax, why, _ = gr.case_ref("convdiff300", 1)
    assert np.all(n_ax == 30) and set(why) == {gr.EXIT_NATURAL, gr.EXIT_CONVERGED}, (n_ax, why)


def test_every_count_of_the_lane_solves_is_decided():
    """131 instances, k_max 60, tol 1e-6: all decided, all converged before k_max, 13 to 37 products, and the counts differ
    inside both full wavefronts."""
    x, n_ax, why, m = gr.lane_ref()
    print(f"lane solves: n_ax {n_ax.min()}..{n_ax.max()}, smallest |ratio - 1| = {m.min():.3e}")
    assert np.all(m > gr.MARGIN), m
    assert np.all(why == gr.EXIT_CONVERGED) and (n_ax.min(), n_ax.max()) == (13, 37)
    assert len(set(n_ax[:64])) > 1 and len(set(n_ax[64:128])) > 1


def test_exits_of_the_reference_itself():
    """A zero system leaves at the residual test with x untouched; a full Krylov space on a small exact solve breaks
    down; convergence (or breakdown) at column 0 leaves x untouched."""
    A = np.diag([2.0, 3.0, 5.0])
    r = gr.gmres_ref(A, np.zeros(3), np.zeros(3), 5, 1e-6)
    assert (r["n_ax"], r["reason"]) == (0, gr.EXIT_SMALL_RESIDUAL) and np.array_equal(r["x"], np.zeros(3))
    r = gr.gmres_ref(A, np.zeros(3), np.array([0.0, 4.0, 0.0]), 5, 0.0)  # (an eigenvector: w - h v0 is exactly 0)
    assert r["reason"] == gr.EXIT_BREAKDOWN and r["n_ax"] == 1 and np.array_equal(r["x"], np.zeros(3))
    r = gr.gmres_ref(2.0 * np.eye(3), np.zeros(3), np.array([1.0, 2.0, 2.0]), 5, 1e-6)
    assert r["reason"] in (gr.EXIT_CONVERGED, gr.EXIT_BREAKDOWN) and r["n_ax"] == 1 and np.array_equal(r["x"], np.zeros(3))


def test_reference_codes_are_the_library_codes():
    assert (gr.EXIT_NATURAL, gr.EXIT_CONVERGED, gr.EXIT_SMALL_RESIDUAL, gr.EXIT_BREAKDOWN, gr.EXIT_NONFINITE) == \
        (cg.EXIT_NATURAL, cg.EXIT_CONVERGED, cg.EXIT_SMALL_RESIDUAL, cg.EXIT_BREAKDOWN, cg.EXIT_NONFINITE)
    for row in (False, True):  # both forms leave the wave mapping at k_max = 56
        assert wave_lds_count(300, 55, row) * 8 <= LDS_LIMIT < wave_lds_count(300, 56, row) * 8


# ---- GPU: the lane kernel -----------------------------------------------------------------------------------------------
def op_id(form):
    if form == "row":
        return row_op("convdiff300")
    return plugin.register_operator(plugin.build_operator(OPS, "ConvDiffOp300", name="convdiff300"))


def lane_solve(form, n, tol=TOL, P=None, Bv=None, X0=None):
    oid = op_id(form)
    assert cg.operator_plan(oid, KMAX) == (form, "lane")
    if P is None:
        P, Bv, X0 = gr.lane_inputs(n)
    return cg.gmres_user(oid, X0, Bv, KMAX, tol, P)


_clean = {}


def clean(form):
    """The batch-131 lane solve of `form` at tol = 1e-6 (computed once per form, left unchanged)."""
    if form not in _clean:
        out = lane_solve(form, NB)
        for a in out:
            a.setflags(write=False)
        _clean[form] = out
    return _clean[form]


def check_against_ref(x, n_ax, why, n, what):
    xr, kr, wr, _ = gr.lane_ref()
    scale = np.max(np.abs(xr[:n]))
    err = np.max(np.abs(x - xr[:n]))
    print(f"{what}: |dx|inf / (1e-9 max|ref|) = {err / (1e-9 * scale):.3e}, n_ax {n_ax.min()}..{n_ax.max()}")
    assert err <= 1e-9 * scale, (what, err)
    assert np.array_equal(n_ax, kr[:n]), (what, n_ax, kr[:n])
    assert np.array_equal(why, wr[:n]), (what, why, wr[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 63, 64, 65, NB])
@pytest.mark.parametrize("form", FORMS)
def test_lane_kernel_counts_and_exits_vs_numpy(form, batch):
    """One lane alone, a ragged workgroup, exactly one, one and a lane, three workgroups with a ragged tail: x within
    1e-9 max|ref|, n_ax and reason exactly the reference's (lanes of one wavefront leave the loop between k = 13 and 37)."""
    x, n_ax, why = clean(form) if batch == NB else lane_solve(form, batch)
    assert x.shape == (batch, 300)
    check_against_ref(x, n_ax, why, batch, f"lane {form} batch {batch}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_lane_kernel_runs_to_k_max_at_tol_zero(form):
    """tol = 0 at batch 131: every lane makes all 60 products and leaves with reason 0; x against the numpy reference."""
    x, n_ax, why = lane_solve(form, NB, tol=0.0)
    assert np.all(n_ax == KMAX) and np.all(why == cg.EXIT_NATURAL)
    xr = gr.solve_batch(gr.LANE_NAME, NB, KMAX, 0.0)
    assert np.all(xr[1] == KMAX) and np.all(xr[2] == gr.EXIT_NATURAL)
    scale, err = np.max(np.abs(xr[0])), np.max(np.abs(x - xr[0]))
    print(f"lane {form} tol 0: |dx|inf / (1e-9 max|ref|) = {err / (1e-9 * scale):.3e}")
    assert err <= 1e-9 * scale, err


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_lane_kernel_exits_beside_working_neighbours(form):
    """Instance 5: b = 0 from x0 = 0 leaves at the residual test (reason 2, no product, x untouched).  Instance 70: a NaN
    in b ends that instance alone (reason 4, every element of x NaN).  Every other instance is bit-identical to the clean
    run.  Reason 3 cannot be reached on this path: a breakdown needs k_max >= len, and the 16-bit index limit
    len (k_max + 1) < 65536 forbids that at every length whose solve leaves the wave mapping for the lane kernel."""
    P, Bv, X0 = gr.lane_inputs(NB)
    Bv[5], X0[5] = 0.0, 0.0
    Bv[70, 123] = np.nan
    x, n_ax, why = lane_solve(form, NB, P=P, Bv=Bv, X0=X0)
    xc, kc, wc = clean(form)
    assert why[5] == cg.EXIT_SMALL_RESIDUAL and n_ax[5] == 0 and np.array_equal(x[5], np.zeros(300))
    assert why[70] == cg.EXIT_NONFINITE and np.all(np.isnan(x[70]))
    rest = np.setdiff1d(np.arange(NB), [5, 70])
    assert x[rest].tobytes() == xc[rest].tobytes()
    assert np.array_equal(n_ax[rest], kc[rest]) and np.array_equal(why[rest], wc[rest])


@pytest.mark.gpu
def test_lane_workspace_is_reused_by_smaller_solves():
    """One operator, one process: batch 131, 1, 65, a wave-path solve at k_max = 20, batch 131 again.  The instances are
    independent and the lane kernel's order does not depend on the batch: the two large results are bit-identical, every
    smaller one is the leading rows of the large one, and the wave solve in between is the golden file's."""
    form = "row"
    first = lane_solve(form, NB)
    for n in (1, 65):
        x, n_ax, why = lane_solve(form, n)
        assert x.tobytes() == first[0][:n].tobytes(), n
        assert np.array_equal(n_ax, first[1][:n]) and np.array_equal(why, first[2][:n]), n
    oid, n = op_id(form), N_INST["convdiff300"]
    assert cg.operator_plan(oid, 20) == (form, "wave")
    P, Bv, X0 = (np.array(a) for a in zip(*[scenario("convdiff300", i) for i in range(n)]))
    x, n_ax, why = cg.gmres_user(oid, X0, Bv, 20, TOLS[0], P)
    ref = fixture("convdiff300")[:n]
    assert np.all(ref[:, 1] == 20)
    assert np.max(np.abs(x - ref[:, 3:])) <= 1e-9 * np.max(np.abs(ref[:, 3:]))
    assert np.array_equal(n_ax, gr.case_ref("convdiff300", 0)[1]) and np.array_equal(why, gr.case_ref("convdiff300", 0)[2])
    again = lane_solve(form, NB)
    assert again[0].tobytes() == first[0].tobytes()
    assert np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    check_against_ref(*again, NB, "lane row batch 131 after the smaller solves")
