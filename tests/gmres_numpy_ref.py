"""A plain fp64 numpy GMRES(k_max), written from the statements of `Gmres::gmres` (include/gmres.hpp of the reference:
r0 and its test :33-41, Arnoldi with modified Gram-Schmidt :46-60, the breakdown test :63-65, the convergence test :93-95,
the solve on the leading columns :100-111) and not from the device kernels: the Hessenberg least-squares problems go to
numpy.linalg.lstsq, no reflector is stored, no sum follows a kernel's order.  What the golden files
tests/golden/user_gmres_*.txt do not hold — the number of products and the exit code of every solve — comes from here;
tests/test_user_gmres_numpy_ref.py pins this solver to those files first.

A count is DECIDED when the residual-to-tol ratio of the reference lies outside [1 - MARGIN, 1 + MARGIN] at the exit
column and at the column before it: the device differs from this solver at rounding level (its x bound is 1e-9, observed
~1e-14), so a ratio that far from 1 cannot fall on the other side of tol there."""
import functools

import numpy as np

from test_user_gmres import CASES, N_INST, TOLS, dense, scenario

EXIT_NATURAL, EXIT_CONVERGED, EXIT_SMALL_RESIDUAL, EXIT_BREAKDOWN, EXIT_NONFINITE = 0, 1, 2, 3, 4
DBL_EPSILON = float(np.finfo(np.float64).eps)
MARGIN = 1e-6

LANE_NAME, LANE_KMAX, LANE_TOL, LANE_BATCH = "convdiff300", 60, 1e-6, 131  # the lane-kernel solves of the exit tests


def gmres_ref(A, x0, b, k_max, tol):
    """-> dict(x, n_ax, reason, ratios): ratios[0] = |r0| / tol, ratios[k + 1] = (residual after column k) / tol."""
    A, x, b = np.asarray(A, dtype=np.float64), np.array(x0, dtype=np.float64), np.asarray(b, dtype=np.float64)
    L = len(b)
    ratio = (lambda r: r / tol) if tol > 0 else (lambda r: np.inf)
    r0 = b - A @ x
    beta = np.sqrt(r0 @ r0)
    ratios = [ratio(beta)]
    if beta < tol:
        return dict(x=x, n_ax=0, reason=EXIT_SMALL_RESIDUAL, ratios=ratios)
    V = np.zeros((k_max + 1, L))
    H = np.zeros((k_max + 1, k_max))
    V[0] = r0 / beta

    def solve(cols):  # the least-squares problem of the first `cols` columns
        if cols == 0:
            return np.zeros(0), beta
        rhs = np.zeros(cols + 1)
        rhs[0] = beta
        y = np.linalg.lstsq(H[:cols + 1, :cols], rhs, rcond=None)[0]
        return y, np.linalg.norm(rhs - H[:cols + 1, :cols] @ y)

    reason, used, n_ax = EXIT_NATURAL, k_max, k_max
    for k in range(k_max):
        w = A @ V[k]
        for i in range(k + 1):
            H[i, k] = V[i] @ w
            w = w - H[i, k] * V[i]
        H[k + 1, k] = np.sqrt(w @ w)
        if H[k + 1, k] < DBL_EPSILON:
            return dict(x=x, n_ax=k + 1, reason=EXIT_BREAKDOWN, ratios=ratios)  # x untouched, as the reference returns
        V[k + 1] = w / H[k + 1, k]
        res = solve(k + 1)[1]
        ratios.append(ratio(res))
        if res < tol:
            reason, used, n_ax = EXIT_CONVERGED, k, k + 1  # column k is not used by the solve
            break
    y = solve(used)[0]
    return dict(x=x + y @ V[:used], n_ax=n_ax, reason=reason, ratios=ratios)


def margin(rec):
    """Distance from 1 of the residual-to-tol ratio at the exit column and at the column before it (the smaller one)."""
    return min(abs(r - 1.0) for r in rec["ratios"][-2:])


def decided(rec):
    return margin(rec) > MARGIN


def solve_batch(name, n, k_max, tol):
    """The reference on instances 0..n-1 of scenario(name, .): (x [n, L], n_ax [n], reason [n], margins [n])."""
    recs = []
    for i in range(n):
        p, b, x0 = scenario(name, i)
        recs.append(gmres_ref(dense(name, p), x0, b, k_max, tol))
    return (np.array([r["x"] for r in recs]), np.array([r["n_ax"] for r in recs], dtype=np.int32),
            np.array([r["reason"] for r in recs], dtype=np.int32), np.array([margin(r) for r in recs]))


@functools.lru_cache(maxsize=None)
def case_ref(name, c):
    """Case c of CASES[name] x TOLS on the N_INST[name] instances of the golden file (computed once, left unchanged)."""
    out = solve_batch(name, N_INST[name], CASES[name][3][c], TOLS[c])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lane_ref():
    """The lane-kernel solves: scenario("convdiff300", i), i < 131, k_max = 60, tol = 1e-6 (computed once)."""
    out = solve_batch(LANE_NAME, LANE_BATCH, LANE_KMAX, LANE_TOL)
    for a in out:
        a.setflags(write=False)
    return out


def lane_inputs(n=LANE_BATCH):
    """(params [n, 2], b [n, 300], x0 [n, 300]) of the lane-kernel solves."""
    P, Bv, X0 = (np.array(a) for a in zip(*[scenario(LANE_NAME, i) for i in range(n)]))
    return P, Bv, X0
