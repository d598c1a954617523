"""GPU: what is new in the row-parallel Newton kernel ("wg+row-newton", csrc/tick_wg.hip.h NWT = 1) since its solver
vectors are held in STAGE OWNERSHIP (csrc/stage_own.hip.h: lane r of an instance's 16-lane row holds the 12 elements
12r .. 12r+11 of its own four stages) — the ragged ends of that ownership where the controller state is handed over
through HBM, the permutation of the exported Krylov basis, and the pads of the state rows.  The ownership edges of the
sweeps themselves are walked by test_gpu_row_newton.py (dv = 33 .. 53, teacher-forced).
Checker: the oracle (oracle/liboracle.so), same seeded inputs.  Bounds: test_gpu_closed_loop.py's and
test_gpu_row_newton.py::test_exported_krylov_arrays_vs_oracle's; v_0 = r0 / |r0| carries no sign freedom and is compared
element by element at the bound of u."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg

pytestmark = pytest.mark.gpu

NAME = "wg+row-newton"
KM = 3
B_MAX = 17       # one full workgroup + one row of a second
WARM, N, CUT = 2, 12, 5  # oracle ticks before the hand-over; device ticks (one launch boundary at 10); first call of the cut run
U_TOL, X_TOL, DUDT_REL = 1e-9, 1e-9, 1e-7  # test_gpu_closed_loop.py, fp64


def _batch(B, dv, tol, km=KM):
    c = cg.CgmresBatch("pendulum", batch=B, dv=dv, k_max=km, tol=tol, variant=2)
    if c.variant_name != NAME:
        name = c.variant_name
        c.close()
        pytest.skip(f"dv = {dv}, k_max = {km}: the library runs this handle on {name}")
    return c


_free_runs = {}


def _oracle_free_run(orc, dv, tol):
    """B_MAX oracle controllers, WARM ticks from the seeded start (so that U and dUdt differ per instance and per stage),
    the state there, and the free run of N further ticks.  Computed once per (dv, tol), never modified."""
    key = (dv, tol)
    if key not in _free_runs:
        x0, u0, p = orc.batch_scenario(0, B_MAX)
        start, end = [], []
        for i in range(B_MAX):
            r = orc.Controller(0, dv, KM, tol)
            orc.start_controller(r, x0[i], u0[i], p[i])
            x = x0[i].copy()
            for _ in range(WARM):
                x = x + r.plant(x, r.control(x)) * r.dt
            start.append((x.copy(),) + r.get_state())
            for _ in range(N):
                u = r.control(x)
                x = x + r.plant(x, u) * r.dt
            end.append((x, u) + r.get_state() + (r.last_solve(),))
        _free_runs[key] = (p, start, end)
    return _free_runs[key]


def _run(c, p, start, B, cuts):
    c.set_ptau_repeat(p[:B])
    c.set_state(start[0][1], np.array([s[2] for s in start[:B]]), np.array([s[3] for s in start[:B]]))
    xd = c.device_buffer((B, 4)).upload(np.array([s[0] for s in start[:B]]))
    ud = c.device_buffer((B, 3))
    for n in cuts:
        c.closed_loop_device(xd, ud, n)
        c.synchronize()
    out = (xd.download(), ud.download()) + c.get_state() + c.get_status()
    xd.free(), ud.free()
    return out


@pytest.mark.parametrize("B", [1, B_MAX])
@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("dv", [33, 49, 50, 52, 53])
def test_hand_over_through_hbm_at_the_ragged_ends_of_the_ownership(orc, dv, tol, B):
    """3 dv mod 12 = 3, 3, 6, 0, 3: the last owning lane holds one stage, one, two, four, one; at dv = 52 lane 13 is empty,
    at dv = 53 it owns 3 elements beyond the last full 16-element group of the HBM row.  B = 1: the batch's last row is the
    workgroup's only live row; B = 17: a ragged second workgroup.  set_state from the oracle, 12 fused ticks (10 + 2: U,
    dUdt and x cross HBM once) against the oracle's free run; the same 12 ticks cut 5 + 7 bit for bit."""
    p, start, end = _oracle_free_run(orc, dv, tol)
    c = _batch(B, dv, tol)
    x, u, t, U, d, n_ax, reason = _run(c, p, start, B, (N,))
    c.close()
    worst = dict(u=0.0, x=0.0, U=0.0, d=0.0)
    for i in range(B):
        x_o, u_o, t_o, U_o, d_o, (k_o, _, reason_o) = end[i]
        worst["u"] = max(worst["u"], float(np.max(np.abs(u[i] - u_o))))
        worst["x"] = max(worst["x"], float(np.max(np.abs(x[i] - x_o))))
        worst["U"] = max(worst["U"], float(np.max(np.abs(U[i] - U_o))))
        worst["d"] = max(worst["d"], float(np.max(np.abs(d[i] - d_o))) / max(1.0, float(np.max(np.abs(d_o)))))
    print(f"dv={dv} tol={tol} B={B}: worst |du| {worst['u']:.3e} |dx| {worst['x']:.3e} |dU| {worst['U']:.3e} rel|ddUdt| {worst['d']:.3e}")
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(U)) and np.all(np.isfinite(d))
    for i in range(B):
        x_o, u_o, t_o, U_o, d_o, (k_o, _, reason_o) = end[i]
        assert abs(t - t_o) <= 1e-12
        assert np.max(np.abs(u[i] - u_o)) <= U_TOL, (i, u[i], u_o)
        assert np.max(np.abs(x[i] - x_o)) <= X_TOL, (i, x[i], x_o)
        assert np.max(np.abs(U[i] - U_o)) <= U_TOL, i
        assert np.max(np.abs(d[i] - d_o)) <= DUDT_REL * max(1.0, float(np.max(np.abs(d_o)))), i
        assert n_ax[i] == k_o and reason[i] == reason_o, (i, n_ax[i], k_o, reason[i], reason_o)
    if tol == 0.0:
        assert np.all(n_ax == KM) and np.all(reason == cg.EXIT_NATURAL)
    c = _batch(B, dv, tol)
    cut = _run(c, p, start, B, (CUT, N - CUT))
    c.close()
    for a, b in zip((x, u, t, U, d, n_ax, reason), cut):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("dv", [33, 53])
def test_exported_basis_element_by_element(orc, dv):
    """get_krylov undoes the HBM row format of the handle's kernel: v_0 against the oracle element by element
    (orthonormality would not notice a wrong permutation), the rotated Hessenberg and the residual vector at the bounds of
    test_gpu_row_newton.py::test_exported_krylov_arrays_vs_oracle."""
    B, tol = B_MAX, 0.0
    p, start, _ = _oracle_free_run(orc, dv, tol)
    c = _batch(B, dv, tol)
    c.set_ptau_repeat(p)
    c.set_state(start[0][1], np.array([s[2] for s in start]), np.array([s[3] for s in start]))
    x = np.array([s[0] for s in start])
    c.control(x)
    n_ax, reason = c.get_status()
    V, H, rho, g = c.get_krylov(with_V=True)
    c.close()
    x0, u0, _ = orc.batch_scenario(0, B)
    k1 = KM + 1
    worst_v = worst_h = worst_r = 0.0
    checks = []
    for i in range(B):
        r = orc.Controller(0, dv, KM, tol)  # (a controller of its own: the shared free run is left as it is)
        orc.start_controller(r, x0[i], u0[i], p[i])
        r.set_state(start[i][1], start[i][2], start[i][3])
        r.control(x[i])
        k_o, _, _ = r.last_solve()
        Vo, Ho, rhoo, _ = r.krylov()
        Vd, Hd = np.asarray(V[i]).reshape(k1, -1), np.asarray(H[i]).reshape(k1, k1)
        dv0 = float(np.max(np.abs(Vd[0] - Vo[0])))
        hs = max(1.0, float(np.max(np.abs(Ho[:k_o, :k_o + 1]))))
        dh = float(np.max(np.abs(np.abs(Hd[:k_o, :k_o + 1]) - np.abs(Ho[:k_o, :k_o + 1])))) / hs
        rs = max(1.0, float(np.max(np.abs(rhoo[:k_o + 1]))))
        dr = float(np.max(np.abs(np.abs(np.asarray(rho[i])[:k_o + 1]) - np.abs(rhoo[:k_o + 1])))) / rs
        worst_v, worst_h, worst_r = max(worst_v, dv0), max(worst_h, dh), max(worst_r, dr)
        checks.append((i, n_ax[i], k_o, dv0, dh, dr, Vd))
    print(f"dv={dv}: worst |v_0 - v_0(oracle)| {worst_v:.3e}, H {worst_h:.3e} (rel), rho {worst_r:.3e} (rel)")
    for i, k_d, k_o, dv0, dh, dr, Vd in checks:
        assert k_d == k_o == KM
        assert dv0 <= 1e-9, (i, dv0)
        assert dh <= 1e-6 and dr <= 1e-6, (i, dh, dr)
        assert np.max(np.abs(Vd @ Vd.T - np.eye(k1))) < 1e-8, i


def test_pads_of_the_state_rows_stay_as_set_state_left_them(orc):
    """One tick at dv = 33 (3 dv = 99, rows of 112 scalars) in the headline mode (tol = 0, fixed k): the last owning lane
    holds the elements 96 .. 107 of which three exist — its stores must stop at 3 dv.  The words 99 .. 111 of every U and
    dUdt row are given distinct values through the C ABI (cgmres_hip_state_rows + memcpy), which set_state leaves alone:
    they come back bit for bit, and the tick's results are the bits of a handle whose pads hold zeros — no pad is read."""
    dv, tol, B = 33, 0.0, B_MAX
    p, start, _ = _oracle_free_run(orc, dv, tol)
    x = np.array([s[0] for s in start])
    lib = cg.load()
    L = 3 * dv

    def tick(mark):
        c = _batch(B, dv, tol)
        rows = c.state_rows()
        assert rows is not None and rows[2] >= L
        Up, dp, pitch = rows
        raw = np.zeros((B, pitch))
        tails = []
        if mark:
            for q, ptr in enumerate((Up, dp)):
                raw[:, L:] = 7.0e77 * (q + 1) + np.arange(B * (pitch - L)).reshape(B, -1)
                cg._check(lib.cgmres_hip_memcpy_h2d(c._h, ptr, raw.ctypes.data, raw.nbytes))
                tails.append(raw[:, L:].copy())
        c.set_ptau_repeat(p)
        c.set_state(start[0][1], np.array([s[2] for s in start]), np.array([s[3] for s in start]))
        for ptr, tail in zip((Up, dp), tails):  # what set_state left there
            cg._check(lib.cgmres_hip_memcpy_d2h(c._h, raw.ctypes.data, ptr, raw.nbytes))
            assert np.array_equal(raw[:, L:], tail)
        u = c.control(x)
        out = (u,) + c.get_state() + c.get_status()
        for ptr, tail in zip((Up, dp), tails):
            cg._check(lib.cgmres_hip_memcpy_d2h(c._h, raw.ctypes.data, ptr, raw.nbytes))
            assert np.array_equal(raw[:, L:].view(np.uint64), tail.view(np.uint64))
        c.close()
        return out

    marked, plain = tick(True), tick(False)
    assert np.all(np.isfinite(marked[0])) and np.all(marked[4] == KM)
    for a, b in zip(marked, plain):
        assert np.array_equal(np.asarray(a), np.asarray(b))
