"""CPU: the independent reference of the horizon tests (tests/horizon_ref.cpp) is pinned to the oracle.  The oracle's C
ABI hands out F but not the trajectories xtau and ltau it builds on the way; the helper restates the same two
recurrences and hands out all three.  Its F must be bit-identical to orc.Controller.F — which pins xtau and ltau[1..dv]
(every element of F reads them) and, through the same loop body, ltau[0]."""
import numpy as np
import pytest

from horizon_helper import HorizonRef

MODELS = (0, 1, 2)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return HorizonRef(tmp_path_factory.mktemp("horizon_ref"))


def _inputs(orc, c, model, dv, seed):
    """A random U around the example's u0 and a ptau that varies along the stages."""
    rng = np.random.default_rng(seed)
    x0, u0, p = orc.shipped_scenario(model)
    U = np.tile(u0, dv) * (1 + 0.05 * rng.standard_normal(c.len)) + 0.01 * rng.standard_normal(c.len)
    x = x0 + 0.1 * rng.standard_normal(c.dim_x)
    ptau = np.tile(p, dv + 1) + 0.05 * rng.standard_normal(c.dim_p * (dv + 1)) + \
        0.02 * np.repeat(np.arange(dv + 1), c.dim_p) if c.dim_p else np.zeros(0)
    return U, x, ptau


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dv", [1, 8, 50])
@pytest.mark.parametrize("model", MODELS)
def test_helper_F_is_the_oracles_bit_for_bit(orc, ref, model, dv, dtype):
    c = orc.Controller(model, dv, 3, -1.0, dtype)
    U, x, ptau = _inputs(orc, c, model, dv, 7 + 10 * model + dv)
    if dtype == "f32":  # (values both sides can take without rounding them differently)
        U, x, ptau = (a.astype(np.float32).astype(np.float64) for a in (U, x, ptau))
    c.set_ptau(ptau)
    for t in (0.0, 0.3):
        xtau, ltau, F = ref(model, dtype, dv, c.Tf, c.alpha, t, x, U, ptau)
        assert np.array_equal(F, c.F(U, x, t)), (model, dv, dtype, t)
        assert np.array_equal(xtau[0], x) and np.all(np.isfinite(xtau)) and np.all(np.isfinite(ltau))
        if t == 0.0:  # dtau = 0: the state never moves and the costate stays the terminal one
            assert np.array_equal(xtau, np.tile(x, (dv + 1, 1))) and np.array_equal(ltau, np.tile(ltau[dv], (dv + 1, 1)))
        else:
            assert not np.array_equal(xtau[dv], x)


@pytest.mark.parametrize("model", MODELS)
def test_helper_F_is_the_compiled_references(orc, ref, model):
    if not orc.have_ref():
        pytest.skip("oracle/_ref/libref.so is not built on this machine")
    from oracle import ref_records
    _, dv, kmax, tol = next(c for c in ref_records.RANDOM_CASES if c[0] == model)
    c = orc.Controller(model, dv, kmax, tol, which="ref")
    U, x, ptau = _inputs(orc, c, model, dv, 3 + model)
    c.set_ptau(ptau)
    for t in (0.0, 0.3):
        assert np.array_equal(ref(model, "f64", dv, c.Tf, c.alpha, t, x, U, ptau)[2], c.F(U, x, t)), (model, t)


def test_helper_serves_a_user_model(tmp_path):
    """Built for tests/user_models/vdp_model.hpp: F against a plain numpy statement of that model's dHdu at the helper's
    own trajectories (the model is small enough to write down)."""
    vdp = HorizonRef(tmp_path, header="tests/user_models/vdp_model.hpp", cls="VdpModel")
    dv, rng = 6, np.random.default_rng(5)
    x, U, ptau = rng.standard_normal(2), 0.3 * rng.standard_normal(3 * dv), 0.2 * rng.standard_normal(2 * (dv + 1))
    xtau, ltau, F = vdp(0, "f64", dv, 1.0, 0.5, 0.4, x, U, ptau)
    dtau = 1.0 * (1 - np.exp(-0.5 * 0.4)) / dv
    u = U.reshape(dv, 3)
    for s in range(dv):
        f = np.array([xtau[s, 1], (1.0 - xtau[s, 0] ** 2) * xtau[s, 1] - xtau[s, 0] + u[s, 0] + ptau[2 * s + 1]])
        assert np.allclose(xtau[s + 1], xtau[s] + f * dtau, rtol=1e-14, atol=1e-15)
        want = [u[s, 0] + ltau[s + 1, 1] + 2.0 * u[s, 2] * u[s, 0], -0.1 + 2.0 * u[s, 2] * u[s, 1],
                u[s, 0] ** 2 + u[s, 1] ** 2 - 4.0]
        assert np.allclose(F[3 * s:3 * s + 3], want, rtol=1e-14, atol=1e-15)
    assert np.allclose(ltau[dv], [(xtau[dv, 0] - ptau[2 * dv]) * 2.0, xtau[dv, 1]], rtol=1e-14)
