"""CPU: the oracle against the compiled reference on long closed loops and seeded random states — bit-exact.  The
reference's outputs are recorded in tests/golden/oracle_vs_ref/ (oracle/ref_records.py, from oracle/_ref/libref.so);
where that library has been built, the live reference must reproduce the records as well."""
import numpy as np
import pytest

from oracle.ref_records import (CASES, FP32_MODELS, RANDOM_CASES, case_path, fp32_path, record_case,
                                record_fp32_reference)


def _assert_same(rec, stored, what):
    assert sorted(rec) == sorted(stored.files), what
    for k in rec:
        assert np.array_equal(rec[k], stored[k]), (what, k)


def _live_ref_agrees(orc, stored, make):
    if orc.have_ref():
        _assert_same(make("ref"), stored, "live reference vs its records")


@pytest.mark.parametrize("model,dv,kmax,tol", CASES)
def test_closed_loop_bit_exact(orc, model, dv, kmax, tol):
    stored = np.load(case_path(model, dv, kmax, tol))
    case = (model, dv, kmax, tol)
    rec = record_case(orc, "oracle", case)
    for k in ("u_newton", "loop_u", "loop_x", "loop_k"):
        assert np.array_equal(rec[k], stored[k]), k
    if case not in RANDOM_CASES:
        _live_ref_agrees(orc, stored, lambda which: record_case(orc, which, case))


@pytest.mark.parametrize("model,dv,kmax,tol", RANDOM_CASES)
def test_random_state_records(orc, model, dv, kmax, tol):
    stored = np.load(case_path(model, dv, kmax, tol))
    case = (model, dv, kmax, tol)
    rec = record_case(orc, "oracle", case)
    for k in ("rs_F", "rs_prepare", "rs_Ax", "rs_u", "rs_k", "rs_t", "rs_U", "rs_dUdt"):
        assert np.array_equal(rec[k], stored[k]), k
    _live_ref_agrees(orc, stored, lambda which: record_case(orc, which, case))


def test_fp32_restatement_close_to_fp32_reference(orc):
    """fp32: not bit-exact by construction (double literals survive in the macro-converted reference)."""
    for model in FP32_MODELS:
        stored = np.load(fp32_path(model))
        b = orc.Controller(model, 50, 10, -1.0, "f32", which="oracle")
        x0, u0, p = orc.shipped_scenario(model)
        orc.start_controller(b, x0, u0, p)
        for tick in range(5):
            b.set_state(stored["t"][tick], stored["U"][tick], stored["dUdt"][tick])
            np.testing.assert_allclose(b.control(x0), stored["u"][tick], rtol=0, atol=1e-4)
        if orc.have_ref():
            _assert_same(record_fp32_reference(orc, model), stored, "live fp32 reference vs its records")
