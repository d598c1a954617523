"""CPU: the oracle against the compiled reference on long closed loops and seeded random states — bit-exact.  The
reference's outputs are recorded in tests/golden/oracle_vs_ref/ (oracle/ref_records.py, from oracle/_ref/libref.so);
where that library has been built, the live reference must reproduce the records as well.  The same holds for the oracle
with run-time tuning constants (orc_create_tuned): the reference was compiled with those constants in place of its
own, so the checker of tests/test_gpu_tuning.py is itself checked."""
import numpy as np
import pytest

from oracle.ref_records import (CASES, FP32_MODELS, RANDOM_CASES, TUNED_CASES, TUNING_SETS, case_path, fp32_path,
                                record_case, record_fp32_reference, record_tuned, tuned_path)


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


@pytest.mark.parametrize("name,model,dv,kmax", TUNED_CASES)
def test_tuned_oracle_bit_exact(orc, name, model, dv, kmax):
    """dt / h / zeta / Tf / alpha given at run time: 400 closed-loop ticks and the seeded random states (F, prepare, Ax,
    control, Arnoldi count, advanced state) equal, bit for bit, what the reference computes with these constants
    compiled in."""
    stored = np.load(tuned_path(name, model, dv, kmax))
    assert np.array_equal(stored["tuning"], [TUNING_SETS[name][k] for k in orc.TUNING_FIELDS])
    _assert_same(record_tuned(orc, "oracle", name, model, dv, kmax), stored, "tuned oracle vs the reference's records")
    _live_ref_agrees(orc, stored, lambda which: record_tuned(orc, which, name, model, dv, kmax))


def test_tuned_records_differ_from_shipped_tuning(orc):
    """The records are not the shipped constants under another name, and a tuning equal to the shipped one reproduces
    orc_create exactly."""
    for model in (0, 1, 2):
        shipped = orc.Controller(model, 8, 3)
        same = dict(zip(orc.TUNING_FIELDS, (shipped.dt, shipped.h, shipped.zeta, shipped.Tf, shipped.alpha)))
        x0, u0, p = orc.shipped_scenario(model)
        runs = []
        for tuning in (None, same, TUNING_SETS["mid"]):
            c = orc.Controller(model, 8, 3, tuning=tuning)
            orc.start_controller(c, x0, u0, p)
            runs.append(orc.closed_loop(c, x0, 20)[0])
        assert np.array_equal(runs[0], runs[1])
        assert not np.array_equal(runs[0], runs[2])


def test_which_tunings_each_library_serves(orc):
    """The oracle takes any constants and reports them back; the reference build, where there is one, only the table
    compiled into it, matched on all five values."""
    odd = dict(TUNING_SETS["mid"], zeta=401.0)
    c = orc.Controller(0, 8, 3, tuning=odd)
    assert (c.dt, c.h, c.zeta, c.Tf, c.alpha) == tuple(odd[k] for k in orc.TUNING_FIELDS)
    with pytest.raises(TypeError):
        orc.Controller(0, 8, 3, tuning=dict(h=1e-3))
    if orc.have_ref():
        with pytest.raises(ValueError):
            orc.Controller(0, 8, 3, which="ref", tuning=odd)
        with pytest.raises(ValueError):
            orc.Controller(0, 50, 10, which="ref", tuning=TUNING_SETS["mid"])
