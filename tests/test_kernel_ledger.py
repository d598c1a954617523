"""CPU ledger of tests/kernel_classes.py: every kernel the wg planner can choose for a configuration of kernel_classes.grid()
has a case in CASES (which tests/test_gpu_kernel_classes.py runs against the oracle), and every case still is what the
table says.  A kernel that becomes reachable in plan_wg without a case, and a case that is deleted, both fail here."""
import pytest

import class_ledger as ledger
import kernel_classes as kc
import plan_probe


@pytest.fixture(scope="module")
def probe():
    return plan_probe.probe()


@pytest.fixture(scope="module")
def members(probe):
    return kc.members(probe)


def test_every_class_of_the_grid_has_a_case_and_no_case_is_outside_it(members):
    ledger.assert_every_class_has_a_case(kc, members)


(test_the_table_is_the_one_the_admission_tool_wrote, test_every_case_resolves_to_its_recorded_class_and_name,
 test_the_allocation_of_every_case_covers_its_layout) = ledger.table_tests(kc, "tools/kernel_case_admission.py")


def test_every_class_has_a_case_usable_with_the_reference_tolerance():
    """Shape of the table only: types, ranges, at most two entries per class, no case at a shape DEVICE_MISSES lists for
    its class.  That a case is usable with tol = 1e-6 is what tools/kernel_case_admission.py measures when it writes the
    table and re-measures in its check mode; nothing here repeats that."""
    per_class = {}
    for case in kc.RECORDS:
        cls, spread = case.cls, case.fp32_spread
        assert (kc.model_of(cls), kc.dtype_of(cls)) == (case.model, case.dtype)
        assert isinstance(case.fixed_k_ok, bool) and isinstance(case.variant_name, str)
        assert case.variant in kc.VARIANTS and case.flags in kc.FLAGS and case.dv in kc.DV and case.k_max in kc.KMAX
        assert (case.dv, case.k_max) not in kc.DEVICE_MISSES.get(cls, {})
        if case.dtype == 0:
            assert spread is None
        elif spread is not None:
            assert len(spread) == 2 and any(spread)
            for mode in spread:
                assert mode is None or (len(mode) == 3 and any(mode) and all(s is None or s > 0 for s in mode))
            assert case.fixed_k_ok or spread[1] is None
        per_class.setdefault(cls, []).append(case)
    assert all(1 <= len(v) <= 2 for v in per_class.values())
