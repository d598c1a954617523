"""CPU ledger of tests/kernel_classes.py: every kernel the wg planner can choose for a configuration of kernel_classes.grid()
has a case in CASES (which tests/test_gpu_kernel_classes.py runs against the oracle), and every case still is what the
table says.  A kernel that becomes reachable in plan_wg without a case, and a case that is deleted, both fail here."""
import pytest

import kernel_classes as kc
import plan_probe
from plan_probe import check_layout, config


@pytest.fixture(scope="module")
def probe():
    return plan_probe.probe()


@pytest.fixture(scope="module")
def members(probe):
    return kc.members(probe)


def test_every_class_of_the_grid_has_a_case_and_no_case_is_outside_it(members):
    have = {case[6] for case in kc.CASES}
    print(f"{len(members)} classes over {len(kc.grid())} configurations, {len(kc.CASES)} cases")
    missing = sorted(set(members) - have)
    stray = sorted(have - set(members))
    assert not missing, "classes without a case: " + ", ".join(
        "%s (%d members, e.g. %s)" % (kc.class_name(c), len(members[c]), kc.case_id(kc.order_a(members[c])[0])) for c in missing)
    assert not stray, "cases of a class the grid does not yield: " + ", ".join(kc.class_name(c) for c in stray)
    assert len({case[:6] for case in kc.CASES}) == len(kc.CASES)


def test_the_table_is_the_one_the_admission_tool_wrote():
    """A guard against an accidental edit (a deleted or changed line), no more: the digest sits in the same file."""
    assert kc.digest(kc.CASES) == kc.CASES_DIGEST, \
        "CASES was edited (a case deleted, added or changed) without tools/kernel_case_admission.py --select --write"


def test_every_case_resolves_to_its_recorded_class_and_name(probe):
    """... at the grid's batch and at the batches and tolerances the GPU test creates its handles with, on a small and a
    large device: the class recorded is the kernel launched there (the GPU test itself can only ask for variant_name)."""
    bad = []
    for case in kc.CASES:
        m, d, dv, k, v, f = case[:6]
        for batch in (kc.BATCH, 20, 11):
            for tol in (kc.TOL, 0.0):
                for cus in (kc.CUS, 8):
                    r, _ = plan_probe.plan(probe, config(m, d, dv, k, batch, v, f, tol), cus)
                    got = None if r is None else (kc.class_of(dict(r, model=m, dtype=d)), r["variant_name"])
                    if got != (case[6], case[7]):
                        bad.append((kc.case_id(case), batch, tol, cus, got, case[6:8]))
    assert not bad, bad[:5]


def test_the_allocation_of_every_case_covers_its_layout(probe):
    """check_layout (tests/plan_probe.py) at the batch sizes the GPU test runs: before any of these shapes reaches a GPU."""
    bad = []
    for case in kc.CASES:
        m, d, dv, k, v, f = case[:6]
        for batch in (kc.BATCH, 20, 11):
            cfg = config(m, d, dv, k, batch, v, f, kc.TOL)
            r, why = plan_probe.plan(probe, cfg, kc.CUS)
            assert r is not None, (kc.case_id(case), why)
            problems = check_layout(probe, cfg, r)
            if problems:
                bad.append((kc.case_id(case), batch, problems))
    assert not bad, bad[:5]


def test_every_class_has_a_case_usable_with_the_reference_tolerance():
    """Shape of the table only: types, ranges, at most two entries per class, no case at a shape DEVICE_MISSES lists for
    its class.  That a case is usable with tol = 1e-6 is what tools/kernel_case_admission.py measures when it writes the
    table and re-measures in its check mode; nothing here repeats that."""
    per_class = {}
    for case in kc.CASES:
        m, d, dv, k, v, f, cls, name, fixed_k_ok, spread = case
        assert cls[:2] == (m, d) and isinstance(fixed_k_ok, bool) and isinstance(name, str)
        assert v in kc.VARIANTS and f in kc.FLAGS and dv in kc.DV and k in kc.KMAX
        assert (dv, k) not in kc.DEVICE_MISSES.get(cls, {})
        if d == 0:
            assert spread is None
        elif spread is not None:
            assert len(spread) == 2 and any(spread)
            for mode in spread:
                assert mode is None or (len(mode) == 3 and any(mode) and all(s is None or s > 0 for s in mode))
            assert fixed_k_ok or spread[1] is None
        per_class.setdefault(cls, []).append(case)
    assert all(1 <= len(v) <= 2 for v in per_class.values())
