"""CPU ledger of tests/user_kernel_classes.py: every kernel the wg planner can choose for a PLUGIN model (one of the five
aliases of tests/user_models/shape_models.hpp) at a configuration of user_kernel_classes.grid(), the wave kernel and the
lane kernel have a case in CASES (which tests/test_gpu_user_kernel_classes.py runs against the oracle), and every case
still is what the table says.  A kernel that becomes reachable for UserDev in plan_wg without a case, and a case that is
deleted, both fail here.  Also: what the planner refuses for user models, and check_layout over the whole grid.  And the
hand-written derivatives of the models against central differences of their own cost and state equation."""
import os
import shutil
import subprocess

import pytest

import class_ledger as ledger
import plan_probe
import user_kernel_classes as uk
from plan_probe import check_layout, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(plan_probe.B.HIPCC):
        pytest.skip("hipcc not available")
    return plan_probe.probe_user()


@pytest.fixture(scope="module")
def members(probe):
    return uk.members(probe)


def test_model_derivatives_match_central_differences_of_cost_and_state_equation(tmp_path):
    """tests/user_models/shape_deriv_check.cpp: dHdx, dHdu, ddHduu, dPhidx of every alias against central differences of
    H = L + lambda^T f and of Phi at three fixed points, bound 1e-7 * max(1, |.|) (step 1e-5: expected error ~1e-10)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "shape_deriv_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "user_models", "shape_deriv_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.count("\n") == len(uk.ALIASES), r.stdout


def test_the_aliases_have_the_shapes_they_are_there_for(probe):
    want = {"Shape110": (1, 1, 0, 1), "Shape321": (3, 2, 1, 1), "Shape262": (2, 6, 2, 1), "Shape431": (4, 3, 1, 1), "Shape521": (5, 2, 1, 0)}
    for a, name in enumerate(uk.ALIASES):
        d = uk.dims(probe, a)
        assert (d["dim_x"], d["dim_u"], d["dim_p"], d["wave_fits"]) == want[name], (name, d)
        nlin = d["dim_x"] ** 2 + d["dim_u"] * d["dim_x"]
        nbw_lin = nlin + (nlin & 1)
        assert d["NSTG"] == (nbw_lin + d["dim_x"] + 1) // 2 * 2, (name, d)  # UserDev::NBW
        # the pads of UserDev::stage_coeffs: Shape321 has both (odd NLIN_RAW, odd NBW_RAW), Shape110 the second alone
        if name in ("Shape321", "Shape110"):
            assert (nbw_lin + d["dim_x"]) % 2 == 1 and (nlin % 2 == 1) == (name == "Shape321")


def test_every_class_of_the_grid_has_a_case_and_no_case_is_outside_it(members):
    ledger.assert_every_class_has_a_case(uk, members, " (+ the lane members)")
    # one wave and one lane class per alias where the wave mapping fits, wg classes for all five
    for a in range(len(uk.ALIASES)):
        kinds = {uk.kind(c) for c in members if uk.alias_of(c) == a}
        assert kinds == ({"wg", "wave", "lane"} if uk.ALIASES[a] != "Shape521" else {"wg", "lane"}), (a, kinds)


(test_the_table_is_the_one_the_admission_tool_wrote, test_every_case_resolves_to_its_recorded_class_and_name,
 test_the_allocation_of_every_case_covers_its_layout) = ledger.table_tests(uk, "tools/user_case_admission.py")


def test_shape_of_the_table():
    per_class = {}
    for case in uk.RECORDS:
        cls = case.cls
        assert uk.alias_of(cls) == case.alias and isinstance(case.fixed_k_ok, bool) and isinstance(case.variant_name, str)
        assert case.member and set(case.member) <= set("ABN")
        assert case.variant in uk.VARIANTS + (1,) and case.flags in uk.FLAGS and case.dv in uk.DV and case.k_max in uk.KMAX
        assert (case.dv, case.k_max) not in uk.DEVICE_MISSES.get(cls, {})
        per_class.setdefault(cls, []).append(case)
    for cls, cases in per_class.items():
        assert 1 <= len(cases) <= len(uk.orders(cls)), uk.class_name(cls)
        assert sorted("".join(c.member for c in cases)) == sorted(w for w, _ in uk.orders(cls)), uk.class_name(cls)
    for cls, misses in uk.DEVICE_MISSES.items():
        assert len(misses) <= 1 and cls in per_class, uk.class_name(cls)


def test_what_the_planner_refuses_for_user_models_and_the_layout_of_everything_it_accepts(probe):
    """Over the WHOLE grid (not only the cases): variant 3 is refused everywhere (DXDT_USES_P); variant 4 is accepted
    exactly where WaveOps::FITS holds, dv <= 63, k_max <= 10 and the wg plan of the sizes exists; the library's own choice
    (variant 0, small and large batch, small and large device) never takes the wave kernel; check_layout is clean for
    every configuration the planner accepts."""
    import time
    t0 = time.perf_counter()
    accepted = checked = 0
    bad = []
    for a in range(len(uk.ALIASES)):
        fits = uk.dims(probe, a)["wave_fits"]
        for dv in uk.DV:
            for k in uk.KMAX:
                for f in uk.FLAGS:
                    cfg2 = config(a, 0, dv, k, uk.BATCH, 2, f, uk.TOL)
                    r2, _ = plan_probe.plan(probe, cfg2, uk.CUS)
                    r3 = uk.resolve(probe, a, dv, k, 3, f)
                    cfg4 = config(a, 0, dv, k, uk.BATCH, 4, f, uk.TOL)
                    r4, _ = plan_probe.plan(probe, cfg4, uk.CUS)
                    if r3 is not None:
                        bad.append(("variant 3 accepted", a, dv, k, f))
                    want4 = bool(fits) and dv <= 63 and k <= 10 and r2 is not None
                    if (r4 is not None) != want4 or (r4 is not None and not r4["wave"]):
                        bad.append(("variant 4", a, dv, k, f, r4 is not None, want4))
                    for r, cfg in ((r2, cfg2), (r4, cfg4)):
                        if r is not None:
                            accepted += 1
                            problems = check_layout(probe, cfg, r)
                            checked += 1
                            if problems:
                                bad.append(("layout", a, dv, k, f, cfg.variant, problems))
                for batch, cus in ((1, 256), (uk.BATCH, 256), (4096, 8)):
                    r0 = uk.resolve(probe, a, dv, k, 0, 0, batch, uk.TOL, cus)
                    if r0 is not None and (r0["wave"] or r0["variant"] != 2):
                        bad.append(("variant 0 left the wg kernel", a, dv, k, batch, cus, r0["variant_name"]))
    a, dv, k = uk.REFUSED_WG
    for batch in (uk.BATCH, 20, 11):
        for v in (2, 4):
            if uk.resolve(probe, a, dv, k, v, 0, batch) is not None:
                bad.append(("REFUSED_WG is accepted", batch, v))
        if uk.resolve(probe, a, dv, k, 0, 0, batch) is not None:  # (the library's choice then goes to the lane mapping)
            bad.append(("REFUSED_WG: variant 0 is planned on wg", batch))
    print(f"{accepted} accepted configurations, {checked} layouts checked, {time.perf_counter() - t0:.1f} s")
    assert accepted > 0 and not bad, (len(bad), bad[:6])
