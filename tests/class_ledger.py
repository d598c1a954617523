"""What the two class tables (tests/kernel_classes.py for the built-in models, tests/user_kernel_classes.py for plugin
models), their admission tools (tools/kernel_case_admission.py, tools/user_case_admission.py) and their CPU ledgers
(tests/test_kernel_ledger.py, tests/test_user_kernel_ledger.py) share.  A plain module: no GPU call, nothing from
conftest.

A table module `t` offers CASES (plain tuples, as its tool writes them), CASES_DIGEST, RECORDS (the same rows as Case
records), members(lib) (class -> Member records), key(r) (the configuration of a case or member), case_id(r),
class_name(c), kind(c), orders(c), cfg(*key, batch, tol), resolve(lib, *key, batch, tol, cus), class_of(r), grid(),
DEVICE_MISSES and the grid's BATCH, TOL, CUS."""
import hashlib
import math

import plan_probe

# the columns both tables have, behind a row's subject: (model, dtype) or (alias,)
CASE_COLUMNS = "dv k_max variant flags cls variant_name fixed_k_ok"
MEMBER_COLUMNS = "dv k_max variant flags lds_bytes variant_name"
# the reference-side measurement both tools make: instances, teacher-forced ticks, free-running ticks, tolerance modes
N_INST, N_TICKS, LOOP_TICKS = 20, 6, 12
TOLS = (1e-6, 0.0)
F64_U, F64_D, F64_LOOP = 1e-10, 1e-8, 1e-8


def f64_admitted(tol, su, sd, agree, sl, agree_l, full):
    """The fp64 rule for one tolerance mode: the two builds' teacher-forced spread of u and dUdt' within a tenth of the
    device bounds with equal counts and reasons, their free runs within F64_LOOP with equal counts and reasons at the
    last tick, and with tol = 0 every tick of the plain build at k_max iterations."""
    finite = all(math.isfinite(v) for v in (su, sd, sl))
    return finite and agree and su <= F64_U and sd <= F64_D and agree_l and sl <= F64_LOOP and (tol > 0 or full)


def worse(a, b):
    return max(a, b) if math.isfinite(b) else math.inf  # (max() drops a NaN)


def order_a(rows):
    """members with k_max >= 3 by dv, then k_max; behind them (a class may have no other) those with k_max < 3 by dv, the
    larger k_max first; among configurations of one shape the plain one (no flag, variant 2) first"""
    return sorted(rows, key=lambda r: (r.k_max < 3, r.dv, r.k_max if r.k_max >= 3 else -r.k_max, r.flags, r.variant))


def order_b(rows):
    """largest lds_bytes, then largest dv, then largest k_max"""
    return sorted(rows, key=lambda r: (-r.lds_bytes, -r.dv, -r.k_max, r.flags, r.variant))


def digest(cases):
    """of the whole table (the plain tuples), columns included: CASES_DIGEST is written with the table, so a case that is
    deleted or edited by hand shows in the table's ledger test"""
    return hashlib.sha256(repr(sorted(cases)).encode()).hexdigest()[:16]


def pick(rows, cls, admission, device_misses, figures):
    """the first member of `rows` admitted with tol = 1e-6 and not among the device misses of class `cls`, and one line per
    horizon passed over on the way (its k_max values and the figures of the first of them)"""
    passed = {}
    for r in rows:
        adm = admission(r)
        miss = device_misses.get(cls, {}).get((r.dv, r.k_max))
        if adm[0][0] and not miss:
            break
        what = "DEVICE MISS, " + miss + "; reference side" if miss else "not admitted"
        ks = passed.setdefault((r.dv, what), ([], figures(adm)))[0]
        if r.k_max not in ks:
            ks.append(r.k_max)
    else:
        r = adm = None
    text = ["dv %d k_max %s %s (k_max %d: %s)" % (dv, ",".join(map(str, ks)), what, ks[0], fig) for (dv, what), (ks, fig) in passed.items()]
    return r, adm, text


def select(t, mem, admission, figures, row, label):
    """The CASES block of table module `t`: per class of `mem` the picks of t.orders(c), one entry where two selections
    pick the same member.  row(c, r, adm, letters, n_members) formats the entry's comment and tuple lines;
    label(c, r, which, mem[c]) makes `letters` of the selections `which` that chose r."""
    lines = ["CASES = ["]
    for c in sorted(mem):
        chosen = []  # [member, adm, passed, selections]
        for which, order in t.orders(c):
            r, adm, passed = pick(order(mem[c]), c, admission, t.DEVICE_MISSES, figures)
            if r is None:
                lines.append("    # %s %s: NO MEMBER ADMITTED" % (t.class_name(c), which))
                lines += ["    #   " + p for p in passed[:6]]
                continue
            same = [ch for ch in chosen if ch[0] == r]
            if same:
                same[0][3].append(which)
            else:
                chosen.append([r, adm, passed, [which]])
        for r, adm, passed, which in chosen:
            lines += ["    # " + p for p in passed]
            lines += row(c, r, adm, label(c, r, which, mem[c]), len(mem[c]))
    lines.append("]")
    return "\n".join(lines)


def write_block(path, text):
    """the CASES block of the table module at `path` and the digest behind it"""
    src = open(path).read()
    head, rest = src.split("# BEGIN CASES", 1)
    first, tail = rest.split("\n", 1)[0], rest.split("# END CASES\n", 1)[1]
    tail = tail.split("\n", 1)[1]  # (the CASES_DIGEST line)
    scope = {}
    exec(text, scope)
    open(path, "w").write(head + "# BEGIN CASES" + first + "\n" + text + "\n# END CASES\nCASES_DIGEST = %r\n" % digest(scope["CASES"]) + tail)


def check(t, admission, figures, columns, recorded, width):
    """re-measure t.RECORDS; 0 when every recorded column (recorded(case) against columns(adm)) is reproduced"""
    bad = 0
    for case in t.RECORDS:
        adm = admission(case)
        ok = adm[0][0] and columns(adm) == recorded(case) and (case.dv, case.k_max) not in t.DEVICE_MISSES.get(case.cls, {})
        bad += not ok
        print("%-*s %s  %s" % (width, t.case_id(case), figures(adm), "ok" if ok else "RECORDED %r, MEASURED %r" % (recorded(case), columns(adm))))
    print("%d cases, %d not reproduced" % (len(t.RECORDS), bad))
    return 1 if bad else 0


def assert_every_class_has_a_case(t, members, note=""):
    have = {case.cls for case in t.RECORDS}
    print(f"{len(members)} classes over {len(t.grid())} configurations{note}, {len(t.RECORDS)} cases")
    missing = sorted(set(members) - have)
    stray = sorted(have - set(members))
    assert not missing, "classes without a case: " + ", ".join(
        "%s (%d members, e.g. %s)" % (t.class_name(c), len(members[c]), t.case_id(order_a(members[c])[0])) for c in missing)
    assert not stray, "cases of a class the grid does not yield: " + ", ".join(t.class_name(c) for c in stray)
    assert len({t.key(case) for case in t.RECORDS}) == len(t.RECORDS)


def table_tests(t, tool):
    """the three tests that are the same for both tables; a ledger module with a `probe` fixture binds them under these names"""

    def test_the_table_is_the_one_the_admission_tool_wrote():
        """A guard against an accidental edit (a deleted or changed line), no more: the digest sits in the same file."""
        assert digest(t.CASES) == t.CASES_DIGEST, \
            "CASES was edited (a case deleted, added or changed) without %s --select --write" % tool

    def test_every_case_resolves_to_its_recorded_class_and_name(probe):
        """... at the grid's batch and at the batches and tolerances the GPU test creates its handles with, on a small and a
        large device: the class recorded is the kernel launched there (the GPU test itself can only ask for variant_name)."""
        bad = []
        for case in t.RECORDS:
            if t.kind(case.cls) == "lane":
                assert (case.variant, case.flags, case.variant_name) == (1, 0, "lane")
                continue
            for batch in (t.BATCH, 20, 11):
                for tol in (t.TOL, 0.0):
                    for cus in (t.CUS, 8):
                        r = t.resolve(probe, *t.key(case), batch, tol, cus)
                        got = None if r is None else (t.class_of(r), r["variant_name"])
                        if got != (case.cls, case.variant_name):
                            bad.append((t.case_id(case), batch, tol, cus, got, (case.cls, case.variant_name)))
        assert not bad, bad[:5]

    def test_the_allocation_of_every_case_covers_its_layout(probe):
        """check_layout (tests/plan_probe.py), the look-ahead rule included, at the batch sizes the GPU test runs: before any
        of these shapes reaches a GPU.  (A wave case: the wg context of its sizes, which the handle keeps for the hooks.)"""
        bad = []
        for case in t.RECORDS:
            if t.kind(case.cls) == "lane":
                continue
            for batch in (t.BATCH, 20, 11):
                cfg = t.cfg(*t.key(case), batch, t.TOL)
                r, why = plan_probe.plan(probe, cfg, t.CUS)
                assert r is not None, (t.case_id(case), why)
                problems = plan_probe.check_layout(probe, cfg, r)
                if problems:
                    bad.append((t.case_id(case), batch, problems))
        assert not bad, bad[:5]

    return (test_the_table_is_the_one_the_admission_tool_wrote, test_every_case_resolves_to_its_recorded_class_and_name,
            test_the_allocation_of_every_case_covers_its_layout)
