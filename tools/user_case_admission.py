"""Which shapes of tests/user_kernel_classes.py can hold a plugin kernel to the oracle at all: measured on the reference
side, on the CPU, without a GPU.  The fp64 rule of tools/kernel_case_admission.py, unchanged, for user models.

    python tools/user_case_admission.py            # re-measure every case of CASES and compare with its recorded columns
    python tools/user_case_admission.py --select   # choose the members of every class; print the CASES block
    python tools/user_case_admission.py --select --write   # ... and put it into tests/user_kernel_classes.py
    python tools/user_case_admission.py ALIAS DV KMAX       # figures of one candidate (ALIAS: 0..4)

Method: tests/user_models/user_oracle.cpp (the oracle's generic controller on the user header) is built for the alias
twice, with -ffp-contract=off and with -ffp-contract=fast -mfma: the same statements in the same order.  Both builds run
the 20 instances of its built-in scenario for 6 ticks, the contracted build teacher-forced from the plain build's
controller state and x every tick, with tol = 1e-6 and with tol = 0.

Admitted for a tolerance mode: every Arnoldi count and exit reason equal, |du| <= 1e-10 * max(1, |u|), |ddUdt'| <= 1e-8 *
max(1, |dUdt'|) (a tenth of the device bounds 1e-9 and 1e-7); the two builds free-running for 12 ticks
from the seeded start end within 1e-8 on u and x with equal counts and reasons at the last tick; with tol = 0 the plain
build runs k_max iterations on every tick.  A candidate that is not admitted with tol = 1e-6 is passed over for the next
member of its class in the same ordering; one admitted with tol = 1e-6 only gets fixed_k_ok = False.  No bound is widened
to keep a shape.  user_kernel_classes.DEVICE_MISSES is passed over in the same way and named in the table."""
import math
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plan_probe  # noqa: E402
import user_kernel_classes as uk  # noqa: E402
import user_oracle  # noqa: E402

N_INST, N_TICKS, LOOP_TICKS = 20, 6, 12
TOLS = (1e-6, 0.0)
F64_U, F64_D, F64_LOOP = 1e-10, 1e-8, 1e-8

_tmp = None
_dims = {}


def exes(alias):
    """(plain, fast) executables of the alias, built once per run into a temporary directory"""
    cls = uk.ALIASES[alias]
    return tuple(user_oracle.build(plan_probe.USER_MODELS_HPP, cls, os.path.join(_tmp, f"{cls}_{name}"), flavour)
                 for name, flavour in (("plain", user_oracle.PLAIN), ("fast", user_oracle.FAST)))


def worse(a, b):
    return max(a, b) if math.isfinite(b) else math.inf  # (max() drops a NaN)


def rel_rows(a, b):
    """worst over instances and ticks of max|a - b| / max(1, max|a|), each taken over one instance's vector at one tick"""
    err = np.max(np.abs(a - b), axis=-1) / np.maximum(1.0, np.max(np.abs(a), axis=-1))
    return float(np.max(err)) if np.all(np.isfinite(err)) else math.inf


def measure(alias, dv, k_max, tol):
    """(su, sd, agree): worst spread of u and dUdt' between the two builds, teacher-forced, relative to max(1, |.|) of
    the plain build's vector, and whether all counts and reasons agreed."""
    plain, fast = exes(alias)
    d = _dims[alias]
    a, text = user_oracle.run_full(plain, d["dim_x"], d["dim_u"], N_INST, N_TICKS, dv, k_max, tol)
    path = os.path.join(_tmp, "forced.txt")
    open(path, "w").write(text)
    b, _ = user_oracle.run_full(fast, d["dim_x"], d["dim_u"], N_INST, N_TICKS, dv, k_max, tol, forced_from=path)
    assert np.array_equal(a["U"], b["U"]) and np.array_equal(a["x"], b["x"])  # the forcing took
    agree = np.array_equal(a["k"], b["k"]) and np.array_equal(a["reason"], b["reason"])
    return rel_rows(a["u"], b["u"]), rel_rows(a["d1"], b["d1"]), bool(agree)


def measure_loop(alias, dv, k_max, tol):
    """The two builds free-running for LOOP_TICKS ticks from the seeded start (what the device loop of the GPU test is
    compared with): (worst |du| and |dx| after the last tick, last tick's counts and reasons equal, every count of every
    tick of the plain build = k_max).  One tick more is run for the x the last plant step left."""
    d = _dims[alias]
    ends = [user_oracle.run_full(e, d["dim_x"], d["dim_u"], N_INST, LOOP_TICKS + 1, dv, k_max, tol)[0] for e in exes(alias)]
    a, b = ends
    n = LOOP_TICKS
    s = max(float(np.max(np.abs(a["u"][:, n - 1] - b["u"][:, n - 1]))), float(np.max(np.abs(a["x"][:, n] - b["x"][:, n]))))
    s = s if math.isfinite(s) else math.inf
    agree = np.array_equal(a["k"][:, n - 1], b["k"][:, n - 1]) and np.array_equal(a["reason"][:, n - 1], b["reason"][:, n - 1])
    return s, bool(agree), bool(np.all(a["k"][:, :n] == k_max))


_cache = {}


def admission(alias, dv, k_max):
    """per tolerance mode: (admitted, figures)"""
    key = (alias, dv, k_max)
    if key not in _cache:
        out = []
        for tol in TOLS:
            su, sd, agree = measure(alias, dv, k_max, tol)
            sl, agree_l, full = measure_loop(alias, dv, k_max, tol)
            finite = all(math.isfinite(v) for v in (su, sd, sl))
            ok = finite and agree and su <= F64_U and sd <= F64_D and agree_l and sl <= F64_LOOP and (tol > 0 or full)
            out.append((ok, (su, sd, agree, sl, agree_l, full)))
        _cache[key] = out
    return _cache[key]


def figures(adm):
    return " | ".join("%.1e %.1e %s, loop %.1e %s%s" % (f[0], f[1], "agree" if f[2] else "COUNTS DIFFER", f[3],
                                                       "agree" if f[4] else "COUNTS DIFFER", "" if f[5] else ", early exits")
                      for _, f in adm)


def pick(rows, cls):
    """the first member of `rows` admitted with tol = 1e-6 and not among the device misses of class `cls`, and one line per
    horizon passed over on the way (its k_max values and the figures of the first of them)"""
    passed = {}
    for r in rows:
        adm = admission(r[0], r[2], r[3])
        miss = uk.DEVICE_MISSES.get(cls, {}).get(r[2:4])
        if adm[0][0] and not miss:
            break
        what = "DEVICE MISS, " + miss + "; reference side" if miss else "not admitted"
        ks = passed.setdefault((r[2], what), ([], figures(adm)))[0]
        if r[3] not in ks:
            ks.append(r[3])
    else:
        r = adm = None
    text = ["dv %d k_max %s %s (k_max %d: %s)" % (dv, ",".join(map(str, ks)), what, ks[0], fig) for (dv, what), (ks, fig) in passed.items()]
    return r, adm, text


def select():
    lib = plan_probe.probe_user()
    mem = uk.members(lib)
    lines = ["CASES = ["]
    for c in sorted(mem):
        chosen = []  # [row, adm, passed, letters]
        for which, order in uk.orders(c):
            r, adm, passed = pick(order(mem[c]), c)
            if r is None:
                lines.append("    # %s %s: NO MEMBER ADMITTED" % (uk.class_name(c), which))
                lines += ["    #   " + t for t in passed[:6]]
                continue
            same = [ch for ch in chosen if ch[0][:6] == r[:6]]
            if same:
                same[0][3] += which
            else:
                chosen.append([r, adm, passed, which])
        for r, adm, passed, which in chosen:
            lines += ["    # " + t for t in passed]
            lines.append("    # %s: %s of %d, lds_bytes %d: %s" % (uk.class_name(c), which, len(mem[c]), r[6], figures(adm)))
            lines.append("    (%d, %d, %d, %d, %d, %r, %r, %r, %r)," % (r[0], r[2], r[3], r[4], r[5], c, r[7], adm[1][0], which))
    lines.append("]")
    return "\n".join(lines)


def write_block(text):
    """the CASES block of tests/user_kernel_classes.py and the digest behind it"""
    path = os.path.join(ROOT, "tests", "user_kernel_classes.py")
    src = open(path).read()
    head, rest = src.split("# BEGIN CASES", 1)
    first, tail = rest.split("\n", 1)[0], rest.split("# END CASES\n", 1)[1]
    tail = tail.split("\n", 1)[1]  # (the CASES_DIGEST line)
    scope = {}
    exec(text, scope)
    open(path, "w").write(head + "# BEGIN CASES" + first + "\n" + text + "\n# END CASES\nCASES_DIGEST = %r\n" % uk.digest(scope["CASES"]) + tail)


def check():
    """re-measure CASES; 0 when every recorded column is reproduced"""
    bad = 0
    for case in uk.CASES:
        adm = admission(case[0], case[1], case[2])
        ok = adm[0][0] and adm[1][0] == case[7] and case[1:3] not in uk.DEVICE_MISSES.get(case[5], {})
        bad += not ok
        print("%-28s %s  %s" % (uk.case_id(case), figures(adm), "ok" if ok else "RECORDED %r, MEASURED %r" % (case[7], adm[1][0])))
    print("%d cases, %d not reproduced" % (len(uk.CASES), bad))
    return 1 if bad else 0


def main(argv):
    global _tmp
    if "fma" not in open("/proc/cpuinfo").read().split():
        sys.exit("this CPU has no fused multiply-add: the contracted flavour cannot run here")
    lib = plan_probe.probe_user()
    for a in range(len(uk.ALIASES)):
        _dims[a] = uk.dims(lib, a)
    _tmp = tempfile.mkdtemp(prefix="user_oracle_")
    try:
        if "--select" in argv:
            text = select()
            print(text)
            if "--write" in argv:
                write_block(text)
            return 0
        if len(argv) == 3:
            a, dv, k = (int(v) for v in argv)
            adm = admission(a, dv, k)
            print(uk.case_id((a, dv, k, 2, 0)), figures(adm), "admitted:", [x[0] for x in adm])
            return 0
        return check()
    finally:
        shutil.rmtree(_tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
