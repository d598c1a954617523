"""Which shapes of tests/user_kernel_classes.py can hold a plugin kernel to the oracle at all: measured on the reference
side, on the CPU, without a GPU.  The fp64 rule of tools/kernel_case_admission.py (tests/class_ledger.py has it, with
the selection and the check loop, for both tools), for user models.

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

import class_ledger as ledger  # noqa: E402
import plan_probe  # noqa: E402
import user_kernel_classes as uk  # noqa: E402
import user_oracle  # noqa: E402
from class_ledger import LOOP_TICKS, N_INST, N_TICKS, TOLS  # noqa: E402

_tmp = None
_dims = {}


def exes(alias):
    """(plain, fast) executables of the alias, built once per run into a temporary directory"""
    cls = uk.ALIASES[alias]
    return tuple(user_oracle.build(plan_probe.USER_MODELS_HPP, cls, os.path.join(_tmp, f"{cls}_{name}"), flavour)
                 for name, flavour in (("plain", user_oracle.PLAIN), ("fast", user_oracle.FAST)))


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


def admission(r):
    """per tolerance mode: (admitted, figures) of the shape of a case or member"""
    key = alias, dv, k_max = (r.alias, r.dv, r.k_max)
    if key not in _cache:
        out = []
        for tol in TOLS:
            su, sd, agree = measure(alias, dv, k_max, tol)
            sl, agree_l, full = measure_loop(alias, dv, k_max, tol)
            out.append((ledger.f64_admitted(tol, su, sd, agree, sl, agree_l, full), (su, sd, agree, sl, agree_l, full)))
        _cache[key] = out
    return _cache[key]


def figures(adm):
    return " | ".join("%.1e %.1e %s, loop %.1e %s%s" % (f[0], f[1], "agree" if f[2] else "COUNTS DIFFER", f[3],
                                                       "agree" if f[4] else "COUNTS DIFFER", "" if f[5] else ", early exits")
                      for _, f in adm)


def fixed_k_ok(adm):
    return adm[1][0]


def row(c, r, adm, letters, n_members):
    return ["    # %s: %s of %d, lds_bytes %d: %s" % (uk.class_name(c), letters, n_members, r.lds_bytes, figures(adm)),
            "    (%d, %d, %d, %d, %d, %r, %r, %r, %r)," % (uk.key(r) + (c, r.variant_name, fixed_k_ok(adm), letters))]


def select():
    return ledger.select(uk, uk.members(plan_probe.probe_user()), admission, figures, row, lambda c, r, which, rows: "".join(which))


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
                ledger.write_block(os.path.join(ROOT, "tests", "user_kernel_classes.py"), text)
            return 0
        if len(argv) == 3:
            r = uk.Member(*(int(v) for v in argv), 2, 0, 0, "")
            adm = admission(r)
            print(uk.case_id(r), figures(adm), "admitted:", [x[0] for x in adm])
            return 0
        return ledger.check(uk, admission, figures, fixed_k_ok, lambda case: case.fixed_k_ok, 28)
    finally:
        shutil.rmtree(_tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
