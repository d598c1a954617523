"""Which shapes of tests/kernel_classes.py can hold a kernel to the oracle at all: measured on the reference side, on
the CPU, without a GPU and without the reference tree.

    python tools/kernel_case_admission.py            # re-measure every case of CASES and compare with its recorded columns
    python tools/kernel_case_admission.py --select   # choose members A and B of every class; print the CASES block
    python tools/kernel_case_admission.py --select --write   # ... and put it into tests/kernel_classes.py
    python tools/kernel_case_admission.py MODEL DTYPE DV KMAX   # figures of one candidate
    python tools/kernel_case_admission.py --inputs   # every case under the per-tick inputs of the fused loop (below)

Method (that of FP32_SPREAD in tests/test_gpu_tuning.py): the oracle is built a second time into a temporary directory
through oracle/Makefile's CXXFLAGS override: the Makefile's own flags with -ffp-contract=fast -mfma in place of
-ffp-contract=off (contraction does nothing on x86-64 unless the target has a fused multiply-add, so the flavour names
one).  Both builds are the same statements in the same order.  The 20 seeded instances of orc.batch_scenario that the
GPU test runs are stepped for 6 ticks, the contracted build teacher-forced from the plain build's controller state and
x every tick, with tol = 1e-6 and with tol = 0.  (A spread taken over the first six instances alone was exceeded by the
two builds themselves on the seventh: pendulum fp32, dv 105, k_max 20, dUdt' 7.4e-4 over six, 1.3e-3 over twenty.)  What
two roundings of the reference's own statements disagree on, no kernel can be held to.

Admitted for a tolerance mode:
    fp64   every Arnoldi count and exit reason equal, |du| <= 1e-10 * max(1, |u|), |ddUdt'| <= 1e-8 * max(1, |dUdt'|): a
           tenth of the device bounds (1e-9, 1e-7).  And, for the device loop of the GPU test: the two
           builds free-running for 12 ticks from the seeded start end within 1e-8 on u and x (a tenth of its 1e-7) with
           equal counts and reasons at the last tick; with tol = 0 the plain build runs k_max iterations on every tick
           (the GPU test asserts exactly that of the device).
    fp32   the figures are finite (the device's counts are not compared in fp32).  A spread of u or of U' above
           1e-4 / 8, or of dUdt' above 5e-3 / 8 relative, is recorded in fp32_spread, each quantity with its own
           figure, and the device bound of that quantity becomes 8 x its spread.  The device loop's bounds are fixed
           (1e-4 on u, x and U, 2e-3 relative on dUdt), so the free-running builds must end within an eighth of them:
           the same margin for the device's other association order.
A candidate that is not admitted with tol = 1e-6 is passed over for the next member of its class in the same ordering;
one that is admitted with tol = 1e-6 only gets fixed_k_ok = False.  kernel_classes.DEVICE_MISSES lists the shapes that were
admitted here and that a kernel then missed on the device with the lane mapping inside its bounds: findings about that
kernel, passed over in the same way and named in the table.  The selection, the check loop and the fp64 rule are those
of tests/class_ledger.py, which tools/user_case_admission.py uses as well.

--inputs: the GPU test also runs every case's 12-tick device loop under a moving reference ("ptau" leg) and under a
moving reference, a process disturbance and a measurement noise ("all" leg), and one plain tick behind it
(tests/class_harness.py: loop_inputs, oracle_loop_inputs).  The two builds run exactly that, each leg, each tolerance
mode the test runs for the case, and a leg is admitted for a case under the loop margins above: fp64 within 1e-8 on u, x
and the follow-up u with equal counts and reasons at the last tick and, with tol = 0, k_max iterations on every tick;
fp32 within 1e-4 / 8.  What it leaves out must be exactly what kernel_classes.leg_skip leaves out, and no class may end
without an admitted leg; its figures are the comment block above kernel_classes.leg_applies."""
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import class_harness as harness  # noqa: E402
import class_ledger as ledger  # noqa: E402
import kernel_classes as kc  # noqa: E402
import plan_probe  # noqa: E402
from class_ledger import LOOP_TICKS, N_INST, N_TICKS, TOLS, worse  # noqa: E402
from oracle import orc  # noqa: E402

F32_U, F32_D, F32_LOOP, F32_LOOP_D = 1e-4 / 8, 5e-3 / 8, 1e-4 / 8, 2e-3 / 8
PLAIN, FAST = "-ffp-contract=off", "-ffp-contract=fast -mfma"


def fast_flags():
    """oracle/Makefile's default CXXFLAGS with the contraction switched on"""
    for line in open(os.path.join(orc.HERE, "Makefile")):
        if line.startswith("CXXFLAGS") and PLAIN in line:
            return line.split("=", 1)[1].strip().replace(PLAIN, FAST)
    sys.exit("oracle/Makefile: no default CXXFLAGS with " + PLAIN)


def build_fast_flavour():
    """oracle/'s sources copied to a temporary directory and built there with fast_flags(); registers it as orc's
    library "fast".  Returns the directory (the caller removes it)."""
    if "fma" not in open("/proc/cpuinfo").read().split():
        sys.exit("this CPU has no fused multiply-add: the contracted flavour cannot run here")
    if not os.path.exists(orc.ORACLE_SO):
        orc.build(ref=False)
    tmp = tempfile.mkdtemp(prefix="oracle_fast_")
    for f in os.listdir(orc.HERE):
        if f.endswith((".cpp", ".hpp", ".h")) or f == "Makefile":
            shutil.copy(os.path.join(orc.HERE, f), tmp)
    subprocess.run(["make", "-C", tmp, "oracle", "CXXFLAGS=" + fast_flags()], check=True, stdout=subprocess.DEVNULL)
    orc.register_library("fast", os.path.join(tmp, "liboracle.so"))
    return tmp


def measure(model, dtype, dv, k_max, tol):
    """(su, sU, sd, agree): worst spread of u, U' and dUdt' between the two builds (fp64: relative to max(1, |.|) of the
    plain build's vector; fp32: u and U' absolute, dUdt' relative, as the device bounds are) and whether all counts and
    reasons agreed."""
    dt_name = kc.DTYPE_NAMES[dtype]
    f32 = dtype == 1
    x0, u0, p = orc.batch_scenario(model, N_INST)
    su = sU = sd = 0.0
    agree = True
    for i in range(N_INST):
        a = orc.Controller(model, dv, k_max, tol, dt_name)
        b = orc.Controller(model, dv, k_max, tol, dt_name, which="fast")
        orc.start_controller(a, x0[i], u0[i], p[i])
        orc.start_controller(b, x0[i], u0[i], p[i])
        x = x0[i].astype(np.float32).astype(np.float64) if f32 else x0[i].copy()
        for _ in range(N_TICKS):
            t, U, d = a.get_state()
            b.set_state(t, U, d)
            ua, ub = a.control(x), b.control(x)
            _, Ua, da = a.get_state()
            _, Ub, db = b.get_state()
            ka, _, ra = a.last_solve()
            kb, _, rb = b.last_solve()
            agree = agree and ka == kb and ra == rb
            scale = (lambda v: 1.0) if f32 else (lambda v: max(1.0, float(np.max(np.abs(v)))))
            su = worse(su, float(np.max(np.abs(ua - ub))) / scale(ua))
            sU = worse(sU, float(np.max(np.abs(Ua - Ub))) / scale(Ua))
            sd = worse(sd, float(np.max(np.abs(da - db))) / max(1.0, float(np.max(np.abs(da)))))
            if f32:
                x = (x.astype(np.float32) + a.plant(x, ua).astype(np.float32) * np.float32(a.dt)).astype(np.float64)
            else:
                x = x + a.plant(x, ua) * a.dt
    return su, sU, sd, agree


def measure_loop(model, dtype, dv, k_max, tol):
    """The two builds free-running for LOOP_TICKS ticks from the seeded start (what the device loop of the GPU test is
    compared with): (worst |du| and |dx| after the last tick, last tick's counts and reasons equal, every count of every
    tick of the plain build = k_max).  fp32: U joins u and x, and the relative spread of dUdt is returned as well (the
    quantities test_gpu_closed_loop.test_closed_loop_device_vs_oracle bounds)."""
    dt_name = kc.DTYPE_NAMES[dtype]
    npdt = np.float32 if dtype == 1 else np.float64
    x0, u0, p = orc.batch_scenario(model, N_INST)
    s, sd, agree, full = 0.0, 0.0, True, True
    for i in range(N_INST):
        ends = []
        for which in ("oracle", "fast"):
            c = orc.Controller(model, dv, k_max, tol, dt_name, which=which)
            orc.start_controller(c, x0[i], u0[i], p[i])
            x = np.array(x0[i], dtype=npdt)
            for _ in range(LOOP_TICKS):
                u = c.control(x)
                x = (x + c.plant(x, u).astype(npdt) * npdt(c.dt)).astype(npdt)
                full = full and (which == "fast" or c.last_solve()[0] == k_max)
            ends.append((u, x.astype(np.float64), c.last_solve(), c.get_state()))
        (ua, xa, la, (_, Ua, da)), (ub, xb, lb, (_, Ub, db)) = ends
        s = worse(s, max(float(np.max(np.abs(ua - ub))), float(np.max(np.abs(xa - xb)))))
        if dtype == 1:
            s = worse(s, float(np.max(np.abs(Ua - Ub))))
            sd = worse(sd, float(np.max(np.abs(da - db))) / max(1.0, float(np.max(np.abs(da)))))
        agree = agree and la[0] == lb[0] and la[2] == lb[2]
    return s, sd, agree, full


_cache = {}


def admission(r):
    """per tolerance mode: (admitted, figures, fp32 spread triple or None) of the shape of a case or member"""
    key = model, dtype, dv, k_max = (r.model, r.dtype, r.dv, r.k_max)
    if key not in _cache:
        out = []
        for tol in TOLS:
            su, sU, sd, agree = measure(model, dtype, dv, k_max, tol)
            sl, sld, agree_l, full = measure_loop(model, dtype, dv, k_max, tol)
            finite = all(math.isfinite(v) for v in (su, sU, sd, sl, sld))
            if dtype == 0:
                ok = finite and ledger.f64_admitted(tol, su, sd, agree, sl, agree_l, full)
                spread = None
            else:
                ok = finite and sl <= F32_LOOP and sld <= F32_LOOP_D
                spread = tuple(float("%.2e" % v) if v > lim else None for v, lim in ((su, F32_U), (sU, F32_U), (sd, F32_D)))
                spread = spread if ok and any(spread) else None
            out.append((ok, (su, sU, sd, agree, sl, agree_l, full), spread))
        _cache[key] = out
    return _cache[key]


def figures(adm):
    return " | ".join("%.1e %.1e %.1e %s, loop %.1e %s%s" % (f[0], f[1], f[2], "agree" if f[3] else "COUNTS DIFFER", f[4],
                                                            "agree" if f[5] else "COUNTS DIFFER", "" if f[6] else ", early exits")
                      for _, f, _ in adm)


def columns(adm):
    """(fixed_k_ok, fp32_spread) of an admitted case"""
    spread = (adm[0][2], adm[1][2] if adm[1][0] else None)
    return adm[1][0], (spread if any(spread) else None)


def row(c, r, adm, letters, n_members):
    return ["    # %s of %d, lds_bytes %d: %s" % (letters, n_members, r.lds_bytes, figures(adm)),
            "    (%d, %d, %d, %d, %d, %d, %r, %r, %r, %r)," % (kc.key(r) + (c, r.variant_name) + columns(adm))]


def label(c, r, which, rows):
    """"A = B" where the member of both selections is also the first of order_b before admission"""
    return "A = B" if which == ["A", "B"] and ledger.order_b(rows)[0] == r else which[0]


def select():
    return ledger.select(kc, kc.members(plan_probe.probe()), admission, figures, row, label)


def measure_inputs(case, tol, leg):
    """The two builds free-running under the leg's sequences of class_harness.loop_inputs, follow-up tick included:
    (worst |du|, |dx| and follow-up |du| between them after the last tick, last tick's counts and reasons equal, every
    count of every tick of the plain build = k_max)."""
    x0, u0, p = orc.batch_scenario(case.model, N_INST)
    dims = orc.Controller(case.model, case.dv, case.k_max)
    npdt = np.float32 if case.dtype == 1 else np.float64
    seq, d, v = harness.leg_of(leg, *harness.loop_inputs((dims.dim_x, dims.dim_p), case.dv, p, npdt))
    a, b = (harness.oracle_loop_inputs(orc, case.model, kc.DTYPE_NAMES[case.dtype], case.dv, case.k_max, tol, x0, u0, p,
                                       seq, d, v, which=which) for which in ("oracle", "fast"))
    s = 0.0
    for q in ("u", "x", "u_next"):
        s = worse(s, float(np.max(np.abs(a[q] - b[q]))))
    agree = bool(np.array_equal(a["k"], b["k"]) and np.array_equal(a["reason"], b["reason"]))
    return s, agree, bool(np.all(a["full"]))


def inputs_admitted(case, tol, s, agree, full):
    """the loop margins of the rule above: fp64 a tenth of the device bound with equal counts and reasons at the last tick
    and, with tol = 0, k_max iterations on every tick; fp32 an eighth of the device bound"""
    if case.dtype == 1:
        return s <= F32_LOOP
    return s <= ledger.F64_LOOP and agree and (tol > 0 or full)


def inputs():
    """Every case of CASES under the per-tick inputs of the GPU test's two legs, each tolerance mode the test runs: one
    line per case, the worst figure per leg and dtype, and whether kernel_classes.leg_skip is exactly what the
    measurement leaves out.  0 when it is and every class keeps an admitted case."""
    shapes, worst, out, held, pairs = {}, {}, {}, set(), set()
    for case in kc.RECORDS:
        words = []
        for leg in harness.LEGS:
            if not kc.leg_applies(case, leg):
                continue
            ok = True
            for tol in TOLS if case.fixed_k_ok else TOLS[:1]:
                key = (case.model, case.dtype, case.dv, case.k_max, tol, leg)
                pairs.add(key[:5])
                if key not in shapes:
                    shapes[key] = measure_inputs(case, tol, leg)
                s, agree, full = shapes[key]
                adm = inputs_admitted(case, tol, s, agree, full)
                ok = ok and adm
                words.append("%s tol %g: %.1e %s%s%s" % (leg, tol, s, "agree" if agree else "COUNTS DIFFER",
                                                        "" if full else ", early exits", "" if adm else " NOT ADMITTED"))
                group = (leg, kc.DTYPE_NAMES[case.dtype], kc.MODEL_NAMES[case.model], adm)
                lo, hi = worst.get(group, (math.inf, 0.0))
                worst[group] = (min(lo, s), worse(hi, s))
            out[(kc.key(case), leg)] = ok
            if ok:
                held.add(case.cls)
        print("%-40s %s" % (kc.case_id(case), " | ".join(words)))
    for (leg, dt, model, adm), (lo, hi) in sorted(worst.items()):
        print("leg %-4s %s %-10s %s: %.1e .. %.1e" % (leg, dt, model, "admitted" if adm else "NOT ADMITTED", lo, hi))
    rejected = sorted(k for k, ok in out.items() if not ok)
    skipped = sorted((kc.key(c), leg) for c in kc.RECORDS for leg in harness.LEGS if kc.leg_applies(c, leg) and kc.leg_skip(c, leg))
    bare = sorted({c.cls for c in kc.RECORDS} - held)
    print("%d cases, %d shape/tolerance pairs; ptau leg: %d cases, all leg: %d cases; %d not admitted, %d skipped by the rule"
          % (len(kc.RECORDS), len(pairs), sum(leg == "ptau" for _, leg in out), sum(leg == "all" for _, leg in out),
             len(rejected), len(skipped)))
    if rejected != skipped:
        print("THE RULE OF kernel_classes.leg_skip DIFFERS FROM THE MEASUREMENT:", sorted(set(rejected) ^ set(skipped)))
    if bare:
        print("CLASSES WITHOUT AN ADMITTED LEG:", [kc.class_name(c) for c in bare])
    return 1 if rejected != skipped or bare else 0


def main(argv):
    tmp = build_fast_flavour()
    try:
        if "--inputs" in argv:
            return inputs()
        if "--select" in argv:
            text = select()
            print(text)
            if "--write" in argv:
                ledger.write_block(os.path.join(ROOT, "tests", "kernel_classes.py"), text)
            return 0
        if len(argv) == 4:
            r = kc.Member(*(int(a) for a in argv), 2, 0, 0, "")
            adm = admission(r)
            print(kc.case_id(r), figures(adm), "admitted:", [a[0] for a in adm], "fp32_spread:", [a[2] for a in adm])
            return 0
        return ledger.check(kc, admission, figures, columns, lambda case: (case.fixed_k_ok, case.fp32_spread), 40)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
