"""ORACLE — TEST INFRASTRUCTURE ONLY.  Recorded outputs of the compiled reference (oracle/_ref/libref.so) that
tests/test_oracle_vs_ref.py holds the oracle to, bit for bit, without the reference at hand:

  * closed loops of the shipped scenarios (1500 ticks, 400 for dv = 100): Newton start, u, x, Arnoldi counts;
  * seeded random controller states: F, prepare, Ax, control, Arnoldi count and the advanced state;
  * fp32: the reference's own state before each of 5 ticks and its control;
  * non-shipped tuning constants (TUNING_SETS, compiled into the reference through the tag structs of
    oracle/ref_harness.cpp): 400-tick closed loops and the seeded random states, which anchor orc_create_tuned.

    python -m oracle.ref_records        (needs oracle/_ref/libref.so: oracle/Makefile `ref`)

writes tests/golden/oracle_vs_ref/*.npz.  record_*() replay the same calls on either library ("ref" or "oracle")."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "oracle_vs_ref")

# (model, dv, kmax, tol); tol = -1: the reference's default
CASES = [(0, 25, 5, -1.0), (0, 50, 10, -1.0), (0, 50, 10, 0.0), (0, 100, 20, -1.0),
         (1, 50, 5, -1.0), (1, 20, 5, -1.0), (1, 50, 10, -1.0),
         (2, 50, 5, -1.0), (2, 50, 10, -1.0), (2, 8, 3, -1.0)]
RANDOM_CASES = CASES[:3] + CASES[4:5] + CASES[7:8]
FP32_MODELS = (0, 1, 2)

# Tuning constants other than the shipped dt = 1e-3, h = 2e-3, zeta = 1000 (1 - zeta*h = -1), Tf = 0.5 | 1, alpha = 0.5:
#   fast: 1 - zeta*h = -0.5, dt != shipped;  long: +0.5, the longest horizon;  mid: -0.2
TUNING_SETS = {
    "fast": dict(dt=5e-4, h=1e-3, zeta=1500.0, Tf=0.25, alpha=4.0),
    "long": dict(dt=1e-3, h=4e-3, zeta=125.0, Tf=1.5, alpha=1.0),
    "mid": dict(dt=1e-3, h=3e-3, zeta=400.0, Tf=1.0, alpha=3.0),
}
# (set, model, dv, kmax): the table of pick_tuned in oracle/ref_harness.cpp
TUNED_CASES = [(s, m, 8, 3) for s in TUNING_SETS for m in (0, 1, 2)] + [("long", m, 50, 10) for m in (0, 1, 2)]
TUNED_TICKS = 400


def case_path(model, dv, kmax, tol):
    return os.path.join(OUT, f"loop_m{model}_dv{dv}_k{kmax}_tol{'ref' if tol < 0 else 'fixed'}.npz")


def fp32_path(model):
    return os.path.join(OUT, f"fp32_m{model}.npz")


def tuned_path(name, model, dv, kmax):
    return os.path.join(OUT, f"tuned_{name}_m{model}_dv{dv}_k{kmax}.npz")


def record_loop(orc, which, model, dv, kmax, tol, tuning=None, ticks=None):
    c = orc.Controller(model, dv, kmax, tol, which=which, tuning=tuning)
    x0, u0, p = orc.shipped_scenario(model)
    un = orc.start_controller(c, x0, u0, p)
    us, xs, ks, _ = orc.closed_loop(c, x0, ticks or (1500 if dv < 100 else 400))
    return {"u_newton": un, "loop_u": us, "loop_x": xs, "loop_k": ks}


def record_random(orc, which, model, dv, kmax, tol, tuning=None):
    rng = np.random.default_rng(99 + model)
    c = orc.Controller(model, dv, kmax, tol, which=which, tuning=tuning)
    x0, u0, p = orc.shipped_scenario(model)
    rec = {k: [] for k in ("rs_F", "rs_prepare", "rs_Ax", "rs_u", "rs_k", "rs_t", "rs_U", "rs_dUdt")}
    for trial in range(10):
        U = np.tile(u0, dv) * (1 + 0.05 * rng.standard_normal(c.len))
        d = 0.1 * rng.standard_normal(c.len) if trial else np.zeros(c.len)
        t = float(rng.uniform(0, 3)) if trial else 0.0
        x = x0 + 0.1 * rng.standard_normal(c.dim_x)
        pt = np.tile(p, dv + 1) + (0.05 * rng.standard_normal(c.dim_p * (dv + 1)) if c.dim_p else 0)
        c.set_ptau(pt)
        c.set_state(t, U, d)
        rec["rs_F"].append(c.F(U, x, t))
        rec["rs_prepare"].append(c.prepare(x))
        rec["rs_Ax"].append(c.Ax(rng.standard_normal(c.len)))
        rec["rs_u"].append(c.control(x))
        rec["rs_k"].append(c.last_solve()[0])
        t1, U1, d1 = c.get_state()
        rec["rs_t"].append(t1), rec["rs_U"].append(U1), rec["rs_dUdt"].append(d1)
    return {k: np.array(v) for k, v in rec.items()}


def record_fp32_reference(orc, model):
    """The fp32 reference's own closed-loop state (t, U, dUdt) before each of 5 ticks at the shipped x0, and its
    control of that tick."""
    a = orc.Controller(model, 50, 10, -1.0, "f32", which="ref")
    x0, u0, p = orc.shipped_scenario(model)
    orc.start_controller(a, x0, u0, p)
    rec = {k: [] for k in ("t", "U", "dUdt", "u")}
    for tick in range(5):
        t, U, d = a.get_state()
        rec["t"].append(t), rec["U"].append(U), rec["dUdt"].append(d)
        rec["u"].append(a.control(x0))
    return {k: np.array(v) for k, v in rec.items()}


def record_case(orc, which, case):
    rec = record_loop(orc, which, *case)
    if case in RANDOM_CASES:
        rec.update(record_random(orc, which, *case))
    return rec


def record_tuned(orc, which, name, model, dv, kmax):
    """Closed loop of the shipped scenario and the seeded random states under TUNING_SETS[name], plus the constants the
    library reports for the instance."""
    tun = TUNING_SETS[name]
    rec = record_loop(orc, which, model, dv, kmax, -1.0, tuning=tun, ticks=TUNED_TICKS)
    rec.update(record_random(orc, which, model, dv, kmax, -1.0, tuning=tun))
    c = orc.Controller(model, dv, kmax, -1.0, which=which, tuning=tun)
    rec["tuning"] = np.array([c.dt, c.h, c.zeta, c.Tf, c.alpha])
    return rec


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import orc
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built: the records come from the compiled reference")
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        np.savez_compressed(case_path(*case), **record_case(orc, "ref", case))
    for model in FP32_MODELS:
        np.savez_compressed(fp32_path(model), **record_fp32_reference(orc, model))
    for case in TUNED_CASES:
        np.savez_compressed(tuned_path(*case), **record_tuned(orc, "ref", *case))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
