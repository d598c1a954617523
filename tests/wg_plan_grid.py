"""The configurations of tests/data/wg_plan_parent.json (see test_wg_plan.py): rows of
(model_id, dtype, dv, k_max, batch, variant, flags, tol); dtype 0 = f64, 1 = f32.  The file holds one result per row of
grid(), in grid()'s order, and the digest of that order."""
import hashlib
FLAGS = {"SERIAL_COSTATE": 1, "IPW8": 2, "NO_BINNING": 4, "TWO_PASS_COSTATE": 8, "NO_WAVE": 16, "WAVE_FRESH_TRIG": 32,
         "WAVE_SERIAL_SWEEPS": 64, "SERIAL_STATE_SWEEP": 128}
PAIRS = [(m, d) for m in (0, 1, 2) for d in (0, 1)]  # pendulum, msd, semiactive x f64, f32
SIZES = [(50, 10), (25, 5), (3, 3), (5, 3), (53, 12), (100, 20)]
TOL = 1e-6


def set_a():
    return [(m, d, dv, k, 4096, v, 0, TOL) for m, d in PAIRS
            for dv in (1, 2, 3, 4, 5, 7, 8, 20, 25, 26, 30, 32, 33, 42, 50, 53, 54, 63, 64, 100, 107)
            for k in (1, 3, 10, 12, 13) for v in (0, 2, 3)]  # (k_max 5 and 20 are in SIZES)


def set_b():
    return [(m, d, dv, k, b, v, 0, TOL) for m, d in PAIRS for dv, k in SIZES
            for b in (1, 16, 1024, 2048, 2049, 4096, 4097, 8192) for v in (0, 2, 3, 4)]


def set_c():
    fl = list(FLAGS.values()) + [FLAGS["SERIAL_COSTATE"] | FLAGS["SERIAL_STATE_SWEEP"], FLAGS["IPW8"] | FLAGS["TWO_PASS_COSTATE"]]
    return [(m, d, dv, k, b, v, f, TOL) for m, d in PAIRS for dv, k in SIZES for b in (16, 4096) for v in (0, 2) for f in fl]


def set_d():
    """every configuration of a variant_name assertion in test_gpu_parity.py, test_gpu_row_newton.py, test_gpu_wave.py"""
    F = FLAGS
    rows = []
    par_cases = [(0, 50, 10, 1e-6, 40, 0), (0, 49, 10, 0.0, 33, 0), (0, 47, 8, 1e-6, 17, 0), (0, 64, 8, 1e-6, 23, 0),
                 (0, 25, 6, 0.0, 21, 0), (0, 24, 6, 1e-6, 19, 0), (0, 16, 5, 1e-6, 20, 0), (0, 7, 3, 1e-6, 18, 0),
                 (0, 4, 3, 0.0, 5, 0), (2, 50, 10, 1e-6, 48, 0), (2, 37, 6, 0.0, 19, 0), (1, 26, 6, 1e-6, 21, 0),
                 (1, 9, 4, 0.0, 16, 0), (1, 50, 10, 1e-6, 35, 0), (0, 100, 20, 1e-6, 19, 0), (0, 100, 20, 1e-6, 33, 1),
                 (0, 53, 12, 0.0, 16, 0)]
    for m, dv, k, tol, b, d in par_cases:  # test_chunk_parallel_costate_vs_serial_and_oracle
        for v, f in ((2, F["SERIAL_STATE_SWEEP"]), (2, F["TWO_PASS_COSTATE"]), (3, 0), (2, F["SERIAL_COSTATE"]), (3, F["SERIAL_COSTATE"])):
            rows.append((m, d, dv, k, b, v, f, tol))
    rows.append((0, 0, 50, 10, 100, 2, F["IPW8"], 1e-6))  # test_eight_instances_per_workgroup_on_request
    for m, d, dv, k, v, f in ((0, 0, 50, 10, 2, 0), (0, 0, 50, 10, 2, F["SERIAL_STATE_SWEEP"]), (0, 0, 40, 10, 2, 0), (0, 0, 54, 10, 2, 0),
                              (0, 1, 50, 10, 2, 0), (0, 0, 53, 12, 2, 0), (0, 0, 53, 12, 2, F["SERIAL_STATE_SWEEP"]), (0, 0, 30, 10, 2, 0),
                              (1, 0, 50, 10, 2, 0), (0, 0, 50, 10, 3, 0), (0, 1, 100, 20, 3, 0), (1, 0, 50, 10, 3, 0),
                              (0, 0, 50, 10, 2, F["SERIAL_COSTATE"]), (0, 0, 5, 3, 3, 0)):
        rows.append((m, d, dv, k, 16, v, f, 0.0))
    # test_gpu_row_newton.py
    for dv, k, d, v, f in ((50, 10, 0, 2, 0), (43, 5, 0, 2, 0), (53, 8, 0, 2, 0), (44, 12, 0, 2, 0), (42, 10, 0, 2, 0), (33, 10, 0, 2, 0),
                           (32, 10, 0, 2, 0), (25, 5, 0, 2, 0), (54, 10, 0, 2, 0), (50, 10, 1, 2, 0), (50, 10, 0, 2, F["SERIAL_STATE_SWEEP"]),
                           (50, 10, 0, 2, F["SERIAL_COSTATE"]), (50, 10, 0, 3, 0), (50, 10, 0, 0, 0)):
        rows.append((0, d, dv, k, 4096, v, f, TOL))
    for m, dv, k, d, f in ((2, 50, 10, 0, 0), (2, 7, 3, 0, 0), (2, 53, 12, 0, 0), (2, 50, 10, 1, 0), (2, 50, 10, 0, F["SERIAL_STATE_SWEEP"]),
                           (2, 50, 10, 0, F["SERIAL_COSTATE"]), (1, 26, 10, 0, 0)):
        rows.append((m, d, dv, k, 4096, 2, f, TOL))
    for dv, k in ((33, 10), (34, 4), (35, 6), (36, 12), (39, 8), (42, 10), (43, 5), (44, 12), (45, 7), (46, 9), (47, 3), (48, 11),
                  (49, 10), (50, 10), (51, 2), (52, 12), (53, 12)):
        rows.append((0, 0, dv, k, 37, 2, 0, 1e-6))
    for dv, k in ((2, 2), (3, 3), (4, 4), (5, 5), (8, 4), (17, 6), (31, 10), (32, 12), (47, 7), (50, 10), (53, 12)):
        rows.append((2, 0, dv, k, 37, 2, 0, 1e-6))
    for b, dv, k, tol, f in ((67, 50, 10, 1e-6, 0), (67, 50, 10, 0.0, 0), (67, 50, 10, 1e-6, F["WAVE_FRESH_TRIG"]), (67, 50, 10, 0.0, F["WAVE_FRESH_TRIG"]),
                             (300, 50, 10, 1e-6, 0), (300, 50, 10, 1e-6, F["SERIAL_STATE_SWEEP"]), (37, 44, 4, 1e-6, 0), (37, 44, 4, 0.0, 0),
                             (19, 50, 10, 1e-6, 0), (19, 50, 10, 0.0, 0)):
        rows.append((0, 0, dv, k, b, 2, f, tol))
    # test_gpu_wave.py
    for m, d, dv, k, b, v, f in ((0, 0, 50, 10, 300, 0, 0), (0, 0, 50, 10, 300, 0, F["NO_WAVE"]), (0, 1, 50, 10, 300, 0, 0), (0, 0, 64, 10, 300, 0, 0),
                                 (0, 0, 50, 12, 300, 0, 0), (2, 0, 50, 10, 64, 0, 0), (1, 0, 50, 10, 64, 0, 0), (0, 0, 64, 10, 8, 4, 0),
                                 (1, 0, 20, 12, 8, 4, 0), (0, 0, 50, 10, 8, 0, 0)):
        rows.append((m, d, dv, k, b, v, f, TOL))
    return rows


def grid():
    seen, out = set(), []
    for r in set_a() + set_b() + set_c() + set_d():
        if r not in seen:
            seen.add(r), out.append(r)
    return out


def digest():
    return hashlib.sha256(repr(grid()).encode()).hexdigest()[:16]


# a result: NAMES index, then the fields below; base_off (8 ints) follows only where one of them is not 0
NAMES = ["wave", "wg", "wg+parallel-costate", "wg+two-pass-costate", "wg+row-newton", "wg+row-scan", "wg-lean",
         "wg-lean+two-pass-costate"]
FIELDS = ["variant_name", "ipw", "maxm", "plan", "par", "cs_chunks", "nwt", "wave", "variant", "lds_bytes", "lds_bytes_hook",
          "lds_bytes_tick", "fh_hbm", "fh_hbm_hook", "binning", "base_off"]
