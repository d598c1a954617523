"""GPU: the plain single-GPU run of bench.py — exactly K timed steps, none of the --full legs — and --dump-outputs:
the arrays of the last timed step, identical from run to run with the same arguments (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(argv),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_once_and_dumps_the_last_step(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _bench("--steps", "30", "--warmup", "10", "--dump-outputs", str(d))
        assert out["steps"] == 30 and out["warmup"] == 10 and out["reps"] == 1
        assert len(out["rep_ms_per_step"]) == 1 and out["ms_per_step"] == out["rep_ms_per_step"][0] > 0
        assert out["value"] == pytest.approx(4096 * 1e3 / out["ms_per_step"], rel=1e-9)
        assert out["unit"] == "control steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        for leg in ("reference_mode", "early_exit_placement", "cpu_baseline", "weak_scaling"):
            assert leg not in out
        assert out["parity"] == {}
        arrays = {}
        for name, shape in (("x", (4096, 4)), ("u", (4096, 3)), ("U_horizon", (4096, 150)),
                            ("dUdt_horizon", (4096, 150))):
            a = np.load(d / f"{name}.npy")
            assert a.shape == shape and a.dtype == np.float64 and np.isfinite(a).all()
            arrays[name] = a
        assert sorted(os.listdir(d)) == ["U_horizon.npy", "dUdt_horizon.npy", "u.npy", "x.npy"]
        runs.append(arrays)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
    # the closed loop has moved away from the seeded start (40 ticks of 1 ms)
    from cgmres_cpp_amd import scenarios
    x0, _, _ = scenarios.batch("pendulum", 4096)
    assert not np.array_equal(runs[0]["x"], x0)
