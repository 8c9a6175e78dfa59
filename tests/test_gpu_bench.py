"""bench.py as every change runs it: a plain `--gpus 1 --steps K --warmup W` run times exactly K steps and prints the
headline line only, and `--dump-outputs` writes the same arrays from run to run (the time-based priming runs on a
throwaway instance, so how many steps it fits into its seconds leaves no trace in the measured one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out, priming_seconds, steps=7, warmup=2, priming=3, batch=32):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--priming", str(priming), "--priming-seconds", str(priming_seconds), "--batch", str(batch),
           "--dump-outputs", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["unit"] == "windows/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - batch * steps / (d["ms_per_step"] * steps * 1e-3)) / d["value"] < 1e-3
    for key in ("step_ms", "roofline", "frac_by_block", "instrumented_ms_per_step", "also", "ref_batch_sizes",
                "cpu_baseline", "detail"):
        assert key not in d, key
    return d, {p.name[:-len(".npy")]: np.load(p) for p in sorted(out.iterdir())}


def test_plain_run_times_the_given_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    d0, a = _plain_run(tmp_path / "a", priming_seconds=0.2)
    _, b = _plain_run(tmp_path / "b", priming_seconds=0.8)
    assert set(a) == set(b) and "loss" in a
    assert any(k.startswith("grad.") for k in a) and any(k.startswith("state.") for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        if k.endswith("num_batches_tracked"):
            assert float(a[k]) == 3 + 2 + 7, k             # priming + warm-up + timed steps of the measured instance
    assert abs(float(a["loss"]) - d0["config"]["final_loss"]) <= 5e-7     # the line rounds it to 6 decimals
    for k in a:
        assert np.array_equal(a[k], b[k]), k
