"""bench.py as a command on the device: a plain run measures the headline
and nothing else, times exactly --steps steps, and with --dump-outputs writes
the last timed step's outputs -- the same arrays from run to run, since the
inputs are seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, WARMUP = 1000, 7, 2  # a ragged batch (no multiple of the 64-lane workgroup), one short AQL plan


def _start(out_dir):
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                             "--warmup", str(WARMUP), "--batch", str(B), "--dump-outputs", str(out_dir)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(proc, out_dir):
    out, err = proc.communicate(timeout=200)
    assert proc.returncode == 0, err[-2000:]
    rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return rec, {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_plain_run_is_lean_and_its_dump_repeats(tmp_path):
    runs = [(_start(tmp_path / d), tmp_path / d) for d in "ab"]  # two processes side by side: start-up is most of a run
    try:
        (rec, a), (_, b) = [_finish(p, d) for p, d in runs]
    finally:
        for p, _ in runs:
            if p.poll() is None:
                p.kill()
                p.wait()
    # the contract's fields, the K timed steps, and none of the --full measurements
    assert rec["steps"] == STEPS and rec["warmup"] == WARMUP and rec["full"] is False
    assert rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["higher_is_better"] is True
    assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 / B - 1) < 0.01  # rounding of ms_per_step only
    assert rec["unit"] == "safe env steps/s" and rec["dtype"] == "f32 rows / f64 QP / f64 env"
    for k in ("cpu_baseline", "cpu_reference_mode", "extra"):
        assert k not in rec, k
    rf = rec["roofline"]
    assert "span" not in rf and "aql_dispatch_times" not in rf and rf["kernel_ms"] is None and rf["frac"] is None
    assert rf["frac_wall"] > 0
    # what safe_step returns (obs, reward, done, the outputs dict) and the env state it leaves
    assert sorted(a) == ["aux", "cost", "done", "obs", "reward", "state", "u"]
    assert {k: v.shape for k, v in a.items()} == {"aux": (B,), "cost": (B,), "done": (B,), "obs": (B, 10),
                                                  "reward": (B,), "state": (B, 10), "u": (B, 1)}
    for k in a:
        assert a[k].dtype == (np.float64 if k in ("state", "aux") else np.float32), k
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64e6
    # the arrays belong to one step: the observation is the one of the dumped state (parity tolerance of obs)
    want = O.cars_obs(a["state"]).astype(np.float32)
    assert np.max(np.abs(a["obs"] - want) / np.maximum(1, np.abs(want))) <= 1e-6
    assert set(np.unique(a["done"])) <= {0.0, 1.0}
