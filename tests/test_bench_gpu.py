"""bench.py's contract on one GPU at a tiny latent: a plain run prints the headline figures and nothing it does not need, ``--steps``
sets the number of timed steps, ``--dump-outputs`` writes the last timed step's UNet output (the same for the same arguments), and
``--full`` adds the measurements around the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "groups", "box", "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--latent", "16", "--frames", "4", *args],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_steps_and_dumped_outputs(tmp_path):
    for steps in (2, 3):
        rec = _bench("--steps", str(steps), "--dump-outputs", str(tmp_path / str(steps)))
        assert HEADLINE <= rec.keys() and not FULL_ONLY & rec.keys()
        assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["dtype"] == "bf16"
        assert rec["value"] == pytest.approx(1e3 / rec["ms_per_step"], rel=1e-9)
    y2, y3 = np.load(tmp_path / "2" / "sample.npy"), np.load(tmp_path / "3" / "sample.npy")
    assert y2.dtype == np.float32 and y2.shape == (8, 4, 4, 16, 16) and np.isfinite(y2).all()
    assert np.array_equal(y2, y3)            # seeded inputs and weights: every step computes the same output


@pytest.mark.gpu
def test_full_adds_the_measurements_around_the_headline():
    rec = _bench("--steps", "1", "--full", "--no-cpu-baseline")
    assert HEADLINE <= rec.keys() and {"roofline", "groups", "box"} <= rec.keys() and "cpu_baseline" not in rec
    assert rec["roofline"]["launches_per_step"] > 0 and rec["roofline"]["achieved"] > 0
    assert rec["box"]["gemm8192_tflops"] > 0 and sum(g["launches"] for g in rec["groups"].values()) > 0
