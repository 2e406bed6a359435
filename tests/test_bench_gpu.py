"""GPU: bench.py's contract at a small size -- a plain run prints the headline and nothing else, `--full` adds the
verified diagnostics, and `--dump-outputs` writes the last timed step's results, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, Q, B = 20000, 8, 8
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B), "--rows", str(ROWS), "--queries", str(Q)]


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_bench_plain_full_and_dumped_outputs(device, tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(B / (plain["ms_per_step"] * 1e-3), rel=1e-3)
    assert "verify" not in plain and "roofline" not in plain and "one_step_in_flight" not in plain

    a = _load(tmp_path / "plain")
    assert set(a) == {"features", "topk_scores", "topk_ids"}
    feats, scores, ids = a["features"], a["topk_scores"], a["topk_ids"]
    assert feats.dtype == np.float32 and feats.shape == (B, 512)
    assert np.allclose(np.linalg.norm(feats, axis=1), 1.0, atol=1e-2)          # the bench encodes with normalize=True
    assert scores.dtype == np.float32 and scores.shape == (Q, 10) and (np.diff(scores, axis=1) <= 0).all()
    assert ids.dtype == np.float64 and ids.shape == (Q, 10)
    assert (ids == np.round(ids)).all() and ids.min() >= 0 and ids.max() < ROWS

    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"))
    assert full["verify"].startswith("ok"), full["verify"]
    assert "roofline" in full and "one_step_in_flight" in full and full["steps"] == 3
    b = _load(tmp_path / "full")
    assert set(b) == set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                                     # same arguments -> same inputs -> same outputs
