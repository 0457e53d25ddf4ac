"""-m gpu: bench.py's plain run — the headline line alone; what else the benchmark measures waits for --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "precision", "roofline_fp16", "crops_16bit", "c3_shard_proxy", "small_batch", "knn_roofline", "c1", "c4", "c5",
             "weak", "strong", "extras_error")


def test_plain_bench_run_is_the_headline_alone(tmp_path):
    """``bench.py --gpus 1 --steps K --warmup W`` in a fresh process: one JSON line with the headline keys and the in-region roofline,
    none of the --full objects, and the last timed step's scores and ids of all 1024 crops under --dump-outputs."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[-4000:]
    line = json.loads(lines[0])
    assert line["metric"] == "glyph-crops/sec end-to-end (encode+kNN), 224x224 bs=1024" and line["unit"] == "glyph-crops/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and (line["steps"], line["warmup"]) == (2, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"], rel=1e-3)
    assert line["roofline"]["launches"] > 0
    assert [k for k in FULL_ONLY if k in line] == []
    scores, ids = np.load(tmp_path / "knn_scores.npy"), np.load(tmp_path / "knn_ids.npy")
    assert scores.shape == ids.shape == (1024, 10) and scores.dtype == np.float32 and ids.dtype == np.float64
    assert ((ids >= 0) & (ids < 10000)).all() and (np.diff(scores, axis=1) <= 0).all()
