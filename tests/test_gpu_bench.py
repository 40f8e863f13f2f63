"""bench.py's plain run (the headline forward alone) and --dump-outputs: the result line says what one timed step took, the extra
measurements stay behind --full, and the dumped predictions do not depend on the number of steps -- inputs and weights are seeded,
so two runs with the same arguments compare output for output.  Each run is its own process, as the benchmark is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(out, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{cmd}\n--- stderr\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_line_and_dumped_predictions(tmp_path):
    a = _bench(tmp_path / "a", 2, 1)
    b = _bench(tmp_path / "b", 3, 0)
    for d, steps in ((a, 2), (b, 3)):
        assert d["steps"] == steps and d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 64) < 0.1          # 64 images per timed step
        for k in ("sustained", "roofline", "train", "nms", "preprocess", "small_batches", "resnet50_variant", "cpu_baseline"):
            assert d[k] is None, k
    pa, pb = np.load(tmp_path / "a" / "predictions.npy"), np.load(tmp_path / "b" / "predictions.npy")
    assert pa.dtype == np.float32 and pa.shape == (64, 7, 7, 30) and np.isfinite(pa).all()
    assert np.array_equal(pa, pb)
