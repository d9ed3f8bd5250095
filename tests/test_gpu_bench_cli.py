"""bench.py's command line on the GPU, at a small batch: a plain run prints the headline line
only and --dump-outputs writes the last timed step's arrays; --full adds the roofline blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_bwd", "mfma", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8",
                        "--steps", "2", "--warmup", "1", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_outputs(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["dtype"] == "bf16"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(8 * 1000 / d["ms_per_step"], rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["logits.npy", "loss.npy", "params_sample.npy"]
    arrays = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert arrays["logits"].shape == (8, 10000) and arrays["loss"].shape == (1,)
    assert arrays["loss"][0] == pytest.approx(d["final_loss"], abs=1e-4)


def test_full_run_adds_the_rooflines():
    d = _bench("--full", "--cpu-baseline", "0")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    for k in ("roofline", "roofline_bwd", "mfma"):
        assert d[k]["frac"] > 0, k
    assert "cpu_baseline" not in d
