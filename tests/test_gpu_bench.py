"""bench.py on one GPU at a small size: the plain run prints the headline line only and --dump-outputs writes the last timed
step's results; --full adds the roofline and CPU-baseline legs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--in-size", "128"]


def _bench(*extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *SMALL, *extra], capture_output=True, text=True, timeout=600,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_line_and_dump_outputs(dev, tmp_path):
    out = tmp_path / "outputs"
    rec = _bench("--dump-outputs", str(out))
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "images/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "bf16" and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    assert "roofline" not in rec and "cpu_baseline" not in rec
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert set(files) == {"loss.npy", "params_sample.npy", "grads_sample.npy"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["loss.npy"].shape == (1,) and files["loss.npy"][0] == np.float32(rec["final_loss"])
    assert files["params_sample.npy"].shape == files["grads_sample.npy"].shape
    assert np.abs(files["grads_sample.npy"]).max() > 0


def test_bench_full_adds_roofline_and_cpu_baseline(dev):
    rec = _bench("--full", "--cpu-images", "1", "--cpu-steps", "1")
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["roofline"]["peak"] > 0 and rec["roofline"]["event_timed_steps"] == 1
    assert rec["cpu_baseline"]["value"] > 0, rec["cpu_baseline"]
