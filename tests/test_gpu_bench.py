"""`python bench.py --gpus 1 --steps K --warmup W` on the MI355X: a plain run prints the headline line alone, with
``ms_per_step`` of exactly K timed steps, and ``--dump-outputs DIR`` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "objects/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    B = d["config"]["objects_per_gpu"]
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - B) < 1e-2 * B  # value: objects per second of the timed steps
    for k in ("stage_ms", "value_serial", "roofline", "accuracy", "cpu_baseline", "scenes8", "training",
              "latency_batch1_ms"):
        assert k not in d, f"{k} belongs to --full"

    arrays = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert set(arrays) == {"refined_poses", "network_poses", "network_rot", "network_trans", "network_conf"}
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert arrays["refined_poses"].shape == arrays["network_poses"].shape == (B, 7)
    assert arrays["network_conf"].shape[0] == B
