"""GPU: bench.py as it is run for every change -- a plain run prints the headline only, --steps sets the timed steps, and
--dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(cuda, tmp_path):
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if not k.startswith("LIPASR_")}  # (A/B knobs of the caller's environment)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pool-clips", "8192",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["metric"] == "utterances/sec (train, 1 s@16 kHz)" and d["unit"] == "utterances/sec" and d["higher_is_better"] is True
    assert d["dtype"].startswith("f32") and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1024 * 1e3 / d["ms_per_step"], rel=1e-3)
    for key in ("roofline", "train_graph_ms", "cpu_baseline", "reference_batch_512", "reference_config_2_pre_extracted_f32"):
        assert key not in d, key  # --full only

    files = sorted(os.listdir(out_dir))
    assert "features.npy" in files and "loss_rows.npy" in files and "product_norms.npy" in files
    assert "block0_dense_kernel.npy" in files and "block0_bn_moving_variance.npy" in files
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20 and d["dumped_outputs"]["bytes"] == total
    assert np.load(out_dir / "features.npy").shape == (1024, 880)
    assert np.load(out_dir / "block0_dense_kernel.npy").shape == (880, 1024)
    assert np.load(out_dir / "loss_rows.npy").mean() == pytest.approx(d["loss"], abs=1e-4)
