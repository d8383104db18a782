"""A plain `bench.py` run (no --full) and `--dump-outputs DIR`: the line carries the headline fields and nothing that
needs extra runs, and the dump holds what the last timed step computed — the loss the line reports among it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--voxels", "40000", "--rotate", "0", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["unit"] == "scenes/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and "value_zorder" not in rec

    files = sorted(os.listdir(out_dir))
    assert {"loss.npy", "params_sample.npy", "grads_sample.npy", "loss_ce.npy", "loss_dice_11.npy"} <= set(files), files
    arrays = {f: np.load(out_dir / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    assert float(arrays["loss.npy"]) == rec["config"]["loss"]
    assert arrays["params_sample.npy"].shape == arrays["grads_sample.npy"].shape == (1 << 20,)
    assert np.abs(arrays["grads_sample.npy"]).max() > 0
