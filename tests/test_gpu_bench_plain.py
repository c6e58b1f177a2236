"""bench.py's plain command (no --full) on the GPU box: the headline steps only, one line whose `ms_per_step` is the time of
one timed step, and --dump-outputs writes what the last timed step computed - held here to the oracle on the same seeded
frames and weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    from ocr_rs_amd import weights as W
    from oracle import torch_ref as T
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--size", "128", "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32"
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / 2 - 1.0) < 0.01      # frames per step / seconds per step
    assert line["roofline"] is None and not {"summary", "cpu_baseline", "bf16", "f32_mfma_only", "postprocess_images_per_s"} & set(line)
    assert line["outputs"]["prob"] == {"shape": [2, 1, 128, 128], "frames": "all"}
    prob, bitmap = np.load(out / "prob.npy"), np.load(out / "bitmap.npy")
    assert prob.dtype == bitmap.dtype == np.float32 and prob.shape == bitmap.shape == (2, 1, 128, 128)
    x = W.synth_image_batch(1, 2, 128, 128)   # the frames and weights bench.py seeds on rank 0
    ref = T.det_forward(W.make_det_weights(0), x)
    assert float(np.abs(prob - ref).max()) < 1e-4
    assert np.array_equal(bitmap, (prob > np.float32(0.6)).astype(np.float32))
