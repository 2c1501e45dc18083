"""bench.py's plain run on the GPU: one timed step, the headline line alone (the information legs are --full's), and
--dump-outputs writes what the timed step returned: the (FRAMES, 1, 9) id log of the one rank, as float32."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_headline_and_dumps_the_timed_ids(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 1 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "audio tokens/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert "roofline" not in res and "cpu_baseline" not in res and "decode_ms_per_frame" not in res     # --full only
    ids = np.load(tmp_path / "frame_ids.npy")
    assert ids.dtype == np.float32 and ids.shape == (1, 74, 1, 9)
    assert (ids[..., 1:] >= 0).all() and (ids == np.round(ids)).all()
