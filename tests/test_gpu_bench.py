"""bench.py's plain line on the GPU: the headline keys only, `--steps` timed steps, and `--dump-outputs` writing what the last timed
step computed -- the same arrays on two runs with the same arguments, and the arrays the line's own output digest was taken of."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_are_reproducible(tmp_path):
    runs = []
    for tag in ("a", "b"):
        d = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--output-digest", "--dump-outputs", str(tmp_path / tag))
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 10 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
        for k in ("roofline", "other_mode", "parity", "power", "sustained", "box_calibration", "cpu_baseline"):
            assert k not in d, k                                    # --full only
        assert d["dump_outputs"]["file"] == "output.npy" and d["dump_outputs"]["stride"] == 1
        y = np.load(tmp_path / tag / "output.npy")
        assert y.dtype == np.float32 and y.shape == (10, 3, 540, 960) and np.isfinite(y).all()
        assert [hashlib.sha256(y.tobytes()).hexdigest()[:16]] == d["output_digest"]["sha256_16_per_10_frame_block"]
        runs.append(y)
    assert np.array_equal(runs[0], runs[1])
