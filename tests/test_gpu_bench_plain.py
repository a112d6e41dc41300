"""-m gpu: bench.py's plain line and --dump-outputs.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) times exactly K steps and prints the headline figures only; --full adds the
rest.  --dump-outputs writes the frames of the last timed step, and two runs with the same arguments write the same arrays (the
clock ramp runs on a second decoder, so the measured one always sees exactly W + K submits)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--channels", "256", "--tiles", "24", "--steps", "6", "--warmup", "2", "--ramp-ms", "20"]
FIELDS = ("channel", "type", "len", "nerr", "flags", "bitpos", "data")


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f"frames_{f}.npy")) for f in FIELDS}


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_repeat(tmp_path):
    a, b, c = (str(tmp_path / x) for x in "abc")
    ja = _bench("--dump-outputs", a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in ja, k
    assert ja["steps"] == 6 and ja["warmup"] == 2 and ja["higher_is_better"] is True and ja["unit"] == "Msamples/s"
    assert abs(ja["value"] - 256 * 24 * 2048 / (ja["ms_per_step"] * 1e-3) / 1e6) < 0.01 * ja["value"]
    assert "roofline" not in ja and "cpu_baseline" not in ja and "other_configs" not in ja
    jb = _bench("--dump-outputs", b)
    jc = _bench("--full", "--no-cpu", "--no-others", "--dump-outputs", c)
    assert "roofline" in jc and "kernel_ms" in jc and jc["frames_per_step_steady"] > 0
    fa, fb, fc = _load(a), _load(b), _load(c)
    n = len(fa["channel"])
    assert n == ja["outputs_dumped"]["frames"] == ja["outputs_dumped"]["of"]
    assert n >= 0.9 * 256                                         # 4915 symbols per channel and step, a frame every 3072
    assert fa["data"].dtype == np.float32 and fa["bitpos"].dtype == np.float64 and fa["data"].shape == (n, 528)
    for f in FIELDS:
        assert np.array_equal(fa[f], fb[f]), f                  # same arguments: the same outputs
        assert np.array_equal(fa[f], fc[f]), f                  # --full measures the same path
    assert np.all(np.diff(fa["channel"]) >= 0)
