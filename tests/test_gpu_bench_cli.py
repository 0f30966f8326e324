"""GPU: the bench's command line on the headline config -- a plain run prints the result line without the
measurements that take runs of their own (``roofline`` / ``cpu_baseline`` are null; ``--full`` adds them), ``--steps``
sets the number of timed steps, and ``--dump-outputs DIR`` writes what the last timed step left with its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_outputs(tmp_path):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                          "--dump-outputs", str(tmp_path / "o")], capture_output=True, text=True, timeout=120, env=e,
                         cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["roofline"] is None and d["cpu_baseline"] is None
    files = {f.name: f for f in (tmp_path / "o").iterdir()}
    assert all(n.endswith(".npy") for n in files)
    assert sum(f.stat().st_size for f in files.values()) <= 64 * 10 ** 6
    for n in ("loss.npy", "features.npy", "param.fc.weight.npy", "grad.fc.weight.npy"):
        assert n in files, sorted(files)
    for n, f in files.items():
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), n
    assert abs(float(np.load(files["loss.npy"])[0]) - d["loss_last_step"]) <= 1e-5
    assert float(np.abs(np.load(files["grad.fc.weight.npy"])).max()) > 0
    assert float(np.abs(np.load(files["features.npy"])).max()) > 0
