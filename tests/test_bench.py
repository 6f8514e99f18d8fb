"""bench.py as it is run for every change: a plain `--gpus 1 --steps K --warmup W` run times exactly K steps, carries the headline
fields and nothing of what `--full` adds, and `--dump-outputs` writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_plain_bench_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()          # the run below shares this device with the pytest process
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1
    assert r["unit"] == "sequences/sec" and r["higher_is_better"] is True and r["dtype"].startswith("f32")
    assert r["ms_per_step"] > 0 and abs(r["value"] - 16 / (r["ms_per_step"] * 1e-3)) <= 0.01 * r["value"]
    assert r["roofline"]["launches_timed"] >= 3 and r["roofline"]["launches_timed"] % 3 == 0 and r["roofline"]["achieved"] > 0
    for k in ("f32_mfma_path", "cfg5", "train_cfg3", "stress_dynamics", "trained_checkpoint", "accuracy_guard", "cpu_baseline", "parity_ok"):
        assert r[k] is None, k
    assert r["config"]["box"] is None
    files = sorted(os.listdir(tmp_path / "dump"))
    assert {"y.npy", "x.npy", "tnocs.npy"} <= set(files) and set(files) <= {"y.npy", "logp_y.npy", "x.npy", "tnocs.npy"}, files
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in files) <= 64 << 20
    x, y, tn = (np.load(tmp_path / "dump" / f) for f in ("x.npy", "y.npy", "tnocs.npy"))
    assert x.shape == y.shape == (16, 10, 2048, 3) and tn.shape[:3] == (16, 10, 2048)
    assert x.dtype == y.dtype == tn.dtype == np.float32
    assert np.isfinite(x).all() and np.isfinite(tn).all() and float(np.abs(x).max()) > 0
