"""`bench.py --dump-outputs DIR`: what the timed path handed its caller after its last step, as DIR/<name>.npy, so that two builds can be
compared output for output; a plain run times its steps only, `--full` adds the figures and checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(n):
    info = torch.randint(0, 5, (n, 17), dtype=torch.int32)
    info[:, 8] = torch.from_numpy(np.full(n, 1.5, np.float32).view(np.int32))
    info[:, 14] = torch.from_numpy(np.full(n, -2.25, np.float32).view(np.int32))
    return bench.host_outputs(torch.randn(n, 64).bfloat16(), torch.randn(n), (torch.rand(n) > 0.5).to(torch.uint8), info)


def test_host_outputs_are_exact_float_arrays():
    o = _outputs(8)
    assert {k: v.dtype for k, v in o.items()} == {"obs": np.float32, "reward": np.float32, "done": np.float32, "info": np.float64}
    assert set(np.unique(o["done"])) <= {0.0, 1.0}
    assert (o["info"][:, 8] == 1.5).all() and (o["info"][:, 14] == -2.25).all()  # float-bit columns decoded
    assert (o["info"][:, :8] == np.round(o["info"][:, :8])).all()


def test_dump_outputs_keeps_the_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    o = _outputs(4096)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), o)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["done.npy", "env_rows.npy", "info.npy", "obs.npy", "reward.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    rows = np.load(tmp_path / "a" / "env_rows.npy").astype(int)
    assert (rows == np.load(tmp_path / "b" / "env_rows.npy")).all()
    assert (np.load(tmp_path / "a" / "obs.npy") == o["obs"][rows]).all()


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--envs-per-gpu", "64"] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0
    assert "roofline" not in plain and "cpu_baseline" not in plain
    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["kernel_launches"] > 0 and full["config"]["obs_finite"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == ["done.npy", "info.npy", "obs.npy", "reward.npy"] and sorted(os.listdir(tmp_path / "full")) == names
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype in (np.float32, np.float64) and len(a) == 64 and np.isfinite(a).all()
        assert (a == b).all(), f  # the same seeded inputs and the same 5 steps
