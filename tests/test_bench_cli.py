"""bench.py's command line: `--dump-outputs` (the helper on the host, and a plain run on the
GPU) and what a plain run leaves to `--full`."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_files(tmp_path):
  import bench
  arrays = {"obs_policy": torch.arange(35, dtype=torch.float64).reshape(7, 5),
            "terminated": torch.tensor([True, False, False, True, False, False, True]),
            "reward": torch.linspace(-1.0, 1.0, 7)}
  bench.dump_outputs(str(tmp_path), arrays)
  assert sorted(os.listdir(tmp_path)) == ["obs_policy.npy", "reward.npy", "terminated.npy"]
  for k, v in arrays.items():
    a = np.load(tmp_path / f"{k}.npy")
    assert a.dtype == np.float32 and a.shape == tuple(v.shape)
    np.testing.assert_array_equal(a, v.to(torch.float32).numpy())
  bench.dump_outputs(str(tmp_path), {"reward": arrays["reward"]}, rank=3)
  assert (tmp_path / "reward_rank3.npy").exists()


def test_dump_outputs_sample_is_capped_and_fixed(tmp_path, monkeypatch):
  """Past the byte cap every array keeps the same seeded, ordered sample of its worlds."""
  import bench
  n = 64
  obs = torch.arange(n * 6, dtype=torch.float32).reshape(n, 6)
  rew = torch.arange(n, dtype=torch.float32)
  monkeypatch.setattr(bench, "DUMP_BYTES_MAX", (obs.numel() + rew.numel()) * 4 // 4)
  bench.dump_outputs(str(tmp_path / "a"), {"obs": obs, "reward": rew})
  bench.dump_outputs(str(tmp_path / "b"), {"obs": obs, "reward": rew})
  a_obs, a_rew = np.load(tmp_path / "a" / "obs.npy"), np.load(tmp_path / "a" / "reward.npy")
  assert a_obs.nbytes + a_rew.nbytes <= bench.DUMP_BYTES_MAX
  assert a_obs.shape == (n // 4, 6) and a_rew.shape == (n // 4,)
  rows = a_rew.astype(np.int64)  # reward[i] == i: the sampled worlds
  assert np.all(np.diff(rows) > 0)
  np.testing.assert_array_equal(a_obs, obs.numpy()[rows])
  np.testing.assert_array_equal(a_obs, np.load(tmp_path / "b" / "obs.npy"))
  np.testing.assert_array_equal(a_rew, np.load(tmp_path / "b" / "reward.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step_and_leaves_full_legs_out(gpu_device, tmp_path):
  """A plain run: `steps` and `ms_per_step` in the line, the legs of `--full` null, and the
  last timed step's env.step outputs as float32 .npy files, one row per world."""
  n = 64
  r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                      "--warmup", "2", "--num-envs", str(n), "--dump-outputs", str(tmp_path / "out")],
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
  assert len(lines) == 1
  d = json.loads(lines[0])
  assert d["steps"] == 3 and d["warmup"] == 2
  assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
  assert d["ms_per_step"] > 0.0
  assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-6)
  assert d["cpu_baseline"] is None and d["roofline"]["single_launch_ms"] is None
  names = sorted(os.listdir(tmp_path / "out"))
  assert {"reward.npy", "terminated.npy", "truncated.npy"} <= set(names)
  assert any(nm.startswith("obs_") for nm in names)
  for nm in names:
    a = np.load(tmp_path / "out" / nm)
    assert a.dtype == np.float32 and a.shape[0] == n and np.isfinite(a).all(), nm
