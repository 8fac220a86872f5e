"""The adaptive failure-bin sampler of the fused tracking step (k_bins and the inverse-CDF draw
of k_rsi, csrc/tracking_task.hip) against the fp64 restatement of commands.py:258-307.

300 envs (more than one 256-thread stride of the env loop, not a multiple of it), three bin
counts: the shipped synthetic motion's (11, kernel size 1), 2 (its first 60 frames) and 265
(past one 256-thread stride of the bin loops), the latter two with a 3-tap smoothing kernel
so that the replicate padding at the last bin matters.  The long motion is the shipped one
tiled (tracking.ensure_synthetic_motion's arrays repeated to 3,310 frames; the sampler reads
only the frame count).  The bin count is T // (1 / step_dt) + 1, and the 265-bin env runs at
decimation 16 (step_dt 0.08 s; no physics step runs here) so that 3,310 frames suffice where
the shipped 0.02 s would need 12,800.

Deterministic part: bin_failed_count, the terminated flags and the time steps are injected,
mjx_track_reset and four mjx_track_observe run with no physics step in between, and after
each the failure counts, the CDF, the three sampling metrics on every env and the EMA are
compared at rtol 1e-5.  Observes 2 and 4 have no resampling env: the reference computes the
sampling metrics inside _resample_command only, so they must keep their values while the EMA
moves bin_failed_count (the kernel used to recompute them on every observe).

Distribution part: every env resets 32 times (the step counter of the counter-based hash is
advanced in between), 9,600 draws.  The histogram of the time steps, grouped by floor(t /
((T - 1) / nbin)), matches the exact group probabilities of ((bin + U) / nbin * (T - 1)).long()
within 5 sigma + 1 (the convention of test_gpu_fused_random.py), and the frame offset inside
the most likely bin is uniform (_uniform_ok of that file).  The same for "uniform" mode."""

import numpy as np
import pytest

import fused_inject as fi
from test_gpu_fused_random import _uniform_ok

pytestmark = pytest.mark.gpu

N = 300
ROUNDS = 32
# name -> (motion frames, smoothing kernel size, decimation); bin count = T // (1 / step_dt) + 1
CASES = {"shipped": (None, None, None), "two_bins": (60, 3, None), "many_bins": (3310, 3, 16)}
BINS = {"two_bins": 2, "many_bins": 265}
RTOL = 1e-5


@pytest.fixture(scope="module", params=list(CASES))
def sampler(request, gpu_device, tmp_path_factory):
  frames, ksize, decimation = CASES[request.param]
  path = None
  if frames is not None:  # the shipped synthetic motion cut or tiled to `frames` frames
    from mjlab_amd.tracking import ensure_synthetic_motion, write_motion_npz
    with np.load(ensure_synthetic_motion(device=gpu_device)) as d:
      base = {k: d[k] for k in d.files}
    reps = -(-frames // len(base["joint_pos"]))
    motion = {k: v if k == "fps" else np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:frames] for k, v in base.items()}
    path = str(tmp_path_factory.mktemp("motion") / f"g1_{frames}.npz")
    write_motion_npz(path, motion)
  env = fi.build_env("tracking", gpu_device, n=N, motion_file=path, sampling_mode="adaptive",
                     kernel_size=ksize, alpha=0.25, decimation=decimation)
  D = fi.live_desc(env)
  want_bins = BINS.get(request.param, fi.golden_desc("tracking")["bin_count"])
  assert D["bin_count"] == want_bins and D["sampling_mode"] == 2
  yield env, D
  del env


def _close(name, got, want, atol=0.0):
  np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=RTOL, atol=atol, err_msg=name)


def _compare(env, D, ref, stage, cdf=True):
  tens = fi.track_tensors(env)
  got = fi.fetch(tens, ["bin_failed_count", "current_bin_failed", "sampling", "metrics"])
  nbin = D["bin_count"]
  assert np.array_equal(got["current_bin_failed"], ref.cbf), f"{stage}: _current_bin_failed"
  _close(f"{stage}: bin_failed_count", got["bin_failed_count"], ref.bfc)
  if cdf:
    _close(f"{stage}: cdf", got["sampling"][:nbin], ref.cdf)
  for m, name in enumerate(("sampling_entropy", "sampling_top1_prob", "sampling_top1_bin")):
    _close(f"{stage}: {name}", got["metrics"][:, 10 + m], np.full(N, ref.metrics[m]))


def _failed_counts(nbin, seed):
  """A known non-uniform bin_failed_count, exact in fp32, with a single largest bin that is
  neither the first nor the last where there are more than two bins."""
  if nbin == 2:
    return np.array([1.75, 0.5], dtype=np.float32)
  rng = np.random.default_rng(seed)
  b = rng.integers(0, 8, nbin) * 0.25
  b[min(nbin - 1, max(1, nbin // 3))] = 4.0
  b[-1] = 1.5 if nbin > 2 else 0.5
  return b.astype(np.float32)


def test_sampler_state_against_reference(sampler):
  env, D = sampler
  nbin, Tn = D["bin_count"], D["nframe"]
  tens = fi.track_tensors(env)
  rng = np.random.default_rng(11)
  ref = fi.SamplerRef(D, _failed_counts(nbin, 1))
  p = fi.T.sampling_probabilities(ref.bfc, ref.ratio, ref.kernel)
  top2 = np.sort(p)[-2:]
  assert top2[1] - top2[0] > 1e-3 * top2[1], "the reference's most likely bin must be unique"
  # ---- reset: every 3rd env resets, every other of those failed, at chosen time steps
  ts = rng.integers(0, Tn - 2, N)
  reset = np.zeros(N, dtype=bool)
  reset[::3] = True
  failed = np.zeros(N, dtype=bool)
  failed[::6] = True
  chosen = [0, Tn // 2, Tn - 1, Tn, Tn]       # Tn: at the motion end, its bin index clamps
  ts[np.nonzero(failed)[0][:len(chosen)]] = chosen
  terminated = failed.copy()
  terminated[1::30] = True                    # terminated envs outside the mask do not count
  fi.inject(tens, {"bin_failed_count": ref.bfc.astype(np.float32), "current_bin_failed": np.zeros(nbin, np.float32),
                   "time_steps": ts, "reset_buf": reset, "terminated": terminated})
  ref.resample(ts, reset, terminated)
  assert ref.cbf.sum() == failed.sum() and ref.cbf[-1] >= 2
  fi.call(env, "mjx_track_reset")
  _compare(env, D, ref, "reset")
  new = fi.fetch(tens, ["time_steps"])["time_steps"]
  assert np.array_equal(new[~reset], ts[~reset])
  assert new[reset].min() >= 0 and new[reset].max() <= Tn - 1
  # ---- four observes, no reset in between; 1, 2 and 4 with no env at the motion end
  quiet = rng.integers(0, Tn - 3, N)
  for k in (1, 2, 3, 4):
    ts = quiet.copy()
    if k == 3:                                # five envs at the motion end, two of them failed
      ts[[3, 9, 100, 257, 299]] = Tn - 1
      terminated = np.zeros(N, dtype=bool)
      terminated[[9, 257, 40]] = True         # env 40 failed but does not resample
    fi.inject(tens, {"time_steps": ts, "terminated": terminated})
    before = ref.metrics.copy()
    ts1, mask = ref.update_command(ts, terminated)
    fi.call(env, "mjx_track_observe")
    _compare(env, D, ref, f"observe {k}", cdf=(k == 3))
    got = fi.fetch(tens, ["time_steps", "resample_mask"])
    assert np.array_equal(got["resample_mask"].astype(bool), mask)
    assert np.array_equal(got["time_steps"][~mask], ts1[~mask])
    if k == 3:
      assert mask.sum() == 5 and ref.cbf.sum() == 0 and not np.allclose(before, ref.metrics, rtol=1e-3)
      assert got["time_steps"][mask].max() <= Tn - 1
    else:
      assert not mask.any() and np.array_equal(before, ref.metrics)


def _draw(env, tens, rounds=ROUNDS):
  """`rounds` resets of every env; the hash's step counter advances as k_action would."""
  fz = env._fused
  out = []
  for _ in range(rounds):
    fz.step_counter += 1
    fi.inject(tens, {"reset_buf": np.ones(N, dtype=bool), "terminated": np.zeros(N, dtype=bool)})
    fi.call(env, "mjx_track_reset")
    out.append(fi.fetch(tens, ["time_steps"])["time_steps"].copy())
  return np.concatenate(out)


def _histogram_ok(counts, prob, what):
  n = counts.sum()
  tol = 5.0 * np.sqrt(n * prob * (1.0 - prob)) + 1.0
  bad = np.nonzero(np.abs(counts - n * prob) > tol)[0]
  assert not len(bad), f"{what}: groups {bad[:8]}: counts {counts[bad][:8]} vs {n * prob[bad][:8]}"


def test_adaptive_start_frames_follow_the_failure_bins(sampler):
  env, D = sampler
  nbin, Tn = D["bin_count"], D["nframe"]
  tens = fi.track_tensors(env)
  bfc = np.zeros(nbin, dtype=np.float32)      # peaked on two bins
  a, b = (1, nbin - 2) if nbin > 3 else (nbin - 1, 0)
  bfc[a], bfc[b] = 5.0, 3.0
  fi.inject(tens, {"bin_failed_count": bfc, "current_bin_failed": np.zeros(nbin, np.float32)})
  ref = fi.SamplerRef(D, bfc)
  ref.resample(np.zeros(N, dtype=np.int64), np.ones(N, dtype=bool), np.zeros(N, dtype=bool))
  ts = _draw(env, tens)
  assert ts.min() >= 0 and ts.max() <= Tn - 1
  L = (Tn - 1) / nbin
  group = np.minimum((np.arange(Tn) / L).astype(np.int64), nbin - 1)
  pf = fi.frame_probabilities(ref.p, Tn)
  prob = np.bincount(group, weights=pf, minlength=nbin)
  assert abs(prob.sum() - 1.0) < 1e-12 and prob.max() > 0.2
  _histogram_ok(np.bincount(group[ts], minlength=nbin).astype(np.float64), prob, "adaptive")
  # frame offset inside the most likely bin: uniform over the frames only that bin reaches
  top = int(np.argmax(ref.p))
  lo, hi = int(np.ceil(top * L)), int(np.floor((top + 1) * L)) - 1
  inside = ts[(ts >= lo) & (ts <= hi)]
  assert len(inside) > 2000
  _uniform_ok((inside - lo + 0.5) / (hi - lo + 1), 0.0, 1.0, "frame offset in the most likely bin")


def test_uniform_start_frames(sampler):
  env, D = sampler
  nbin, Tn = D["bin_count"], D["nframe"]
  fz, tens = env._fused, fi.track_tensors(env)
  fz._desc.sampling_mode = 1                  # the kernels' mode; the descriptor is re-uploaded
  fz.upload()
  try:
    ts = _draw(env, tens)
    metrics = fi.fetch(tens, ["metrics"])["metrics"]
  finally:
    fz._desc.sampling_mode = 2
    fz.upload()
  assert ts.min() >= 0 and ts.max() <= Tn - 1
  group = (np.arange(Tn) * nbin) // Tn
  prob = np.bincount(group, minlength=nbin) / Tn
  _histogram_ok(np.bincount(group[ts], minlength=nbin).astype(np.float64), prob, "uniform")
  _uniform_ok((ts + 0.5) / Tn, 0.0, 1.0, "uniform start frame")
  np.testing.assert_allclose(metrics[:, 10:13], np.tile([1.0, 1.0 / nbin, 0.5], (N, 1)), rtol=1e-6)
