"""ObservationManager history / delay (mjlab_amd/managers.py) on a mock env, CPU only.

Known answers restated from the reference's cases (tests/test_observation_history.py,
tests/test_observation_delay.py: inputs and expected values only), and a numpy restatement
of compute_group (observation_manager.py:169-208, with the ring + pointer buffers of
utils/buffers/circular_buffer.py) that the torch manager must equal bit for bit."""

import numpy as np
import pytest
import torch

from mjlab_amd.managers import ObservationGroupCfg, ObservationManager, ObservationTermCfg

N = 4


class MockEnv:
  def __init__(self, num_envs=N):
    self.num_envs = num_envs
    self.device = "cpu"
    self.scene = None


class Counter:
  """Observation function: every call returns the next integer in all `width` columns
  (times `gain`).  The manager calls it once while it measures the term dims, so the first
  computed observation is 2."""

  def __init__(self, width=3, gain=1.0):
    self.k, self.width, self.gain = 0, width, gain

  def __call__(self, env):
    self.k += 1
    return torch.full((env.num_envs, self.width), self.k * self.gain)


def _manager(terms, env=None, **group):
  cfg = {"policy": ObservationGroupCfg(terms=terms, **group)}
  return ObservationManager(cfg, env or MockEnv())


def _row(obs):
  return obs["policy"][0].tolist()


def test_default_has_no_history_or_delay():
  m = _manager({"a": ObservationTermCfg(func=Counter())})
  assert m.group_obs_dim["policy"] == (3,)
  assert m.compute()["policy"].shape == (N, 3)
  assert not m.has_buffers
  c = ObservationTermCfg(func=None)
  assert (c.delay_per_env, c.delay_hold_prob, c.delay_update_period, c.delay_per_env_phase) == \
      (True, 0.0, 0, True)


def test_term_history_flattened_backfill_then_shift():
  m = _manager({"a": ObservationTermCfg(func=Counter(width=2), history_length=3)})
  assert m.group_obs_dim["policy"] == (6,)
  assert m.group_obs_term_dim["policy"] == [(6,)]
  assert _row(m.compute(update_history=True)) == [2., 2., 2., 2., 2., 2.]
  assert _row(m.compute(update_history=True)) == [2., 2., 2., 2., 3., 3.]
  assert _row(m.compute(update_history=True)) == [2., 2., 3., 3., 4., 4.]
  assert _row(m.compute(update_history=True)) == [3., 3., 4., 4., 5., 5.]


def test_unflattened_history_shape():
  m = _manager({"a": ObservationTermCfg(func=Counter(), history_length=2, flatten_history_dim=False)})
  assert m.group_obs_dim["policy"] == (2, 3)
  o = m.compute(update_history=True)["policy"]
  assert o.shape == (N, 2, 3)
  o2 = m.compute(update_history=True)["policy"]
  assert o2[0, :, 0].tolist() == [2., 3.]
  assert o[0, :, 0].tolist() == [2., 2.]  # an earlier result is not rewritten by the shift


def test_group_history_overrides_terms():
  terms = {"a": ObservationTermCfg(func=Counter(width=2), history_length=5),
           "b": ObservationTermCfg(func=Counter(width=1), history_length=0,
                                   flatten_history_dim=False)}
  m = _manager(terms, history_length=2, flatten_history_dim=True)
  assert m.group_obs_term_dim["policy"] == [(4,), (2,)]
  assert m.group_obs_dim["policy"] == (6,)
  for c in m._group_obs_term_cfgs["policy"]:
    assert c.history_length == 2 and c.flatten_history_dim
  m.compute(update_history=True)
  assert _row(m.compute(update_history=True)) == [2., 2., 3., 3., 2., 3.]


def test_group_history_none_keeps_term_settings():
  terms = {"a": ObservationTermCfg(func=Counter(width=1), history_length=3)}
  m = _manager(terms)  # history_length=None
  assert m.group_obs_dim["policy"] == (3,)


def test_mixed_group_is_term_major():
  terms = {"h": ObservationTermCfg(func=Counter(width=2), history_length=3),
           "p": ObservationTermCfg(func=Counter(width=1, gain=10.0))}
  m = _manager(terms)
  assert m.group_obs_dim["policy"] == (7,)
  m.compute(update_history=True)
  m.compute(update_history=True)
  # term h: frames 2, 3, 4 of width 2, oldest first; then term p's current value
  assert _row(m.compute(update_history=True)) == [2., 2., 3., 3., 4., 4., 40.]


def test_update_history_false_returns_cache_and_does_not_push():
  f = Counter(width=1)
  m = _manager({"a": ObservationTermCfg(func=f, history_length=2, delay_min_lag=1, delay_max_lag=1)})
  o1 = m.compute(update_history=True)
  hist = m._group_obs_term_history_buffer["policy"]["a"]
  delay = m._group_obs_term_delay_buffer["policy"]["a"]
  assert hist.current_length.tolist() == [1] * N and delay._buffer.current_length.tolist() == [1] * N
  calls = f.k
  for _ in range(3):
    assert m.compute() is o1
  assert f.k == calls
  assert hist.current_length.tolist() == [1] * N and delay._buffer.current_length.tolist() == [1] * N
  m.compute(update_history=True)
  assert hist.current_length.tolist() == [2] * N and delay._buffer.current_length.tolist() == [2] * N


def test_uninitialised_history_is_pushed_even_without_update():
  m = _manager({"a": ObservationTermCfg(func=Counter(width=1), history_length=2)})
  assert _row(m.compute(update_history=False)) == [2., 2.]
  # compute_group without update on an initialised buffer reads it without pushing
  assert m.compute_group("policy", update_history=False)[0].tolist() == [2., 2.]


def test_cache_dropped_and_rows_backfilled_on_reset():
  m = _manager({"a": ObservationTermCfg(func=Counter(width=1), history_length=3)})
  for _ in range(3):
    o = m.compute(update_history=True)
  assert _row(o) == [2., 3., 4.]
  m.reset(env_ids=torch.tensor([1, 3]))
  assert m._obs_buffer is None
  hist = m._group_obs_term_history_buffer["policy"]["a"]
  assert hist.current_length.tolist() == [3, 0, 3, 0]
  # no cache, so recomputed; an initialised buffer is only pushed with update_history, so
  # the reset rows read zeros until then
  o = m.compute()["policy"]
  assert o.tolist()[1] == [0., 0., 0.] and o.tolist()[0] == [2., 3., 4.]
  o = m.compute(update_history=True)["policy"]
  assert o.tolist()[0] == [3., 4., 6.] and o.tolist()[1] == [6., 6., 6.]
  m.reset()  # all envs
  assert hist.current_length.tolist() == [0] * N


def test_constant_delay_two():
  m = _manager({"a": ObservationTermCfg(func=Counter(), delay_min_lag=2, delay_max_lag=2)})
  assert m.group_obs_dim["policy"] == (3,)
  got = [_row(m.compute(update_history=True))[0] for _ in range(5)]
  assert got == [2., 2., 2., 3., 4.]  # o0 o0 o0 o1 o2


def test_lag_one_delay():
  m = _manager({"a": ObservationTermCfg(func=Counter(), delay_min_lag=1, delay_max_lag=1)})
  got = [_row(m.compute(update_history=True))[0] for _ in range(5)]
  assert got == [2., 2., 3., 4., 5.]


def test_delay_feeds_history():
  m = _manager({"a": ObservationTermCfg(func=Counter(), delay_min_lag=1, delay_max_lag=1,
                                        history_length=2, flatten_history_dim=False)})
  assert m.group_obs_dim["policy"] == (2, 3)
  got = [m.compute(update_history=True)["policy"][0, :, 0].tolist() for _ in range(3)]
  # delayed stream 2, 2, 3 -> history [2 2], [2 2], [2 3]
  assert got == [[2., 2.], [2., 2.], [2., 3.]]


def test_delay_after_scale():
  m = _manager({"a": ObservationTermCfg(func=Counter(), scale=2.0, delay_min_lag=1, delay_max_lag=1)})
  got = [_row(m.compute(update_history=True))[0] for _ in range(3)]
  assert got == [4., 4., 6.]


def test_mixed_delay_and_plain_terms():
  terms = {"d": ObservationTermCfg(func=Counter(width=3), delay_min_lag=1, delay_max_lag=1),
           "p": ObservationTermCfg(func=Counter(width=2, gain=10.0))}
  m = _manager(terms)
  assert m.group_obs_dim["policy"] == (5,)
  rows = [_row(m.compute(update_history=True)) for _ in range(3)]
  assert [r[0] for r in rows] == [2., 2., 3.] and [r[3] for r in rows] == [20., 30., 40.]


def test_delay_policy_fields_reach_the_buffer():
  c = ObservationTermCfg(func=Counter(), delay_min_lag=1, delay_max_lag=4, delay_per_env=False,
                         delay_hold_prob=0.25, delay_update_period=5, delay_per_env_phase=False)
  m = _manager({"a": c})
  d = m._group_obs_term_delay_buffer["policy"]["a"]
  assert (d.min_lag, d.max_lag, d.per_env, d.hold_prob, d.update_period, d.per_env_phase) == \
      (1, 4, False, 0.25, 5, False)
  # shared lag through the manager (no hold: a hold is decided per env)
  m = _manager({"a": ObservationTermCfg(func=Counter(), delay_min_lag=1, delay_max_lag=4,
                                        delay_per_env=False)})
  d = m._group_obs_term_delay_buffer["policy"]["a"]
  for _ in range(7):
    m.compute(update_history=True)
    assert torch.all(d.current_lags == d.current_lags[0])  # shared lag


def test_delay_update_period_in_the_manager():
  torch.manual_seed(0)
  c = ObservationTermCfg(func=Counter(), delay_min_lag=0, delay_max_lag=7,
                         delay_update_period=3, delay_per_env_phase=False)
  m = _manager({"a": c}, env=MockEnv(16))
  d = m._group_obs_term_delay_buffer["policy"]["a"]
  lags = []
  for _ in range(12):
    m.compute(update_history=True)
    lags.append(d.current_lags.clone())
  assert len(lags) == 12
  for k in range(12):
    if k % 3:
      assert torch.equal(lags[k], lags[k - 1])


def test_delay_hold_prob_one_in_the_manager():
  c = ObservationTermCfg(func=Counter(), delay_min_lag=1, delay_max_lag=3, delay_hold_prob=1.0)
  m = _manager({"a": c})
  d = m._group_obs_term_delay_buffer["policy"]["a"]
  for _ in range(6):
    m.compute(update_history=True)
    assert d.current_lags.tolist() == [0] * N


def test_partial_reset_restarts_the_delay_rows():
  m = _manager({"a": ObservationTermCfg(func=Counter(width=1), delay_min_lag=2, delay_max_lag=2)})
  for _ in range(4):
    o = m.compute(update_history=True)["policy"]
  assert o[:, 0].tolist() == [3.] * N
  m.reset(env_ids=torch.tensor([1, 3]))
  o = m.compute(update_history=True)["policy"]
  assert o[:, 0].tolist() == [4., 6., 4., 6.]  # reset rows see their newest frame again


# ------------------------------------------------------------------ numpy restatement
class NpRing:
  """utils/buffers/circular_buffer.py restated: time-major ring + pointer."""

  def __init__(self, max_len, n):
    self.L, self.n, self.ptr, self.buf = max_len, n, -1, None
    self.pushes = np.zeros(n, dtype=np.int64)

  def append(self, x):
    if self.buf is None:
      self.buf = np.zeros((self.L, *x.shape), dtype=x.dtype)
    self.ptr = (self.ptr + 1) % self.L
    self.buf[self.ptr] = x
    first = self.pushes == 0
    self.buf[:, first] = x[first]
    self.pushes += 1

  def reset(self, ids):
    self.pushes[ids] = 0
    if self.buf is not None:
      self.buf[:, ids] = 0.0

  def chronological(self):
    idx = (np.arange(self.L) + self.ptr + 1) % self.L
    return self.buf[idx].transpose(1, 0, 2)

  def lagged(self, lag):
    lag = np.maximum(np.minimum(lag, np.minimum(self.pushes, self.L) - 1), 0)
    return self.buf[(self.ptr - lag) % self.L, np.arange(self.n)]


class NpTerm:
  def __init__(self, n, width, offset, clip=None, scale=None, lag=0, hist=0):
    self.n, self.width, self.offset, self.clip, self.scale = n, width, offset, clip, scale
    self.lag, self.hist = lag, hist
    self.delay = NpRing(lag + 1, n) if lag > 0 else None
    self.ring = NpRing(hist, n) if hist > 0 else None

  def raw(self, k):
    # exactly representable in fp32: step + 16 env + column / 8 + term offset
    e = np.arange(self.n, dtype=np.float32)[:, None]
    c = np.arange(self.width, dtype=np.float32)[None, :]
    return (np.float32(k) + 16 * e + c / 8 + np.float32(self.offset)).astype(np.float32)

  def step(self, k):
    x = self.raw(k).copy()
    if self.clip:
      x = np.clip(x, *self.clip)
    if self.scale is not None:
      x = x * np.float32(self.scale)
    if self.delay is not None:
      self.delay.append(x)
      x = self.delay.lagged(np.full(self.n, self.lag))
    if self.ring is not None:
      self.ring.append(x)
      return self.ring.chronological().reshape(self.n, -1)
    return x

  def reset(self, ids):
    for r in (self.delay, self.ring):
      if r is not None:
        r.reset(ids)


class StepEnv(MockEnv):
  k = 0


def _signal(width, offset):
  def f(env):
    e = torch.arange(env.num_envs, dtype=torch.float32)[:, None]
    c = torch.arange(width, dtype=torch.float32)[None, :]
    return env.k + 16 * e + c / 8 + offset
  return f


# (width, offset, clip, scale, constant lag, history) per term of the two groups
_LAYOUT = {
  "policy": [(3, 0.0, None, None, 0, 3), (2, 0.5, (4.0, 40.0), 0.5, 2, 1), (4, 0.25, None, None, 0, 0)],
  "critic": [(3, 0.0, None, None, 2, 0), (2, 0.5, None, None, 0, 3), (1, 0.75, None, None, 2, 3)],
}


def _twin(n):
  env = StepEnv(n)
  cfg, model = {}, {}
  for g, layout in _LAYOUT.items():
    terms = {}
    for i, (w, off, clip, scale, lag, hist) in enumerate(layout):
      terms[f"t{i}"] = ObservationTermCfg(func=_signal(w, off), clip=clip, scale=scale,
                                          delay_min_lag=lag, delay_max_lag=lag, history_length=hist)
    cfg[g] = ObservationGroupCfg(terms=terms)
    model[g] = [NpTerm(n, w, off, clip, scale, lag, hist) for w, off, clip, scale, lag, hist in layout]
  return env, ObservationManager(cfg, env), model


@pytest.mark.parametrize("masked", [False, True])
def test_manager_equals_numpy_restatement(masked):
  n = 5
  env, m, model = _twin(n)
  assert m.group_obs_dim == {"policy": (3 * 3 + 2 * 1 + 4,), "critic": (3 + 2 * 3 + 1 * 3,)}
  ids = np.array([0, 3])
  for k in range(12):
    if k == 5:  # partial reset between steps 4 and 5
      for terms in model.values():
        for t in terms:
          t.reset(ids)
      if masked:
        mask = torch.zeros(n, dtype=torch.bool)
        mask[ids] = True
        m.reset_masked(mask)
      else:
        m.reset(env_ids=torch.as_tensor(ids))
    env.k = k
    got = m.compute(update_history=True)
    for g, terms in model.items():
      want = np.concatenate([t.step(k) for t in terms], axis=-1)
      assert got[g].dtype == torch.float32 and want.dtype == np.float32
      assert np.array_equal(got[g].numpy(), want), (g, k)


def test_reset_masked_matches_reset_ids_in_the_manager():
  n = 6
  env_a, a, _ = _twin(n)
  env_b, b, _ = _twin(n)
  mask = torch.tensor([True, False, True, False, False, True])
  for k in range(10):
    env_a.k = env_b.k = k
    oa, ob = a.compute(update_history=True), b.compute(update_history=True)
    for g in oa:
      assert torch.equal(oa[g], ob[g])
    if k in (3, 4, 8):
      a.reset(env_ids=mask.nonzero().squeeze(-1))
      b.reset_masked(mask)
      assert a._obs_buffer is None and b._obs_buffer is None
    for ba, bb in zip(a._buffers(), b._buffers()):
      fa = ba._buffer if hasattr(ba, "_buffer") else ba
      fb = bb._buffer if hasattr(bb, "_buffer") else bb
      assert torch.equal(fa.buffer, fb.buffer) and torch.equal(fa.current_length, fb.current_length)
