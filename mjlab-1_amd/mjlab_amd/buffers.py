"""History and delay buffers of the observation manager.

API mirror of `src/mjlab/utils/buffers/{circular_buffer,delay_buffer}.py`: a batched
fixed-length history (`CircularBuffer`) and a lagged read of it (`DelayBuffer`).

The storage differs from the reference's ring + pointer: frames are kept in chronological
order, `[batch, max_len, ...]`, and an append shifts every row down by one frame.  That is
the layout the fused observe kernels use for their history blocks (mjx355_task.h), it makes
`buffer` a plain view, and every operation is a fixed sequence of tensor ops with no
data-dependent branch, so a step that appends / resets by mask records into a HIP graph.
All state tensors are updated in place for the same reason.
"""

from __future__ import annotations

from typing import Sequence

import torch


def _rows(batch_ids):
  return slice(None) if batch_ids is None else batch_ids


class CircularBuffer:
  """The last `max_len` frames of a `[batch, ...]` signal, per batch row.

  The first frame a row receives (after construction or after its reset) fills all of the
  row's slots, so a reader never sees unwritten history.  A reset zeroes the row and its
  push count.
  """

  def __init__(self, max_len: int, batch_size: int, device: str) -> None:
    if max_len < 1:
      raise ValueError(f"Buffer size must be >= 1, got {max_len}")
    self._max_len = int(max_len)
    self._batch_size = int(batch_size)
    self._device = device
    self._frames: torch.Tensor | None = None  # [batch, max_len, ...], oldest first
    self._num_pushes = torch.zeros(batch_size, dtype=torch.long, device=device)
    self._all_rows = torch.arange(batch_size, device=device)

  @property
  def batch_size(self) -> int:
    return self._batch_size

  @property
  def device(self) -> str:
    return self._device

  @property
  def max_length(self) -> int:
    return self._max_len

  @property
  def num_pushes(self) -> torch.Tensor:
    return self._num_pushes

  @property
  def current_length(self) -> torch.Tensor:
    """Valid frames per row, `[batch]`."""
    return self._num_pushes.clamp(max=self._max_len)

  @property
  def is_initialized(self) -> bool:
    return self._frames is not None

  @property
  def buffer(self) -> torch.Tensor:
    """`[batch, max_len, ...]`, oldest frame first."""
    if self._frames is None:
      raise RuntimeError("Buffer not initialized. Call append() first.")
    return self._frames

  def reset(self, batch_ids: Sequence[int] | torch.Tensor | None = None) -> None:
    rows = _rows(batch_ids)
    self._num_pushes[rows] = 0
    if self._frames is not None:
      self._frames[rows] = 0.0

  def reset_masked(self, mask: torch.Tensor) -> None:
    """`reset(mask.nonzero())` without the index list (no host sync)."""
    self._num_pushes.masked_fill_(mask, 0)
    if self._frames is not None:
      self._frames.masked_fill_(mask.view(-1, *([1] * (self._frames.dim() - 1))), 0.0)

  def append(self, data: torch.Tensor, mask: torch.Tensor | None = None) -> None:
    """`mask` (`[batch]` bool): only these rows take the frame; the others keep their frames
    and push count (no index list: records into a HIP graph)."""
    if data.shape[0] != self._batch_size:
      raise ValueError(f"Expected batch size {self._batch_size}, got {data.shape[0]}")
    data = data.to(self._device)
    if self._frames is None:
      self._frames = torch.zeros((self._batch_size, self._max_len, *data.shape[1:]),
                                 dtype=data.dtype, device=self._device)
    new = data.unsqueeze(1)
    shifted = torch.cat([self._frames[:, 1:], new], dim=1)
    fresh = (self._num_pushes == 0).view(-1, *([1] * (shifted.dim() - 1)))
    if mask is None:
      self._frames.copy_(torch.where(fresh, new, shifted))
      self._num_pushes += 1
      return
    rows = mask.view(-1, *([1] * (shifted.dim() - 1)))
    self._frames.copy_(torch.where(rows, torch.where(fresh, new, shifted), self._frames))
    self._num_pushes += mask.to(self._num_pushes.dtype)

  def __getitem__(self, key: torch.Tensor | int) -> torch.Tensor:
    """Frame `key` steps back per row (0 = newest), the lag clamped to what the row holds."""
    if self._frames is None:
      raise RuntimeError("Buffer not initialized. Call append() first.")
    if isinstance(key, int):
      key = torch.full((self._batch_size,), key, dtype=torch.long, device=self._device)
    else:
      if key.ndim == 0:
        key = key.expand(self._batch_size)
      key = key.to(device=self._device, dtype=torch.long)
    if key.numel() != self._batch_size:
      raise ValueError(f"Expected {self._batch_size} lags, got {key.numel()}")
    held = self._num_pushes.clamp(min=1, max=self._max_len)
    lag = torch.minimum(key, held - 1).clamp_min(0)
    return self._frames[self._all_rows, self._max_len - 1 - lag]


class DelayBuffer:
  """A signal read `lag` steps late, `lag` drawn in `[min_lag, max_lag]`.

  Each step: `append(obs)`, then `compute()` updates the lags and returns frame `t - lag`
  per row (clamped to the frames the row has).  Lag policy: with `update_period = N > 0` a
  row redraws only when `(steps + phase) % N == 0` (`per_env_phase` draws a phase per row
  in `[0, N)`), otherwise every step; a redraw is skipped with probability `hold_prob`;
  `per_env=False` draws one lag for the whole batch.  A reset clears the rows' history,
  lag and step count and redraws their phase.
  """

  def __init__(self, min_lag: int = 0, max_lag: int = 3, batch_size: int = 1,
               device: str = "cpu", per_env: bool = True, hold_prob: float = 0.0,
               update_period: int = 0, per_env_phase: bool = True,
               generator: torch.Generator | None = None) -> None:
    if min_lag < 0:
      raise ValueError(f"min_lag must be >= 0, got {min_lag}")
    if max_lag < min_lag:
      raise ValueError(f"max_lag ({max_lag}) must be >= min_lag ({min_lag})")
    if not 0.0 <= hold_prob <= 1.0:
      raise ValueError(f"hold_prob must be in [0, 1], got {hold_prob}")
    if update_period < 0:
      raise ValueError(f"update_period must be >= 0, got {update_period}")
    self.min_lag, self.max_lag = int(min_lag), int(max_lag)
    self.batch_size, self.device = int(batch_size), device
    self.per_env, self.hold_prob = bool(per_env), float(hold_prob)
    self.update_period, self.per_env_phase = int(update_period), bool(per_env_phase)
    self.generator = generator
    self._buffer = CircularBuffer(max_len=self.max_lag + 1, batch_size=batch_size, device=device)
    self._current_lags = torch.zeros(batch_size, dtype=torch.long, device=device)
    self._step_count = torch.zeros(batch_size, dtype=torch.long, device=device)
    self._phase_offsets = torch.zeros(batch_size, dtype=torch.long, device=device)
    if self._phased:
      self._phase_offsets.copy_(self._draw(0, self.update_period, batch_size))

  @property
  def _phased(self) -> bool:
    return self.update_period > 0 and self.per_env_phase

  def _draw(self, lo: int, hi: int, n: int) -> torch.Tensor:
    return torch.randint(lo, hi, (n,), dtype=torch.long, device=self.device,
                         generator=self.generator)

  @property
  def is_initialized(self) -> bool:
    return self._buffer.is_initialized

  @property
  def current_lags(self) -> torch.Tensor:
    return self._current_lags

  def set_lags(self, lags: torch.Tensor, batch_ids=None) -> None:
    self._current_lags[_rows(batch_ids)] = lags.clamp(self.min_lag, self.max_lag)

  def reset(self, batch_ids: Sequence[int] | torch.Tensor | slice | None = None) -> None:
    if isinstance(batch_ids, slice):
      batch_ids = list(range(*batch_ids.indices(self.batch_size)))
    self._buffer.reset(batch_ids=batch_ids)
    rows = _rows(batch_ids)
    self._current_lags[rows] = 0
    self._step_count[rows] = 0
    if self._phased:
      self._phase_offsets[rows] = self._draw(0, self.update_period, self.batch_size)[rows]

  def reset_masked(self, mask: torch.Tensor) -> None:
    self._buffer.reset_masked(mask)
    self._current_lags.masked_fill_(mask, 0)
    self._step_count.masked_fill_(mask, 0)
    if self._phased:
      drawn = self._draw(0, self.update_period, self.batch_size)
      self._phase_offsets.copy_(torch.where(mask, drawn, self._phase_offsets))

  def append(self, data: torch.Tensor, mask: torch.Tensor | None = None) -> None:
    self._buffer.append(data, mask)

  def compute(self, mask: torch.Tensor | None = None, hold: torch.Tensor | None = None) -> torch.Tensor:
    """`mask` (`[batch]` bool): only these rows advance (lag redraw, step count), the others
    read the frame of the lag they hold.  `hold`: rows that keep their lag through the redraw."""
    if not self.is_initialized:
      raise RuntimeError("Buffer not initialized. Call append() first.")
    self._update_lags(mask, hold)
    return self._buffer[self._current_lags]  # __getitem__ clamps to the frames held

  def _update_lags(self, mask: torch.Tensor | None = None, hold: torch.Tensor | None = None) -> None:
    if self.update_period > 0:
      due = (self._step_count + self._phase_offsets) % self.update_period == 0
    else:
      due = torch.ones(self.batch_size, dtype=torch.bool, device=self.device)
    if self.per_env:
      drawn = self._draw(self.min_lag, self.max_lag + 1, self.batch_size)
    else:
      drawn = self._draw(self.min_lag, self.max_lag + 1, 1).expand(self.batch_size)
    if self.hold_prob > 0.0:
      u = torch.rand(self.batch_size, dtype=torch.float32, device=self.device,
                     generator=self.generator)
      due = due & (u >= self.hold_prob)
    if hold is not None:
      due = due & ~hold
    if mask is not None:
      due = due & mask
    self._current_lags.copy_(torch.where(due, drawn, self._current_lags))
    self._step_count += 1 if mask is None else mask.to(self._step_count.dtype)
