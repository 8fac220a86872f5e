"""Observation history / delay tail of the task descriptors (mjxObsState,
include/mjx355_task.h) at the C ABI: mjx_task_create / mjx_track_create check the segment
tables against the task's layout and the compiled capacities before anything reaches the
device, in the manner of tests/test_task_validation.py (whose descriptor builders these
cases reuse).  No GPU: a consistent descriptor gets as far as "hipMalloc failed" here."""

import ctypes

import pytest

from test_task_validation import NF, NJ, _create, _velocity_desc, lib  # noqa: F401

# the velocity layout's terms: policy head + command, then the critic's foot terms
POLICY_W = [3, 3, 3, NJ, NJ, NJ, 3]
CRITIC_W = POLICY_W + [NF, NF, NF, 3 * NF]


def _with_history(hp=3, hc=0):
  from mjlab_amd.fused import _U8
  d = _velocity_desc()
  for g, (widths, h) in enumerate(((POLICY_W, hp), (CRITIC_W, hc))):
    G = d.obs.group[g]
    G.nterm = len(widths)
    for s, w in enumerate(widths):
      G.seg[s].width, G.seg[s].history = w, h
  d.npolicy = sum(POLICY_W) * max(hp, 1)
  d.ncritic = sum(CRITIC_W) * max(hc, 1)
  d.obs.fresh = ctypes.cast(ctypes.c_void_p(0x1000), _U8)
  return d


def _passed(rc, msg):
  return rc == 0 or "hipMalloc" in msg or "upload" in msg


def test_zero_tail_is_the_single_frame_layout(lib):
  d = _velocity_desc()
  assert d.obs.group[0].nterm == 0 and d.obs.group[1].nterm == 0 and not d.obs.fresh
  rc, msg = _create(lib, d)
  assert _passed(rc, msg), msg


def test_descriptor_sizes_match_the_library(lib):
  from mjlab_amd.fused import TaskDesc
  from mjlab_amd.fused_tracking import TrackDesc
  lib.mjx_task_desc_size.restype = ctypes.c_size_t
  lib.mjx_track_desc_size.restype = ctypes.c_size_t
  assert lib.mjx_task_desc_size() == ctypes.sizeof(TaskDesc)
  assert lib.mjx_track_desc_size() == ctypes.sizeof(TrackDesc)


def test_history_tables_pass_validation(lib):
  for hp, hc in ((3, 0), (3, 2), (1, 0)):
    rc, msg = _create(lib, _with_history(hp, hc))
    assert _passed(rc, msg), msg


def test_widths_that_do_not_match_the_table(lib):
  d = _with_history(3, 0)
  d.npolicy -= 3  # one frame of a 3-wide term short
  rc, msg = _create(lib, d)
  assert rc != 0 and "segment table" in msg, msg
  d = _with_history(3, 0)
  d.obs.group[0].seg[3].width = NJ - 1  # frame no longer the layout's
  d.npolicy -= 3
  rc, msg = _create(lib, d)
  assert rc != 0 and "segment table" in msg, msg
  d = _velocity_desc()  # no table: the history width without its table
  d.npolicy *= 3
  rc, msg = _create(lib, d)
  assert rc != 0 and "observation widths" in msg, msg


def test_history_past_capacity(lib):
  from mjlab_amd.fused import MAX_HISTORY
  d = _with_history(MAX_HISTORY + 1, 0)
  rc, msg = _create(lib, d)
  assert rc != 0 and "history" in msg and str(MAX_HISTORY) in msg, msg


def test_history_without_the_fresh_flags(lib):
  d = _with_history(3, 0)
  d.obs.fresh = None
  rc, msg = _create(lib, d)
  assert rc != 0 and "fresh" in msg, msg


def test_delay_needs_its_state(lib):
  from mjlab_amd.fused import MAX_LAG, _FP, _I32
  d = _with_history(2, 0)
  seg = d.obs.group[0].seg[3]
  seg.min_lag, seg.max_lag = 2, 2
  rc, msg = _create(lib, d)
  assert rc != 0 and "ring" in msg, msg
  d.obs.group[0].delay_ring[3] = ctypes.cast(ctypes.c_void_p(0x1000), _FP)
  rc, msg = _create(lib, d)
  assert rc != 0 and "push-count" in msg, msg
  d.obs.delay_pushes = ctypes.cast(ctypes.c_void_p(0x1000), _I32)
  d.obs.delay_lag = ctypes.cast(ctypes.c_void_p(0x1000), _I32)
  rc, msg = _create(lib, d)
  assert _passed(rc, msg), msg
  seg.max_lag = MAX_LAG + 1
  rc, msg = _create(lib, d)
  assert rc != 0 and "lags" in msg, msg
  seg.min_lag, seg.max_lag = 3, 2
  rc, msg = _create(lib, d)
  assert rc != 0 and "lags" in msg, msg


def test_one_group_without_a_table(lib):
  d = _with_history(3, 0)
  d.obs.group[1].nterm = 0
  rc, msg = _create(lib, d)
  assert rc != 0 and "terms outside" in msg, msg
