"""The term / metric / command kinds and the capacities that mjlab_amd/fused.py and
fused_tracking.py write into the task descriptors, against include/mjx355_task.h: every
MJX_* constant of the two modules equals the header's enumerator or define of that name, the
modules name every one the header has, and the kind tables hold only values it defines.

No GPU and no library: the header is parsed as text."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mjx355_task.h")
PREFIXES = ("MJX_RW_", "MJX_TM_", "MJX_MT_", "MJX_CMD_", "MJX_TR_", "MJX_TT_", "MJX_TASK_MAX_",
            "MJX_TRACK_")


def _header():
  """name -> value of every enumerator and integer define of the header."""
  text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
  out = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(MJX_\w+)\s+(\d+)\s*$", text, re.M)}
  for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
    for name, val in re.findall(r"\b(MJX_\w+)\s*=\s*(\d+)", body):
      assert name not in out, name
      out[name] = int(val)
  return out


def _python():
  from mjlab_amd import fused, fused_tracking
  out = {}
  for mod in (fused, fused_tracking):
    for name, val in vars(mod).items():
      if name.startswith("MJX_"):
        assert out.get(name, val) == val, name
        out[name] = val
  return out


def _group(consts, prefix):
  return {v for k, v in consts.items() if k.startswith(prefix)}


def test_header_parses():
  h = _header()
  assert h["MJX_RW_IS_ALIVE"] == 23 and h["MJX_TASK_MAX_JOINTS"] == 64 and h["MJX_TT_BODY_POS"] == 5
  for p in PREFIXES:
    assert _group(h, p), p


def test_python_constants_equal_the_header():
  h, py = _header(), _python()
  for name, val in py.items():
    assert name in h, f"{name} is not in include/mjx355_task.h"
    assert h[name] == val, f"{name}: python {val}, header {h[name]}"
  missing = [n for n in h if n.startswith(PREFIXES) and n not in py]
  assert not missing, f"header names without a Python constant: {missing}"


def test_capacity_aliases():
  from mjlab_amd import fused, fused_tracking
  h = _header()
  assert (fused.MAXJ, fused.MAXF, fused.MAXT, fused.MAXC) == (
    h["MJX_TASK_MAX_JOINTS"], h["MJX_TASK_MAX_FEET"], h["MJX_TASK_MAX_TERMS"],
    h["MJX_TASK_MAX_CONTACT_SLOTS"])
  assert (fused.MAX_OBS_TERMS, fused.MAX_HISTORY, fused.MAX_LAG) == (
    h["MJX_TASK_MAX_OBS_TERMS"], h["MJX_TASK_MAX_HISTORY"], h["MJX_TASK_MAX_LAG"])
  assert (fused_tracking.MAXB, fused_tracking.NMETRIC) == (h["MJX_TRACK_MAX_BODIES"], h["MJX_TRACK_NMETRIC"])
  assert fused.NMETRIC == h["MJX_MT_COUNT"] == len(fused._METRIC_KEYS)
  assert len(fused_tracking.METRIC_NAMES) == h["MJX_TRACK_NMETRIC"]


def test_kind_tables_hold_header_values():
  from mjlab_amd import fused, fused_tracking
  h = _header()
  rw, mt = _group(h, "MJX_RW_"), _group(h, "MJX_MT_") - {h["MJX_MT_COUNT"]}
  tr, tt = _group(h, "MJX_TR_"), _group(h, "MJX_TT_")
  assert set(fused._REWARD_KIND.values()) <= rw
  assert set(fused._JUMP_REWARD_KIND.values()) <= rw
  assert set(fused._METRIC_OF_KIND) <= rw and set(fused._METRIC_OF_KIND.values()) <= mt
  assert set(fused_tracking._REWARDS.values()) <= tr
  assert set(fused_tracking._TERMS.values()) == tt
  # a table maps each term function to one kind, and no two functions to the same kind
  for table in (fused._REWARD_KIND, fused._JUMP_REWARD_KIND, fused_tracking._REWARDS, fused_tracking._TERMS):
    assert len(set(table.values())) == len(table)
