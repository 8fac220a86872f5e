"""LDS carve invariants of csrc/carve.h make_lds that the step kernels assume and nothing
states (no GPU: a stand-alone host program, tests/carve_invariants.cpp, compiled with the
host compiler against csrc/engine.h and the ROCm headers, and run here).

For every csrc/specs.inc entry and a sweep of generic dims (nv 6 .. 64, row capacities 8 ..
256, contacts 4 .. 64, with and without a heightfield) the program checks that

  - the J-in-global carve make_lds(d, 1, true) keeps `ints`, `M`, `qacc_smooth`, `qfrc_smooth`,
    `efc_aref`, `efc_D` and every B-pack offset up to `efc_J` where make_lds(d, 1) has them
    (the kernels of phase codes 9, 10 and 11 fill that carve from a pack laid out by the full
    one; csrc/carve.h states the same for the compiled specs as a static_assert);
  - the copy that fills it ends at or before the first region outside the pack, inside the
    carve;
  - a row-class carve (Dims with njmax = the class capacity) keeps [ints M qacc_smooth
    qfrc_smooth efc_aref] at the full carve's offsets and its `efc_D` / `efc_J` regions hold
    the class capacity without touching the next region;
  - phase C's `packC_sub`, `packC_b` and `pack_len` are ordered and inside the carve;
  - no phase carve of a model the engine admits exceeds the 160 KiB of a CU;

and reports the largest dynamic LDS the launches of phase codes 9 - 12 can ask for, which
decides what csrc/engine.hip prepare_step must raise the 64 KiB default for.

The same program checks the host-only launch decisions of csrc/launch_select.h: that over the
sweep prepare_step's rule (lds_need_max) covers every launch the selection functions can
return, the selection's known answers under default knobs, and -- run as `carve_invariants
select` under each knob environment of tests/test_gpu_kernel_variants.py KNOB_SETS -- that the
selection names the phase code that test expects to have launched.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mjlab-1_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "carve_invariants.cpp")


def _rocm_include():
  for base in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
    if base and os.path.exists(os.path.join(base, "include", "hip", "hip_runtime.h")):
      return os.path.join(base, "include")
  raise AssertionError("ROCm headers (hip/hip_runtime.h) not found: set ROCM_PATH")


def _build(tmp, extra=(), csrc=CSRC):
  cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
  assert cxx, "no host C++ compiler"
  exe = os.path.join(str(tmp), "carve_invariants")
  cmd = [cxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{_rocm_include()}", f"-I{csrc}",
         *extra, SRC, "-o", exe]
  return subprocess.run(cmd, capture_output=True, text=True), exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  r, exe = _build(tmp_path_factory.mktemp("carve"))
  assert r.returncode == 0, f"carve_invariants.cpp does not compile:\n{r.stderr[-4000:]}"
  return exe


@pytest.fixture(scope="module")
def report(program):
  run = subprocess.run([program], capture_output=True, text=True, timeout=120)
  lines = run.stdout.strip().splitlines()
  assert lines, run.stderr
  words = lines[-1].split()
  summary = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
  return run.returncode, lines[:-1], summary


def test_carve_invariants_hold(report):
  code, fails, summary = report
  assert code == 0 and summary["failures"] == 0 and not fails, "\n".join(fails[:40])
  # the sweep ran: 17 specs.inc entries and 59 x 32 x 16 x 2 generic dims, each with its carves
  assert summary["dims"] > 60000 and summary["carves"] > 500000, summary


def test_dynamic_lds_of_codes_9_to_12(report):
  """prepare_step raises hipFuncAttributeMaxDynamicSharedMemorySize where a launch can need
  more than the 64 KiB default.  The J-in-global carve (codes 9, 10) never does; the chain of
  code 11 (with phases C and A) and the full fast carve of code 12 can, within the 160 KiB
  the engine admits -- so prepare_step's loop covers every phase code, and the program's sweep
  (test_carve_invariants_hold) finds no launch that asks for more than it raises."""
  _, _, s = report
  assert s["max_jg_bytes"] <= 64 * 1024, s
  assert s["max_cap_bytes"] <= 64 * 1024 < s["max_cap256_bytes"] <= 160 * 1024, s
  assert 64 * 1024 < s["max_chain_jg_bytes"] <= 160 * 1024, s
  assert s["launches"] >= 20, s  # the fixed launches and every code the selection can return


def _selection(program, knobs):
  env = {k: v for k, v in os.environ.items() if not k.startswith("MJX355_")}
  run = subprocess.run([program, "select"], capture_output=True, text=True, timeout=30, env={**env, **knobs})
  assert run.returncode == 0, run.stderr
  words = run.stdout.split()
  return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def _knob_sets():
  import test_gpu_kernel_variants as variants  # (its tests are GPU tests; the table is plain data)
  return variants.KNOB_SETS


def test_default_selection(program):
  """test_gpu_kernel_variants.test_baseline_launches: the capped latency Newton for the
  full-capacity class, the bulk class's chain, the range chain, the masked forward as one launch."""
  assert _selection(program, {}) == {"cls0": 12, "cls1": 6, "masked_cls": 8, "masked_nocls": 8, "nocls": 6}


@pytest.mark.parametrize("knob_set", sorted(_knob_sets()))
def test_selection_of_knob_set(knob_set, program):
  """Under each knob environment the selection returns codes the GPU test expects to have
  launched (for the full-capacity class, the bulk class, the masked forward, a range without
  classes), none it expects not to have, and the default's where it expects the baseline's."""
  knobs, _, _, expect = _knob_sets()[knob_set]
  got, default = _selection(program, knobs), _selection(program, {})
  for kind, keys in (("cls", {"step": ("cls0", "cls1"), "masked": ("masked_cls",)}),
                     ("nocls", {"step": ("nocls",), "masked": ("masked_nocls",)})):
    if kind not in expect:
      continue
    for stage, names in keys.items():
      for name in names:
        if stage not in expect[kind]:
          assert got[name] == default[name], (knob_set, name, got)
          continue
        ran, not_ran = expect[kind][stage]
        assert got[name] in ran and got[name] not in not_ran, (knob_set, name, got, sorted(ran))


def test_a_moved_jg_offset_is_caught(tmp_path):
  """The check is live: with one offset of make_lds(..., true) moved (a copy of carve.h whose
  J-in-global carve pads `efc_D`), the static_assert beside make_lds refuses to compile, and
  with that assert compiled out the program reports the moved offsets."""
  csrc = tmp_path / "csrc"
  shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("build*", "*.o"))
  carve = csrc / "carve.h"
  text = carve.read_text()
  old = "{&Lds::efc_aref, R, A | B}, {&Lds::efc_D, R, A | B}"
  assert text.count(old) == 1
  carve.write_text(text.replace(old, "{&Lds::efc_aref, R + (ph == 1 && jglobal ? 4 : 0), A | B}, "
                                     "{&Lds::efc_D, R, A | B}"))
  r, _ = _build(tmp_path, csrc=str(csrc))
  assert r.returncode != 0 and "J-in-global carve moves a B-pack offset" in r.stderr, r.stderr[-2000:]
  text = carve.read_text()
  assert text.count("static_assert(jg_carve_agrees") == 1
  carve.write_text(text.replace("static_assert(jg_carve_agrees", "static_assert(true || jg_carve_agrees"))
  r, exe = _build(tmp_path, csrc=str(csrc))
  assert r.returncode == 0, r.stderr[-2000:]
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 1
  assert "LJ.efc_D == LB.efc_D" in run.stdout and "LJ.efc_J == LB.efc_J" in run.stdout, run.stdout[:2000]
