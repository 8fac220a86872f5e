"""Every step-kernel launch variant a knob or a batch-size threshold selects, at small batches.

DESIGN.md section 3 rests on one invariant: a world's substep rounds identically whichever
kernel, LDS carve or launch topology ran it.  The variants chosen by a cached MJX355_* knob or
by the batch size alone (the J-in-global Newton kernels of phase codes 9 / 10 / 11, the
unchained bulk class, the capped and uncapped latency Newton, the three-launch and fast-carve
masked forwards, the range chain on and off) are pinned here: each knob set runs in a fresh
child process (tests/variant_child.py; the engine caches the knobs in function-local statics),
and

  1. every array the child records -- all of parity_util.DATA_FIELDS, the per-world counters,
     the event counts, after each of three single steps, a fused 4-substep step, a masked
     forward and (for the topologies a shipped configuration selects) a graph-captured fused
     step -- equals the baseline child's (no knob set) bit for bit, over all worlds;
  2. the launch counts (mjx_launch_counts) show that the targeted phase code ran and the one
     it replaces did not (KNOB_SETS, derived from csrc/engine.hip launch_step).

One documented exception: g1_small runs generic kernels in its fast
carve and specialised ones in its max carve, and the two families factor M and the Newton
Hessian in different elimination orders (dense natural order against the tree form of the
reversed matrix).  Its masked forward therefore rounds differently in the fast carve
(MJX355_MASKED_BIG=0) than in the max carve (the baseline): qacc_smooth and what follows from
it (measured: qacc_smooth differs by at most 3.3e-6 of the field's largest entry, 28 of its
ulps, which is 4,314 ulps of a baseline entry a thousandth of that size; qacc 3.5e-6,
contact_force 4.9e-6, cacc 1.9e-6, sensordata 1.5e-7, qfrc_constraint 6.0e-8).  For that
scenario and those two knob
sets the masked worlds' rounding-dependent fields are compared with the fp64 oracle at the
test_gpu_parity tolerances instead; every other field and every unmasked world stays bit for
bit.  g1_small_cls is the same case with generic kernels in both carves: bit for bit.

The baseline itself is tied to the fp64 oracle first: its first single step, every world of
every scenario, at the tolerances and the exact-ncon rule of test_gpu_parity.test_step_parity
and test_gpu_hfield._check_step; and the row-count populations the scenarios were chosen for
(worlds on both sides of the class capacity, worlds past the small fast carve) are asserted.

The parent process never touches the GPU.  A child that is killed at its time limit, exits
with 134 / 139 / a negative status or reports a HIP illegal access sets a module flag, and
every later test of the module fails at once without starting anything.

Child time limit: the baseline child (five scenarios, graph stage included) took 2.5 s wall
on an MI355X (2.05 s in the script, the rest interpreter start-up); the limit is about five
times that, rounded up: CHILD_TIMEOUT = 20 s.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import variant_child as vc
from parity_util import diff_detail, differing_outputs, oracle_step

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 20  # seconds (module docstring)
ALL_SCENARIOS = ("g1", "g1_small", "g1_small_cls", "hfield", "go1")
STEP, FUSED, MASKED = ("step1", "step2", "step3"), ("fused4", "graph4"), ("masked",)
CLASS_CAP = 60  # rows of the G1 48 / 160 carve's bulk class (choose_row_classes)
SMALL = (20, 80)
CLASSIFY = 13

_faulted = []  # the module flag: why no further child may start


def _run_child(tmp, tag, scenarios, graph, knobs):
  if _faulted:
    pytest.fail(f"not run: an earlier child faulted ({_faulted[0]})")
  job, out = os.path.join(tmp, f"{tag}.json"), os.path.join(tmp, f"{tag}.npz")
  with open(job, "w") as fh:
    json.dump({"scenarios": list(scenarios), "graph": bool(graph)}, fh)
  cmd = [sys.executable, os.path.join(HERE, "variant_child.py"), job, out]
  try:
    r = subprocess.run(cmd, env={**os.environ, **knobs}, timeout=CHILD_TIMEOUT,
                       capture_output=True, text=True)
  except subprocess.TimeoutExpired:
    _faulted.append(f"{tag}: killed at its {CHILD_TIMEOUT} s limit")
    pytest.fail(f"child {tag} hung: {_faulted[0]}")
  text = (r.stdout or "") + (r.stderr or "")
  if r.returncode in (134, 139) or r.returncode < 0 or "illegal memory access" in text:
    _faulted.append(f"{tag}: exit status {r.returncode}")
    pytest.fail(f"child {tag} faulted ({r.returncode}):\n{text[-3000:]}")
  assert r.returncode == 0, f"child {tag} failed ({r.returncode}):\n{text[-3000:]}"
  with np.load(out) as z:
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def baseline(gpu_device, tmp_path_factory):
  tmp = str(tmp_path_factory.mktemp("variants"))
  return _run_child(tmp, "baseline", ALL_SCENARIOS, True, {})


@pytest.fixture(scope="module")
def oracle():
  """First-step fp64 references, computed once: scenario -> (model, rows-160 refs, rows-300
  refs of the worlds a (20, 80) fast carve re-solves or None)."""
  out = {}
  for name in ("g1", "hfield", "go1"):
    _, m, n = vc.scenario_cfg(name)
    q, qv, ctrl = vc.scenario_states(name, m, n)
    ref = oracle_step(m, q, qv, np.zeros_like(qv), ctrl, step=True, nconmax=64, njmax=160)
    big = None
    if name == "g1":
      big = oracle_step(m, q, qv, np.zeros_like(qv), ctrl, step=True, nconmax=64, njmax=300)
    out[name] = (m, ref, big)
  out["g1_small"] = out["g1_small_cls"] = out["g1"]
  return out


def _counts(ref):
  return np.array([r["ncon"] for r in ref]), np.array([r["nefc"] for r in ref])


def test_oracle_row_counts(oracle):
  """The conditions the scenarios were chosen for, re-derived on the fp64 oracle."""
  nc, ne = _counts(oracle["g1"][1])
  assert ((ne <= CLASS_CAP).sum(), (ne == 0).sum(), (ne > CLASS_CAP).sum(), ne.max()) == (59, 21, 37, 112)
  assert nc.max() <= 48 and not any(r["overflow"] for r in oracle["g1"][1])
  assert ((ne > SMALL[1]) | (nc > SMALL[0])).sum() >= 27 and (ne > SMALL[1]).sum() >= 27
  nc, ne = _counts(oracle["hfield"][1])
  # (10 worlds without a row: in two of them the hfield narrowphase used to put a foot sphere
  # 3.5 cm above the surface 2 cm into the extended plane of a triangle past a ridge)
  assert ((ne <= CLASS_CAP).sum(), (ne == 0).sum(), (ne > CLASS_CAP).sum(), ne.max()) == (16, 10, 48, 136)
  assert nc.max() <= 34 and not any(r["overflow"] for r in oracle["hfield"][1])
  nc, ne = _counts(oracle["go1"][1])
  assert (ne.min(), ne.max()) == (4, 32) and nc.max() <= 8


@pytest.mark.parametrize("name", ALL_SCENARIOS)
def test_baseline_matches_oracle(name, baseline, oracle):
  """The baseline's first single step against the fp64 oracle, every world (tolerances and
  the exact contact count of test_gpu_parity.test_step_parity / test_gpu_hfield._check_step);
  the worlds the small fast carve re-solves against the oracle at 64 contacts / 300 rows."""
  m, ref, big = oracle[name]
  g = {k: baseline[f"{name}.step1.{k}"] for k in ("ncon", "nefc", "qacc", "qvel", "qpos", "sensordata",
                                                  "actuator_force", "solver_niter")}
  ncon, nefc, niter = (g[k].reshape(-1) for k in ("ncon", "nefc", "solver_niter"))
  n = len(ref)
  resolved = (ncon > SMALL[0]) | (nefc > SMALL[1]) if name.startswith("g1_small") else np.zeros(n, bool)
  hit = niter_equal = 0
  for i in range(n):
    r = big[i] if resolved[i] else ref[i]
    assert ncon[i] == r["ncon"], f"world {i}: ncon {ncon[i]} vs {r['ncon']}"
    hit += r["ncon"] > 0
    sc = max(1.0, np.abs(r["qacc"]).max())
    np.testing.assert_allclose(g["qacc"][i], r["qacc"], atol=2e-3 * sc, err_msg=f"qacc world {i}")
    np.testing.assert_allclose(g["qvel"][i], r["qvel"], atol=2e-3 * sc * m.timestep + 1e-5)
    np.testing.assert_allclose(g["qpos"][i], r["qpos"], atol=2e-3 * sc * m.timestep ** 2 + 1e-5)
    np.testing.assert_allclose(g["actuator_force"][i], r["actuator_force"], atol=1e-3, rtol=1e-4)
    ssc = max(1.0, np.abs(r["sensordata"]).max())
    np.testing.assert_allclose(g["sensordata"][i], r["sensordata"], atol=3e-3 * ssc, err_msg=f"sens {i}")
    assert abs(int(niter[i]) - r["niter"]) <= 1, f"world {i}: niter {niter[i]} vs {r['niter']}"
    niter_equal += int(niter[i]) == r["niter"]
  assert hit >= n // 2 and niter_equal >= 0.9 * n
  info = dict(zip(vc.INFO_KEYS + ("unsupported",), baseline[f"{name}.info"].tolist()))
  assert info["unsupported"] == 0


def test_baseline_populations(baseline):
  """Class populations and capacities from the baseline's own nefc and sim.info()."""
  info = {s: dict(zip(vc.INFO_KEYS, baseline[f"{s}.info"].tolist())) for s in ALL_SCENARIOS}
  cap = lambda s: (info[s]["nconmax"], info[s]["njmax"], info[s]["nconmax_max"], info[s]["njmax_max"])
  assert cap("g1") == cap("hfield") == (48, 160, 300, 300)
  assert cap("g1_small") == cap("g1_small_cls") == (*SMALL, 300, 300) and cap("go1") == (16, 64, 300, 300)
  # specialised kernels but for the small carve's fast kernels; the re-solve wired everywhere
  assert all(info[s]["spec"] > 0 for s in ("g1", "hfield", "go1"))
  assert all(info[s]["resolve_list"] > 0 for s in ALL_SCENARIOS)
  assert all(info[s]["spec_max"] > 0 for s in ALL_SCENARIOS if s != "g1_small_cls")
  # the small carve: generic fast kernels; the max carve's specialised, or (g1_small_cls) generic too
  assert info["g1_small"]["spec"] == info["g1_small_cls"]["spec"] == info["g1_small_cls"]["spec_max"] == 0
  # KNOB_SETS' expectations hold for these topologies: one row class (G1 fast carves; forced
  # onto the small carve's second scenario), none (Go1, and the small carve by default)
  assert [info[s]["row_classes"] for s in ALL_SCENARIOS] == [1, 0, 1, 1, 0]
  for s in ("g1", "hfield"):
    nefc, ncon = baseline[f"{s}.step1.nefc"].reshape(-1), baseline[f"{s}.step1.ncon"].reshape(-1)
    n = len(nefc)
    assert (nefc <= CLASS_CAP).sum() >= n // 4 and (nefc > CLASS_CAP).sum() >= n // 4, sorted(nefc)
    assert nefc.max() <= 160 and ncon.max() <= 48
  assert baseline["go1.step1.nefc"].max() <= 64 and baseline["go1.step1.ncon"].max() <= 16
  for s in ("g1", "hfield", "go1"):  # no world overflows its fast carve in any stage
    for st in STEP + FUSED + MASKED:
      assert baseline[f"{s}.{st}.event_counts"].tolist() == [0, 0, 0, 0], (s, st)
  for s in ("g1_small", "g1_small_cls"):
    ev = baseline[f"{s}.step1.event_counts"].tolist()
    assert ev[:3] == [0, 0, 0] and ev[3] >= 20, ev
    # ... also among the masked worlds' fresh states (the fast-carve masked forward's skip)
    assert _masked_over_small(baseline, s) >= 5
    # the class capacity forced on the second one has worlds on both sides below the carve
    nefc = baseline[f"{s}.step1.nefc"].reshape(-1)
    assert (nefc <= vc.SMALL_CLASS_CAP).sum() >= 20 and ((nefc > vc.SMALL_CLASS_CAP) & (nefc <= SMALL[1])).sum() >= 10


def _masked_over_small(baseline, s):
  """Masked worlds whose fresh state overflows the small fast carve (masked stage)."""
  nefc, ncon = (baseline[f"{s}.masked.{k}"].reshape(-1) for k in ("nefc", "ncon"))
  mk = vc.masked_worlds(len(nefc))
  return int(((nefc > SMALL[1]) | (ncon > SMALL[0]))[mk].sum())


def test_baseline_launches(baseline):
  """The default topology at these batch sizes (launch_step): with a row class, per substep a
  classify, the capped latency Newton (12) with its piped C (2) and next A (0) for the
  full-capacity class, the bulk class's chain (6), the re-solve chain (5, and 4 while a next
  substep follows); without classes the range chain (6) and the re-solve chain; the masked
  forward as one launch in the max carve (8)."""
  for s in ALL_SCENARIOS:
    cls = s in ("g1", "hfield", "g1_small_cls")
    want1 = {0: 1, 5: 1, 6: 1, **({2: 1, 12: 1, CLASSIFY: 1} if cls else {})}
    want4 = {0: 4 if cls else 1, 4: 3, 5: 4, 6: 4, **({2: 4, 12: 4, CLASSIFY: 4} if cls else {})}
    for stages, want in ((STEP, want1), (FUSED, want4), (MASKED, {8: 1})):
      for st in stages:
        got = baseline[f"{s}.{st}.launch_counts"].tolist()
        assert got == [want.get(c, 0) for c in range(vc.NCODES)], (s, st, got)


# Knob set -> (environment, scenarios, graph stage, expectations).  An expectation is, per
# stage kind, (codes that must have launched, codes that must not have); a stage kind that is
# not named must show the baseline's launch counts exactly.  "cls" scenarios have one Newton
# row class (g1, hfield, g1_small_cls), the others none (g1_small, go1: range chain at these
# batch sizes).  Derived from csrc/engine.hip launch_step:
#   class_chain(cls): chained (chain_env) -> step_chain 6 (bulk), 7 (full class, latency form),
#     11 (that with J in global memory, NEWTON_JG=1); unchained -> Newton 1 (bulk) / 9, 10
#     (NEWTON_JG=1, 2) / 12 (heavy_cap) / 3 for the full class, then C (2) and the next A (0);
#   masked forward: step_masked 8 in the max carve, or A / latency Newton / C (0, 3, 2) there
#     (MASKED_FUSED=0), or in the fast carve A (0), Newton 9 (J in global memory; 3 with
#     MASKED_JG=0; 1 without row classes), C (2) and the in-line re-solve (5);
#   without classes: the range chain 6, or A / B / C (0, 1, 2; B as 10 with NEWTON_JG=2).
CLS, NOCLS = ("g1", "hfield", "g1_small_cls"), ("g1_small", "go1")
JG, CH, HC = "MJX355_NEWTON_JG", "MJX355_CHAIN", "MJX355_HEAVY_CAP"
MB, MJ, MF, RC = "MJX355_MASKED_BIG", "MJX355_MASKED_JG", "MJX355_MASKED_FUSED", "MJX355_RANGE_CHAIN"
SAME = {}  # every stage kind shows the baseline's launch counts
KNOB_SETS = {
  # exactly what jg_mode / chain_env choose above 8,192 worlds
  "jg2_chain0": ({JG: "2", CH: "0"}, ("g1", "g1_small", "g1_small_cls", "hfield"), True,
                 {"cls": {"step": ({10, 1, 2, 0, 5, CLASSIFY}, {3, 12, 6, 7, 9, 11})}, "nocls": SAME}),
  "jg1": ({JG: "1"}, ("g1", "g1_small", "g1_small_cls", "hfield"), False,
          {"cls": {"step": ({9, 6, 2}, {3, 12, 10, 11, 7, 1})}, "nocls": SAME}),
  "jg2": ({JG: "2"}, ("g1",), False, {"cls": {"step": ({10, 6, 2}, {3, 12, 9, 11, 7, 1})}}),
  "jg1_chain1": ({JG: "1", CH: "1"}, ("g1",), False,
                 {"cls": {"step": ({11, 6}, {3, 12, 9, 10, 7, 1, 2})}}),
  "chain0": ({CH: "0"}, ("g1", "hfield"), False, {"cls": {"step": ({12, 1, 2}, {6, 7, 11, 3, 9, 10})}}),
  "chain1": ({CH: "1"}, ("g1", "hfield"), False, {"cls": {"step": ({7, 6}, {12, 3, 1, 2, 11, 9, 10})}}),
  "chain3": ({CH: "3"}, ("g1", "hfield"), False, {"cls": {"step": ({7, 1, 2}, {6, 12, 3, 11, 9, 10})}}),
  "heavy_cap0": ({HC: "0"}, ("g1", "hfield"), False, {"cls": {"step": ({3, 6}, {12, 1, 9, 10})}}),
  "heavy_cap1": ({HC: "1"}, ("g1", "hfield"), False, {"cls": SAME}),  # (the default up to 160 rows)
  "newton_lat0": ({"MJX355_NEWTON_LAT": "0"}, ("g1",), False, {"cls": {"step": ({1, 6}, {3, 12, 7, 9, 10})}}),
  "class_pipe0": ({"MJX355_CLASS_PIPE": "0"}, ("g1",), False,
                  {"cls": {"step": ({12, 1, 2, 0, 5}, {6, 7, 4, 3})}}),
  "masked_fused0": ({MF: "0"}, ("g1", "hfield", "go1"), False,
                    {"cls": {"masked": ({0, 3, 2}, {8, 1, 9, 5})}, "nocls": {"masked": ({0, 3, 2}, {8, 1, 9, 5})}}),
  "masked_big0": ({MB: "0"}, ("g1", "g1_small", "g1_small_cls", "hfield"), True,
                  {"cls": {"masked": ({0, 9, 2, 5}, {8, 3, 1, CLASSIFY})},
                   "nocls": {"masked": ({0, 1, 2, 5}, {8, 3, 9, 6})}}),
  "masked_big0_jg0": ({MB: "0", MJ: "0"}, ("g1", "g1_small", "g1_small_cls", "hfield"), False,
                      {"cls": {"masked": ({0, 3, 2, 5}, {8, 9, 1, CLASSIFY})},
                       "nocls": {"masked": ({0, 1, 2, 5}, {8, 3, 9, 6})}}),
  "range_chain0": ({RC: "0"}, ("go1",), True, {"nocls": {"step": ({0, 1, 2, 5}, {6, 4, 10})}}),
  "range_chain1": ({RC: "1"}, ("go1",), True, {"nocls": SAME}),  # (the default at this batch size)
  # NEWTON_JG=2 reaches a model without row classes only where no range chain runs
  "jg2_go1": ({JG: "2"}, ("go1",), False, {"nocls": SAME}),
  "jg2_range_chain0": ({JG: "2", RC: "0"}, ("go1", "g1_small"), False,
                       {"nocls": {"step": ({0, 10, 2, 5}, {6, 4, 1})}}),
}
# exact counts where the fused stage tells more than "ran": launches per 4 substeps
FUSED_COUNTS = {
  "jg1_chain1": {0: 1, 11: 4, 6: 4},        # each class's next A inside its chain
  "chain1": {0: 1, 7: 4, 6: 4},
  "class_pipe0": {0: 4, 2: 4, 5: 4, 4: 0},  # A and C over every world each substep
  "range_chain0": {0: 4, 1: 4, 2: 4, 5: 4},
  "jg2_chain0": {10: 4, 1: 4, 2: 8, 0: 7},  # both classes: B, C, and the next A three times
}


# (knob set, scenario, stage) whose masked worlds round differently from the baseline by a
# written cause (module docstring), and the fields that depend on that rounding
ROUNDING_EXCEPTIONS = {("masked_big0", "g1_small", "masked"), ("masked_big0_jg0", "g1_small", "masked")}
ROUNDING_FIELDS = ("qacc", "qacc_smooth", "cacc", "sensordata", "qfrc_constraint", "contact_force")


@pytest.fixture(scope="module")
def oracle_masked():
  """fp64 forward of the fresh states the masked G1 worlds get (64 contacts / 300 rows)."""
  _, m, n = vc.scenario_cfg("g1_small")
  q, qv, ctrl = vc.scenario_states("g1_small", m, n, fresh=True)
  mk = np.nonzero(vc.masked_worlds(n))[0]
  ref = oracle_step(m, q[mk], qv[mk], np.zeros_like(qv[mk]), ctrl[mk], step=False, nconmax=64, njmax=300)
  return mk, ref


def _check_rounding_exception(knob_set, s, base, got, pre, names, oracle_masked):
  """The masked worlds' ROUNDING_FIELDS against the oracle (test_gpu_parity tolerances), the
  largest difference from the baseline in ulps printed; returns the baseline with those entries
  taken from the variant, so that everything else is still compared bit for bit."""
  mk, ref = oracle_masked
  ncon = got[pre + "ncon"].reshape(-1)
  for j, w in enumerate(mk):
    r = ref[j]
    assert ncon[w] == r["ncon"], f"{knob_set} {s} world {w}: ncon {ncon[w]} vs {r['ncon']}"
    sc = max(1.0, np.abs(r["qacc_smooth"]).max())
    np.testing.assert_allclose(got[pre + "qacc_smooth"][w], r["qacc_smooth"], atol=1e-3 * sc)
    sc = max(1.0, np.abs(r["qacc"]).max())
    np.testing.assert_allclose(got[pre + "qacc"][w], r["qacc"], atol=2e-3 * sc, err_msg=f"qacc world {w}")
    ssc = max(1.0, np.abs(r["sensordata"]).max())
    np.testing.assert_allclose(got[pre + "sensordata"][w], r["sensordata"], atol=3e-3 * ssc)
  out = dict(base)
  for k in ROUNDING_FIELDS:
    a, b = base[k], got[pre + k]
    # (entries below 1e-3 of the field's largest are measured in ulps of that floor)
    mag = np.maximum(np.abs(a[mk]), 1e-3 * np.abs(a[mk]).max()).astype(np.float32)
    ulp = np.abs(a[mk].astype(np.float64) - b[mk]) / np.spacing(mag)
    rel = np.abs(a[mk].astype(np.float64) - b[mk]).max() / max(np.abs(a[mk]).max(), 1e-30)
    print(f"rounding exception {knob_set} {s} {k}: largest difference {ulp.max():.0f} ulps of the "
          f"baseline entry, {rel:.2e} of the field's largest entry")
    merged = a.copy()
    merged[mk] = b[mk]
    out[k] = merged
  return out


@pytest.mark.parametrize("knob_set", list(KNOB_SETS))
def test_variant_bit_identical(knob_set, baseline, tmp_path, oracle_masked):
  knobs, scenarios, graph, expect = KNOB_SETS[knob_set]
  got = _run_child(str(tmp_path), knob_set, scenarios, graph, knobs)
  problems = []
  for s in scenarios:
    kind = expect["cls" if s in CLS else "nocls"]
    for st in STEP + FUSED + MASKED:
      if st == "graph4" and not graph:
        continue
      pre = f"{s}.{st}."
      names = [k[len(pre):] for k in baseline if k.startswith(pre) and not k.endswith("launch_counts")]
      assert len(names) == len(vc_fields()) and all(pre + k in got for k in names), (s, st)
      # the re-solve count (event_counts[3]) is not a world's output: a fast-carve masked
      # forward re-solves the masked worlds past the fast carve, the max-carve one has none to
      base_ev, got_ev = baseline[pre + "event_counts"].copy(), got[pre + "event_counts"].copy()
      if MB in knobs and s.startswith("g1_small") and st in ("masked", "graph4"):
        base_ev[3] += _masked_over_small(baseline, s)
      base = {**{k: baseline[pre + k] for k in names}, "event_counts": base_ev}
      if (knob_set, s, st) in ROUNDING_EXCEPTIONS:
        base = _check_rounding_exception(knob_set, s, base, got, pre, names, oracle_masked)
      # 1. every recorded array bit for bit (raw bytes: -0.0 is not 0.0 here)
      if any(base[k].tobytes() != got[pre + k].tobytes() or
             base[k].shape != got[pre + k].shape for k in names):
        import torch
        a = {k: torch.from_numpy(base[k]) for k in names}
        b = {k: torch.from_numpy(got[pre + k]) for k in names}
        bad = differing_outputs(a, b)
        problems.append(f"{knob_set} {s} {st}: differs from the baseline in {bad or 'sign of zero'}: "
                        f"{diff_detail(a, b, bad)}")
      # 2. the targeted phase code ran, the one it replaces did not
      lc, base_lc = got[pre + "launch_counts"].tolist(), baseline[pre + "launch_counts"].tolist()
      stage_kind = "step" if st in STEP + FUSED else "masked"
      if stage_kind not in kind:
        if lc != base_lc:
          problems.append(f"{knob_set} {s} {st}: launches {lc}, baseline {base_lc}")
        continue
      ran, not_ran = kind[stage_kind]
      if any(lc[c] == 0 for c in ran) or any(lc[c] != 0 for c in not_ran):
        problems.append(f"{knob_set} {s} {st}: launches {lc}: expected {sorted(ran)} > 0, {sorted(not_ran)} = 0")
      if st in FUSED and knob_set in FUSED_COUNTS and s in CLS + ("go1",):
        want = FUSED_COUNTS[knob_set]
        if any(lc[c] != v for c, v in want.items()):
          problems.append(f"{knob_set} {s} {st}: launches {lc}: expected {want}")
  assert not problems, "\n".join(problems)


def vc_fields():
  from parity_util import DATA_FIELDS
  return tuple(DATA_FIELDS) + ("engine_counters[0,1,5]", "event_counts")
