"""The specialisation record (no GPU): the shipped table csrc/specs.inc is what
scripts/gen_specs.py writes and what jit.parse_specs reads back, and one rule
(jit.ineligible, the Python side of csrc/engine.h spec_can_hold) says which models run the
generic kernels only.  (The key derived twice: tests/test_model_tables.py.)"""

import importlib.util
import os

import pytest

from mjlab_amd import jit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = os.path.join(ROOT, "mjlab-1_amd", "csrc", "specs.inc")

# id -> scene, (nconmax, njmax), role (1 = a fast carve, 2 = a max carve)
TABLE = {1: ("g1_velocity", (48, 160), 1), 2: ("go1_velocity", (16, 64), 1), 3: ("g1_tracking", (56, 200), 1),
         4: ("g1_jump", (48, 160), 1), 5: ("g1_jump_hfield", (48, 160), 1),
         6: ("g1_velocity_rough", (48, 160), 1), 7: ("go1_velocity_rough", (24, 96), 1),
         8: ("go1_velocity", (48, 160), 1), 9: ("g1_tracking", (48, 160), 1),
         10: ("go1_velocity_rough", (48, 160), 1), 11: ("g1_velocity", (300, 300), 2),
         12: ("go1_velocity", (300, 300), 2), 13: ("g1_tracking", (250, 250), 2), 14: ("g1_jump", (300, 300), 2),
         15: ("g1_jump_hfield", (300, 300), 2), 16: ("g1_velocity_rough", (300, 300), 2),
         17: ("go1_velocity_rough", (300, 300), 2)}


def test_specs_inc_is_what_gen_specs_writes(tmp_path, capsys):
  spec = importlib.util.spec_from_file_location("gen_specs", os.path.join(ROOT, "scripts", "gen_specs.py"))
  gen = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(gen)
  out = tmp_path / "specs.inc"
  gen.main(str(out))
  capsys.readouterr()
  assert out.read_bytes() == open(SPECS, "rb").read()


def test_parse_specs_reads_the_table_back():
  from mjlab_amd.scenes import load_scene
  text = open(SPECS).read()
  entries = jit.parse_specs(text)
  assert {e["id"]: (e["scene"], (e["dims"]["nconmax"], e["dims"]["njmax"]), e["role"]) for e in entries} == TABLE
  assert [e["id"] for e in entries] == list(range(1, 18))
  # every line of the file is a comment or a parsed entry
  assert len([ln for ln in text.splitlines() if not ln.startswith("//")]) == len(entries)
  for e in entries:
    m = load_scene(e["scene"])
    assert e["ncyl"] == 0 == jit.cylinder_pairs(m)
    assert e["par"] == jit.dof_tree(m)
    want = jit.spec_dims(m)
    assert {k: v for k, v in e["dims"].items() if k not in ("nconmax", "njmax")} == \
           {k: int(v) for k, v in want.items() if k not in ("nconmax", "njmax")}
    # and a written entry reads back as itself
    line = jit.spec_line(e["id"], e["scene"], e["role"], e["ncyl"], e["dims"], e["par"])
    assert jit.parse_specs(line) == [e]


def _model(kind):
  if kind == "plain":
    from mjlab_amd.scenes import load_scene
    return load_scene("go1_velocity")
  if kind == "equality":
    import equality_scenes as es
    return es.model("lock")
  if kind == "condim":
    import condim_scenes as sc
    return sc.model("spin_plane6")
  import elliptic_scenes as el
  return el.model("slider")


@pytest.mark.parametrize("kind,names", [("plain", None), ("equality", "equality constraints"),
                                        ("condim", "condim 4 or 6"), ("elliptic", "elliptic friction cones")])
def test_one_eligibility_rule(kind, names, monkeypatch, tmp_path):
  m = _model(kind)
  why = jit.ineligible(m)
  if names is None:
    assert why is None
    return
  assert names in why
  # no library, and the compiler is never asked for one
  monkeypatch.setattr(jit, "HIPCC", str(tmp_path / "no_such_hipcc"))
  monkeypatch.setattr(jit, "CACHE", str(tmp_path / "cache"))
  monkeypatch.setattr(jit.subprocess, "run", lambda *a, **k: pytest.fail("the compiler was invoked"))
  assert jit.ensure_library(m, 48, 160, 1, compile_ok=True) is None
  assert not os.path.exists(str(tmp_path / "cache"))
