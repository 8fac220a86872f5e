"""Contact order of phase A at up to 64 contacts: the rank sort through registers.

One free "raft" body carries n sphere geoms in a grid just above a plane, every sphere within
the margin, so a step holds exactly n contacts (one per sphere-plane pair) and 4 n pyramid
rows.  The narrowphase appends contacts in whatever order the lanes' atomics land; the sort
must return them ascending by pair index.  n covers nothing to sort (0, 1), the smallest
sorts (2, 3), more contacts than dofs' lanes (33) and a full wave (64).  The generic kernels
run (MJX355_JIT=0: the scenes match no compiled specialisation and nothing is compiled).

Asserted after one step: ncon == n, contact_geom equal to the pair list in pair order,
nefc == 4 n; and one fused 4-substep step bit-equal to 4 single steps on every mjData output.
The n = 33 raft is also dropped from above the margin, so the contacts appear mid-step.
"""

import numpy as np
import pytest
import torch

from mjlab_amd.compiler.mjcf import parse_mjcf_string
from mjlab_amd.compiler.model import EntitySpec, compile_scene
from parity_util import diff_detail, differing_outputs, output_snapshot, restore_state

pytestmark = pytest.mark.gpu

RADIUS, PITCH, MARGIN = 0.02, 0.06, 0.01
NWORLD = 8
_STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time")


def raft_model(n):
  side = max(1, int(np.ceil(np.sqrt(n))))
  geoms = []
  for k in range(n):
    x, y = (k % side - 0.5 * (side - 1)) * PITCH, (k // side - 0.5 * (side - 1)) * PITCH
    geoms.append(f'<geom name="s{k}" type="sphere" size="{RADIUS}" pos="{x!r} {y!r} 0" margin="{MARGIN}"/>')
  xml = ('<mujoco><worldbody><body name="raft" pos="0 0 0.5"><freejoint/>'
         '<inertial pos="0 0 0" mass="2" diaginertia="0.05 0.05 0.08"/>'
         + "".join(geoms) + "</body></worldbody></mujoco>")
  return compile_scene([EntitySpec("raft", parse_mjcf_string(xml))], terrain="plane", timestep=0.004)


def make_sim(m, n, device, height, monkeypatch):
  from mjlab_amd.sim import MujocoCfg, Simulation, SimulationCfg
  monkeypatch.setenv("MJX355_JIT", "0")
  cfg = SimulationCfg(nconmax=max(n, 1), njmax=max(4 * n, 4),
                      mujoco=MujocoCfg(timestep=m.timestep, iterations=10, ls_iterations=20))
  sim = Simulation(NWORLD, cfg, m, device)
  assert sim.info()["spec"] == 0, "the generic kernels are under test"
  rng = np.random.default_rng(n)
  q = np.tile(np.asarray(m.qpos0, np.float32), (NWORLD, 1))
  q[:, 2] = height
  q[:, :2] += rng.uniform(-0.2, 0.2, (NWORLD, 2)).astype(np.float32)
  d = sim.data
  d.qpos[:] = torch.as_tensor(q)
  d.qvel.zero_()
  d.qacc_warmstart.zero_()
  return sim


def expected_geoms(m):
  """(geom1, geom2) of every sphere-plane pair, ascending pair index."""
  return np.stack([np.asarray(m.arrays["pair_geom1"]).reshape(-1),
                   np.asarray(m.arrays["pair_geom2"]).reshape(-1)], axis=1).astype(np.int64)


def check_order(sim, m, n):
  d = sim.data
  st = sim.stats()
  assert st["unsupported"] == 0 and st["con_overflow"] == 0, st
  ncon = d.ncon.cpu().numpy().reshape(-1)
  assert (ncon == n).all(), ncon
  want = expected_geoms(m)
  assert len(want) == n
  geom = d.contact_geom.reshape(NWORLD, -1, 2).cpu().numpy()[:, :n]
  for w in range(NWORLD):
    assert np.array_equal(geom[w], want), (w, geom[w].tolist())
  assert (d.nefc.cpu().numpy().reshape(-1) == 4 * n).all()


def fused_equals_single(sim):
  state = {k: getattr(sim.data, k).clone() for k in _STATE}
  sim.step(nsubstep=4)
  torch.cuda.synchronize()
  fused = output_snapshot(sim)
  restore_state(sim, state)
  for _ in range(4):
    sim.step()
  torch.cuda.synchronize()
  single = output_snapshot(sim)
  bad = differing_outputs(fused, single)
  assert not bad, f"fused 4-substep step != 4 single steps in {bad}: {diff_detail(fused, single, bad)}"


@pytest.mark.parametrize("n", [0, 1, 2, 3, 33, 64])
def test_contacts_in_pair_order(n, gpu_device, monkeypatch):
  m = raft_model(n)
  # resting height: the spheres 2 mm above the plane, inside the margin
  sim = make_sim(m, n, gpu_device, RADIUS + 0.002, monkeypatch)
  sim.step()
  torch.cuda.synchronize()
  check_order(sim, m, n)
  fused_equals_single(sim)
  check_order(sim, m, n)


def test_contacts_appear_mid_step(gpu_device, monkeypatch):
  n = 33
  m = raft_model(n)
  # 4 mm above the margin and falling at 2 m/s: no contact at the first substep's
  # collision (gap 14 mm > margin 10 mm), all n of them from the second on (8 mm per substep)
  sim = make_sim(m, n, gpu_device, RADIUS + MARGIN + 0.004, monkeypatch)
  sim.data.qvel[:, 2] = -2.0
  sim.forward()
  torch.cuda.synchronize()
  assert int(sim.data.ncon.max()) == 0
  fused_equals_single(sim)
  check_order(sim, m, n)
