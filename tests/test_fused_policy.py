"""FusedPolicy checks the kernel's limits when it is built, without a GPU: what
`csrc/policy.hip` cannot run is a ValueError naming the limit, never a torch fallback."""

import pytest
import torch

from mjlab_amd.rl.fused_policy import FusedPolicy
from mjlab_amd.rl.ppo import ActorCritic


def _policy(hidden, activation):
  obs = {"policy": torch.zeros(4, 9), "critic": torch.zeros(4, 11)}
  return ActorCritic(obs, {"policy": ["policy"], "critic": ["critic"]}, 3, actor_hidden_dims=hidden,
                     critic_hidden_dims=(16,), activation=activation)


@pytest.mark.parametrize("hidden, activation, limit", [
    ((513, 64), "elu", "hidden width 513 exceeds 512"),
    ((32, 32), "gelu", "activation GELU"),
    ((8, 8, 8, 8, 8), "elu", "6 linear layers"),
])
def test_outside_the_kernels_limits_is_a_value_error(hidden, activation, limit):
  with pytest.raises(ValueError, match=limit):
    FusedPolicy(_policy(hidden, activation))


def test_within_the_limits_builds_without_a_gpu():
  fp = FusedPolicy(_policy((512, 256, 128), "tanh"))
  assert fp.num_actions == 3 and fp.launches == 0
