"""A discrete action space of more than 64 actions through both algorithms: ``collect()`` and ``step()``, twice, on
``walk_env(4, 100)`` (tests/_envs.py) run the wave-per-row sampler and the wave-per-sample fused loss; a four-action
space beside it launches neither.  (Before these kernels the first ``collect()`` raised ``ValueError`` from
rl8_categorical_sample_logp_f32.)"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, RecurrentAlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402

from ._envs import walk_env  # noqa: E402

WIDE = {"categorical_sample_logp_wide", "ppo_loss_categorical_wide"}


def run(cfg_cls, n_actions):
    torch.manual_seed(3)
    # (the recurrent default of 8 sequences of 4 steps per state reset does not divide a horizon of 8)
    extra = dict(seqs_per_state_reset=2) if cfg_cls is RecurrentAlgorithmConfig else {}
    algo = cfg_cls(num_envs=64, horizon=8, **extra).build(walk_env(4, n_actions))
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = [algo.collect()]
        actions = algo.buffer[DataKeys.ACTIONS][:, :8].clone()  # (the first rollout's, before a step() takes the buffer)
        logp = algo.buffer[DataKeys.LOGP][:, :8].clone()
        stats += [algo.step(), algo.collect(), algo.step()]  # (a step() consumes its collect())
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    for s in stats:
        for key, value in s.items():
            assert math.isfinite(value), (key, value)
    assert stats[0]["env/steps"] == 64 * 8
    assert int(actions.min()) >= 0 and int(actions.max()) < n_actions
    assert torch.isfinite(logp).all()
    return algo, stats, launched, actions


@pytest.mark.parametrize("cfg_cls", [AlgorithmConfig, RecurrentAlgorithmConfig], ids=["feedforward", "recurrent"])
def test_a_hundred_actions_collect_and_step_on_the_wide_kernels(cfg_cls):
    algo, stats, launched, actions = run(cfg_cls, 100)
    assert WIDE <= set(launched), sorted(launched)
    assert launched["categorical_sample_logp_wide"]["launches"] == 2 * 8  # one draw per timestep of two rollouts
    assert launched["categorical_sample_logp_wide"]["units_per_launch"] == 64
    assert "ppo_loss_categorical" not in launched
    # 512 draws from a fresh policy over 100 classes: not one class, and classes beyond the first 64
    assert len(torch.unique(actions)) > 50 and int(actions.max()) >= 64
    assert stats[1]["losses/total"] != stats[3]["losses/total"]  # the first update moved the policy


@pytest.mark.parametrize("cfg_cls", [AlgorithmConfig, RecurrentAlgorithmConfig], ids=["feedforward", "recurrent"])
def test_four_actions_launch_no_wide_entry(cfg_cls):
    _, _, launched, _ = run(cfg_cls, 4)
    assert not (WIDE & set(launched)), sorted(launched)
    assert "ppo_loss_categorical" in launched
