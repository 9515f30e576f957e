"""``RecurrentAlgorithm`` on dict observations: ``LSTMTrader`` on ``AlgoTrading`` through ``collect()`` / ``step()`` --
the fused and the generic rollout, fused and eager training (the embedding in front of the LSTM is trained through
the fused node's input gradient), whole-buffer and shuffled minibatches, carried observations and states -- and a
tensor-observation run that launches what it launched before."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import RecurrentAlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.distributions import Categorical  # noqa: E402
from rl8_amd.env import DiscreteDummyEnv  # noqa: E402
from rl8_amd.envs import AlgoTrading, LSTMTrader  # noqa: E402
from rl8_amd.nn import fused_lstm  # noqa: E402

from .test_first_update_gpu import Recorder, assert_update  # noqa: E402

DEV = "cuda"
N, H, L = 16, 8, 4
LEAVES = {"action_mask": (torch.bool, 3), "invested": (torch.int64, 1), "LOG_CHANGE(price)": (torch.float32, 1),
          "LOG_CHANGE(price, position)": (torch.float32, 1)}
EMBEDDING = "invested_embedding.weight"


class UnlistedCategorical(Categorical):
    """The same distribution under a class ``AlgoTrading.fused_distributions`` does not list: the generic rollout."""


def build(seed: int = 0, **overrides):
    torch.manual_seed(seed)  # (the model's initial weights and the env's reset stream)
    config = dict(num_envs=N, horizon=H, seq_len=L, seqs_per_state_reset=2, model_cls=LSTMTrader)
    config.update(overrides)
    return RecurrentAlgorithmConfig(**config).build(AlgoTrading)


def noise(seed: int = 1) -> torch.Tensor:
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty(H, N, 1, 3, device=DEV).exponential_(generator=gen)


def buffers(algo) -> dict[str, torch.Tensor]:
    buf = algo.buffer
    out = {k: buf[k].clone() for k in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.VALUES, DataKeys.REWARDS)}
    out.update({f"obs/{k}": v.clone() for k, v in buf[DataKeys.OBS].items()})
    out.update({f"states/{k}": v.clone() for k, v in buf[DataKeys.STATES].items()})
    return out


def test_builds_collects_and_steps():
    algo = build()
    assert algo._fusable() and algo._tm_obs is not None
    obs = algo.buffer[DataKeys.OBS]
    assert list(obs.keys()) == list(LEAVES)
    for leaf, (dtype, d) in LEAVES.items():
        assert obs[leaf].dtype == dtype and obs[leaf].shape == (N, H + 1, d), leaf
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = algo.collect()
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert stats["env/steps"] == N * H
    assert launched["rollout_step_algotrading"]["launches"] == H and "rollout_scatter_leaves" not in launched
    mask, invested = obs["action_mask"], obs["invested"]
    assert torch.equal(mask[..., 2:], invested == 1) and torch.equal(mask[..., 1:2], invested == 0)
    assert bool(mask[:, :H].gather(2, algo.buffer[DataKeys.ACTIONS][:, :H]).all()), "a masked action was taken"
    assert bool(obs["LOG_CHANGE(price)"][:, 1:].abs().sum() > 0)
    step_stats = algo.step()
    assert all(torch.isfinite(torch.tensor(float(v))) for k, v in step_stats.items() if k.startswith("losses/"))


def test_fused_and_generic_rollouts_fill_the_same_buffer():
    """With injected noise the one-launch-per-timestep rollout and policy.sample -> env.step ->
    rollout_scatter_leaves write the same buffer: bit for bit, floats included, as
    test_algotrading_gpu.py::test_fused_step_equals_sampler_plus_step_plus_bookkeeping holds the launch itself to."""
    fused, generic = build(), build(distribution_cls=UnlistedCategorical)
    assert fused._fusable() and not generic._fusable()
    generic.policy.model.load_state_dict(fused.policy.model.state_dict())
    out = []
    for algo in (fused, generic):
        algo.injected_noise = noise()
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            algo.collect()
            out.append((buffers(algo), hip.timer.summary()))
        finally:
            hip.timer.enabled = False
            hip.timer.reset()
    (a, launched_fused), (b, launched_generic) = out
    assert launched_generic["rollout_scatter_leaves"]["launches"] == H and "rollout_step_algotrading" not in launched_generic
    assert "rollout_scatter_leaves" not in launched_fused
    for k in a:
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def test_fused_and_eager_training_agree_and_train_the_embedding():
    """One step() on the same buffer with the fused node (LSTM + heads + dx) and with ``fused_lstm.ENABLED = False``
    (the ``nn.LSTM`` module): the first update's losses at the bars of test_first_update_gpu.py (rel 1e-5), every
    parameter gradient -- the embedding's, which only the new input gradient reaches, included -- within
    2e-5 max|w| + 1e-9."""
    results = {}
    for enabled in (True, False):
        algo = build(num_sgd_iters=1)
        algo.injected_noise = noise()
        algo.collect()  # (both rollouts on the fused forward: the same buffer)
        fused_lstm.ENABLED = enabled
        try:
            hip.timer.reset()
            hip.timer.enabled = True
            with Recorder(algo) as rec:
                algo.step()
            names = set(hip.timer.summary())
        finally:
            fused_lstm.ENABLED = True
            hip.timer.enabled = False
            hip.timer.reset()
        assert len(rec.updates) == 1
        assert ("lstm_narrow_input_grad" in names) == enabled and ("lstm_narrow_backward" in names) == enabled
        assert "gather_sequences" in names
        results[enabled] = (rec.updates[0], rec.first_grads)
    (got, grads), (want, eager) = results[True], results[False]
    assert_update(got, want, "fused vs eager")
    assert set(grads) == set(eager) == {k for k, _ in build().policy.model.named_parameters()}
    for k, w in eager.items():
        bar = 2e-5 * float(w.abs().max()) + 1e-9
        err = float((grads[k] - w).abs().max())
        print(f"fused vs eager gradient of {k}: max |w| {float(w.abs().max()):.3e}, max difference {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (k, err, bar)
    assert float(grads[EMBEDDING].abs().max()) > 0.0 and float(eager[EMBEDDING].abs().max()) > 0.0


def test_whole_buffer_and_shuffled_minibatches(monkeypatch):
    calls = []
    real = hip.gather_sequences

    def spy(index, seq_len, h, leaves):
        calls.append((None if index is None else index.clone(), seq_len, h, [leaf.dtype for leaf in leaves]))
        return real(index, seq_len, h, leaves)

    monkeypatch.setattr(hip, "gather_sequences", spy)
    seqs = N * (H // L)
    iters = 3
    whole = build(num_sgd_iters=iters)
    whole.collect()
    seen = []
    real_iter = whole._iter_minibatches

    def watch(sgd_iter):
        for batch in real_iter(sgd_iter):
            seen.append(batch is whole._flat_full)
            yield batch

    whole._iter_minibatches = watch
    whole.step()
    # one gather in buffer order, kept as _flat_full and read by every SGD iteration
    assert len(calls) == 1 and calls[0][0] is None and calls[0][1:3] == (L, H)
    assert calls[0][3] == [torch.bool, torch.int64, torch.float32, torch.float32]
    assert seen == [True] * iters

    calls.clear()
    shuffled = build(num_sgd_iters=iters, sgd_minibatch_size=8)
    shuffled.collect()
    gen = torch.Generator().manual_seed(5)
    perms = [torch.randperm(seqs, generator=gen) for _ in range(iters)]
    shuffled.injected_permutations = perms
    stats = shuffled.step()
    assert shuffled._flat_full is None
    assert len(calls) == iters * (seqs // 8)
    for i, (index, *_rest) in enumerate(calls):
        it, mb = divmod(i, seqs // 8)
        assert torch.equal(index.cpu(), perms[it][8 * mb:8 * mb + 8])
    assert all(torch.isfinite(torch.tensor(float(v))) for k, v in stats.items() if k.startswith("losses/"))


def test_second_collect_carries_observations_and_states():
    algo = build(horizons_per_env_reset=2, seqs_per_state_reset=4)  # (no state reset at the second rollout's start)
    algo.collect()
    first = buffers(algo)
    env_state = algo.env.state.clone()
    algo.step()
    algo.collect()
    second = buffers(algo)
    for k in first:
        if k.startswith(("obs/", "states/")):
            assert torch.equal(second[k][:, 0], first[k][:, H]), k
    assert bool(first["states/" + DataKeys.HIDDEN_STATES][:, H].abs().sum() > 0)
    assert not torch.equal(algo.env.state, env_state)
    assert algo.state.seqs == 2 * (H // L)


def test_width_256_trains_through_the_module():
    """No fused family returns an input gradient at 256: the model runs its ``nn.LSTM`` itself, and the embedding
    is trained all the same."""
    algo = build(num_sgd_iters=1, model_config={"hidden_size": 256})
    assert fused_lstm._family(algo.policy.model.lstm) == "256"
    algo.collect()
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        with Recorder(algo) as rec:
            algo.step()
        names = set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert not {n for n in names if n.startswith("lstm_")}, names
    assert float(rec.first_grads[EMBEDDING].abs().max()) > 0.0
    assert all(torch.isfinite(g).all() for g in rec.first_grads.values())


#: What a tensor-observation recurrent run (DiscreteDummyEnv, hidden width 64, one SGD iteration over the whole
#: buffer) launches, by ``hip.timer`` name, read off the code as it was before dict observations: the rollout's
#: timestep (lean: the narrow LSTM step and the heads inside the sampler + env kernel; plumbed: LSTM, heads, then the
#: sampler + env kernel), the bootstrap's LSTM step and heads, the stats, GAE, one whole-buffer gather, and the
#: one-node training pass with the fused loss.
COMMON = {"lstm_narrow_forward", "linear_heads_narrow_forward", "rollout_stats", "gae_scan", "advantage_normalise",
          "gather_minibatch", "ppo_loss_categorical", "linear_heads_narrow_backward", "lstm_narrow_backward",
          "lstm_narrow_reduce"}
TENSOR_OBS_NAMES = {True: COMMON | {"rollout_step_dummy_heads_narrow"}, False: COMMON | {"rollout_step_dummy"}}


@pytest.mark.parametrize("lean", [True, False], ids=["lean", "plumbed"])
def test_tensor_observations_launch_what_they_launched_before(lean):
    torch.manual_seed(0)
    algo = RecurrentAlgorithmConfig(num_envs=N, horizon=H, seq_len=L, seqs_per_state_reset=2, num_sgd_iters=1,
                                    model_config={"hidden_size": 64}).build(DiscreteDummyEnv)
    algo.lean_rollout = lean
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        algo.collect()
        algo.step()
        names = set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert names == TENSOR_OBS_NAMES[lean], (sorted(names - TENSOR_OBS_NAMES[lean]), sorted(TENSOR_OBS_NAMES[lean] - names))
