"""Golden vectors for the recurrent algorithm on dict observations: the reference's ``RecurrentAlgorithm`` on its
AlgoTrading environment (``examples/algotrading/env.py``) with a twin of ``rl8_amd.envs.LSTMTrader`` written here
against the REFERENCE's ``RecurrentModel`` (same layers, same parameter names, same order of the LSTM's inputs).

N = 16, H = 16, seq_len = 4, seqs_per_state_reset = 2, one SGD iteration over the whole buffer. Stored: the initial
weights, the reset state, the categorical noise of every step, the buffer after ``collect()``, ``CollectStats``, the
reward scale, the first update's losses, the gradient handed to the first optimizer step and its norm -- and the same
quantities under the prefix ``f64_`` from a run whose twin computes in fp64 (its parameters, the LSTM's inputs and
states in double; logits, values and states rounded to fp32 where they leave the model, so the sampler draws from
the same fp32 probabilities with the same random numbers). The difference of the two runs is the reference's own
fp32 error in the model, which the test may allow three times over.

Like ``generate_composite_fixtures.py`` this runs only where the reference is checked out next to the repository,
on the CPU, through the stubs; it imports the reference (through ``generate_fixtures``) only when it generates.
Fixtures hold arrays only.

Usage::

    python tests/golden/generate_recurrent_composite_fixtures.py

"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

LC, LCP = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"
SHORT = {"action_mask": "action_mask", "invested": "invested", LC: "log_change", LCP: "log_change_position",
         "position": "position", "f": "f", "k_cyclic": "k_cyclic", "k_market": "k_market", "t": "t", "price": "price"}
NUM_ENVS, HORIZON, SEQ_LEN, SEQS_PER_STATE_RESET = 16, 16, 4, 2


def lstm_trader_cls():
    """The twin of ``rl8_amd/envs/algotrading_models.py:LSTMTrader`` against the reference's ``RecurrentModel``. It
    computes in the dtype of its parameters (``.double()`` makes the fp64 run) and hands fp32 out."""
    import torch.nn as nn
    from rl8.data import DataKeys
    from rl8.models import RecurrentModel
    from tensordict import TensorDict
    from torchrl.data import Composite, Unbounded

    floor = torch.finfo(torch.float32).min

    class LSTMTraderTwin(RecurrentModel):
        def __init__(self, observation_spec, action_spec, /, invested_embed_dim=2, hidden_size=64):
            super().__init__(observation_spec, action_spec, invested_embed_dim=invested_embed_dim,
                             hidden_size=hidden_size)
            self.state_spec = Composite({
                DataKeys.HIDDEN_STATES: Unbounded(shape=torch.Size([1, hidden_size]), device=action_spec.device),
                DataKeys.CELL_STATES: Unbounded(shape=torch.Size([1, hidden_size]), device=action_spec.device),
            })
            self.invested_embedding = nn.Embedding(2, invested_embed_dim)
            self.lstm = nn.LSTM(invested_embed_dim + 2, hidden_size, num_layers=1, batch_first=True)
            self.feature_head = nn.Linear(hidden_size, 3)
            nn.init.uniform_(self.feature_head.weight, a=-1e-3, b=1e-3)
            nn.init.zeros_(self.feature_head.bias)
            self.vf_head = nn.Linear(hidden_size, 1)
            self._value = None

        def forward(self, batch, states, /):
            obs = batch[DataKeys.OBS]
            dtype = self.lstm.weight_ih_l0.dtype
            invested = obs["invested"]
            b, t = invested.shape[:2]
            x = torch.cat([self.invested_embedding(invested.reshape(b, t)), obs[LCP].to(dtype), obs[LC].to(dtype)], dim=-1)
            h_0 = states[DataKeys.HIDDEN_STATES][:, 0, ...].permute(1, 0, 2).contiguous().to(dtype)
            c_0 = states[DataKeys.CELL_STATES][:, 0, ...].permute(1, 0, 2).contiguous().to(dtype)
            latents, (h_n, c_n) = self.lstm(x, (h_0, c_0))
            latents = latents.reshape(b * t, -1)
            mask = torch.clamp(torch.log(obs["action_mask"].to(dtype)), min=floor)
            logits = self.feature_head(latents).reshape(-1, 1, 3) + mask.reshape(-1, 1, 3)
            self._value = self.vf_head(latents).reshape(-1, 1).float()
            return (
                TensorDict({"logits": logits.float()}, batch_size=logits.size(0), device=logits.device),
                TensorDict({DataKeys.HIDDEN_STATES: h_n.permute(1, 0, 2).float(),
                            DataKeys.CELL_STATES: c_n.permute(1, 0, 2).float()}, batch_size=b),
            )

        def value_function(self):
            return self._value

    return LSTMTraderTwin


def run(gf, *, double: bool) -> dict:
    from examples.algotrading.env import AlgoTrading
    from rl8 import RecurrentAlgorithmConfig

    torch.manual_seed(42)
    algo = RecurrentAlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, device="cpu", model_cls=lstm_trader_cls(),
                                    seq_len=SEQ_LEN, seqs_per_state_reset=SEQS_PER_STATE_RESET,
                                    num_sgd_iters=1).build(AlgoTrading)
    arrays: dict = {f"init_{k}": v.clone() for k, v in algo.policy.model.state_dict().items()}
    if double:
        # the optimizer holds these very parameters: .double() converts them in place
        algo.policy.model.double()
        assert all(p.dtype == torch.float64 for group in algo.optimizer.param_groups for p in group["params"])
    with gf.Recorder() as rec:
        real_reset = algo.env.reset
        resets = []

        def reset(*, config=None):
            out = real_reset(config=config)
            resets.append({f"it0_reset_{short}": algo.env.state[key].clone() for key, short in SHORT.items()})
            return out

        algo.env.reset = reset
        collect_stats = algo.collect()
        algo.env.reset = real_reset
        for k, v in algo.buffer.items():
            if torch.is_tensor(v):
                arrays[f"it0_collect_{k}"] = v.clone()
            else:
                for leaf, t in v.items():
                    arrays[f"it0_collect_{k}_{SHORT.get(leaf, leaf)}"] = t.clone()
        arrays["it0_reward_scale"] = np.float64(algo.state.reward_scale)
        with gf.UpdateRecorder(algo) as urec:
            step_stats = algo.step()
    assert len(resets) == 1 and len(urec.updates) == 1
    arrays.update(resets[0])
    arrays["it0_cat_q"] = torch.stack(rec.cat_q[:HORIZON])  # (the draws of collect(): one per timestep)
    collect_keys = sorted(k for k in collect_stats if not k.startswith("profiling"))
    step_keys = sorted(k for k in step_stats if not k.startswith("profiling"))
    arrays["it0_collect_stats"] = np.array([collect_stats[k] for k in collect_keys], np.float64)
    arrays["collect_stat_keys"] = np.array(collect_keys)
    arrays["sgd1_step_stats"] = np.array([step_stats[k] for k in step_keys], np.float64)
    arrays["step_stat_keys"] = np.array(step_keys)
    arrays["sgd1_updates"] = np.array(urec.updates, np.float64)
    total_sq = 0.0
    for k, gval in urec.first_grads.items():
        arrays[f"sgd1_grad_{k}"] = gval.double() if double else gval
        total_sq += float((gval.double() ** 2).sum())
    arrays["sgd1_clipped_grad_norm"] = np.float64(total_sq ** 0.5)
    arrays["stat_keys"] = np.array(gf.STAT_KEYS + ("reduce",))
    return arrays


def main() -> None:
    sys.path.insert(0, HERE)
    import generate_fixtures as gf  # imports the reference (and the stubs it needs)

    single, double = run(gf, double=False), run(gf, double=True)
    assert single["it0_cat_q"].shape == (HORIZON, NUM_ENVS, 1, 3)
    # the same experiment twice: same weights, same reset, same noise, and -- the sampler sees fp32 probabilities in
    # both -- the same actions, hence the same env trajectory
    exact = [k for k in single if k.startswith(("init_", "it0_reset_"))]
    exact += ["it0_cat_q", "it0_collect_actions", "it0_collect_rewards"]
    exact += [f"it0_collect_obs_{SHORT[leaf]}" for leaf in ("action_mask", "invested", LC, LCP)]
    for k in exact:
        assert np.array_equal(np.asarray(single[k]), np.asarray(double[k]), equal_nan=True), f"fp64 run differs: {k}"
    for k in ("it0_collect_rewards", "it0_collect_logp", "it0_collect_values"):
        assert np.isfinite(np.asarray(single[k])).all(), k  # (masked logits: nothing forbidden was drawn)
    # coverage the test relies on: both values of `invested`, every action, states that were re-initialised mid-rollout
    assert set(np.unique(np.asarray(single["it0_collect_actions"]))) == {0, 1, 2}
    assert set(np.unique(np.asarray(single["it0_collect_obs_invested"]))) == {0, 1}
    assert float(np.abs(np.asarray(single["sgd1_grad_invested_embedding.weight"])).max()) > 0
    arrays = dict(single)
    for k, v in double.items():
        if k not in exact and not k.endswith("_keys"):
            arrays[f"f64_{k}"] = v
    gf.save("first_update_rec_algotrading.npz", **arrays)


if __name__ == "__main__":
    main()
