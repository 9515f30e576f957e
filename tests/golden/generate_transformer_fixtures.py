"""Golden vectors for ``rl8_amd.envs.TransformerTrader``: the reference's ``Algorithm`` with its own
``AttentiveAlpaca`` (``examples/algotrading/models/transformer.py``: the rolling window of price changes through a
parameter-sharing self-attention stack and a masked average, in front of two BatchNorm towers) on its ``AlgoTrading``
environment, through ``collect()`` and a one-iteration ``step()``.

The twin of ``generate_windowed_fixtures.py``: the same array names, the same two runs (the reference as it is in fp32,
and the reference's own code on the same trajectory with every floating-point tensor in double precision), the same way
of importing the reference unmodified only when it generates. The fixture holds arrays only.

``tests/test_transformer_trader_first_update_gpu.py`` asks for exactly the reference's actions, which only means
something if no draw of the trajectory sits on a rounding edge. So this generator asserts, and refuses to write the
fixture otherwise, that

* the fp64 re-evaluation draws the action of the fp32 run at every one of the N x H draws, and
* the smallest relative gap between the best and the second-best ``p / q`` of a draw is at least 1e-5.

Both hold for ``torch.manual_seed(42)`` (printed below when it runs). Should a later torch change the draws, pick
another seed for which both hold and say which.

Usage::

    python tests/golden/generate_transformer_fixtures.py

"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

NUM_ENVS, HORIZON, SEQ_LEN, SEED = 64, 32, 4, 42
MIN_RELATIVE_GAP = 1e-5


def gen_transformer_first_update(gf, gc) -> None:
    from examples.algotrading.env import AlgoTrading
    from examples.algotrading.models.transformer import AttentiveAlpaca
    from rl8 import AlgorithmConfig
    from rl8.data import DataKeys

    def build():
        torch.manual_seed(SEED)
        return AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, device="cpu", model_cls=AttentiveAlpaca,
                               model_config={"seq_len": SEQ_LEN}, num_sgd_iters=1).build(AlgoTrading)

    # ---- fp32: the reference as it is ----
    algo = build()
    init = {k: v.clone() for k, v in algo.policy.model.state_dict().items()}
    print(f"state dict: {len(init)} tensors, {sum(v.numel() for v in init.values())} elements")
    arrays: dict = {f"init_{k}": v for k, v in init.items()}
    with gf.Recorder() as rec:
        real_reset = algo.env.reset

        def reset(*, config=None):
            out = real_reset(config=config)
            gc.state_arrays(algo.env.state, "it0_reset", arrays)
            return out

        algo.env.reset = reset
        collect_stats = algo.collect()
        algo.env.reset = real_reset
        buffer = algo.buffer.clone()
        for k, v in buffer.items():
            if torch.is_tensor(v):
                arrays[f"it0_collect_{k}"] = v.clone()
            else:
                for leaf, t in v.items():
                    arrays[f"it0_collect_{k}_{gc.SHORT[leaf]}"] = t.clone()
        reward_scale = algo.state.reward_scale
        with gf.UpdateRecorder(algo) as urec:
            step_stats = algo.step()
    assert len(urec.updates) == 1 and len(rec.cat_q) == HORIZON
    cat_q = torch.stack(rec.cat_q)
    arrays["it0_cat_q"] = cat_q
    arrays["it0_perms"] = torch.stack(rec.perms)
    arrays["it0_reward_scale"] = np.float64(reward_scale)
    collect_keys = sorted(k for k in collect_stats if not k.startswith("profiling"))
    step_keys = sorted(k for k in step_stats if not k.startswith("profiling"))
    arrays["it0_collect_stats"] = np.array([collect_stats[k] for k in collect_keys], np.float64)
    arrays["collect_stat_keys"] = np.array(collect_keys)
    arrays["step_stat_keys"] = np.array(step_keys)
    arrays["sgd1_updates"] = np.array(urec.updates, np.float64)
    arrays["sgd1_step_stats"] = np.array([step_stats[k] for k in step_keys], np.float64)
    total_sq = 0.0
    for k, gval in urec.first_grads.items():
        arrays[f"sgd1_grad_{k}"] = gval
        total_sq += float((gval.double() ** 2).sum())
    arrays["sgd1_clipped_grad_norm"] = np.float64(total_sq ** 0.5)
    for k, v in algo.policy.model.state_dict().items():
        arrays[f"sgd1_final_{k}"] = v.clone()
    arrays["stat_keys"] = np.array(gf.STAT_KEYS + ("reduce",))
    for k in ("it0_collect_rewards", "it0_collect_logp", "it0_collect_values"):
        assert np.isfinite(arrays[k].numpy()).all(), k  # (masked logits: nothing forbidden was drawn, no +inf reward)

    # ---- fp64: the same code and trajectory, every floating-point tensor in double precision ----
    algo64 = build()
    model64 = algo64.policy.model
    model64.load_state_dict(init)
    model64.double()
    for k, v in model64.state_dict().items():
        if v.is_floating_point():
            assert v.dtype == torch.float64 and torch.equal(v, init[k].double()), k

    def double(x):
        return x.double() if x.is_floating_point() else x.clone()

    buffer64 = buffer.apply(double)
    actions = buffer64[DataKeys.ACTIONS]
    flips, smallest_gap = 0, float("inf")
    for t in range(HORIZON + 1):  # Policy.sample as collect() calls it (training mode: BatchNorm on batch statistics)
        sample = algo64.policy.sample(
            buffer64[:, : (t + 1), ...], kind="last", deterministic=False, inplace=False, requires_grad=False,
            return_actions=False, return_logp=False, return_values=True, return_views=False,
        )
        assert sample[DataKeys.VALUES].dtype == torch.float64
        buffer64[DataKeys.VALUES][:, t, ...] = sample[DataKeys.VALUES]
        if t < HORIZON:
            dist = algo64.policy.distribution_cls(sample[DataKeys.FEATURES], model64)
            buffer64[DataKeys.LOGP][:, t, ...] = dist.logp(actions[:, t, ...])
            # the draw the fp64 model makes from the fp32 run's noise: argmax p / q, and how close the runner-up came
            logits = sample[DataKeys.FEATURES]["logits"]
            ratio = torch.softmax(logits, dim=-1) / cat_q[t].double().reshape(logits.shape)
            top = ratio.topk(2, dim=-1)
            flips += int((top.indices[..., 0] != actions[:, t, ...]).sum())
            smallest_gap = min(smallest_gap, float(((top.values[..., 0] - top.values[..., 1]) / top.values[..., 0]).min()))
    draws = NUM_ENVS * HORIZON
    print(f"seed {SEED}: {flips} of {draws} draws differ between the fp32 run and its fp64 re-evaluation;"
          f" smallest relative gap between the best and the second-best p / q {smallest_gap:.3e}")
    assert flips == 0, f"{flips} draws flip in fp64: pick another seed"
    assert smallest_gap >= MIN_RELATIVE_GAP, f"a draw is decided by {smallest_gap:.3e}: pick another seed"
    arrays["f64_collect_values"] = buffer64[DataKeys.VALUES].clone()
    arrays["f64_collect_logp"] = buffer64[DataKeys.LOGP].clone()
    algo64.buffer = buffer64
    algo64.state.buffered = True
    algo64.state.horizons = 1
    algo64.state.reward_scale = reward_scale
    with gf.UpdateRecorder(algo64) as urec64:
        algo64.step()
    assert len(urec64.updates) == 1 and set(urec64.first_grads) == set(urec.first_grads)
    arrays["f64_sgd1_updates"] = np.array(urec64.updates, np.float64)
    for k, gval in urec64.first_grads.items():
        assert gval.dtype == torch.float64, k
        arrays[f"f64_sgd1_grad_{k}"] = gval

    # the reference's own fp32 rounding, per quantity (printed for DESIGN.md; the test recomputes it from the arrays)
    for key in ("values", "logp"):
        a, b = arrays[f"it0_collect_{key}"].double(), arrays[f"f64_collect_{key}"]
        print(f"reference fp32 vs fp64, {key}: max |diff| {float((a - b).abs().max()):.3e}"
              f" (max |value| {float(b.abs().max()):.3e})")
    err_sq = ref_sq = 0.0
    for k, g64 in urec64.first_grads.items():
        g32 = urec.first_grads[k].double()
        err_sq += float(((g32 - g64) ** 2).sum())
        ref_sq += float((g64 ** 2).sum())
        print(f"reference fp32 vs fp64, grad {k}: max |diff| {float((g32 - g64).abs().max()):.3e}"
              f" (max |grad| {float(g64.abs().max()):.3e})")
    print(f"reference fp32 vs fp64, gradient: relative L2 {(err_sq / ref_sq) ** 0.5:.3e}")
    print("reference fp32 vs fp64, updates:", np.array(urec.updates[0]) - np.array(urec64.updates[0]))
    gf.save("first_update_ff_algotrading_transformer.npz", **arrays)


def main() -> None:
    sys.path.insert(0, HERE)
    import generate_composite_fixtures as gc
    import generate_fixtures as gf  # imports the reference (and the stubs it needs)

    gen_transformer_first_update(gf, gc)


if __name__ == "__main__":
    main()
