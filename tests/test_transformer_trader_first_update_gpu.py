"""``rl8_amd.envs.TransformerTrader`` against the reference's ``AttentiveAlpaca`` on its AlgoTrading environment
(``tests/golden/first_update_ff_algotrading_transformer.npz``; generator:
``tests/golden/generate_transformer_fixtures.py``): the reference's initial weights, reset state, categorical noise and
permutations (N = 64, H = 32, seq_len = 4) through ``collect()`` and a one-iteration ``step()`` on the window kernels,
torch's ``nn.MultiheadAttention`` and the masked-pool kernel.  The twin of ``tests/test_mlp_trader_first_update_gpu.py``.

Bars.  Actions, the action mask and ``invested`` exact -- the generator refuses to write a fixture in which a draw is
decided by less than 1e-5 relative or flips in float64, so exact actions are a fair demand; log-changes, rewards and
the reversed discounted returns at 2e-6 as for ``first_update_ff_algotrading.npz`` (tests/test_algotrading_gpu.py); the
first ``StatTracker.update`` at the project's 1e-5 (``assert_update``).  Values, log-probabilities and the gradient go
through attention, LayerNorm and BatchNorm, whose reductions are taken in another order here than on the CPU; their bar
is DESIGN.md's "3x + floor" rule: three times the reference's own fp32-against-fp64 difference of that quantity (the
fixture holds both runs) plus the floor the neighbouring tests use (rtol 1e-5 / atol 2e-6 for values and logp; 2e-5 of
a tensor's largest entry + 1e-9 per gradient tensor, 1e-5 for the whole gradient's relative L2 error).  Gradients are
compared per name as the reference recorded them (a shared attention layer is recorded once, under ``layers.0``).
Each figure is printed before it is asserted."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402

from .test_first_update_gpu import Recorder, assert_update  # noqa: E402

DEV = "cuda"
NUM_ENVS, HORIZON, SEQ_LEN = 64, 32, 4
LC, LCP = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"
SHORT = {"action_mask": "action_mask", "invested": "invested", LC: "log_change", LCP: "log_change_position",
         "position": "position", "f": "f", "k_cyclic": "k_cyclic", "k_market": "k_market", "t": "t", "price": "price"}
FIXTURE = "first_update_ff_algotrading_transformer.npz"


def build(golden):
    g = golden(FIXTURE)
    algo = AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, model_cls=TransformerTrader,
                           model_config={"seq_len": SEQ_LEN}, num_sgd_iters=1).build(AlgoTrading)
    # the reference's state_dict as it is: the shared layer under both of its names, BatchNorm buffers included (strict)
    algo.policy.model.load_state_dict({k[len("init_"):]: torch.from_numpy(g[k]) for k in g if k.startswith("init_")})
    real_reset = algo.env.reset

    def reset(*, config=None):  # the reference's reset state instead of this build's Philox draws
        real_reset(config=config)
        algo.env.load_state({key: torch.from_numpy(g[f"it0_reset_{short}"]) for key, short in SHORT.items()})
        return algo.env.observe()

    algo.env.reset = reset
    assert g["it0_cat_q"].shape == (HORIZON, NUM_ENVS, 1, 3)
    algo.injected_noise = torch.from_numpy(g["it0_cat_q"]).to(DEV)
    algo.injected_permutations = [torch.from_numpy(p) for p in g["it0_perms"]]
    return algo, g


def within_three_times_the_reference_s_rounding(got, ref32, ref64, *, rtol, atol, label):
    """|got - ref32| <= 3 max|ref32 - ref64| + (atol + rtol |ref32|), elementwise; prints the measured ratio of this
    build's deviation to the reference's own."""
    got, ref32, ref64 = (np.asarray(x, np.float64) for x in (got, ref32, ref64))
    own = float(np.abs(ref32 - ref64).max())
    err = np.abs(got - ref32)
    print(f"transformer trader first update, {label}: max deviation {float(err.max()):.3e}, the reference's fp32 vs fp64"
          f" {own:.3e}, ratio {float(err.max()) / own if own else float('inf'):.2f}")
    bound = 3.0 * own + atol + rtol * np.abs(ref32)
    assert (err <= bound).all(), (label, float(err.max()), own, float((err - bound).max()))


def timed(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        out = fn()
        return out, hip.timer.summary()
    finally:
        hip.timer.enabled = False


def test_first_update_matches_the_reference_s_attentive_alpaca(golden):
    algo, g = build(golden)
    assert not algo._identity_views() and algo._window_plan() is not None and algo._window_plan().sizes == [1, 1, 5, 1]
    stats, launched = timed(algo.collect)
    assert launched["window_last"]["launches"] == HORIZON + 1
    assert launched["masked_pool"]["launches"] == HORIZON + 1  # (the attended window, pooled once per forward pass)

    buf = algo.buffer
    assert np.array_equal(buf[DataKeys.ACTIONS][:, :HORIZON].cpu().numpy(), g["it0_collect_actions"][:, :HORIZON])
    for leaf in ("action_mask", "invested"):
        assert np.array_equal(buf[DataKeys.OBS][leaf].cpu().numpy(), g[f"it0_collect_obs_{SHORT[leaf]}"]), leaf
    for leaf in (LC, LCP):
        np.testing.assert_allclose(buf[DataKeys.OBS][leaf].cpu().numpy(), g[f"it0_collect_obs_{SHORT[leaf]}"],
                                   rtol=2e-6, atol=2e-6, err_msg=leaf)
    for key in ("rewards", "reversed_discounted_returns"):
        print(f"transformer trader first update, max deviation of {key} from the reference: "
              f"{float(np.abs(buf[key].cpu().numpy() - g[f'it0_collect_{key}']).max()):.3e}")
        np.testing.assert_allclose(buf[key].cpu().numpy(), g[f"it0_collect_{key}"], rtol=2e-6, atol=2e-6, err_msg=key)
    within_three_times_the_reference_s_rounding(
        buf[DataKeys.LOGP].cpu().numpy()[:, :HORIZON], g["it0_collect_logp"][:, :HORIZON],
        g["f64_collect_logp"][:, :HORIZON], rtol=1e-5, atol=2e-6, label="logp")
    within_three_times_the_reference_s_rounding(
        buf[DataKeys.VALUES].cpu().numpy(), g["it0_collect_values"], g["f64_collect_values"], rtol=1e-5, atol=2e-6,
        label="values")
    for k, w in zip(g["collect_stat_keys"], g["it0_collect_stats"]):
        assert stats[str(k)] == pytest.approx(w, rel=1e-5, abs=1e-5), k
    assert algo.state.reward_scale == pytest.approx(float(g["it0_reward_scale"]), rel=1e-5)

    views_all = []
    forward_backward = algo._minibatch_forward_backward
    algo._minibatch_forward_backward = lambda *a: (views_all.append(algo._views_all), forward_backward(*a))[1]
    with Recorder(algo) as rec:
        _, launched = timed(algo.step)
    assert views_all == [None]
    assert "gather_windows" in launched  # (the views of the one minibatch; no view of the whole buffer: views_all)
    assert launched["masked_pool"]["launches"] == 1 and launched["masked_pool_backward"]["launches"] == 1
    assert len(rec.updates) == 1
    print("transformer trader first update, StatTracker.update - the reference's:",
          np.array(rec.updates[0]) - g["sgd1_updates"][0], "the reference's fp32 - fp64:",
          g["sgd1_updates"][0] - g["f64_sgd1_updates"][0])
    assert_update(rec.updates[0], g["sgd1_updates"][0], "algotrading transformer trader")

    want = {k[len("sgd1_grad_"):]: g[k] for k in g if k.startswith("sgd1_grad_")}
    assert set(want) == set(rec.first_grads)
    err_sq = ref_sq = own_sq = 0.0
    for k, w in want.items():
        got = rec.first_grads[k].double().cpu().numpy()
        w64 = g[f"f64_sgd1_grad_{k}"]
        err_sq += float(((got - w) ** 2).sum())
        own_sq += float(((w.astype(np.float64) - w64) ** 2).sum())
        ref_sq += float((w.astype(np.float64) ** 2).sum())
        within_three_times_the_reference_s_rounding(got, w, w64, rtol=0.0, atol=2e-5 * float(np.abs(w).max()) + 1e-9,
                                                    label=f"grad {k}")
    err, own = (err_sq / ref_sq) ** 0.5, (own_sq / ref_sq) ** 0.5
    print(f"transformer trader first update, gradient relative L2 error {err:.3e}, the reference's fp32 vs fp64 {own:.3e},"
          f" ratio {err / own:.2f}")
    assert err < 3.0 * own + 1e-5, (err, own)
    assert ref_sq ** 0.5 == pytest.approx(float(g["sgd1_clipped_grad_norm"]), rel=1e-6)
