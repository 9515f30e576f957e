"""The wide categorical kernels against numbers the REFERENCE produced (tests/golden/wide_categorical.npz and
first_update_ff_walk100*.npz, written by tests/golden/generate_wide_categorical_fixtures.py from the unmodified
reference): picks on torch's own multinomial noise bit for bit, losses and autograd gradients at the bars of
tests/test_hip_kernels.py::test_ppo_loss_matches_reference_autograd, and a rollout and first update on a walk with
100 actions at the bars tests/test_first_update_gpu.py holds ``ff_walk4`` to."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle  # noqa: E402  (LOSS_KEYS only)

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402

from . import test_first_update_gpu as first_update  # noqa: E402
from ._envs import walk_env  # noqa: E402
from .test_algorithm_gpu import inject  # noqa: E402
from .test_hip_kernels import _hp_from, _losses_from_sums, dev, host  # noqa: E402

NUM_ENVS, HORIZON = first_update.NUM_ENVS, first_update.HORIZON


def test_sampler_picks_on_recorded_multinomial_noise_are_bit_exact(golden):
    g = golden("wide_categorical.npz")
    assert len(g["sampler_cases"]) == 6
    for case in g["sampler_cases"]:
        logits, q = dev(g[f"{case}_logits"]), dev(g[f"{case}_q"])
        assert logits.shape[-1] > hip.MAX_CLASSES
        actions, logp = hip.categorical_sample_logp_wide(logits, q)
        assert np.array_equal(host(actions), g[f"{case}_actions"]), case
        np.testing.assert_allclose(host(logp), g[f"{case}_logp"], rtol=1e-5, atol=1e-6, err_msg=case)
        mode, _ = hip.categorical_sample_logp_wide(logits, None, deterministic=True)
        assert np.array_equal(host(mode), g[f"{case}_mode"]), case


def test_loss_matches_reference_autograd(golden):
    g = golden("wide_categorical.npz")
    assert len(g["cases"]) == 6
    seen = set()
    for case in g["cases"]:
        m = g[f"{case}_values"].shape[0]
        kw, gscale = _hp_from(g[f"{case}_hparams"], m)
        seen.add((kw["dual_clip_param"] is not None, kw["entropy_coeff"] != 0))
        hp = hip.ppo_hparams(grad_scale=gscale, **kw)
        sums, g_logits, g_value = hip.ppo_loss_categorical_wide(
            dev(g[f"{case}_feat_logits"]), dev(g[f"{case}_values"]), dev(g[f"{case}_actions"]),
            dev(g[f"{case}_logp_old"]), dev(g[f"{case}_advantages"]), dev(g[f"{case}_returns"]), hp)
        np.testing.assert_allclose(host(g_logits), g[f"{case}_grad_logits"], rtol=2e-5, atol=1e-8, err_msg=case)
        np.testing.assert_allclose(host(g_value), g[f"{case}_grad_values"], rtol=2e-5, atol=1e-9, err_msg=case)
        got = _losses_from_sums(host(sums), kw)
        for i, name in enumerate(oracle.LOSS_KEYS):
            assert got[i] == pytest.approx(g[f"{case}_losses"][i], rel=1e-5, abs=1e-7), (case, name)
    assert len(seen) == 4  # plain, dual clip, entropy, both


# --------------------------------------------------------------------------- #
# walk_env(4, 100) through collect() / step()
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def walk100(golden):
    g = dict(golden("first_update_ff_walk100.npz"))
    for part in ("init", "grad", "final"):
        g.update(golden(f"first_update_ff_walk100_{part}.npz"))
    assert float(g["min_top_two_gap"]) > 1e-4  # no recorded draw is a near tie: the actions are held bit for bit
    return g


def build(g, **overrides):
    algo = AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, **overrides).build(walk_env(4, 100))
    algo.policy.model.load_state_dict({k[len("init_"):]: torch.from_numpy(g[k]) for k in g if k.startswith("init_")})
    inject(algo, g, 0)
    return algo


def test_rollout_matches_reference(walk100):
    """tests/test_first_update_gpu.py::test_env_rollout_matches_reference, on the 100-action walk."""
    g = walk100
    algo = build(g)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = algo.collect()
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert launched["categorical_sample_logp_wide"]["launches"] == HORIZON
    buf = algo.buffer
    assert np.array_equal(buf[DataKeys.ACTIONS][:, :HORIZON].cpu().numpy(), g["it0_collect_actions"][:, :HORIZON])
    assert g["it0_collect_actions"].max() >= 64
    for key in ("obs", "rewards", "reversed_discounted_returns"):
        np.testing.assert_allclose(buf[key].cpu().numpy(), g[f"it0_collect_{key}"], rtol=2e-6, atol=2e-6, err_msg=key)
    np.testing.assert_allclose(buf[DataKeys.LOGP].cpu().numpy()[:, :HORIZON], g["it0_collect_logp"][:, :HORIZON],
                               rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(buf[DataKeys.VALUES].cpu().numpy(), g["it0_collect_values"], rtol=1e-5, atol=2e-6)
    for k, w in zip(g["collect_stat_keys"], g["it0_collect_stats"]):
        assert stats[str(k)] == pytest.approx(w, rel=1e-5, abs=1e-5), k
    assert algo.state.reward_scale == pytest.approx(float(g["it0_reward_scale"]), rel=1e-5)


def test_one_sgd_iteration_matches_reference_to_1e5(walk100):
    """tests/test_first_update_gpu.py::check_one_sgd_iteration, on the 100-action walk: StepStats, the clipped
    gradient of the optimizer step and the weights after it."""
    g = walk100
    REL, ABS = first_update.REL, first_update.ABS
    algo = build(g, num_sgd_iters=1, sgd_minibatch_size=None)
    algo.collect()
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        with first_update.Recorder(algo) as rec:
            stats = algo.step()
        launched = set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert "ppo_loss_categorical_wide" in launched and "ppo_loss_categorical" not in launched, launched
    assert len(rec.updates) == 1
    first_update.assert_update(rec.updates[0], g["sgd1_updates"][0], "ff_walk100")
    for k, w in zip(g["step_stat_keys"], g["sgd1_step_stats"]):
        assert stats[str(k)] == pytest.approx(w, rel=REL, abs=ABS.get(str(k), 1e-9)), k
    want = {k[len("sgd1_grad_"):]: g[k] for k in g if k.startswith("sgd1_grad_")}
    assert set(want) == set(rec.first_grads)
    err_sq = ref_sq = 0.0
    for k, w in want.items():
        got = rec.first_grads[k].double().cpu().numpy()
        err_sq += float(((got - w) ** 2).sum())
        ref_sq += float((w.astype(np.float64) ** 2).sum())
        np.testing.assert_allclose(got, w, rtol=0, atol=2e-5 * float(np.abs(w).max()) + 1e-9, err_msg=k)
    assert (err_sq / ref_sq) ** 0.5 < 1e-5, (err_sq / ref_sq) ** 0.5
    assert ref_sq ** 0.5 == pytest.approx(float(g["sgd1_clipped_grad_norm"]), rel=1e-6)
    lr = 1e-3
    for k, p in algo.policy.model.named_parameters():
        w, gw = g[f"sgd1_final_{k}"], want[k]
        solid = np.abs(gw) > 1e-3 * np.abs(gw).max()
        np.testing.assert_allclose(p.detach().cpu().numpy()[solid], w[solid], rtol=0, atol=0.02 * lr,
                                   err_msg=f"weights {k}")


def test_first_minibatch_of_traced_config_matches_reference_to_1e5(walk100):
    """tests/test_first_update_gpu.py::test_first_minibatch_of_traced_config_matches_reference_to_1e5."""
    g = walk100
    algo = build(g)
    algo.collect()
    with first_update.Recorder(algo) as rec:
        algo.step()
    want = g["traced_updates"]
    assert len(rec.updates) == len(want)
    first_update.assert_update(rec.updates[0], want[0], "ff_walk100")
    got = np.array(rec.updates)
    assert np.array_equal(got[:, -1], want[:, -1])
    np.testing.assert_allclose(got[1:, :-1], want[1:, :-1], rtol=2e-2, atol=2e-3)
