"""``rl8_amd.envs.algotrading.AlgoTrading`` against the reference's environment (``tests/golden/
algotrading_env_steps.npz``, ``first_update_ff_algotrading.npz``; generator: ``tests/golden/
generate_composite_fixtures.py``) and against itself at the kernels' edges."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.envs import AlgoTrading  # noqa: E402
from rl8_amd.models import Model  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402
from rl8_amd.views import ViewRequirement  # noqa: E402

from .test_first_update_gpu import Recorder, assert_update  # noqa: E402

DEV = "cuda"
LC, LCP = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"
#: fixture member names of the reference's state keys
SHORT = {"action_mask": "action_mask", "invested": "invested", LC: "log_change", LCP: "log_change_position",
         "position": "position", "f": "f", "k_cyclic": "k_cyclic", "k_market": "k_market", "t": "t", "price": "price"}
LEAVES = ("action_mask", "invested", LC, LCP)
EDGE_SIZES = [1, 255, 256, 257, 4099]
FINFO = torch.finfo(torch.float32)


class MaskedTrader(Model):
    """The twin of the generator's model (tests/golden/generate_composite_fixtures.py, same parameter names) against
    this package's ``Model``: an embedding of ``invested`` next to the two log-changes, one hidden layer each for
    policy and value, logits plus ``clamp(log(action_mask), finfo.min, finfo.max)``.  ``window > 0`` reads the newest
    entry of a tuple-key rolling window of the price changes: the same function through the windowed route."""

    def __init__(self, observation_spec, action_spec, /, embed_dim=2, hidden=64, window=0):
        super().__init__(observation_spec, action_spec, embed_dim=embed_dim, hidden=hidden, window=window)
        self.window = window
        if window:
            self.view_requirements[(DataKeys.OBS, LC)] = ViewRequirement(shift=window)
        self.invested_embedding = nn.Embedding(2, embed_dim)
        self.policy_hidden = nn.Linear(embed_dim + 2, hidden)
        self.policy_head = nn.Linear(hidden, 3)
        self.value_hidden = nn.Linear(embed_dim + 2, hidden)
        self.value_head = nn.Linear(hidden, 1)
        self._value = None

    def forward(self, batch, /):
        obs = batch[DataKeys.OBS]
        log_change = obs[LC]
        if self.window:
            log_change = log_change[DataKeys.INPUTS][:, -1]
        x = torch.cat([self.invested_embedding(obs["invested"].flatten()), log_change, obs[LCP]], dim=-1)
        logits = self.policy_head(torch.relu(self.policy_hidden(x)))
        logits = logits + torch.clamp(torch.log(obs["action_mask"].to(torch.float32)), FINFO.min, FINFO.max)
        self._value = self.value_head(torch.relu(self.value_hidden(x)))
        return TensorDict({"logits": logits.reshape(-1, 1, 3)}, batch_size=batch.batch_size, device=logits.device)

    def value_function(self):
        return self._value


# --------------------------------------------------------------------------- #
# Step parity against the reference env.
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def stepped(golden):
    """Every (state, action) of the fixture -- 128 steps x 16 envs -- through ONE launch of the step kernel: the
    fixture, the kernel's outputs and the fp64 evaluation of the same fp32 inputs, shared by the tests below."""
    g = golden("algotrading_env_steps.npz")
    m = g["actions"].size
    before = {key: torch.from_numpy(g[f"before_{short}"].reshape(m, -1)) for key, short in SHORT.items()}
    env = AlgoTrading(m, device=DEV)
    env.load_state(before)
    out = env.step(torch.from_numpy(g["actions"].reshape(m, 1)).to(DEV))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in env.state_dict().items()}
    obs = {k: out[DataKeys.OBS][k].cpu().numpy() for k in LEAVES}
    reward = out[DataKeys.REWARDS].cpu().numpy()
    want = {key: g[f"after_{short}"].reshape(m, -1) for key, short in SHORT.items()}

    # fp64 evaluation of the fixture's fp32 inputs (examples/algotrading/env.py:131-183)
    b = {k: v.numpy().astype(np.float64) for k, v in before.items() if k != "action_mask"}
    a = g["actions"].reshape(m, 1)
    old = b["price"]
    inv = np.where(a == 1, 1.0, np.where(a == 2, 0.0, b["invested"]))
    pos = np.where(a == 1, old, b["position"])
    with np.errstate(divide="ignore"):
        r64 = np.where(a == 2, np.log(old) - np.log(pos), 0.0)
    pos = np.where(inv == 1, pos, old)
    r64 = np.where((inv == 1) & (a == 0), b[LC], r64)
    price = old * ((1 + b["k_market"]) * (1 + b["k_cyclic"] * np.sin((b["t"] + 1) * b["f"])))
    exact = {"price": price, LC: np.log(price) - np.log(old), LCP: np.log(price) - np.log(pos), "reward": r64}
    return dict(g=g, m=m, got=got, obs=obs, reward=reward, want=want, want_reward=g["rewards"].reshape(m, 1), exact=exact)


def test_step_matches_the_reference_env(stepped):
    """invested, t and the mask exact; price at rtol 1e-6; the log-changes and the reward at atol 1e-5 -- the
    reference's own fp32 error against fp64 over 128 steps x 4096 envs is 2.2e-7 relative in price, 1.4e-6 in the
    log-changes and 1.1e-6 in the reward, the bars about five times that.  position, f and the k's are copies: exact.
    The fixture covers all three actions from both invested states (so forbidden ones) and SELLs on a fresh reset's
    position of 0, where the reward is +inf here as there."""
    s = stepped
    got, want, g = s["got"], s["want"], s["g"]
    inv, act = g["before_invested"].reshape(-1), g["actions"].reshape(-1)
    for i in (0, 1):
        for a in (0, 1, 2):
            assert ((inv == i) & (act == a)).any(), (i, a)
    fresh_sell = (g["before_position"].reshape(-1) == 0) & (act == 2)
    assert fresh_sell.any() and np.isposinf(s["want_reward"].reshape(-1)[fresh_sell]).all()
    assert np.isposinf(s["reward"].reshape(-1)[fresh_sell]).all()

    for key in ("invested", "t", "action_mask", "position", "f", "k_cyclic", "k_market"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(s["obs"]["action_mask"], want["action_mask"]) and s["obs"]["action_mask"].dtype == np.bool_
    assert np.array_equal(s["obs"]["invested"], want["invested"]) and s["obs"]["invested"].dtype == np.int64
    np.testing.assert_allclose(got["price"], want["price"], rtol=1e-6, atol=0)
    for key in (LC, LCP):
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=1e-5, err_msg=key)
        assert np.array_equal(s["obs"][key], got[key]), key  # (the observation is the state's leaf)
    assert np.array_equal(np.isposinf(s["reward"]), np.isposinf(s["want_reward"]))
    np.testing.assert_allclose(s["reward"], s["want_reward"], rtol=0, atol=1e-5)


def test_step_error_against_fp64_is_within_three_times_the_reference_s(stepped):
    """Against an fp64 evaluation of the fixture's fp32 inputs the kernel may err at most 3x as far as the reference's
    own fp32 results do (its error on this fixture is the floor of the bar).  The measured maxima are in DESIGN.md
    section 5; the test prints them before it asserts."""
    s = stepped
    finite = np.isfinite(s["exact"]["reward"])
    assert np.array_equal(finite, np.isfinite(s["want_reward"]))

    def errors(price, lc, lcp, reward):
        e = s["exact"]
        return {
            "price (relative)": float(np.max(np.abs(price - e["price"]) / e["price"])),
            "log-changes": float(max(np.max(np.abs(lc - e[LC])), np.max(np.abs(lcp - e[LCP])))),
            "reward": float(np.max(np.abs(reward[finite] - e["reward"][finite]))),
        }

    ref = errors(s["want"]["price"], s["want"][LC], s["want"][LCP], s["want_reward"])
    got = errors(s["got"]["price"], s["got"][LC], s["got"][LCP], s["reward"])
    for k in ref:
        print(f"algotrading step, max error against fp64, {k}: kernel {got[k]:.3e}, reference {ref[k]:.3e}")
    for k in ref:
        assert ref[k] > 0 and got[k] <= 3 * ref[k], (k, got[k], ref[k])


# --------------------------------------------------------------------------- #
# Kernel edges.
# --------------------------------------------------------------------------- #
def _warm_env(n: int, steps: int = 3) -> AlgoTrading:
    """``n`` envs a few random steps past a reset: both invested states, positions, non-zero log-changes."""
    env = AlgoTrading(n, device=DEV)
    env.seed, env.reset_count = 99, 3
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(17)
    for _ in range(steps):
        env.step(torch.randint(0, 3, (n, 1), device=DEV, generator=g))
    return env


@pytest.fixture(scope="module")
def big():
    """One 8192-env batch (state before, action, outputs and state after one step) the smaller runs are compared with."""
    n = 8192
    env = _warm_env(n)
    before = {k: v.clone() for k, v in env.state_dict().items()}
    action = torch.randint(0, 3, (n, 1), device=DEV, generator=torch.Generator(device=DEV).manual_seed(23))
    out = env.step(action)
    assert before["invested"].sum() not in (0, n)
    return dict(before=before, action=action, obs=out[DataKeys.OBS], reward=out[DataKeys.REWARDS], after=env.state_dict())


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_step_does_not_depend_on_the_grid(big, n):
    env = AlgoTrading(n, device=DEV)
    env.load_state({k: v[:n] for k, v in big["before"].items()})
    for k, v in env.state_dict().items():  # load_state / state_dict round-trip
        assert torch.equal(v, big["before"][k][:n]), k
    out = env.step(big["action"][:n].contiguous())
    for k in LEAVES:
        assert torch.equal(out[DataKeys.OBS][k], big["obs"][k][:n]), k
    assert torch.equal(out[DataKeys.REWARDS].view(torch.int32), big["reward"][:n].view(torch.int32))
    for k, v in env.state_dict().items():
        assert torch.equal(v, big["after"][k][:n]), k


def _masked_logits(env: AlgoTrading, g: torch.Generator) -> torch.Tensor:
    mask = env.observe()["action_mask"]
    logits = torch.randn(env.num_envs, 3, device=DEV, generator=g) * 2
    return (logits + torch.clamp(torch.log(mask.to(torch.float32)), FINFO.min, FINFO.max)).reshape(-1, 1, 3)


@pytest.mark.parametrize("injected", [True, False])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_fused_step_equals_sampler_plus_step_plus_bookkeeping(big, n, injected):
    """``rl8_rollout_step_algotrading_f32`` writes, bit for bit, what ``categorical_sample_logp`` +
    ``algotrading_step`` + ``rollout_scatter_leaves`` write -- with injected noise and with the Philox stream's --
    and with masked logits never draws a forbidden class."""
    g = torch.Generator(device=DEV).manual_seed(100 + n)
    fused_env, env = AlgoTrading(n, device=DEV), AlgoTrading(n, device=DEV)
    start = {k: v[:n] for k, v in big["before"].items()}
    fused_env.load_state(start), env.load_state(start)
    logits = _masked_logits(env, g)
    noise = torch.empty(n, 1, 3, device=DEV).exponential_(generator=g) if injected else None
    value, rdr_t = torch.randn(n, 1, device=DEV, generator=g), torch.randn(n, 1, device=DEV, generator=g)
    gamma, seed, step, offset = 0.95, 1234, 5, 7
    mask_before = env.observe()["action_mask"]

    def columns():
        obs = {key: torch.zeros(n, d, dtype=dtype, device=DEV) for key, dtype, d in hip.ALGOTRADING_LEAVES}
        return (torch.full((n, 1), -1, dtype=torch.int64, device=DEV),
                *(torch.full((n, 1), float("nan"), device=DEV) for _ in range(4)), obs)

    fa, fl, fv, fr, frdr, fobs = columns()
    fused_env.fused_rollout_step(
        squashed=False, features=logits, features2=None, value=value, noise=noise, action_col=fa, logp_col=fl,
        value_col=fv, reward_col=fr, obs_col_next=fobs, rdr_t=rdr_t, rdr_t1=frdr, gamma=gamma, seed=seed, step=step,
        env_offset=offset, deterministic=False)

    actions, logp = hip.categorical_sample_logp(logits, noise, seed=seed, step=step, row_offset=offset)
    out = env.step(actions)
    ca, cl, cv, cr, crdr, cobs = columns()
    hip.rollout_scatter_leaves(actions, logp, value, out[DataKeys.REWARDS], [out[DataKeys.OBS][k] for k in LEAVES],
                               ca, cl, cv, cr, [cobs[k] for k in LEAVES], rdr_t, crdr, gamma)
    torch.cuda.synchronize()
    assert torch.equal(fa, ca)
    for name, a, b in (("logp", fl, cl), ("value", fv, cv), ("reward", fr, cr), ("rdr", frdr, crdr)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    for k in LEAVES:
        assert torch.equal(fobs[k], cobs[k]), k
    for (k, a), b in zip(fused_env.state_dict().items(), env.state_dict().values()):
        assert torch.equal(a, b), k
    assert bool(mask_before.gather(1, fa).all()), "a forbidden action was drawn from masked logits"
    assert torch.isfinite(fl).all() and torch.isfinite(fr).all()


def test_deterministic_fused_step_takes_the_allowed_mode():
    n = 257
    env = _warm_env(n)
    logits = _masked_logits(env, torch.Generator(device=DEV).manual_seed(4))
    mask = env.observe()["action_mask"]
    cols = [torch.empty(n, 1, device=DEV) for _ in range(3)]
    action = torch.empty(n, 1, dtype=torch.int64, device=DEV)
    obs = {key: torch.zeros(n, d, dtype=dtype, device=DEV) for key, dtype, d in hip.ALGOTRADING_LEAVES}
    env.fused_rollout_step(squashed=False, features=logits, features2=None, value=torch.zeros(n, 1, device=DEV),
                           noise=None, action_col=action, logp_col=cols[0], value_col=cols[1], reward_col=cols[2],
                           obs_col_next=obs, rdr_t=None, rdr_t1=None, gamma=0.9, seed=1, step=0, env_offset=0,
                           deterministic=True)
    assert torch.equal(action, logits.reshape(n, 3).argmax(-1, keepdim=True)) and bool(mask.gather(1, action).all())


# --------------------------------------------------------------------------- #
# Reset.
# --------------------------------------------------------------------------- #
def _reset(n: int, *, reset_count: int = 0, env_offset: int = 0, config=None):
    env = AlgoTrading(n, device=DEV)
    env.seed, env.reset_count, env.env_offset = 2024, reset_count, env_offset
    obs = env.reset(config=config)
    return env, obs


def test_reset_draws_the_reference_s_ranges():
    n = 4099
    env, obs = _reset(n)
    s = env.state_dict()
    assert env.reset_count == 1
    assert bool(((s["f"] >= 0) & (s["f"] <= math.pi)).all()) and float(s["f"].max()) > 0.99 * math.pi
    for k in ("k_cyclic", "k_market"):
        assert bool((s[k].abs() <= 0.05).all()) and float(s[k].min()) < -0.049 and float(s[k].max()) > 0.049, k
    assert s["t"].dtype == torch.int64 and sorted(s["t"].unique().tolist()) == list(range(10))
    assert bool(((s["price"] >= 100) & (s["price"] <= 10000)).all())
    assert float(s["price"].min()) < 200 and float(s["price"].max()) > 9900
    for k in ("invested", "position", LC, LCP):
        assert not s[k].any(), k
    want_mask = torch.tensor([True, True, False], device=DEV).expand(n, 3)
    assert torch.equal(obs["action_mask"], want_mask) and torch.equal(s["action_mask"], want_mask)
    assert obs["invested"].dtype == torch.int64 and not obs["invested"].any() and not obs[LC].any() and not obs[LCP].any()
    env.observation_spec.assert_is_in(obs)
    # independent draws: no two of the four uniform fields are the same numbers rescaled
    u = torch.stack([s["f"] / math.pi, s["k_cyclic"] / 0.1 + 0.5, s["k_market"] / 0.1 + 0.5, (s["price"] - 100) / 9900])
    corr = torch.corrcoef(u.reshape(4, n).double())
    assert float((corr - torch.eye(4, device=DEV)).abs().max()) < 0.06  # (4 sigma of 1 / sqrt(4099))

    bounds = {"f_bounds": 1.0, "k_cyclic_bounds": 0.01, "k_market_bounds": 0.2}
    env2, _ = _reset(n, config=bounds)
    s2 = env2.state_dict()
    assert float(s2["f"].max()) <= 1.0 and float(s2["k_cyclic"].abs().max()) <= 0.01
    assert 0.19 < float(s2["k_market"].abs().max()) <= 0.2
    assert (env2.f_bounds, env2.k_cyclic_bounds, env2.k_market_bounds) == (1.0, 0.01, 0.2)


def test_reset_is_keyed_by_seed_count_and_offset():
    n = 4099
    base = _reset(n)[0].state_dict()
    again = _reset(n)[0].state_dict()
    later = _reset(n, reset_count=1)[0].state_dict()
    shifted = _reset(n, env_offset=5)[0].state_dict()
    for k in ("f", "k_cyclic", "k_market", "t", "price"):
        assert torch.equal(base[k], again[k]), k
        assert not torch.equal(base[k], later[k]), k
        assert not torch.equal(base[k], shifted[k]), k
        assert torch.equal(base[k][5:], shifted[k][:-5]), k  # (env i of the shard is global env i + offset)


# --------------------------------------------------------------------------- #
# First update against the reference.
# --------------------------------------------------------------------------- #
NUM_ENVS, HORIZON = 64, 32


def _build(golden, window: int, **overrides):
    g = golden("first_update_ff_algotrading.npz")
    algo = AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, model_cls=MaskedTrader,
                           model_config={"window": window}, **overrides).build(AlgoTrading)
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


@pytest.mark.parametrize("window", [0, 3], ids=["identity-views", "tuple-key-window"])
def test_first_update_matches_the_reference(golden, window):
    """The reference's initial weights, reset state, categorical noise and permutations (N = 64, H = 32) through
    collect() and a one-iteration step(), at the bars of tests/test_first_update_gpu.py for the classic envs: actions
    exact, observations / rewards / rdr at 2e-6, logp / values at rtol 1e-5, the first StatTracker.update and the
    first gradient at 1e-5.  Identity views run the fused per-timestep kernel; the tuple-key window (the same function
    of the buffer, as the generator asserts of the reference) the generic route with the several-leaf bookkeeping."""
    algo, g = _build(golden, window, num_sgd_iters=1)
    assert algo._identity_views() == (window == 0) and algo._fusable() == (window == 0)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = algo.collect()
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
    if window == 0:
        assert launched["rollout_step_algotrading"]["launches"] == HORIZON and "rollout_scatter_leaves" not in launched
    else:
        assert launched["rollout_scatter_leaves"]["launches"] == HORIZON and "rollout_step_algotrading" not in launched
        assert launched["algotrading_step"]["launches"] == HORIZON

    buf = algo.buffer
    assert np.array_equal(buf[DataKeys.ACTIONS][:, :HORIZON].cpu().numpy(), g["it0_collect_actions"][:, :HORIZON])
    for leaf in ("action_mask", "invested"):
        assert np.array_equal(buf[DataKeys.OBS][leaf].cpu().numpy(), g[f"it0_collect_obs_{SHORT[leaf]}"]), leaf
    for leaf in (LC, LCP):
        np.testing.assert_allclose(buf[DataKeys.OBS][leaf].cpu().numpy(), g[f"it0_collect_obs_{SHORT[leaf]}"],
                                   rtol=2e-6, atol=2e-6, err_msg=leaf)
    for key in ("rewards", "reversed_discounted_returns"):
        print(f"algotrading first update (window={window}), max deviation of {key} from the reference: "
              f"{float(np.abs(buf[key].cpu().numpy() - g[f'it0_collect_{key}']).max()):.3e}")
        np.testing.assert_allclose(buf[key].cpu().numpy(), g[f"it0_collect_{key}"], rtol=2e-6, atol=2e-6, err_msg=key)
    np.testing.assert_allclose(buf[DataKeys.LOGP].cpu().numpy()[:, :HORIZON], g["it0_collect_logp"][:, :HORIZON],
                               rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(buf[DataKeys.VALUES].cpu().numpy(), g["it0_collect_values"], rtol=1e-5, atol=2e-6)
    for k, w in zip(g["collect_stat_keys"], g["it0_collect_stats"]):
        assert stats[str(k)] == pytest.approx(w, rel=1e-5, abs=1e-5), k
    assert algo.state.reward_scale == pytest.approx(float(g["it0_reward_scale"]), rel=1e-5)

    with Recorder(algo) as rec:
        algo.step()
    assert len(rec.updates) == 1
    assert_update(rec.updates[0], g["sgd1_updates"][0], f"algotrading window={window}")
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
