"""Dict (``Composite``) observations through the feed-forward ``Algorithm``: the per-leaf buffer, the rollout
bookkeeping launch for several leaves (``rl8_rollout_scatter_leaves_f32``), the view minibatches, and what stays
refused (recurrent + composite, composite action specs)."""

from __future__ import annotations

from typing import Any

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, RecurrentAlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.env import Env  # noqa: E402
from rl8_amd.models import DefaultDiscreteModel, Model  # noqa: E402
from rl8_amd.specs import Categorical, Composite, Unbounded  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402
from rl8_amd.views import ViewRequirement  # noqa: E402

DEV = "cuda"
LEAVES = ("x", "count", "flags")


class DictEnv(Env):
    """Leaves f32[2], int64[1] and bool[3]; keeps every observation it returns."""

    def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
        super().__init__(num_envs, horizon, device=device)
        self.observation_spec = Composite({
            "x": Unbounded(2, device=device),
            "count": Categorical(1 << 20, shape=torch.Size([1]), device=device, dtype=torch.int64),
            "flags": Categorical(2, shape=torch.Size([3]), device=device, dtype=torch.bool),
        })
        self.action_spec = Categorical(2, shape=torch.Size([1]), device=device)
        self.resets: list[TensorDict] = []
        self.steps: list[TensorDict] = []

    def _obs(self, action: torch.Tensor) -> TensorDict:
        flags = torch.cat([self.x > 0, action == 1], dim=1)
        return TensorDict({"x": self.x.clone(), "count": self.count.clone(), "flags": flags}, batch_size=self.num_envs,
                          device=self.device)

    def reset(self, *, config: None | dict[str, Any] = None) -> TensorDict:
        start = 0.25 * len(self.resets)
        self.x = torch.linspace(-1.5 + start, 1.0 + start, 2 * self.num_envs, device=self.device).reshape(-1, 2)
        self.count = torch.full((self.num_envs, 1), 7 * len(self.resets), dtype=torch.int64, device=self.device)
        obs = self._obs(torch.zeros(self.num_envs, 1, dtype=torch.int64, device=self.device))
        self.resets.append(obs.clone())
        return obs

    def step(self, action: torch.Tensor) -> TensorDict:
        self.x = 0.5 * self.x + (2 * action - 1).to(torch.float32)
        self.count = self.count + 1 + action
        obs = self._obs(action)
        self.steps.append(obs.clone())
        return TensorDict({DataKeys.OBS: obs, DataKeys.REWARDS: -self.x.abs().sum(-1, keepdim=True)},
                          batch_size=self.num_envs, device=self.device)


class DictModel(Model):
    """Reads every leaf; ``window > 0`` takes the last ``window + 1`` values of ``x`` through a tuple-key view."""

    def __init__(self, observation_spec, action_spec, /, window: int = 0) -> None:
        super().__init__(observation_spec, action_spec, window=window)
        self.window = window
        if window:
            self.view_requirements[(DataKeys.OBS, "x")] = ViewRequirement(shift=window)
        self.body = nn.Linear(2 * (window + 1) + 1 + 3, 16)
        self.head = nn.Linear(16, 2)
        self.vf = nn.Linear(16, 1)
        self._value = None

    def forward(self, batch: TensorDict, /) -> TensorDict:
        obs = batch[DataKeys.OBS]
        x = obs["x"]
        if self.window:
            assert x[DataKeys.PADDING_MASK].shape == (batch.batch_size[0], self.window + 1)
            x = x[DataKeys.INPUTS].flatten(start_dim=1)
        z = torch.relu(self.body(torch.cat([x, obs["count"].to(torch.float32) * 0.01, obs["flags"].to(torch.float32)], -1)))
        self._value = self.vf(z)
        return TensorDict({"logits": self.head(z).reshape(-1, 1, 2)}, batch_size=batch.batch_size, device=z.device)

    def value_function(self) -> torch.Tensor:
        return self._value


def test_dict_observations_build_collect_and_step():
    """Fails without the feature (``_allocate_buffer`` refused every Composite observation spec).  After collect()
    column t + 1 of every leaf is, bit for bit, what the env returned at step t; column 0 the reset output."""
    torch.manual_seed(0)
    n, h = 8, 4
    algo = AlgorithmConfig(num_envs=n, horizon=h, model_cls=DictModel, horizons_per_env_reset=2).build(DictEnv)
    env = algo.env
    assert algo._identity_views()
    assert algo.buffer[DataKeys.OBS].batch_size == torch.Size([n, h + 1])
    for leaf, dtype, width in (("x", torch.float32, 2), ("count", torch.int64, 1), ("flags", torch.bool, 3)):
        got = algo.buffer[DataKeys.OBS][leaf]
        assert got.shape == (n, h + 1, width) and got.dtype == dtype
        assert algo._tm_obs[leaf].is_contiguous() and algo._tm_obs[leaf].shape == (h + 1, n, width)  # time-major slabs
    env.resets.clear(), env.steps.clear()  # (validate() stepped the env once)

    stats = algo.collect()
    assert stats["env/resets"] == n and len(env.resets) == 1 and len(env.steps) == h
    for leaf in LEAVES:
        col = algo.buffer[DataKeys.OBS][leaf]
        assert torch.equal(col[:, 0], env.resets[0][leaf]), leaf
        for t in range(h):
            assert torch.equal(col[:, t + 1], env.steps[t][leaf]), (leaf, t)
    last = {leaf: algo.buffer[DataKeys.OBS][leaf][:, h].clone() for leaf in LEAVES}
    step_stats = algo.step()
    assert all(torch.isfinite(torch.tensor(step_stats[k])) for k in ("losses/policy", "losses/vf", "losses/total"))
    for leaf in LEAVES:  # the flat rule per leaf: columns 0 .. H-1 zeroed, column H kept
        col = algo.buffer[DataKeys.OBS][leaf]
        assert not col[:, :h].any() and torch.equal(col[:, h], last[leaf]), leaf

    # second collect() of the same episode: no reset, column 0 is the previous column H
    stats = algo.collect()
    assert stats["env/resets"] == 0 and len(env.resets) == 1 and len(env.steps) == 2 * h
    for leaf in LEAVES:
        col = algo.buffer[DataKeys.OBS][leaf]
        assert torch.equal(col[:, 0], last[leaf]), leaf
        for t in range(h):
            assert torch.equal(col[:, t + 1], env.steps[h + t][leaf]), (leaf, t)
    algo.step()
    algo.collect()  # ... and the third resets again
    assert len(env.resets) == 2
    assert torch.equal(algo.buffer[DataKeys.OBS]["x"][:, 0], env.resets[1]["x"])


def _offset_like(src: torch.Tensor, offset: int) -> tuple[torch.Tensor, torch.Tensor]:
    """A destination for ``src`` that starts ``offset`` bytes into a 16-byte aligned allocation of 0xA5 bytes."""
    nbytes = src.numel() * src.element_size()
    raw = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0 and offset % src.element_size() == 0
    dst = raw[offset:offset + nbytes].view(src.dtype).reshape(src.shape)
    return raw, dst


@pytest.mark.parametrize("with_rdr", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_scatter_leaves_copies_every_leaf_bit_for_bit(n, with_rdr):
    """Rows of 1, 3, 4, 8 and 20 bytes, destinations 0 / 1 / 3 / 4 / 8 bytes past a 16-byte boundary (so the 16-, 8-,
    4- and 1-byte copies all occur over the five sizes), nothing written outside them; the five other columns as
    ``hip.rollout_scatter`` writes them."""
    g = torch.Generator(device=DEV).manual_seed(n)
    leaves = [
        (torch.rand(n, 1, device=DEV, generator=g) > 0.5, 1),                                     # 1-byte rows
        (torch.rand(n, 3, device=DEV, generator=g) > 0.5, 3),                                     # bool[3]
        (torch.randn(n, 1, device=DEV, generator=g), 4),                                          # 4-byte rows
        (torch.randint(-(1 << 40), 1 << 40, (n, 1), device=DEV, generator=g), 8),                 # 8-byte rows
        (torch.randn(n, 5, device=DEV, generator=g), 0),                                          # 20-byte rows, aligned
        (torch.randn(n, 5, device=DEV, generator=g), 4),                                          # 20-byte rows, offset
    ]
    action = torch.randint(0, 3, (n, 1), device=DEV, generator=g)
    logp, value, reward = (torch.randn(n, 1, device=DEV, generator=g) for _ in range(3))
    rdr_t = torch.randn(n, 1, device=DEV, generator=g) if with_rdr else None
    gamma = 0.95

    def columns():
        return (torch.full_like(action, -1), *(torch.full_like(logp, float("nan")) for _ in range(3)),
                torch.full_like(logp, float("nan")) if with_rdr else None)

    dsts = [_offset_like(src, off) for src, off in leaves]
    a_col, l_col, v_col, r_col, rdr_t1 = columns()
    hip.rollout_scatter_leaves(action, logp, value, reward, [src for src, _ in leaves], a_col, l_col, v_col, r_col,
                               [dst for _, dst in dsts], rdr_t, rdr_t1, gamma)
    # the reference columns: the single-slab entry on a float observation of its own
    obs = torch.randn(n, 2, device=DEV, generator=g)
    wa, wl, wv, wr, wrdr = columns()
    obs_next = torch.empty_like(obs)
    hip.rollout_scatter(action, logp, value, reward, obs, wa, wl, wv, wr, obs_next, rdr_t, wrdr, gamma)
    torch.cuda.synchronize()
    assert torch.equal(a_col, wa) and torch.equal(a_col, action)
    for got, want, src in ((l_col, wl, logp), (v_col, wv, value), (r_col, wr, reward)):
        assert torch.equal(got, want) and torch.equal(got, src)
    if with_rdr:
        assert torch.equal(rdr_t1.view(torch.int32), wrdr.view(torch.int32))
    for (src, off), (raw, dst) in zip(leaves, dsts):
        nbytes = src.numel() * src.element_size()
        assert torch.equal(dst.contiguous().view(torch.uint8).reshape(-1), src.view(torch.uint8).reshape(-1)), (src.dtype, off)
        assert bool((raw[:off] == 0xA5).all()) and bool((raw[off + nbytes:] == 0xA5).all()), (src.dtype, off)


def test_scatter_leaves_wrapper_refuses_mismatched_leaves():
    n = 4
    f = torch.zeros(n, 1, device=DEV)
    a = torch.zeros(n, 1, dtype=torch.int64, device=DEV)
    args = (a, f, f, f)
    cols = (a.clone(), f.clone(), f.clone(), f.clone())
    with pytest.raises(ValueError):
        hip.rollout_scatter_leaves(*args, [f], *cols, [torch.zeros(n, 2, device=DEV)], None, None, 0.9)
    with pytest.raises(ValueError):
        hip.rollout_scatter_leaves(*args, [f], *cols, [a.clone()], None, None, 0.9)
    with pytest.raises(ValueError):
        hip.rollout_scatter_leaves(*args, [], *cols, [], None, None, 0.9)
    with pytest.raises(ValueError):
        hip.rollout_scatter_leaves(*args, [f] * 9, *cols, [f.clone() for _ in range(9)], None, None, 0.9)


def line_env(composite: bool) -> type[Env]:
    """``DiscreteDummyEnv``'s arithmetic in Python (no ``fused_rollout_step``): ``state += 2 a - 1``, reward
    ``-|state|``; the observation is the state, alone or next to a bool leaf."""

    class Line(Env):
        def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
            super().__init__(num_envs, horizon, device=device)
            state = Unbounded(1, device=device)
            flag = Categorical(2, shape=torch.Size([1]), device=device, dtype=torch.bool)
            self.observation_spec = Composite({"state": state, "flag": flag}) if composite else state
            self.action_spec = Categorical(2, shape=torch.Size([1]), device=device)

        def _obs(self):
            if not composite:
                return self.state.clone()
            return TensorDict({"state": self.state.clone(), "flag": self.state > 0}, batch_size=self.num_envs,
                              device=self.device)

        def reset(self, *, config: None | dict[str, Any] = None):
            self.state = torch.linspace(-3.0, 3.0, self.num_envs, device=self.device).reshape(-1, 1)
            return self._obs()

        def step(self, action: torch.Tensor) -> TensorDict:
            self.state = self.state + (2 * action - 1).to(torch.float32)
            return TensorDict({DataKeys.OBS: self._obs(), DataKeys.REWARDS: -self.state.abs()},
                              batch_size=self.num_envs, device=self.device)

    return Line


class StateOnly(DefaultDiscreteModel):
    """The default towers on the ``"state"`` leaf (or on a tensor observation as it is)."""

    def __init__(self, observation_spec, action_spec, /, **config: Any) -> None:
        leaf = observation_spec["state"] if isinstance(observation_spec, Composite) else observation_spec
        super().__init__(leaf, action_spec, **config)

    def forward(self, batch: TensorDict, /) -> TensorDict:
        obs = batch[DataKeys.OBS]
        if not torch.is_tensor(obs):
            batch = TensorDict({DataKeys.OBS: obs["state"]}, batch_size=batch.batch_size, device=obs["state"].device)
        return super().forward(batch)


def _run_line(composite: bool, minibatch: None | int, noise: torch.Tensor, perms: list[torch.Tensor]):
    torch.manual_seed(5)
    n, h = noise.shape[1], noise.shape[0]
    algo = AlgorithmConfig(num_envs=n, horizon=h, model_cls=StateOnly, sgd_minibatch_size=minibatch,
                           num_sgd_iters=2).build(line_env(composite))
    assert (algo._tm_obs is not None) == composite and not algo._fusable()
    algo.injected_noise = noise.clone()
    algo.injected_permutations = perms
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        algo.collect()
        launched = set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
    assert ("rollout_scatter_leaves" in launched) == composite
    buf = {k: algo.buffer[k].clone() for k in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.VALUES, DataKeys.REWARDS,
                                               DataKeys.REVERSED_DISCOUNTED_RETURNS)}
    obs = algo.buffer[DataKeys.OBS]
    buf["state"] = (obs["state"] if composite else obs).clone()
    if composite:
        assert torch.equal(obs["flag"], obs["state"] > 0)
    stats = algo.step()
    params = torch.cat([p.detach().reshape(-1) for p in algo.policy.model.parameters()])
    return buf, stats, params


@pytest.mark.parametrize("minibatch", [None, 128])
def test_composite_route_equals_the_flat_route(minibatch):
    """The same env, model, seed and injected noise with the observation as a tensor and as a dict: the rollouts are
    bit-identical (the same towers on the same rows; the bookkeeping launches only copy), and one step() agrees at the
    bars of test_mlp_narrow_gpu.py::test_one_update_matches_the_eager_modules -- only the minibatch route differs
    (views of the buffer indexed per minibatch against the flat prefix / the packed gather)."""
    n, h = 64, 8
    g = torch.Generator(device=DEV).manual_seed(3)
    noise = torch.empty(h, n, 1, 2, device=DEV).exponential_(generator=g)
    perms = [torch.randperm(n * h, generator=torch.Generator().manual_seed(i)) for i in range(2)]
    b0, s0, p0 = _run_line(False, minibatch, noise, perms)
    b1, s1, p1 = _run_line(True, minibatch, noise, perms)
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


def test_recurrent_and_composite_actions_stay_refused():
    with pytest.raises(NotImplementedError, match="composite specs are outside the accelerated path"):
        RecurrentAlgorithmConfig(num_envs=8, horizon=4).build(DictEnv)

    class DictActions(DictEnv):
        def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Unbounded(1, device=device)
            self.action_spec = Composite({"a": Categorical(2, shape=torch.Size([1]), device=device)})

    with pytest.raises(NotImplementedError, match="composite specs are outside the accelerated path"):
        AlgorithmConfig(num_envs=8, horizon=4).build(DictActions)

    class ScalarLeaf(DictEnv):
        def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Composite({"x": Unbounded(2, device=device), "s": Unbounded((), device=device)})

    with pytest.raises(AssertionError, match="non-empty shape"):  # (every leaf has a shape, as for tensor specs)
        AlgorithmConfig(num_envs=8, horizon=4, model_cls=DictModel).build(ScalarLeaf)

    class Nested(DictEnv):
        def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Composite({"outer": Composite({"x": Unbounded(2, device=device)})})

    with pytest.raises(NotImplementedError, match="composite specs are outside the accelerated path"):
        AlgorithmConfig(num_envs=8, horizon=4, model_cls=DictModel).build(Nested)


def test_tuple_key_window_trains_on_a_dict_env():
    """``("obs", "x")`` with ``shift=3``: not identity views, the generic rollout with the several-leaf bookkeeping
    launch, the windows of the whole buffer indexed per minibatch."""
    torch.manual_seed(1)
    n, h = 8, 6
    algo = AlgorithmConfig(num_envs=n, horizon=h, model_cls=DictModel, model_config={"window": 3},
                           sgd_minibatch_size=16).build(DictEnv)
    assert not algo._identity_views() and not algo._fusable()
    before = [p.detach().clone() for p in algo.policy.model.parameters()]
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        algo.collect()
        views = algo.policy.model.apply_view_requirements(algo.buffer[:, :-1, ...], kind="all")
        window = views[DataKeys.OBS]["x"]
        assert window[DataKeys.INPUTS].shape == (n * h, 4, 2) and window[DataKeys.PADDING_MASK].shape == (n * h, 4)
        assert views[DataKeys.OBS]["count"].shape == (n * h, 1) and views[DataKeys.OBS]["flags"].dtype == torch.bool
        # sample (env 2, t 4): the window is x of columns 1 .. 4 (this rollout's steps 0 .. 3), nothing padded
        want = torch.cat([s["x"][2:3] for s in algo.env.steps[-h:][:4]])
        assert torch.equal(window[DataKeys.INPUTS][2 * h + 4], want)
        assert not window[DataKeys.PADDING_MASK][2 * h + 4].any() and window[DataKeys.PADDING_MASK][2 * h][:3].all()
        stats = algo.step()
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
    assert launched["rollout_scatter_leaves"]["launches"] == h and "gather_minibatch" in launched
    assert all(torch.isfinite(torch.tensor(stats[k])) for k in ("losses/policy", "losses/vf", "losses/total"))
    assert any(not torch.equal(b, p.detach()) for b, p in zip(before, algo.policy.model.parameters()))
