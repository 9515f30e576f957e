"""AlgoTrading as a batched HIP kernel.

Same task as the reference's ``examples/algotrading/env.py`` (``AlgoTrading`` :23-183): an asset whose price follows
``y[k + 1] = (1 + km) * (1 + kc * sin(f * t)) * y[k]`` with ``km``, ``kc``, ``f`` and ``y[0]`` drawn per environment;
three discrete actions (hold / buy / sell); the reward is the log-change of the price while invested and holding, and
of the price against the position when selling; ``max_horizon = 128``. Observations are a dict::

    {"action_mask": bool[3], "invested": int64[1], "LOG_CHANGE(price)": f32[1], "LOG_CHANGE(price, position)": f32[1]}

The mask says which actions make sense (buy only when not invested, sell only when invested); like the reference,
``step`` does not enforce it -- models add ``log(action_mask)`` to their logits.

State is struct-of-arrays ``[9, num_envs]`` float32 (``hip.ALGOTRADING_STATE_ROWS``; ``invested`` is 0 / 1 and ``t`` a
small integer, both exact). ``step`` is one launch of ``rl8_algotrading_step_f32``, and inside
``Algorithm.collect()`` the sampler, the step and the buffer bookkeeping are one launch per timestep
(``rl8_rollout_step_algotrading_f32``).

"""

from __future__ import annotations

import math
from typing import Any, Mapping

import torch

from .. import hip
from ..data import DataKeys, Device
from ..distributions import Categorical as CategoricalDistribution
from ..env import Env, default_seed
from ..specs import Categorical, Composite, Unbounded
from ..tensordict import TensorDict


class AlgoTrading(Env):
    """A mock of algorithmic trading on a simulated asset price."""

    max_horizon = 128

    #: ``[9, num_envs]`` rows ``hip.ALGOTRADING_STATE_ROWS``.
    state: torch.Tensor

    #: Distributions the fused per-timestep kernel implements for this env.
    fused_distributions = (CategoricalDistribution,)

    def __init__(
        self,
        num_envs: int,
        /,
        horizon: None | int = None,
        *,
        device: Device = "cpu",
    ) -> None:
        super().__init__(num_envs, horizon, device=device)
        self.observation_spec = Composite(
            {
                "action_mask": Categorical(2, shape=torch.Size([3]), device=device, dtype=torch.bool),
                "invested": Categorical(2, shape=torch.Size([1]), device=device, dtype=torch.long),
                "LOG_CHANGE(price)": Unbounded(1, device=device, dtype=torch.float32),
                "LOG_CHANGE(price, position)": Unbounded(1, device=device, dtype=torch.float32),
            }
        )
        self.action_spec = Categorical(3, shape=torch.Size([1]), device=device)
        self.f_bounds = math.pi
        self.k_cyclic_bounds = 0.05
        self.k_market_bounds = 0.05
        self.seed = default_seed()
        self.reset_count = 0

    def _new_obs(self) -> TensorDict:
        return TensorDict(
            {key: torch.empty(self.num_envs, d, dtype=dtype, device=self.device) for key, dtype, d in hip.ALGOTRADING_LEAVES},
            batch_size=self.num_envs,
            device=self.device,
        )

    def reset(self, *, config: dict[str, Any] | None = None) -> TensorDict:
        config = config or {}
        self.f_bounds = config.get("f_bounds", self.f_bounds)
        self.k_cyclic_bounds = config.get("k_cyclic_bounds", self.k_cyclic_bounds)
        self.k_market_bounds = config.get("k_market_bounds", self.k_market_bounds)
        self.state = torch.empty(len(hip.ALGOTRADING_STATE_ROWS), self.num_envs, dtype=torch.float32, device=self.device)
        obs = self._new_obs()
        hip.algotrading_reset(self.state, float(self.f_bounds), float(self.k_cyclic_bounds), float(self.k_market_bounds),
                              self.seed, self.reset_count, self.env_offset, obs)
        self.reset_count += 1
        return obs

    def step(self, action: torch.Tensor) -> TensorDict:
        if action.dtype != torch.int64:
            action = action.to(torch.int64)
        obs = self._new_obs()
        reward = torch.empty(self.num_envs, 1, dtype=torch.float32, device=self.device)
        hip.algotrading_step(self.state, action.contiguous(), obs, reward)
        return TensorDict(
            {DataKeys.OBS: obs, DataKeys.REWARDS: reward},
            batch_size=self.num_envs,
            device=self.device,
        )

    def fused_rollout_step(self, *, squashed: bool, features: torch.Tensor, features2: Any, **kw: Any) -> None:
        """``kw["obs_col_next"]`` maps the four leaf names to their ``t+1`` columns."""
        del squashed, features2
        hip.rollout_step_algotrading(logits=features, state=self.state, **kw)

    # -- the state in the reference's terms (tests start the env from a fixture) --
    def state_dict(self) -> dict[str, torch.Tensor]:
        """The reference's ``state`` tensordict: ``[N, 1]`` leaves, ``invested`` / ``t`` int64, ``action_mask``
        ``[N, 3]`` bool."""
        out: dict[str, torch.Tensor] = {}
        for row, key in enumerate(hip.ALGOTRADING_STATE_ROWS):
            leaf = self.state[row].reshape(-1, 1).clone()
            out[key] = leaf.to(torch.int64) if key in ("invested", "t") else leaf
        invested = out["invested"] == 1
        out["action_mask"] = torch.cat([torch.ones_like(invested), ~invested, invested], dim=1)
        return out

    def load_state(self, mapping: Mapping[str, Any]) -> None:
        """Start from ``mapping`` (keys of :meth:`state_dict`; ``action_mask`` follows from ``invested`` and is
        ignored)."""
        state = torch.empty(len(hip.ALGOTRADING_STATE_ROWS), self.num_envs, dtype=torch.float32, device=self.device)
        for row, key in enumerate(hip.ALGOTRADING_STATE_ROWS):
            leaf = torch.as_tensor(mapping[key]).to(self.device).reshape(-1)
            if leaf.numel() != self.num_envs:
                raise ValueError(f"state leaf {key!r} must hold one element per env")
            state[row] = leaf.to(torch.float32)
        self.state = state

    def observe(self) -> TensorDict:
        """The observation of the current state (what ``reset`` / ``step`` last returned)."""
        state = self.state_dict()
        return TensorDict({key: state[key] for key, _, _ in hip.ALGOTRADING_LEAVES}, batch_size=self.num_envs,
                          device=self.device)
