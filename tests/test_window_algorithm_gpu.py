"""Feed-forward ``Algorithm`` with windowed views on the window kernels against the same run with
``RL8_AMD_WINDOW_KERNELS=0`` (torch ops: ``pad_last_sequence`` per timestep, every window of the buffer built up
front and indexed per minibatch).  The kernels only move data and both routes hand the model dense tensors of the
same values, so everything is compared bit for bit: the buffer after every ``collect()``, ``CollectStats``,
``StepStats`` and every parameter after every ``step()``.

The rollout keeps ``env.step`` plus the bookkeeping launch for windowed models on every env (tests/test_algotrading_gpu
.py, tests/test_algorithm_gpu.py and tests/test_composite_obs_gpu.py pin that route); what changes is where the
model's input comes from: one ``rl8_window_last`` launch per column."""

from __future__ import annotations

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.env import DiscreteDummyEnv  # noqa: E402
from rl8_amd.envs import AlgoTrading  # noqa: E402
from rl8_amd.models import Model  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402
from rl8_amd.views import ViewRequirement  # noqa: E402

N, H, SHIFT = 257, 8, 3
LC, LCP = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"
FINFO = torch.finfo(torch.float32)


def _window_features(window: TensorDict) -> torch.Tensor:
    """Every cell of the window and its padding mask, as one dense row per sample."""
    inputs, mask = window[DataKeys.INPUTS], window[DataKeys.PADDING_MASK]
    assert inputs.shape[1] == SHIFT + 1 and mask.shape == inputs.shape[:2] and mask.dtype == torch.bool
    return torch.cat([inputs.flatten(start_dim=1), mask.to(torch.float32)], dim=-1)


class WindowedWalker(Model):
    """Tensor observations through ``"obs" -> ViewRequirement(shift=SHIFT)``."""

    def __init__(self, observation_spec, action_spec, /):
        super().__init__(observation_spec, action_spec)
        self.view_requirements = {DataKeys.OBS: ViewRequirement(shift=SHIFT)}
        self.body = nn.Linear(2 * (SHIFT + 1), 32)
        self.head = nn.Linear(32, 2)
        self.vf = nn.Linear(32, 1)
        self._value = None

    def forward(self, batch, /):
        z = torch.relu(self.body(_window_features(batch[DataKeys.OBS])))
        self._value = self.vf(z)
        return TensorDict({"logits": self.head(z).reshape(-1, 1, 2)}, batch_size=batch.batch_size, device=z.device)

    def value_function(self):
        return self._value


class WindowedTrader(Model):
    """Dict observations with ``("obs", "LOG_CHANGE(price)") -> ViewRequirement(shift=SHIFT)`` on top of the default
    view: the window beside the three unwindowed leaves."""

    def __init__(self, observation_spec, action_spec, /):
        super().__init__(observation_spec, action_spec)
        self.view_requirements[(DataKeys.OBS, LC)] = ViewRequirement(shift=SHIFT)
        self.invested_embedding = nn.Embedding(2, 2)
        self.body = nn.Linear(2 + 2 * (SHIFT + 1) + 1, 32)
        self.head = nn.Linear(32, 3)
        self.vf = nn.Linear(32, 1)
        self._value = None

    def forward(self, batch, /):
        obs = batch[DataKeys.OBS]
        x = torch.cat([self.invested_embedding(obs["invested"].flatten()), _window_features(obs[LC]), obs[LCP]], dim=-1)
        z = torch.relu(self.body(x))
        self._value = self.vf(z)
        logits = self.head(z) + torch.clamp(torch.log(obs["action_mask"].to(torch.float32)), FINFO.min, FINFO.max)
        return TensorDict({"logits": logits.reshape(-1, 1, 3)}, batch_size=batch.batch_size, device=z.device)

    def value_function(self):
        return self._value


CASES = {"tensor-obs": (DiscreteDummyEnv, WindowedWalker), "tuple-key": (AlgoTrading, WindowedTrader)}
SGD_ITERS = 2


def _leaves(buffer: TensorDict, prefix: str = "") -> dict[str, torch.Tensor]:
    out = {}
    for k, v in buffer.items():
        if torch.is_tensor(v):
            out[prefix + k] = v.clone()
        else:
            out.update(_leaves(v, prefix + k + "/"))
    return out


def _run(case: str, num_minibatches: int, kernels: bool, monkeypatch):
    """collect / step three times with ``horizons_per_env_reset = 2``: a reset, a carry, and the reset at the
    boundary.  Returns everything the two routes must agree on, and what was launched."""
    monkeypatch.setenv("RL8_AMD_WINDOW_KERNELS", "1" if kernels else "0")
    env_cls, model_cls = CASES[case]
    torch.manual_seed(11)
    algo = AlgorithmConfig(num_envs=N, horizon=H, model_cls=model_cls, horizons_per_env_reset=2, num_sgd_iters=SGD_ITERS,
                           sgd_minibatch_size=N * H // num_minibatches, entropy_coeff=0.01).build(env_cls)
    assert algo.hparams.num_minibatches == num_minibatches
    assert not algo._identity_views() and not algo._fusable() and (algo._window_plan() is not None) == kernels
    views_all_stayed_none = []
    forward_backward = algo._minibatch_forward_backward

    def watched(batch, *args):
        views_all_stayed_none.append(algo._views_all is None)
        return forward_backward(batch, *args)

    algo._minibatch_forward_backward = watched
    record = []
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        for round_ in range(3):
            collect = algo.collect()
            record.append(("reset", round_, collect["env/resets"]))
            record.append(("collect", round_, {k: v for k, v in collect.items() if not k.startswith("profiling/")}))
            record.append(("buffer", round_, _leaves(algo.buffer)))
            algo.injected_permutations = [torch.randperm(N * H, generator=torch.Generator().manual_seed(100 * round_ + i))
                                          for i in range(SGD_ITERS)]
            step = algo.step()
            record.append(("step", round_, {k: v for k, v in step.items() if not k.startswith("profiling/")}))
            record.append(("params", round_, {k: v.detach().clone() for k, v in algo.policy.model.state_dict().items()}))
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
    assert [r[2] for r in record if r[0] == "reset"] == [N, 0, N]  # (reset, carry, the boundary)
    return record, launched, views_all_stayed_none


@pytest.mark.parametrize("num_minibatches", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_route_equals_the_torch_route_bit_for_bit(case, num_minibatches, monkeypatch):
    on, launched_on, stayed_none = _run(case, num_minibatches, True, monkeypatch)
    off, launched_off, built = _run(case, num_minibatches, False, monkeypatch)
    assert len(on) == len(off)
    for (kind, round_, a), (_, _, b) in zip(on, off):
        if kind in ("buffer", "params"):
            assert a.keys() == b.keys()
            for k in a:
                same = torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) if a[k].dtype == torch.float32 \
                    else torch.equal(a[k], b[k])
                assert same, (kind, round_, k)
        elif kind != "reset":
            assert a.keys() == b.keys()
            for k in a:  # (floats from the same bits: equal, or NaN in both -- the std of one sample)
                assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (kind, round_, k, a[k], b[k])

    # the kernel route never builds the windows of the whole buffer; the torch route holds them through step()
    assert stayed_none and all(stayed_none) and len(stayed_none) == 3 * SGD_ITERS * num_minibatches
    assert built and not any(built)
    # one window launch per column (H timesteps and the bootstrap value) per collect(); one gather per minibatch, or
    # one per step() for a whole-buffer minibatch
    assert launched_on["window_last"]["launches"] == 3 * (H + 1)
    assert launched_on["gather_windows"]["launches"] == 3 * (1 if num_minibatches == 1 else SGD_ITERS * num_minibatches)
    assert "window_last" not in launched_off and "gather_windows" not in launched_off
    # the other training leaves stay on rl8_gather_minibatch, the rollout on env.step + one bookkeeping launch
    assert launched_on["gather_minibatch"]["launches"] == launched_off["gather_minibatch"]["launches"] \
        == 3 * SGD_ITERS * num_minibatches
    for launched in (launched_on, launched_off):
        assert not any(name.startswith("rollout_step") for name in launched), sorted(launched)
        if case == "tuple-key":
            assert launched["rollout_scatter_leaves"]["launches"] == launched["algotrading_step"]["launches"] == 3 * H


def test_rolling_window_models_keep_the_torch_route_and_its_error():
    class Dropping(WindowedWalker):
        def __init__(self, observation_spec, action_spec, /):
            super().__init__(observation_spec, action_spec)
            self.view_requirements = {DataKeys.OBS: ViewRequirement(shift=SHIFT, method="rolling_window")}

        def forward(self, batch, /):
            window = batch[DataKeys.OBS]
            pad = window.new_zeros(window.shape[0], SHIFT + 1 - window.shape[1], *window.shape[2:])
            window = torch.cat([pad, window], dim=1)
            mask = torch.zeros(window.shape[:2], dtype=torch.bool, device=window.device)
            return super().forward(TensorDict({DataKeys.OBS: TensorDict(
                {DataKeys.INPUTS: window, DataKeys.PADDING_MASK: mask}, batch_size=window.shape[0])},
                batch_size=batch.batch_size))

    algo = AlgorithmConfig(num_envs=64, horizon=H, model_cls=Dropping).build(DiscreteDummyEnv)
    assert algo._window_plan() is None
    algo.collect()
    with pytest.raises(ValueError, match="one window per sample"):
        algo.step()


def test_dict_observations_with_identity_views_gather_through_the_window_kernel(monkeypatch):
    """Every leaf at size 1: the per-minibatch views come from one ``rl8_gather_windows`` launch (a plain gather) and
    are the rows ``_views_all[index]`` holds on the torch route."""
    from .test_algotrading_gpu import MaskedTrader

    def run(kernels: bool):
        monkeypatch.setenv("RL8_AMD_WINDOW_KERNELS", "1" if kernels else "0")
        torch.manual_seed(4)
        algo = AlgorithmConfig(num_envs=N, horizon=H, model_cls=MaskedTrader, num_sgd_iters=1,
                               sgd_minibatch_size=N * H // 4).build(AlgoTrading)
        assert algo._identity_views() and algo._fusable()
        algo.collect()
        algo.injected_permutations = [torch.randperm(N * H, generator=torch.Generator().manual_seed(1))]
        stats = algo.step()
        return stats, [p.detach().clone() for p in algo.policy.model.parameters()]

    s_on, p_on = run(True)
    s_off, p_off = run(False)
    for k in ("losses/policy", "losses/vf", "losses/total", "monitors/kl_div"):
        assert s_on[k] == s_off[k], k
    for a, b in zip(p_on, p_off):
        assert torch.equal(a, b)
