"""Wide-head towers (width 256 with heads of 9 to 128 outputs in all, rl8_amd/csrc/mlp_wide_out_kernels.hip): forward
and all six parameter gradients through ``fused_mlp.tower_forward`` against fp64 torch, beside torch's own fp32 at the
same inputs (the helpers and bars of tests/test_wide_input_tower_gpu.py, imported); ReLU'(0) = 0; run-to-run bit
equality, also across the backward's row segments and between the rollout and the training forward; two concatenated
heads; the routing of ``tower_forward``; the weight-gradient entry's ``accumulate``; and one collect() + step() of PPO on
an 18-action walk and on a 6-dimensional continuous env against the same runs on the torch modules."""

import itertools
from typing import Any

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.env import Env  # noqa: E402
from rl8_amd.nn import fused_mlp  # noqa: E402
from rl8_amd.specs import Unbounded  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402

from ._envs import walk_env  # noqa: E402
from .test_wide_input_tower_gpu import (  # noqa: E402
    DEV, HIDDEN, NAMES, _autograd, _away_from_kinks, _check, _check_forward, _fused, _params, _rel, _tower, _trunk)

SWITCH = "RL8_AMD_WIDE_HEAD_TOWERS"

# first width past the old limit, both sides of the k-granule of 8 (15, 16, 17) and of the 32-column tile (31, 32, 33),
# two and four tiles, the maximum
N_OUTS = (9, 15, 16, 17, 31, 32, 33, 64, 100, 128)
# both sides of the old input families (<= 16: the plane towers; >= 17: the wide-input towers), one input, the maximum
D_INS = (1, 4, 16, 17, 24, 128)
MS = (1, 63, 64, 65, 4097)
# every n_out, every d_in and every m at least once, and the grid-stride loop (more tiles than workgroups)
GRADIENT_CASES = [*zip(N_OUTS, itertools.cycle(D_INS), itertools.cycle(MS)), (18, 4, 70_001)]


def _case(seed, m, d_in, n_out):
    """x, the parameters and dout from a CPU generator (so that the seeds below can be chosen without a GPU), at the
    scales of ``_params``."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, d_in, generator=g)
    p = {
        "w1": torch.randn(HIDDEN, d_in, generator=g) * 0.5,
        "b1": torch.randn(HIDDEN, generator=g) * 0.1,
        "w2": torch.randn(HIDDEN, HIDDEN, generator=g) / HIDDEN ** 0.5,
        "b2": torch.randn(HIDDEN, generator=g) * 0.1,
        "w3": torch.randn(n_out, HIDDEN, generator=g) / HIDDEN ** 0.5,
        "b3": torch.randn(n_out, generator=g),
    }
    dout = torch.randn(m, n_out, generator=g)
    return x.to(DEV), {k: v.to(DEV) for k, v in p.items()}, dout.to(DEV)


def _seed(n_out, d_in, m):
    return 100_000 * n_out + 1000 * d_in + m % 997


def _kept(x, p, dout):
    """``_away_from_kinks(dout)`` and the assertion that it left enough to measure: at these scales about 2 % of the
    rows come within 1e-5 of a kink; the seeds were chosen (in fp64, from the same CPU generator) so that at least 90 %
    stay for m >= 63 and the one row stays for m = 1."""
    kept = _away_from_kinks(x, p, dout)
    m = x.shape[0]
    alive = int((kept != 0).any(1).sum())
    assert alive >= (1 if m == 1 else 0.9 * m), (alive, m)
    return kept


@pytest.mark.parametrize("n_out", N_OUTS)
def test_forward_against_fp64_at_every_pair_of_widths(n_out):
    m = 65
    for d_in in D_INS:
        x, p, _ = _case(_seed(n_out, d_in, m), m, d_in, n_out)
        with torch.no_grad():
            want = _tower(x.double(), {k: v.double() for k, v in p.items()})
            eager = _tower(x, p)
        _check_forward(_fused(x, p)[0], x, p, want, eager)


@pytest.mark.parametrize("n_out,d_in,m", GRADIENT_CASES)
def test_forward_and_gradients_against_fp64(n_out, d_in, m):
    x, p, dout = _case(_seed(n_out, d_in, m), m, d_in, n_out)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        _check(x, p, _kept(x, p, dout))
        launched = hip.timer.summary()
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert launched["mlp_wide_out_forward_save"]["launches"] == 1 and launched["mlp_wide_out_backward"]["launches"] == 1
    assert launched["mlp_wide_out_wgrad"]["launches"] == 2 and launched["mlp_wgrad"]["launches"] == 1  # dW1 and dW3; dW2
    assert not any(k.startswith("mlp_wide_in") or k.startswith("mlp_tower") for k in launched), sorted(launched)


def test_the_cases_cover_every_width_and_row_count():
    assert {c[0] for c in GRADIENT_CASES} >= set(N_OUTS) and {c[1] for c in GRADIENT_CASES} == set(D_INS)
    assert {c[2] for c in GRADIENT_CASES} == set(MS) | {70_001}


@pytest.mark.parametrize("d_in,n_out", [(4, 18), (24, 33)])
def test_relu_derivative_at_zero_is_zero(d_in, n_out):
    """Rows of x = 0 with b1 = 0 on half the units and b2 = 0 on half: z1 and z2 are exactly 0 there, and the
    gradients must take ReLU'(0) = 0 as torch does."""
    g = torch.Generator(device=DEV).manual_seed(7)
    m = 4099
    p = _params(g, HIDDEN, d_in, n_out)
    p["b1"][: HIDDEN // 2] = 0.0
    p["b1"][HIDDEN // 2:] = -0.5
    p["b2"][: HIDDEN // 2] = 0.0
    x = torch.randn(m, d_in, device=DEV, generator=g)
    x[::2] = 0.0
    dout = torch.randn(m, n_out, device=DEV, generator=g)
    _, grads = _check(x, p, dout)
    # (with ReLU'(0) = 1 instead, the zero rows alone would give b1 / b2 gradients on the zero-bias units)
    ones = _autograd(x[::2], p, dout[::2], torch.float64)[1]
    assert float(ones["b1"][: HIDDEN // 2].abs().max()) == 0.0 and float(ones["b2"][: HIDDEN // 2].abs().max()) == 0.0
    zero_rows = _fused(x[::2].contiguous(), p, dout[::2].contiguous())[1]
    assert float(zero_rows["b1"][: HIDDEN // 2].abs().max()) == 0.0
    assert float(zero_rows["b2"][: HIDDEN // 2].abs().max()) == 0.0
    assert float(zero_rows["w1"].abs().max()) == 0.0  # (x = 0 on every row)
    assert torch.isfinite(grads["b1"]).all()


def test_two_runs_are_bit_identical():
    m, d_in, n_out = 70_001, 24, 33
    g = torch.Generator(device=DEV).manual_seed(m)
    p = _params(g, HIDDEN, d_in, n_out)
    x = torch.randn(m, d_in, device=DEV, generator=g)
    dout = torch.randn(m, n_out, device=DEV, generator=g)
    (out_a, a), (out_b, b) = _fused(x, p, dout), _fused(x, p, dout)
    assert torch.equal(out_a, out_b)
    assert torch.equal(out_a, _fused(x, p)[0])  # (the rollout variant stores nothing and computes the same bits)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


def test_the_segment_walk_holds_the_bars_and_repeats_bit_for_bit(monkeypatch):
    """Three whole segments and one of five rows.  (One segment against four may differ in the last bits: the sums are
    taken in another order; no equality is asserted between them.)"""
    monkeypatch.setattr(fused_mlp, "WIDE_INPUT_SEGMENT_ROWS", 4096)
    m, d_in, n_out = 3 * 4096 + 5, 17, 18
    x, p, dout = _case(_seed(n_out, d_in, m), m, d_in, n_out)
    dout = _kept(x, p, dout)
    launches: dict = {}
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        _, a = _check(x, p, dout)
        launches.update(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert launches["mlp_wide_out_forward_save"]["launches"] == 1
    assert launches["mlp_wide_out_backward"]["launches"] == 4 and launches["mlp_wide_out_wgrad"]["launches"] == 8
    assert launches["mlp_wgrad"]["launches"] == 4
    b = _fused(x, p, dout)[1]
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


def test_two_concatenated_heads_and_a_weight_changed_in_place():
    torch.manual_seed(3)
    trunk = _trunk(24, HIDDEN)
    heads = [nn.Linear(HIDDEN, 6).to(DEV), nn.Linear(HIDDEN, 6).to(DEV)]
    x = torch.randn(300, 24, device=DEV)
    out = fused_mlp.tower_forward(trunk, heads, x)
    assert out is not None and out.shape == (300, 12) and out.requires_grad
    want = torch.cat([h(trunk(x)) for h in heads], -1)
    torch.testing.assert_close(out, want, rtol=1e-4, atol=1e-5)
    dout = torch.randn(300, 12, device=DEV)
    params = [*trunk.parameters(), *[q for h in heads for q in h.parameters()]]
    got = torch.autograd.grad(out, params, dout)
    ref = torch.autograd.grad(want, params, dout)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and _rel(a, b) <= 1e-4
    with torch.no_grad():  # (the optimizer's kind of change: the next call must see every one of them)
        heads[1].weight.mul_(-1.5)
        heads[0].bias.add_(0.25)
        trunk[0][0].weight.mul_(0.5)
        trunk[0][2].weight.add_(0.01)
        again = fused_mlp.tower_forward(trunk, heads, x)
        assert again is not None and not torch.equal(again, out.detach())
        torch.testing.assert_close(again, torch.cat([h(trunk(x)) for h in heads], -1), rtol=1e-4, atol=1e-5)


def _launched(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        fn()
        return set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()


def test_routing(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    for d_in, n_out in ((4, 9), (24, 12), (128, 128)):
        trunk, head = _trunk(d_in, HIDDEN), nn.Linear(HIDDEN, n_out).to(DEV)
        x = torch.randn(100, d_in, device=DEV)
        out = []
        names = _launched(lambda: out.append(fused_mlp.tower_forward(trunk, [head], x)))
        assert out[0] is not None and out[0].shape == (100, n_out) and out[0].requires_grad
        assert "mlp_wide_out_forward_save" in names, names
        torch.testing.assert_close(out[0], head(trunk(x)), rtol=1e-4, atol=1e-5)
    trunk, head = _trunk(24, HIDDEN), nn.Linear(HIDDEN, 12).to(DEV)
    x = torch.randn(100, 24, device=DEV)
    with torch.no_grad():
        names = _launched(lambda: out.append(fused_mlp.tower_forward(trunk, [head], x.clone().requires_grad_(True))))
        assert out[-1] is not None and names == {"mlp_wide_out_forward"}  # (no gradient can follow: the rollout variant)
    # declined: the caller runs the modules
    assert fused_mlp.tower_forward(trunk, [head], x.clone().requires_grad_(True)) is None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert fused_mlp.tower_forward(trunk, [head], x) is None
    assert fused_mlp.tower_forward(trunk.double(), [head.double()], x.double()) is None
    trunk, head = trunk.float(), head.float()
    assert fused_mlp.tower_forward(trunk, [head], torch.randn(24, 100, device=DEV).T) is None
    assert fused_mlp.tower_forward(trunk, [head], x[:0]) is None
    assert fused_mlp.tower_forward(trunk, [head], x[:, :23].contiguous()) is None
    for width in (64, 128):
        assert fused_mlp.tower_forward(_trunk(24, width), [nn.Linear(width, 12).to(DEV)], x) is None
    monkeypatch.setenv(SWITCH, "0")
    assert fused_mlp.tower_forward(trunk, [head], x) is None
    monkeypatch.setenv(SWITCH, "1")
    assert fused_mlp.tower_forward(trunk, [head], x) is not None
    monkeypatch.delenv(SWITCH, raising=False)
    # up to 8 outputs every other family launches what it launched: none of the new kernels
    for d_in in (4, 24):
        trunk, head = _trunk(d_in, HIDDEN), nn.Linear(HIDDEN, 4).to(DEV)
        x4 = torch.randn(100, d_in, device=DEV)
        names = _launched(lambda: fused_mlp.tower_forward(trunk, [head], x4).sum().backward())
        assert names and not any(k.startswith("mlp_wide_out") for k in names), names


@pytest.mark.parametrize("c", [9, 100])
def test_the_weight_gradient_accumulates_into_out(c):
    """``accumulate`` adds a launch's product to what ``out`` holds; without it ``out`` is overwritten, whatever it
    held.  Both orientations of the result."""
    g = torch.Generator(device=DEV).manual_seed(c)
    m = 5000
    a, b = torch.randn(m, HIDDEN, device=DEV, generator=g), torch.randn(m, c, device=DEV, generator=g)
    for transpose in (False, True):
        whole = hip.mlp_wide_out_wgrad(a, b, transpose=transpose)
        want = a.double().T @ b.double()
        want = want.T if transpose else want
        assert whole.shape == want.shape and _rel(whole, want) <= 5e-6
        out = torch.full_like(whole, float("nan"))
        assert hip.mlp_wide_out_wgrad(a[:3000], b[:3000], out=out, transpose=transpose) is out
        first = out.clone()
        hip.mlp_wide_out_wgrad(a[3000:], b[3000:], out=out, accumulate=True, transpose=transpose)
        # (the same <= 160 fp32 terms -- one per workgroup slab and the first product -- in another association: at
        # most 160 roundings of 2^-24 apart, relative to the largest entry's terms)
        second = hip.mlp_wide_out_wgrad(a[3000:], b[3000:], transpose=transpose)
        assert _rel(out, first + second) <= 160 * 2.0 ** -24
        assert not torch.equal(out, first) and _rel(out, want) <= 5e-6


def push_env(d: int, a: int) -> type[Env]:
    """A point in ``d`` dimensions pushed by a continuous action of ``a`` dimensions (clamped to [-1, 1]) on its first
    ``a`` coordinates: ``state <- 0.75 * state + push - 0.25``, reward ``-sum |state|``."""

    class Push(Env):
        def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Unbounded(d, device=device)
            self.action_spec = Unbounded(shape=torch.Size([a]), device=device)

        def reset(self, *, config: None | dict[str, Any] = None) -> torch.Tensor:
            self.state = torch.empty(self.num_envs, d, device=self.device).uniform_(-1.0, 1.0)
            return self.state

        def step(self, action: torch.Tensor) -> TensorDict:
            push = torch.zeros_like(self.state)
            push[:, :a] = action.reshape(-1, a).clamp(-1.0, 1.0)
            self.state = 0.75 * self.state + push - 0.25
            rewards = -self.state.abs().sum(-1, keepdim=True)
            return TensorDict({DataKeys.OBS: self.state, DataKeys.REWARDS: rewards}, batch_size=self.num_envs,
                              device=self.device)

    Push.__name__ = f"Push{d}x{a}"
    return Push


def _run_algo(env, kernels):
    torch.manual_seed(11)
    algo = AlgorithmConfig(num_envs=64, horizon=8).build(env)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        algo.collect()
        step = algo.step()
        kernels.update(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    return step, torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])


@pytest.mark.parametrize("env", ["walk_4x18", "push_24x6"])
def test_one_update_matches_the_torch_modules(env, monkeypatch):
    """Losses at rel 1e-5 / abs 1e-8; parameters at rtol 1e-4 and atol 1e-5: the bars and the reasoning of
    tests/test_wide_input_tower_gpu.py::test_one_update_matches_the_torch_modules.  The discrete model's policy tower
    is 4 -> 256 -> 256 -> 18, the continuous model's 24 -> 256 -> 256 -> [6 | 6]."""
    cls = walk_env(4, 18) if env == "walk_4x18" else push_env(24, 6)
    monkeypatch.delenv(SWITCH, raising=False)
    on: dict = {}
    s0, p0 = _run_algo(cls, on)
    assert {"mlp_wide_out_forward", "mlp_wide_out_forward_save", "mlp_wide_out_backward", "mlp_wide_out_wgrad"} <= set(on), sorted(on)
    monkeypatch.setenv(SWITCH, "0")
    off: dict = {}
    s1, p1 = _run_algo(cls, off)
    assert not any(k.startswith("mlp_wide_out") for k in off), sorted(off)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)
