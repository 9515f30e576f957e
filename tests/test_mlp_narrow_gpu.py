"""Narrow towers (hidden width 64 / 128, rl8_amd/csrc/mlp_narrow_kernels.hip): forward and all six parameter gradients
against fp64 torch, at least as close as torch's own fp32 at the same inputs; run-to-run bit equality; the routing of
``fused_mlp.tower_forward``; and one collect() + step() of PPO fused against the same run on the eager modules."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.distributions import SquashedNormal  # noqa: E402
from rl8_amd.env import ContinuousDummyEnv, DiscreteDummyEnv  # noqa: E402
from rl8_amd.nn import fused_mlp  # noqa: E402

DEV = "cuda:0"
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def _params(g, hidden, d_in, n_out):
    return {
        "w1": torch.randn(hidden, d_in, device=DEV, generator=g) * 0.5,
        "b1": torch.randn(hidden, device=DEV, generator=g) * 0.1,
        "w2": torch.randn(hidden, hidden, device=DEV, generator=g) / hidden ** 0.5,
        "b2": torch.randn(hidden, device=DEV, generator=g) * 0.1,
        "w3": torch.randn(n_out, hidden, device=DEV, generator=g) / hidden ** 0.5,
        "b3": torch.randn(n_out, device=DEV, generator=g),
    }


def _tower(x, p):
    h1 = torch.relu(x @ p["w1"].T + p["b1"])
    h2 = torch.relu(h1 @ p["w2"].T + p["b2"])
    return h2 @ p["w3"].T + p["b3"]


def _autograd(x, p, dout, dtype):
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    out = _tower(x.to(dtype), q)
    out.backward(dout.to(dtype))
    return out.detach(), {k: q[k].grad for k in NAMES}


def _rel(got, want):
    return float((got.double() - want.double()).abs().max()) / (float(want.abs().max()) + 1e-30)


def _away_from_kinks(x, p, dout):
    """dout with the rows zeroed whose pre-activations come within 1e-5 (relative) of a ReLU kink: there fp32 rounding
    may take the ReLU either way, in the kernel as in torch, and one row decided differently moves the gradients by
    far more than rounding does.  The rows with exact zeros are tested on their own (ReLU'(0) = 0)."""
    q = {k: v.double() for k, v in p.items()}
    z1 = x.double() @ q["w1"].T + q["b1"]
    z2 = torch.relu(z1) @ q["w2"].T + q["b2"]
    near = ((z1.abs() < 1e-5 * float(z1.abs().max())).any(1) | (z2.abs() < 1e-5 * float(z2.abs().max())).any(1))
    return dout.masked_fill(near[:, None], 0.0)


def _check(x, p, dout):
    want, gwant = _autograd(x, p, dout, torch.float64)
    eager, geager = _autograd(x, p, dout, torch.float32)
    out = hip.mlp_narrow_forward(x, *(p[k] for k in NAMES))
    assert torch.isfinite(out).all()
    # (relative to the size of the head's terms, |h2| |w3|^T + |b3|: a single output that cancels to nearly zero
    # -- m = 1, n_out = 1 -- would otherwise measure luck)
    q = {k: v.double() for k, v in p.items()}
    terms = float((torch.relu(torch.relu(x.double() @ q["w1"].T + q["b1"]) @ q["w2"].T + q["b2"]) @ q["w3"].abs().T
                   + q["b3"].abs()).max())
    err, err32 = (float((o.double() - want).abs().max()) / terms for o in (out, eager))
    assert err <= max(2 * err32, 1e-6), (err, err32)
    g = hip.mlp_narrow_backward(x, dout, *(p[k] for k in NAMES[:5]))
    for k in NAMES:
        assert g[k].shape == p[k].shape and torch.isfinite(g[k]).all(), k
        assert _rel(g[k], gwant[k]) <= max(3 * _rel(geager[k], gwant[k]), 5e-6), (k, _rel(g[k], gwant[k]),
                                                                                   _rel(geager[k], gwant[k]))
    return out, g


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097, 70_001, (1 << 20) + 17])
@pytest.mark.parametrize("d_in", [1, 2, 5, 8, 9, 16])
def test_forward_and_gradients_against_fp64(hidden, m, d_in):
    for n_out in (1, 2, 3, 8):
        g = torch.Generator(device=DEV).manual_seed(1000 * hidden + 10 * d_in + n_out + m % 997)
        x = torch.randn(m, d_in, device=DEV, generator=g)
        p = _params(g, hidden, d_in, n_out)
        _check(x, p, _away_from_kinks(x, p, torch.randn(m, n_out, device=DEV, generator=g)))


@pytest.mark.parametrize("hidden", [64, 128])
def test_relu_derivative_at_zero_is_zero(hidden):
    """Rows of x = 0 with b1 = 0 on half the units and b2 = 0 on half: z1 and z2 are exactly 0 there, and the
    gradients must take ReLU'(0) = 0 as torch does."""
    g = torch.Generator(device=DEV).manual_seed(7)
    m, d_in, n_out = 4099, 5, 3
    p = _params(g, hidden, d_in, n_out)
    p["b1"][: hidden // 2] = 0.0
    p["b1"][hidden // 2:] = -0.5
    p["b2"][: hidden // 2] = 0.0
    x = torch.randn(m, d_in, device=DEV, generator=g)
    x[::2] = 0.0
    dout = torch.randn(m, n_out, device=DEV, generator=g)
    _, grads = _check(x, p, dout)
    # (with ReLU'(0) = 1 instead, the zero rows alone would give b1 / b2 gradients on the zero-bias units)
    ones = _autograd(x[::2], p, dout[::2], torch.float64)[1]
    assert float(ones["b1"][: hidden // 2].abs().max()) == 0.0 and float(ones["b2"][: hidden // 2].abs().max()) == 0.0
    assert torch.isfinite(grads["b1"]).all()


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("m", [4097, 70_001])
def test_two_launches_are_bit_identical(hidden, m):
    g = torch.Generator(device=DEV).manual_seed(m)
    p = _params(g, hidden, 9, 3)
    x = torch.randn(m, 9, device=DEV, generator=g)
    dout = torch.randn(m, 3, device=DEV, generator=g)
    args = [p[k] for k in NAMES]
    assert torch.equal(hip.mlp_narrow_forward(x, *args), hip.mlp_narrow_forward(x, *args))
    a, b = hip.mlp_narrow_backward(x, dout, *args[:5]), hip.mlp_narrow_backward(x, dout, *args[:5])
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


def _run_algo(env_cls, hiddens, enabled, kernels=None, **config):
    before = fused_mlp.ENABLED
    fused_mlp.ENABLED = enabled
    try:
        torch.manual_seed(11)
        algo = AlgorithmConfig(num_envs=256, horizon=16, model_config={"hiddens": hiddens}, **config).build(env_cls)
        if kernels is not None:
            hip.timer.reset()
            hip.timer.enabled = True
        collect = algo.collect()
        step = algo.step()
        if kernels is not None:
            hip.timer.enabled = False
            kernels.update(hip.timer.summary())
        params = torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])
    finally:
        fused_mlp.ENABLED = before
        hip.timer.enabled = False
    return collect, step, params


@pytest.mark.parametrize("hiddens", [(64, 64), (128, 128)])
@pytest.mark.parametrize("env_cls", [DiscreteDummyEnv, ContinuousDummyEnv])
def test_default_models_route_narrow_towers_to_the_kernels(env_cls, hiddens, monkeypatch):
    calls = []
    real = torch.nn.functional.linear
    monkeypatch.setattr(torch.nn.functional, "linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    kernels: dict = {}
    _run_algo(env_cls, hiddens, True, kernels)
    assert {"mlp_narrow_forward", "mlp_narrow_backward", "mlp_narrow_reduce"} <= set(kernels)
    assert not calls, "an eager nn.Linear ran"


def test_width_256_models_run_no_narrow_kernel():
    kernels: dict = {}
    _run_algo(DiscreteDummyEnv, (256, 256), True, kernels)
    assert "mlp_tower_forward" in kernels
    assert not any(k.startswith("mlp_narrow") for k in kernels)


def _trunk(d_in, h1, h2, bias=True, act=nn.ReLU):
    return nn.Sequential(nn.Sequential(nn.Linear(d_in, h1, bias=bias), act(), nn.Linear(h1, h2, bias=bias)),
                         act()).to(DEV)


@pytest.mark.parametrize("case", ["mixed", "96", "bias_free", "tanh", "d_in_17"])
def test_other_towers_stay_eager(case):
    d_in, h1, h2, bias, act = 4, 64, 64, True, nn.ReLU
    if case == "mixed":
        h2 = 128
    elif case == "96":
        h1 = h2 = 96
    elif case == "bias_free":
        bias = False
    elif case == "tanh":
        act = nn.Tanh
    else:
        d_in = 17
    trunk = _trunk(d_in, h1, h2, bias, act)
    head = nn.Linear(h2, 2, bias=bias).to(DEV)
    x = torch.randn(100, d_in, device=DEV)
    assert fused_mlp.tower_forward(trunk, [head], x) is None
    if case in ("mixed", "96", "d_in_17"):  # (the same tower at a narrow width is taken: the refusal is the shape's)
        ok = _trunk(min(d_in, 16), 64, 64)
        assert fused_mlp.tower_forward(ok, [nn.Linear(64, 2).to(DEV)], x[:, :min(d_in, 16)].contiguous()) is not None


def _cartpole():
    from rl8_amd.envs.cartpole import CartPole
    return CartPole


@pytest.mark.parametrize("hiddens", [(64, 64), (128, 128)])
@pytest.mark.parametrize("env", ["dummy", "cartpole", "continuous_squashed"])
def test_one_update_matches_the_eager_modules(env, hiddens):
    """Losses at the bars of test_enable_amp_keeps_the_fused_fp32_towers; parameters at rtol 1e-4 and atol 1e-5 (1 % of
    Adam's first step, lr = 1e-3): the fused and eager towers round differently, and a ReLU that rounding decides the
    other way for one sample moves a few weights by ~2e-6 (seen at H = 128 on the squashed-normal policy)."""
    config = {}
    if env == "dummy":
        env_cls = DiscreteDummyEnv
    elif env == "cartpole":
        env_cls = _cartpole()
    else:
        env_cls, config = ContinuousDummyEnv, {"distribution_cls": SquashedNormal}
    c0, s0, p0 = _run_algo(env_cls, hiddens, True, **config)
    c1, s1, p1 = _run_algo(env_cls, hiddens, False, **config)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


def test_headline_row_count():
    """One forward + backward at 2^25 rows, H = 128, d_in = 1, n_out = 2, against eager fp32."""
    g = torch.Generator(device=DEV).manual_seed(25)
    m = 1 << 25
    p = _params(g, 128, 1, 2)
    x = torch.randn(m, 1, device=DEV, generator=g)
    dout = _away_from_kinks(x, p, torch.randn(m, 2, device=DEV, generator=g) / m)
    out = hip.mlp_narrow_forward(x, *(p[k] for k in NAMES))
    grads = hip.mlp_narrow_backward(x, dout, *(p[k] for k in NAMES[:5]))
    eager, geager = _autograd(x, p, dout, torch.float32)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out, eager, rtol=1e-4, atol=1e-6)
    for k in NAMES:
        assert torch.isfinite(grads[k]).all(), k
        scale = float(geager[k].abs().max())
        torch.testing.assert_close(grads[k], geager[k], rtol=1e-4, atol=1e-6 * max(scale, 1.0), msg=k)
