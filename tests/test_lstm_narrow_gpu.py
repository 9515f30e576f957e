"""Narrow LSTMs (hidden width 64 / 128, rl8_amd/csrc/lstm_narrow_kernels.hip): forward and the four parameter
gradients against torch in fp32 and fp64, at least as close as torch's own fp32; the two launch modes and two backward
launches bit for bit; the routing of ``fused_lstm.lstm_forward``; and the default recurrent models and one
collect() + step() of PPO fused against the eager modules."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import RecurrentAlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.distributions import SquashedNormal  # noqa: E402
from rl8_amd.env import ContinuousDummyEnv, DiscreteDummyEnv  # noqa: E402
from rl8_amd.models_recurrent import DefaultContinuousRecurrentModel, DefaultDiscreteRecurrentModel  # noqa: E402
from rl8_amd.nn import fused_lstm  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402

DEV = "cuda:0"
GRADS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
SHAPES = [(1, 1, 1), (31, 3, 4), (64, 4, 5), (257, 8, 16), (4097, 2, 3)]


def _lstm(hidden, d_in, seed=0, scale=1.0):
    torch.manual_seed(seed)
    lstm = nn.LSTM(d_in, hidden, batch_first=True).to(DEV)
    if scale != 1.0:
        with torch.no_grad():
            for p in lstm.parameters():
                p.mul_(scale)
    return lstm


def _inputs(b, l, d_in, hidden, seed=1, x_scale=1.0, c_scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, l, d_in, device=DEV, generator=g) * x_scale
    h0 = torch.randn(b, hidden, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, hidden, device=DEV, generator=g) * c_scale
    return x, h0, c0


def _params(lstm):
    return [getattr(lstm, k).detach() for k in GRADS]


def _torch(lstm, x, h0, c0, dtype):
    """hs, h_n, c_n of the module in ``dtype`` (cuDNN / MIOpen off)."""
    ref = nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        hs, (hn, cn) = ref(x.to(dtype), (h0[None].to(dtype), c0[None].to(dtype)))
    return hs, hn[0], cn[0]


def _torch_grads(lstm, x, h0, c0, dhs, dtype):
    ref = nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    with torch.backends.cudnn.flags(enabled=False):
        hs, _ = ref(x.to(dtype), (h0[None].to(dtype), c0[None].to(dtype)))
        (hs * dhs.to(dtype)).sum().backward()
    return {k: getattr(ref, k).grad for k in GRADS}


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("b,l,d_in", SHAPES)
def test_forward_matches_torch(hidden, b, l, d_in):
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(b, l, d_in, hidden)
    hs, hn, cn, gates, cs = hip.lstm_narrow_forward(x, h0, c0, *_params(lstm), save=True)
    hs_i, hn_i, cn_i, none_g, none_c = hip.lstm_narrow_forward(x, h0, c0, *_params(lstm))
    assert none_g is None and none_c is None
    for a, e in ((hs, hs_i), (hn, hn_i), (cn, cn_i)):
        assert torch.equal(a, e), "inference and training launches differ"
    assert torch.equal(hs[:, -1], hn) and torch.equal(cs[:, -1], cn)
    f32 = _torch(lstm, x, h0, c0, torch.float32)
    f64 = _torch(lstm, x, h0, c0, torch.float64)
    torch.testing.assert_close(hs, f32[0], rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(hn, f32[1], rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(cn, f32[2], rtol=0, atol=4e-6)
    for ours, t32, want in zip((hs, hn, cn), f32, f64):
        err = float((ours.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        assert err <= max(2 * err32, 2e-6), (err, err32)
    # the saved gates reproduce the cell update and the output
    i, f, gg, o = gates.double().unbind(2)
    c_prev = torch.cat([c0[:, None].double(), cs[:, :-1].double()], 1)
    torch.testing.assert_close(cs.double(), f * c_prev + i * gg, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(hs.double(), o * torch.tanh(cs.double()), rtol=1e-5, atol=2e-6)


def _check_grads(ours, want, t32):
    for k, ok in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b"), ("bias_hh_l0", "b")):
        g = ours[ok].double()
        scale = float(want[k].abs().max())
        err = float((g - want[k]).abs().max())
        err32 = float((t32[k].double() - want[k]).abs().max())
        assert torch.isfinite(ours[ok]).all(), k
        assert err / scale < 2e-5, (k, err, scale)
        assert err <= max(3 * err32, 1e-6 * scale), (k, err, err32, scale)


def _narrow_grads(lstm, x, h0, c0, dhs):
    hs, _, _, gates, cs = hip.lstm_narrow_forward(x, h0, c0, *_params(lstm), save=True)
    return hip.lstm_narrow_backward(x, h0, c0, lstm.weight_hh_l0.detach(), hs, gates, cs, dhs)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("b,l,d_in", [(1, 1, 1), (1, 5, 4), (31, 3, 4), (64, 1, 5), (257, 8, 16), (4097, 2, 3)])
@pytest.mark.parametrize("where", ["every_step", "h_n_only"])
def test_backward_matches_fp64_autograd(hidden, b, l, d_in, where):
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(b, l, d_in, hidden)
    g = torch.Generator(device=DEV).manual_seed(7)
    dhs = torch.randn(b, l, hidden, device=DEV, generator=g)
    if where == "h_n_only":
        dhs[:, :-1] = 0
    ours = _narrow_grads(lstm, x, h0, c0, dhs)
    _check_grads(ours, _torch_grads(lstm, x, h0, c0, dhs, torch.float64),
                 _torch_grads(lstm, x, h0, c0, dhs, torch.float32))


@pytest.mark.parametrize("hidden", [64, 128])
def test_backward_repeats_bit_for_bit(hidden):
    lstm = _lstm(hidden, 4)
    x, h0, c0 = _inputs(3000, 4, 4, hidden)
    dhs = torch.randn(3000, 4, hidden, device=DEV)
    a, b = _narrow_grads(lstm, x, h0, c0, dhs), _narrow_grads(lstm, x, h0, c0, dhs)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("hidden", [64, 128])
def test_saturated_gates_and_large_cell_states(hidden):
    """|c0| ~ 4e3 and pre-activations driven into saturation by inputs x 50: finite, within the bars above."""
    lstm = _lstm(hidden, 3)
    x, h0, c0 = _inputs(200, 4, 3, hidden, x_scale=50.0, c_scale=4e3)
    hs, hn, cn, _, _ = hip.lstm_narrow_forward(x, h0, c0, *_params(lstm), save=True)
    f32, f64 = _torch(lstm, x, h0, c0, torch.float32), _torch(lstm, x, h0, c0, torch.float64)
    assert torch.isfinite(hs).all() and torch.isfinite(cn).all()
    torch.testing.assert_close(hs, f32[0], rtol=1e-5, atol=2e-6)
    for ours, t32, want in zip((hs, hn, cn), f32, f64):
        err = float((ours.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        assert err <= max(2 * err32, 2e-6), (err, err32)
    dhs = torch.randn(200, 4, hidden, device=DEV)
    _check_grads(_narrow_grads(lstm, x, h0, c0, dhs), _torch_grads(lstm, x, h0, c0, dhs, torch.float64),
                 _torch_grads(lstm, x, h0, c0, dhs, torch.float32))


def _count_module_calls(monkeypatch):
    calls = []
    real = nn.LSTM.forward
    monkeypatch.setattr(nn.LSTM, "forward", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    return calls


def _timed(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        out = fn()
    finally:
        hip.timer.enabled = False
    return out, set(hip.timer.summary())


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("d_in", [1, 4, 16])
def test_lstm_forward_routes_narrow_lstms_to_the_kernels(hidden, d_in, monkeypatch):
    calls = _count_module_calls(monkeypatch)
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(50, 3, d_in, hidden)

    def run():
        out = fused_lstm.lstm_forward(lstm, x, h0, c0)
        assert out is not None
        out[0].sum().backward()
        return out

    _, names = _timed(run)
    assert {"lstm_narrow_forward", "lstm_narrow_backward", "lstm_narrow_reduce"} <= names
    assert not calls


@pytest.mark.parametrize("case", ["h96", "h32", "d17", "layers2", "nobias", "time_major", "proj", "bidirectional",
                                  "fp64", "cpu", "disabled"])
def test_lstm_forward_leaves_other_lstms_to_the_module(case, monkeypatch):
    hidden, d_in, kw, dev, dtype = 64, 4, {}, DEV, torch.float32
    if case == "h96":
        hidden = 96
    elif case == "h32":
        hidden = 32
    elif case == "d17":
        d_in = 17
    elif case == "layers2":
        kw = {"num_layers": 2}
    elif case == "nobias":
        kw = {"bias": False}
    elif case == "proj":
        kw = {"proj_size": 16}
    elif case == "bidirectional":
        kw = {"bidirectional": True}
    elif case == "fp64":
        dtype = torch.float64
    elif case == "cpu":
        dev = "cpu"
    lstm = nn.LSTM(d_in, hidden, batch_first=case != "time_major", **kw).to(dev, dtype)
    x = torch.randn(8, 3, d_in, device=dev, dtype=dtype)
    h0 = torch.zeros(8, hidden, device=dev, dtype=dtype)
    if case == "disabled":
        monkeypatch.setattr(fused_lstm, "ENABLED", False)
    assert fused_lstm.lstm_forward(lstm, x, h0, h0) is None


def _model(model_cls, env_cls, hidden, seed=2):
    env = env_cls(4, 8, device=DEV)
    torch.manual_seed(seed)
    return model_cls(env.observation_spec, env.action_spec, hidden_size=hidden).to(DEV)


MODELS = [(DefaultDiscreteRecurrentModel, DiscreteDummyEnv), (DefaultContinuousRecurrentModel, ContinuousDummyEnv)]


def _model_pass(model, hidden, enabled, b=300, l=4):
    g = torch.Generator(device=DEV).manual_seed(0)
    d_in = model.lstm.input_size
    obs = torch.randn(b, l, d_in, device=DEV, generator=g) * 3
    states = TensorDict(
        {DataKeys.HIDDEN_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g) * 0.3,
         DataKeys.CELL_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g)}, batch_size=[b, l])
    before = fused_lstm.ENABLED
    fused_lstm.ENABLED = enabled
    try:
        model.zero_grad()
        feats, new_states = model(TensorDict({DataKeys.OBS: obs}, batch_size=[b, l]), states)
        outs = [feats[k] for k in sorted(feats.keys())] + [model.value_function()]
        loss = sum((o * torch.randn(o.shape, device=DEV, generator=g)).sum() for o in outs)
        loss.backward()
        return ([o.detach().clone() for o in outs]
                + [new_states[DataKeys.HIDDEN_STATES].detach().clone(), new_states[DataKeys.CELL_STATES].detach().clone()],
                {k: p.grad.clone() for k, p in model.named_parameters()})
    finally:
        fused_lstm.ENABLED = before


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("model_cls,env_cls", MODELS)
def test_default_recurrent_models_match_the_eager_modules(model_cls, env_cls, hidden, monkeypatch):
    """The bars of test_lstm_gpu.py::test_fused_recurrent_model_matches_the_eager_modules."""
    model = _model(model_cls, env_cls, hidden)
    calls = _count_module_calls(monkeypatch)
    (fused, fgrads), names = _timed(lambda: _model_pass(model, hidden, True))
    assert not calls and "lstm_narrow_forward" in names and "lstm_narrow_backward" in names
    eager, egrads = _model_pass(model, hidden, False)
    for a, e in zip(fused, eager):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)
    for k in egrads:
        scale = float(egrads[k].abs().max()) + 1e-12
        assert float((fgrads[k] - egrads[k]).abs().max()) / scale < 5e-5, k


@pytest.mark.parametrize("hidden", [64, 128])
def test_forward_after_an_in_place_optimizer_step_sees_the_new_weights(hidden):
    model = _model(DefaultDiscreteRecurrentModel, DiscreteDummyEnv, hidden)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    _model_pass(model, hidden, True)
    opt.step()
    fused, _ = _model_pass(model, hidden, True)
    eager, _ = _model_pass(model, hidden, False)
    for a, e in zip(fused, eager):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)


def _run_algo(env_cls, hidden, enabled, **config):
    before = fused_lstm.ENABLED
    fused_lstm.ENABLED = enabled
    try:
        torch.manual_seed(11)
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=32, model_config={"hidden_size": hidden},
                                        **config).build(env_cls)
        collect = algo.collect()
        step = algo.step()
        params = torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])
    finally:
        fused_lstm.ENABLED = before
    return collect, step, params


@pytest.mark.parametrize("hidden,env", [(64, "discrete"), (128, "continuous"), (64, "continuous"), (128, "discrete")])
def test_collect_and_step_route_to_the_kernels(hidden, env, monkeypatch):
    env_cls, config = (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv,
                                                                          {"distribution_cls": SquashedNormal})
    calls = _count_module_calls(monkeypatch)
    _, names = _timed(lambda: _run_algo(env_cls, hidden, True, **config))
    assert {"lstm_narrow_forward", "lstm_narrow_backward", "lstm_narrow_reduce"} <= names
    assert not calls, "an eager nn.LSTM ran"


def test_width_256_runs_no_narrow_kernel():
    _, names = _timed(lambda: _run_algo(DiscreteDummyEnv, 256, True))
    assert not any(n.startswith("lstm_narrow") for n in names), names


@pytest.mark.parametrize("hidden,env", [(64, "discrete"), (128, "continuous")])
def test_one_update_matches_the_eager_modules(hidden, env):
    """Losses at rel 1e-5; parameters at the bar of test_mlp_narrow_gpu.py::test_one_update_matches_the_eager_modules."""
    env_cls, config = (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv,
                                                                          {"distribution_cls": SquashedNormal})
    _, s0, p0 = _run_algo(env_cls, hidden, True, **config)
    _, s1, p1 = _run_algo(env_cls, hidden, False, **config)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


def test_training_pass_at_full_size():
    """2^19 sequences x L = 4 (2^21 row-steps) at H = 128, d_in = 1: sampled rows of hs against fp64 at the forward
    bars, the four gradients against fp32 autograd at the bar of test_mlp_narrow_gpu.py::test_headline_row_count."""
    b, l, hidden = 1 << 19, 4, 128
    lstm = _lstm(hidden, 1)
    x, h0, c0 = _inputs(b, l, 1, hidden)
    dhs = torch.randn(b, l, hidden, device=DEV) / b
    hs, _, _, gates, cs = hip.lstm_narrow_forward(x, h0, c0, *_params(lstm), save=True)
    grads = hip.lstm_narrow_backward(x, h0, c0, lstm.weight_hh_l0.detach(), hs, gates, cs, dhs)
    assert torch.isfinite(hs).all()
    rows = torch.randint(0, b, (2048,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    sub = _lstm(hidden, 1)
    want = _torch(sub, x[rows], h0[rows], c0[rows], torch.float64)[0]
    got32 = _torch(sub, x[rows], h0[rows], c0[rows], torch.float32)[0]
    torch.testing.assert_close(hs[rows], want.float(), rtol=1e-5, atol=2e-6)
    assert float((hs[rows].double() - want).abs().max()) <= max(2 * float((got32.double() - want).abs().max()), 2e-6)
    del gates, cs
    want_g = _torch_grads(lstm, x, h0, c0, dhs, torch.float32)
    for k, ok in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b"), ("bias_hh_l0", "b")):
        assert torch.isfinite(grads[ok]).all(), k
        scale = float(want_g[k].abs().max())
        torch.testing.assert_close(grads[ok], want_g[k], rtol=1e-4, atol=1e-6 * max(scale, 1.0), msg=k)
