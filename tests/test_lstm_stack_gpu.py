"""Stacked LSTMs (num_layers >= 2, hidden width 64 / 128; lstm_narrow_stack_* kernels): the whole stack through
``fused_lstm.lstm_stack_forward`` against ``nn.LSTM`` in fp32 and fp64 -- forward, all ``4 * layers`` parameter
gradients (the only witness of the input gradient dx: a wrong one shows in the lower layers' weights), the two launch
modes and two backward passes bit for bit -- then the routing, the default recurrent models and one collect() +
step() of PPO fused against the eager modules, and one training pass at full size."""

import gc

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
# (b, l, d_in): both sides of the 16 / 32-row tiles and of the 64-row weight-gradient stages; d_in 1, 4 and 16
SHAPES = [(1, 1, 1), (1, 5, 4), (31, 3, 16), (33, 2, 1), (257, 8, 4), (4097, 2, 16)]
STACK_LABELS = {"lstm_stack_forward", "lstm_stack_backward", "lstm_stack_reduce"}


@pytest.fixture(autouse=True)
def _release_device_memory():
    """Hand the allocator's cached blocks back after each test (the full-size pass and the eager runs leave > 100 GiB
    cached): later files of the suite decide by the free device memory whether their full-size tests run."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _grad_names(layers):
    return [f"{n}_l{k}" for k in range(layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _lstm(hidden, d_in, layers, seed=0, **kw):
    torch.manual_seed(seed)
    return nn.LSTM(d_in, hidden, num_layers=layers, batch_first=True, **kw).to(DEV)


def _inputs(b, l, d_in, hidden, layers, seed=1, x_scale=1.0, c_scale=1.0):
    """x [B, L, d], h0 / c0 [B, layers, H]: the rollout buffer's layout."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, l, d_in, device=DEV, generator=g) * x_scale
    h0 = torch.randn(b, layers, hidden, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, layers, hidden, device=DEV, generator=g) * c_scale
    return x, h0, c0


def _ref(lstm, dtype):
    ref = nn.LSTM(lstm.input_size, lstm.hidden_size, num_layers=lstm.num_layers, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    return ref


def _torch(lstm, x, h0, c0, dtype):
    """hs [B, L, H], h_n, c_n [B, layers, H] of the module in ``dtype`` (cuDNN / MIOpen off)."""
    ref = _ref(lstm, dtype)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        hs, (hn, cn) = ref(x.to(dtype), (h0.transpose(0, 1).contiguous().to(dtype),
                                         c0.transpose(0, 1).contiguous().to(dtype)))
    return hs, hn.transpose(0, 1), cn.transpose(0, 1)


def _torch_grads(lstm, x, h0, c0, dhs, dtype):
    ref = _ref(lstm, dtype)
    with torch.backends.cudnn.flags(enabled=False):
        hs, _ = ref(x.to(dtype), (h0.transpose(0, 1).contiguous().to(dtype), c0.transpose(0, 1).contiguous().to(dtype)))
        (hs * dhs.to(dtype)).sum().backward()
    return {k: getattr(ref, k).grad for k in _grad_names(lstm.num_layers)}


def _stack_grads(lstm, x, h0, c0, dhs):
    lstm.zero_grad()
    out = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)
    assert out is not None
    (out[0] * dhs).sum().backward()
    return {k: getattr(lstm, k).grad.clone() for k in _grad_names(lstm.num_layers)}


def _check_forward(ours, f32, f64, what):
    """The one-layer bars against torch fp32 (rtol 1e-5, atol 2e-6; atol 4e-6 on c_n), and the bar that decides over
    several layers: the error against fp64 at most 3x torch-fp32's own on the same inputs, the one-layer atol as the
    floor. Every row of every output is compared."""
    for name, a, t32, want, atol in zip(("hs", "h_n", "c_n"), ours, f32, f64, (2e-6, 2e-6, 4e-6)):
        assert a.shape == want.shape, (what, name, a.shape, want.shape)
        assert torch.isfinite(a).all(), (what, name)
        err = float((a.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        print(f"{what} {name}: err vs fp64 {err:.3e}, torch fp32 vs fp64 {err32:.3e}")
        assert err <= max(3 * err32, atol), (what, name, err, err32)
        torch.testing.assert_close(a, t32, rtol=1e-5, atol=atol, msg=lambda m: f"{what} {name}: {m}")


def _check_grads(ours, want, t32, what=""):
    """The bars of test_lstm_narrow_gpu.py::_check_grads, for every parameter of every layer."""
    for k in want:
        g = ours[k].double()
        scale = float(want[k].abs().max())
        err = float((g - want[k]).abs().max())
        err32 = float((t32[k].double() - want[k]).abs().max())
        print(f"{what} {k}: err {err:.3e}, torch fp32 {err32:.3e}, scale {scale:.3e}")
        assert torch.isfinite(ours[k]).all(), k
        assert err / scale < 2e-5, (k, err, scale)
        assert err <= max(3 * err32, 1e-6 * scale), (k, err, err32, scale)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("b,l,d_in", SHAPES)
def test_forward_matches_torch(hidden, layers, b, l, d_in):
    lstm = _lstm(hidden, d_in, layers)
    x, h0, c0 = _inputs(b, l, d_in, hidden, layers)
    train = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)  # parameters require a gradient: gates and cells saved
    with torch.no_grad():
        infer = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)
    assert train is not None and infer is not None and train[0].requires_grad and not infer[0].requires_grad
    for a, e in zip(train, infer):
        assert torch.equal(a.detach(), e), "inference and training launches differ"
    assert torch.equal(infer[0][:, -1], infer[1][:, -1]), "h_n of the top layer is not the last step of hs"
    _check_forward(infer, _torch(lstm, x, h0, c0, torch.float32), _torch(lstm, x, h0, c0, torch.float64),
                   f"H{hidden} layers{layers} b{b} l{l} d{d_in}")


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("b,l", [(1, 1), (33, 2), (257, 8)])
def test_one_upper_layer_matches_a_one_layer_module(hidden, b, l):
    """The hip-level entries of one upper layer (an H-wide x) against nn.LSTM(H, H): hs of every step, the saved
    gates and cell states, and dx against fp64 autograd's gradient of x."""
    torch.manual_seed(3)
    ref = nn.LSTM(hidden, hidden, batch_first=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(b, l, hidden, device=DEV, generator=g) * 2 - 1  # (a lower layer's outputs lie in (-1, 1))
    h0 = torch.randn(b, hidden, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, hidden, device=DEV, generator=g)
    dhs = torch.randn(b, l, hidden, device=DEV, generator=g)
    w = [p.detach() for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)]
    hs, hn, cn, gates, cs = hip.lstm_stack_forward(x, h0, c0, *w, save=True)
    assert torch.equal(hs[:, -1], hn) and torch.equal(cs[:, -1], cn)
    i, f, gg, o = gates.double().unbind(2)
    c_prev = torch.cat([c0[:, None].double(), cs[:, :-1].double()], 1)
    torch.testing.assert_close(cs.double(), f * c_prev + i * gg, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(hs.double(), o * torch.tanh(cs.double()), rtol=1e-5, atol=2e-6)
    got = hip.lstm_stack_backward(x, h0, c0, w[0], w[1], hs, gates, cs, dhs)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        m = nn.LSTM(hidden, hidden, batch_first=True).to(DEV, dtype)
        m.load_state_dict(ref.state_dict())
        xd = x.to(dtype).requires_grad_()
        with torch.backends.cudnn.flags(enabled=False):
            out, _ = m(xd, (h0[None].to(dtype), c0[None].to(dtype)))
            (out * dhs.to(dtype)).sum().backward()
        grads[dtype] = {"dx": xd.grad, "w_ih": m.weight_ih_l0.grad, "w_hh": m.weight_hh_l0.grad, "b": m.bias_ih_l0.grad,
                        "hs": out.detach()}
    err = float((hs.double() - grads[torch.float64]["hs"]).abs().max())
    err32 = float((grads[torch.float32]["hs"].double() - grads[torch.float64]["hs"]).abs().max())
    assert err <= max(3 * err32, 2e-6), (err, err32)
    for k in ("dx", "w_ih", "w_hh", "b"):
        want = grads[torch.float64][k]
        scale = float(want.abs().max())
        e = float((got[k].double() - want).abs().max())
        e32 = float((grads[torch.float32][k].double() - want).abs().max())
        print(f"H{hidden} b{b} l{l} {k}: err {e:.3e}, torch fp32 {e32:.3e}, scale {scale:.3e}")
        assert e / scale < 2e-5, (k, e, scale)
        assert e <= max(3 * e32, 1e-6 * scale), (k, e, e32, scale)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("b,l,d_in", SHAPES)
@pytest.mark.parametrize("where", ["every_step", "h_n_only"])
def test_backward_matches_fp64_autograd(hidden, layers, b, l, d_in, where):
    lstm = _lstm(hidden, d_in, layers)
    x, h0, c0 = _inputs(b, l, d_in, hidden, layers)
    g = torch.Generator(device=DEV).manual_seed(7)
    dhs = torch.randn(b, l, hidden, device=DEV, generator=g)
    if where == "h_n_only":
        dhs[:, :-1] = 0
    ours = _stack_grads(lstm, x, h0, c0, dhs)
    _check_grads(ours, _torch_grads(lstm, x, h0, c0, dhs, torch.float64),
                 _torch_grads(lstm, x, h0, c0, dhs, torch.float32), f"H{hidden} layers{layers} b{b} l{l} d{d_in} {where}")


@pytest.mark.parametrize("hidden", [64, 128])
def test_backward_repeats_bit_for_bit(hidden):
    lstm = _lstm(hidden, 4, 3)
    x, h0, c0 = _inputs(3000, 4, 4, hidden, 3)
    dhs = torch.randn(3000, 4, hidden, device=DEV)
    a, b = _stack_grads(lstm, x, h0, c0, dhs), _stack_grads(lstm, x, h0, c0, dhs)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("hidden", [64, 128])
def test_saturated_gates_and_large_cell_states(hidden):
    """|c0| ~ 4e3 and pre-activations driven into saturation by inputs x 50 (the narrow test's inputs): finite,
    within the forward bar."""
    lstm = _lstm(hidden, 3, 2)
    x, h0, c0 = _inputs(200, 4, 3, hidden, 2, x_scale=50.0, c_scale=4e3)
    with torch.no_grad():
        ours = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)
    f32, f64 = _torch(lstm, x, h0, c0, torch.float32), _torch(lstm, x, h0, c0, torch.float64)
    for name, a, t32, want in zip(("hs", "h_n", "c_n"), ours, f32, f64):
        assert torch.isfinite(a).all(), name
        err = float((a.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        print(f"saturated H{hidden} {name}: err {err:.3e}, torch fp32 {err32:.3e}")
        assert err <= max(3 * err32, 2e-6), (name, err, err32)
    torch.testing.assert_close(ours[0], f32[0], rtol=1e-5, atol=2e-6)
    dhs = torch.randn(200, 4, hidden, device=DEV)
    _check_grads(_stack_grads(lstm, x, h0, c0, dhs), _torch_grads(lstm, x, h0, c0, dhs, torch.float64),
                 _torch_grads(lstm, x, h0, c0, dhs, torch.float32), f"saturated H{hidden}")


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


def _run_algo(env_cls, hidden, enabled, layers=2, **config):
    before = fused_lstm.ENABLED
    fused_lstm.ENABLED = enabled
    try:
        torch.manual_seed(11)
        model_config = {"hidden_size": hidden, "num_layers": layers} if layers != 1 else {"hidden_size": hidden}
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=32, model_config=model_config, **config).build(env_cls)
        collect = algo.collect()
        step = algo.step()
        params = torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])
    finally:
        fused_lstm.ENABLED = before
    return collect, step, params


def _env(env):
    return (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv, {"distribution_cls": SquashedNormal})


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_collect_and_step_of_a_two_layer_model_run_the_module_when_disabled(hidden, env, monkeypatch):
    """The eager route of a stacked model (run first: no test built one before)."""
    env_cls, config = _env(env)
    calls = _count_module_calls(monkeypatch)
    (_, step, params), names = _timed(lambda: _run_algo(env_cls, hidden, False, **config))
    assert calls, "the module did not run"
    assert not any(n.startswith(("lstm_stack", "lstm_narrow")) for n in names), names
    assert torch.isfinite(params).all() and all(v == v for v in step.values() if isinstance(v, float))


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_collect_and_step_of_a_two_layer_model_route_to_the_kernels(hidden, env, monkeypatch):
    env_cls, config = _env(env)
    calls = _count_module_calls(monkeypatch)
    _, names = _timed(lambda: _run_algo(env_cls, hidden, True, **config))
    assert STACK_LABELS | {"lstm_narrow_forward", "lstm_narrow_backward", "lstm_narrow_reduce"} <= names, names
    assert not calls, "an eager nn.LSTM ran"


def test_a_one_layer_model_runs_no_stack_kernel():
    _, names = _timed(lambda: _run_algo(DiscreteDummyEnv, 64, True, layers=1))
    assert "lstm_narrow_forward" in names and not any(n.startswith("lstm_stack") for n in names), names


@pytest.mark.parametrize("case", ["h256", "h96", "nobias", "dropout", "d17", "layers1", "time_major", "proj",
                                  "bidirectional", "fp64", "cpu", "disabled"])
def test_lstm_stack_forward_leaves_other_lstms_to_the_module(case, monkeypatch):
    hidden, d_in, kw, dev, dtype = 64, 4, {"num_layers": 2}, DEV, torch.float32
    if case == "h256":
        hidden = 256
    elif case == "h96":
        hidden = 96
    elif case == "nobias":
        kw["bias"] = False
    elif case == "dropout":
        kw["dropout"] = 0.1
    elif case == "d17":
        d_in = 17
    elif case == "layers1":
        kw["num_layers"] = 1
    elif case == "proj":
        kw["proj_size"] = 16
    elif case == "bidirectional":
        kw["bidirectional"] = True
    elif case == "fp64":
        dtype = torch.float64
    elif case == "cpu":
        dev = "cpu"
    lstm = nn.LSTM(d_in, hidden, batch_first=case != "time_major", **kw).to(dev, dtype)
    x = torch.randn(8, 3, d_in, device=dev, dtype=dtype)
    h0 = torch.zeros(8, kw["num_layers"], hidden, device=dev, dtype=dtype)
    if case == "disabled":
        monkeypatch.setattr(fused_lstm, "ENABLED", False)
    assert fused_lstm.lstm_stack_forward(lstm, x, h0, h0) is None


def test_lstm_forward_still_leaves_a_stack_to_its_own_entry():
    lstm = _lstm(64, 4, 2)
    x, h0, _ = _inputs(8, 3, 4, 64, 2)
    assert fused_lstm.lstm_forward(lstm, x, h0[:, 0], h0[:, 0]) is None
    assert fused_lstm.lstm_stack_forward(lstm, x, h0, h0) is not None


def _model(model_cls, env_cls, hidden, layers=2, seed=2):
    env = env_cls(4, 8, device=DEV)
    torch.manual_seed(seed)
    return model_cls(env.observation_spec, env.action_spec, hidden_size=hidden, num_layers=layers).to(DEV)


MODELS = [(DefaultDiscreteRecurrentModel, DiscreteDummyEnv), (DefaultContinuousRecurrentModel, ContinuousDummyEnv)]


def _model_pass(model, hidden, enabled, layers=2, b=300, l=4):
    g = torch.Generator(device=DEV).manual_seed(0)
    d_in = model.lstm.input_size
    obs = torch.randn(b, l, d_in, device=DEV, generator=g) * 3
    states = TensorDict(
        {DataKeys.HIDDEN_STATES: torch.randn(b, l, layers, hidden, device=DEV, generator=g) * 0.3,
         DataKeys.CELL_STATES: torch.randn(b, l, layers, hidden, device=DEV, generator=g)}, batch_size=[b, l])
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
    """Outputs, values and new states at the forward bar; gradients at the bar of
    test_lstm_gpu.py::test_fused_recurrent_model_matches_the_eager_modules."""
    model = _model(model_cls, env_cls, hidden)
    calls = _count_module_calls(monkeypatch)
    (fused, fgrads), names = _timed(lambda: _model_pass(model, hidden, True))
    assert not calls and STACK_LABELS <= names, names
    eager, egrads = _model_pass(model, hidden, False)
    assert calls
    assert fused[-1].shape == (300, 2, hidden)
    for a, e in zip(fused, eager):
        assert a.shape == e.shape
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)
    assert set(fgrads) == set(egrads)
    for k in egrads:
        scale = float(egrads[k].abs().max()) + 1e-12
        assert float((fgrads[k] - egrads[k]).abs().max()) / scale < 5e-5, k


@pytest.mark.parametrize("hidden", [64, 128])
def test_forward_after_an_in_place_optimizer_step_sees_the_new_weights(hidden):
    model = _model(DefaultDiscreteRecurrentModel, DiscreteDummyEnv, hidden, layers=3)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    before, _ = _model_pass(model, hidden, True, layers=3)
    opt.step()
    fused, _ = _model_pass(model, hidden, True, layers=3)
    eager, _ = _model_pass(model, hidden, False, layers=3)
    assert not torch.equal(before[-1][:, 2], fused[-1][:, 2])
    for a, e in zip(fused, eager):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("hidden,env", [(64, "discrete"), (128, "continuous")])
def test_one_update_matches_the_eager_modules(hidden, env):
    """Losses at rel 1e-5, parameters at rtol 1e-4 / atol 1e-5: the bars of test_lstm_narrow_gpu.py."""
    env_cls, config = _env(env)
    _, s0, p0 = _run_algo(env_cls, hidden, True, **config)
    _, s1, p1 = _run_algo(env_cls, hidden, False, **config)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


def test_training_pass_at_full_size():
    """2^19 sequences x L = 4 (2^21 row-steps) at H = 128, 2 layers, d_in = 1: finite everywhere, sampled rows of the
    top hs against fp64 at the forward bar, every gradient against fp32 autograd at
    rtol 1e-4, atol 1e-6 max(scale, 1)."""
    b, l, hidden, layers = 1 << 19, 4, 128, 2
    lstm = _lstm(hidden, 1, layers)
    x, h0, c0 = _inputs(b, l, 1, hidden, layers)
    dhs = torch.randn(b, l, hidden, device=DEV) / b
    lstm.zero_grad()
    hs, hn, cn = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)
    (hs * dhs).sum().backward()
    hs, hn, cn = hs.detach(), hn.detach(), cn.detach()  # (drops the graph and with it the saved gates and cell states)
    grads = {k: getattr(lstm, k).grad.clone() for k in _grad_names(layers)}
    lstm.zero_grad(set_to_none=True)
    assert torch.isfinite(hs).all() and torch.isfinite(hn).all() and torch.isfinite(cn).all()
    rows = torch.randint(0, b, (2048,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    f64 = _torch(lstm, x[rows], h0[rows], c0[rows], torch.float64)
    f32 = _torch(lstm, x[rows], h0[rows], c0[rows], torch.float32)
    _check_forward((hs[rows], hn[rows], cn[rows]), f32, f64, "full size")
    del hs, hn, cn
    torch.cuda.empty_cache()
    want_g = _torch_grads(lstm, x, h0, c0, dhs, torch.float32)
    for k in _grad_names(layers):
        assert torch.isfinite(grads[k]).all(), k
        scale = float(want_g[k].abs().max())
        torch.testing.assert_close(grads[k], want_g[k], rtol=1e-4, atol=1e-6 * max(scale, 1.0), msg=k)
