"""Stacked LSTMs of width 256 (num_layers >= 2; rl8_amd/csrc/lstm_stack256_kernels.hip) on the GPU, against
``torch.nn.LSTM`` in float32 and float64 (cudnn flags off) on the same fp32 inputs and parameters: the upper-layer forward
and the dx / db launch alone, whole stacks through ``fused_lstm.lstm_stack256_forward`` on the all-fp32 and the default
plane route, then the routing, the default recurrent models and one collect() + step() of PPO against the eager modules.

Yardstick (``holds``, that of tests/test_lstm_wide_input_gpu.py): with ``ref64`` the float64 evaluation and ``ref32``
torch's float32 one, a kernel result ``k`` passes when ``max|k - ref64| <= 3 max|ref32 - ref64| + 2^-23 max|ref64|`` over
ALL elements."""

import functools
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
H = 256
ULP = 2.0 ** -23
NEW_LABELS = {"lstm_stack256_forward", "lstm_stack256_dx"}


@pytest.fixture(autouse=True)
def _switch_on_and_release(monkeypatch):
    """The family's switch on whatever the environment says; the allocator's cached blocks handed back afterwards (later
    files of the suite decide by the free device memory whether their full-size tests run)."""
    monkeypatch.setenv("RL8_AMD_LSTM_STACK_256", "1")
    yield
    gc.collect()
    torch.cuda.empty_cache()


def holds(name, k, ref32, ref64):
    """The yardstick of the module docstring; prints its figures before it asserts."""
    err = float((k.double() - ref64).abs().max())
    own = float((ref32.double() - ref64).abs().max())
    bound = 3.0 * own + ULP * float(ref64.abs().max())
    print(f"{name}: |k - ref64| = {err:.3e}, |ref32 - ref64| = {own:.3e}, bound = {bound:.3e}")
    assert err <= bound, (name, err, own, bound)


# --- the upper-layer forward alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,l", [(1, 1), (31, 3), (33, 2), (257, 3), (16417, 1)])
def test_upper_layer_forward_holds_to_fp64(b, l):
    """A lone row, both sides of the 32-row tile, several tiles, and more tiles than the grid has workgroups."""
    torch.manual_seed(b + l)
    ref = nn.LSTM(H, H, batch_first=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(b)
    x = torch.rand(b, l, H, device=DEV, generator=g) * 2 - 1  # (a lower layer's outputs lie in (-1, 1))
    h0 = torch.randn(b, H, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, H, device=DEV, generator=g)
    refs = []
    for dtype in (torch.float32, torch.float64):
        m = nn.LSTM(H, H, batch_first=True).to(DEV, dtype)
        m.load_state_dict(ref.state_dict())
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            out, (hn, cn) = m(x.to(dtype), (h0[None].to(dtype), c0[None].to(dtype)))
        refs.append((out, hn[0], cn[0]))
    packed = hip.lstm_stack256_pack(ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)
    assert packed.numel() == 1024 * 520
    hs, hn, cn, gates, cs = hip.lstm_stack256_forward(x, h0, c0, packed, save=True)
    for name, k, r32, r64 in zip(("hs", "h_n", "c_n"), (hs, hn, cn), *refs):
        holds(f"b{b} l{l} {name}", k, r32, r64)
    assert torch.equal(hs[:, -1], hn) and torch.equal(cs[:, -1], cn)
    # saved gates reproduce the cell update: c_t = f c_{t-1} + i g, h_t = o tanh(c_t)
    i, f, gg, o = gates.unbind(2)
    c_prev = torch.cat([c0.unsqueeze(1), cs[:, :-1]], 1)
    torch.testing.assert_close(cs, f * c_prev + i * gg, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(hs, o * torch.tanh(cs), rtol=1e-5, atol=2e-6)
    # inference launch: same bits, nothing saved
    hs2, hn2, cn2, none_g, none_c = hip.lstm_stack256_forward(x, h0, c0, packed)
    assert none_g is None and none_c is None
    assert torch.equal(hs2, hs) and torch.equal(hn2, hn) and torch.equal(cn2, cn)


# --- dx / db alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 31, 33, 2049, 20001])
def test_dx_and_db_hold_to_fp64_and_repeat_bit_for_bit(m):
    """A lone row, both sides of the 32-row tile, a ragged last tile behind 64 full ones, and more tiles (626) than the
    grid has workgroups (512)."""
    g = torch.Generator(device=DEV).manual_seed(m)
    dgates = torch.randn(m, 4 * H, device=DEV, generator=g)
    w_ih = torch.randn(4 * H, H, device=DEV, generator=g) / 16
    wiht = hip.lstm_pack_transposed(w_ih)
    dx, db = hip.lstm_stack256_dx(dgates, wiht)
    assert dx.shape == (m, H) and db.shape == (4 * H,)
    holds(f"m{m} dx", dx, dgates @ w_ih, dgates.double() @ w_ih.double())
    holds(f"m{m} db", db, dgates.sum(0), dgates.double().sum(0))
    dx2, db2 = hip.lstm_stack256_dx(dgates, wiht)
    assert torch.equal(dx2, dx) and torch.equal(db2, db)


# --- whole stacks ------------------------------------------------------------------------------------------------------------------
STACKS = [(1, 1, 1, 2), (31, 3, 7, 2), (33, 2, 8, 2), (32, 4, 24, 3), (127, 2, 4, 3), (129, 2, 4, 3), (257, 3, 128, 2),
          (4097, 2, 1, 2)]


def _grad_names(layers):
    return [f"{n}_l{k}" for k in range(layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _lstm(d_in, layers, seed=0, **kw):
    torch.manual_seed(seed)
    return nn.LSTM(d_in, H, num_layers=layers, batch_first=True, **kw).to(DEV)


def _inputs(b, l, d_in, layers, seed=1, x_scale=1.0, c_scale=1.0):
    """x [B, L, d], h0 / c0 [B, layers, 256] (the rollout buffer's layout), dhs [B, L, 256]."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, l, d_in, device=DEV, generator=g) * x_scale
    h0 = torch.randn(b, layers, H, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, layers, H, device=DEV, generator=g) * c_scale
    return x, h0, c0, torch.randn(b, l, H, device=DEV, generator=g) / (b * l)


def _torch(lstm, x, h0, c0, dhs, dtype):
    """((hs, h_n, c_n as [B, layers, 256]), parameter gradients) of the module in ``dtype`` (cuDNN / MIOpen off)."""
    ref = nn.LSTM(lstm.input_size, H, num_layers=lstm.num_layers, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    with torch.backends.cudnn.flags(enabled=False):
        hs, (hn, cn) = ref(x.to(dtype), (h0.transpose(0, 1).contiguous().to(dtype), c0.transpose(0, 1).contiguous().to(dtype)))
        (hs * dhs.to(dtype)).sum().backward()
    return ((hs.detach(), hn.detach().transpose(0, 1), cn.detach().transpose(0, 1)),
            {k: getattr(ref, k).grad for k in _grad_names(lstm.num_layers)})


@functools.lru_cache(maxsize=None)
def _case(b, l, d_in, layers):
    """The module, its inputs and torch's float32 / float64 results for one shape: made once, shared by both routes,
    never written to."""
    lstm = _lstm(d_in, layers, seed=b + l)
    data = _inputs(b, l, d_in, layers, seed=b + d_in)
    return lstm, data, _torch(lstm, *data, torch.float32), _torch(lstm, *data, torch.float64)


def _stack_grads(lstm, x, h0, c0, dhs):
    lstm.zero_grad()
    out = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
    assert out is not None
    (out[0] * dhs).sum().backward()
    grads = {k: getattr(lstm, k).grad.clone() for k in _grad_names(lstm.num_layers)}
    lstm.zero_grad()
    return out, grads


def _check_forward(ours, f32, f64, what):
    """``_check_forward`` of tests/test_lstm_stack_gpu.py: the one-layer bars against torch fp32 (rtol 1e-5, atol 2e-6;
    atol 4e-6 on c_n), and against fp64 at most 3x torch-fp32's own error, the one-layer atol as the floor."""
    for name, a, t32, want, atol in zip(("hs", "h_n", "c_n"), ours, f32, f64, (2e-6, 2e-6, 4e-6)):
        assert a.shape == want.shape, (what, name, a.shape, want.shape)
        assert torch.isfinite(a).all(), (what, name)
        err = float((a.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        print(f"{what} {name}: err vs fp64 {err:.3e}, torch fp32 vs fp64 {err32:.3e}")
        assert err <= max(3 * err32, atol), (what, name, err, err32)
        torch.testing.assert_close(a, t32, rtol=1e-5, atol=atol, msg=lambda m: f"{what} {name}: {m}")


@pytest.mark.parametrize("b,l,d_in,layers", STACKS)
def test_stack_forward_matches_torch(b, l, d_in, layers):
    """Layer 0 on each of its families (d_in 1, 4, 7 | 8, 24, 128), two and three layers, both sides of the 32-row tile
    and of the four-gate weight gradient's 128 sequences; the states of every layer, not the top one's alone."""
    lstm, (x, h0, c0, _), (f32, _), (f64, _) = _case(b, l, d_in, layers)
    train = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)  # parameters require a gradient: gates and cells saved
    with torch.no_grad():
        infer = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
    assert train is not None and infer is not None and train[0].requires_grad and not infer[0].requires_grad
    assert infer[1].shape == (b, layers, H) and infer[2].shape == (b, layers, H)
    for a, e in zip(train, infer):
        assert torch.equal(a.detach(), e), "inference and training launches differ"
    assert torch.equal(infer[0][:, -1], infer[1][:, -1]), "h_n of the top layer is not the last step of hs"
    _check_forward(infer, f32, f64, f"b{b} l{l} d{d_in} layers{layers}")


@pytest.mark.parametrize("b,l,d_in,layers", STACKS)
def test_stack_gradients_on_the_fp32_route_hold_to_fp64(b, l, d_in, layers, monkeypatch):
    """All 4 * layers parameter gradients -- the lower layers' are the only witness of dx -- with every product in fp32."""
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", "f32")
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", False)
    lstm, data, (_, g32), (_, g64) = _case(b, l, d_in, layers)
    _, ours = _stack_grads(lstm, *data)
    for k in _grad_names(layers):
        holds(f"fp32 route b{b} l{l} d{d_in} layers{layers} {k}", ours[k], g32[k], g64[k])


@pytest.mark.parametrize("b,l,d_in,layers", STACKS)
def test_stack_gradients_on_the_default_route_match_autograd(b, l, d_in, layers):
    """The plane routes (rows backward, fp16-plane weight gradients) within 2e-5 of the largest entry off torch's fp32
    autograd: the one-layer bar of test_lstm_gpu.py::test_lstm_backward_on_planes_matches_autograd, for every layer."""
    lstm, data, (_, g32), _ = _case(b, l, d_in, layers)
    _, ours = _stack_grads(lstm, *data)
    worst = []
    for k in _grad_names(layers):
        scale = float(g32[k].abs().max())
        err = float((ours[k] - g32[k]).abs().max())
        print(f"default route b{b} l{l} d{d_in} layers{layers} {k}: err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e}")
        assert torch.isfinite(ours[k]).all(), k
        if not err / scale < 2e-5:
            worst.append((k, err, scale))
    assert not worst, worst


def test_backward_repeats_bit_for_bit():
    lstm = _lstm(4, 3)
    data = _inputs(3000, 4, 4, 3)
    (_, a), (_, b) = _stack_grads(lstm, *data), _stack_grads(lstm, *data)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_weights_changed_in_place_are_repacked_for_every_layer():
    lstm = _lstm(4, 3, seed=5)
    x, h0, c0, dhs = _inputs(40, 3, 4, 3)
    with torch.no_grad():
        first = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
        params = [tuple(getattr(lstm, f"{n}_l{k}") for n in fused_lstm._STACK_PARAMS) for k in range(3)]
        kinds = ["split", "stack256", "stack256"]
        kept = [fused_lstm._layer_packs(p, kind) for p, kind in zip(params, kinds)]
        fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
        for p, kind, pack in zip(params, kinds, kept):  # cached while nothing changes
            assert fused_lstm._layer_packs(p, kind) is pack
        for k in range(3):
            getattr(lstm, f"weight_ih_l{k}").mul_(0.5)
            getattr(lstm, f"bias_hh_l{k}").add_(0.25)
        second = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
        for p, kind, pack in zip(params, kinds, kept):
            assert fused_lstm._layer_packs(p, kind) is not pack
    f32, _ = _torch(lstm, x, h0, c0, dhs, torch.float32)
    f64, _ = _torch(lstm, x, h0, c0, dhs, torch.float64)
    assert not torch.equal(first[0], second[0])
    _check_forward(second, f32, f64, "repacked")
    # ... and the backward's packs: gradients after the change are the changed module's
    _, ours = _stack_grads(lstm, x, h0, c0, dhs)
    _, g32 = _torch(lstm, x, h0, c0, dhs, torch.float32)
    for k in _grad_names(3):
        scale = float(g32[k].abs().max())
        assert float((ours[k] - g32[k]).abs().max()) / scale < 2e-5, k


def test_saturated_gates_and_large_cell_states():
    """|c0| ~ 4e3 and pre-activations driven into saturation by inputs x 50: finite, within the forward bar."""
    lstm = _lstm(3, 2)
    x, h0, c0, dhs = _inputs(200, 4, 3, 2, x_scale=50.0, c_scale=4e3)
    with torch.no_grad():
        ours = fused_lstm.lstm_stack256_forward(lstm, x, h0, c0)
    f32, _ = _torch(lstm, x, h0, c0, dhs, torch.float32)
    f64, _ = _torch(lstm, x, h0, c0, dhs, torch.float64)
    for name, a, t32, want in zip(("hs", "h_n", "c_n"), ours, f32, f64):
        assert torch.isfinite(a).all(), name
        err = float((a.double() - want).abs().max())
        err32 = float((t32.double() - want).abs().max())
        print(f"saturated {name}: err {err:.3e}, torch fp32 {err32:.3e}")
        assert err <= max(3 * err32, 2e-6), (name, err, err32)
    torch.testing.assert_close(ours[0], f32[0], rtol=1e-5, atol=2e-6)


# --- routing -----------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("which", ["x", "h0", "c0"])
def test_an_input_that_requires_a_gradient_is_declined_under_grad_mode_only(which):
    lstm = _lstm(4, 2)
    x, h0, c0, _ = _inputs(8, 3, 4, 2)
    {"x": x, "h0": h0, "c0": c0}[which].requires_grad_()
    out, names = _timed(lambda: fused_lstm.lstm_stack256_forward(lstm, x, h0, c0))
    assert out is None and not any(n.startswith("lstm") for n in names), names
    with torch.no_grad():
        out, names = _timed(lambda: fused_lstm.lstm_stack256_forward(lstm, x, h0, c0))
    assert out is not None and "lstm_stack256_forward" in names, names


@pytest.mark.parametrize("case", ["dropout", "nobias", "d129", "layers1", "time_major", "proj", "bidirectional", "fp64", "cpu",
                                  "disabled", "switch0"])
def test_lstm_stack256_forward_leaves_other_lstms_to_the_module(case, monkeypatch):
    d_in, kw, dev, dtype = 4, {"num_layers": 2}, DEV, torch.float32
    if case == "nobias":
        kw["bias"] = False
    elif case == "dropout":
        kw["dropout"] = 0.1
    elif case == "d129":
        d_in = 129
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
    lstm = nn.LSTM(d_in, H, batch_first=case != "time_major", **kw).to(dev, dtype)
    x = torch.randn(8, 3, d_in, device=dev, dtype=dtype)
    h0 = torch.zeros(8, kw["num_layers"], H, device=dev, dtype=dtype)
    if case == "disabled":
        monkeypatch.setattr(fused_lstm, "ENABLED", False)
    elif case == "switch0":
        monkeypatch.setenv("RL8_AMD_LSTM_STACK_256", "0")
    with torch.no_grad():
        assert fused_lstm.lstm_stack256_forward(lstm, x, h0, h0) is None


def test_the_other_entries_still_decline_a_256_wide_stack():
    lstm = _lstm(4, 2)
    x, h0, _, _ = _inputs(8, 3, 4, 2)
    with torch.no_grad():
        assert fused_lstm.lstm_forward(lstm, x, h0[:, 0], h0[:, 0]) is None
        assert fused_lstm.lstm_stack_forward(lstm, x, h0, h0) is None
        assert fused_lstm.lstm_stack256_forward(lstm, x, h0, h0) is not None


# --- the default recurrent models ----------------------------------------------------------------------------------------------------
def _model(model_cls, env_cls, layers, seed=2):
    env = env_cls(4, 8, device=DEV)
    torch.manual_seed(seed)
    return model_cls(env.observation_spec, env.action_spec, num_layers=layers).to(DEV)


def _model_pass(model, enabled, layers, b=300, l=4):
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.randn(b, l, model.lstm.input_size, device=DEV, generator=g) * 3
    states = TensorDict(
        {DataKeys.HIDDEN_STATES: torch.randn(b, l, layers, H, device=DEV, generator=g) * 0.3,
         DataKeys.CELL_STATES: torch.randn(b, l, layers, H, device=DEV, generator=g)}, batch_size=[b, l])
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


@pytest.mark.parametrize("model_cls,env_cls,layers", [(DefaultDiscreteRecurrentModel, DiscreteDummyEnv, 2),
                                                      (DefaultContinuousRecurrentModel, ContinuousDummyEnv, 2),
                                                      (DefaultDiscreteRecurrentModel, DiscreteDummyEnv, 3)])
def test_default_recurrent_models_match_the_eager_modules(model_cls, env_cls, layers, monkeypatch):
    """One training pass: outputs, values and new states at the forward bar (rtol 1e-5 / atol 2e-6), gradients within
    5e-5 of the largest entry; the module's own forward never runs on the fused side."""
    model = _model(model_cls, env_cls, layers)
    assert model.lstm.hidden_size == H and model.lstm.num_layers == layers
    calls = _count_module_calls(monkeypatch)
    (fused, fgrads), names = _timed(lambda: _model_pass(model, True, layers))
    assert not calls and {"lstm_stack256_forward_save", "lstm_stack256_dx"} <= names, names
    eager, egrads = _model_pass(model, False, layers)
    assert calls
    assert fused[-1].shape == (300, layers, H)
    for a, e in zip(fused, eager):
        assert a.shape == e.shape
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)
    assert set(fgrads) == set(egrads)
    for k in egrads:
        scale = float(egrads[k].abs().max()) + 1e-12
        ratio = float((fgrads[k] - egrads[k]).abs().max()) / scale
        print(f"layers{layers} {k}: {ratio:.3e} of the largest entry")
        assert ratio < 5e-5, k


def _run_algo(env_cls, enabled, **config):
    before = fused_lstm.ENABLED
    fused_lstm.ENABLED = enabled
    try:
        torch.manual_seed(11)
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=32, model_config={"num_layers": 2}, **config).build(env_cls)
        assert algo.policy.model.lstm.hidden_size == H and algo.policy.model.lstm.num_layers == 2
        collect = algo.collect()
        step = algo.step()
        params = torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])
    finally:
        fused_lstm.ENABLED = before
    return collect, step, params


def _env(env):
    return (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv, {"distribution_cls": SquashedNormal})


@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_collect_and_step_of_the_default_two_layer_model_route_to_the_kernels(env, monkeypatch):
    """``model_config={"num_layers": 2}`` at the default width: no eager nn.LSTM, both new kernels timed."""
    env_cls, config = _env(env)
    calls = _count_module_calls(monkeypatch)
    _, names = _timed(lambda: _run_algo(env_cls, True, **config))
    assert not calls, "an eager nn.LSTM ran"
    assert NEW_LABELS <= names, names


@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_the_switch_at_zero_runs_the_module(env, monkeypatch):
    env_cls, config = _env(env)
    monkeypatch.setenv("RL8_AMD_LSTM_STACK_256", "0")
    calls = _count_module_calls(monkeypatch)
    (_, step, params), names = _timed(lambda: _run_algo(env_cls, True, **config))
    assert calls, "the module did not run"
    assert not any(n.startswith("lstm_stack256") for n in names), names
    assert torch.isfinite(params).all() and all(v == v for v in step.values() if isinstance(v, float))


@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_one_update_matches_the_eager_modules(env):
    """Losses at rel 1e-5, parameters at rtol 1e-4 / atol 1e-5: the bars of
    tests/test_lstm_stack_gpu.py::test_one_update_matches_the_eager_modules."""
    env_cls, config = _env(env)
    _, s0, p0 = _run_algo(env_cls, True, **config)
    _, s1, p1 = _run_algo(env_cls, False, **config)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        print(f"{env} {k}: fused {s0[k]!r}, eager {s1[k]!r}")
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    print(f"{env} parameters: max |fused - eager| = {float((p0 - p1).abs().max()):.3e}")
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)
