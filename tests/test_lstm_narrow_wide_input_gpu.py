"""Width-64 / 128 LSTMs behind 17 to 128 input floats (rl8_amd/csrc/lstm_narrow_wide_in_kernels.hip) on the GPU, against
``torch.nn.LSTM`` in float64 on the same fp32 inputs and parameters (cudnn flags off).

Forward: the yardstick of tests/test_lstm_wide_input_gpu.py (``holds``): ``max|k - ref64| <= 3 max|ref32 - ref64| +
2^-23 max|ref64|``.  Gradients: the bars of tests/test_lstm_narrow_gpu.py::_check_grads, relative error < 2e-5 and
<= max(3 x torch fp32's error, 1e-6 of the scale), for the four parameters and for ``x``."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import RecurrentAlgorithmConfig, hip, models_recurrent  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.nn import fused_lstm  # noqa: E402
from rl8_amd.specs import Categorical as CategoricalSpec, Unbounded  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402

from ._envs import walk_env  # noqa: E402
from .test_lstm_narrow_gpu import GRADS, _count_module_calls, _inputs, _lstm, _params, _timed, _torch  # noqa: E402
from .test_lstm_wide_input_gpu import holds  # noqa: E402

DEV = "cuda:0"
SWITCH = "RL8_AMD_NARROW_WIDE_INPUT_LSTM"
NEW = {"lstm_narrow_wide_in_proj", "lstm_narrow_wide_in_wgrad", "lstm_narrow_wide_in_reduce"}
HIDDEN = pytest.mark.parametrize("hidden", [64, 128])


@HIDDEN
@pytest.mark.parametrize("b,l,d_in", [(1, 1, 17), (31, 3, 20), (33, 2, 32), (64, 4, 33), (100, 5, 127), (257, 3, 128),
                                      (16417, 1, 24)])
def test_forward_holds_to_fp64(hidden, b, l, d_in):
    """One row at the first width (a padded k-group); both sides of the 32-row tile at exact k-groups; one column into
    a new group; the top of the range; one partial tile beyond the grid cap at both widths."""
    lstm = _lstm(hidden, d_in, seed=b + l)
    x, h0, c0 = _inputs(b, l, d_in, hidden, seed=b, x_scale=3.0)
    hs, hn, cn, gates, cs = hip.lstm_narrow_wide_in_forward(x, h0, c0, *_params(lstm), save=True)
    ref32, ref64 = _torch(lstm, x, h0, c0, torch.float32), _torch(lstm, x, h0, c0, torch.float64)
    for name, k, r32, r64 in zip(("hs", "h_n", "c_n"), (hs, hn, cn), ref32, ref64):
        holds(name, k, r32, r64)
    assert torch.equal(hs[:, -1], hn) and torch.equal(cs[:, -1], cn)
    hs2, hn2, cn2, none_g, none_c = hip.lstm_narrow_wide_in_forward(x, h0, c0, *_params(lstm))
    assert none_g is None and none_c is None
    assert torch.equal(hs2, hs) and torch.equal(hn2, hn) and torch.equal(cn2, cn), "inference and training launches differ"


def _module_grads(lstm, x, h0, c0, dhs, dtype):
    """The four parameter gradients and that of ``x`` from the module's autograd in ``dtype``."""
    ref = nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    xr = x.detach().to(dtype).requires_grad_()
    with torch.backends.cudnn.flags(enabled=False):
        hs, _ = ref(xr, (h0[None].to(dtype), c0[None].to(dtype)))
        (hs * dhs.to(dtype)).sum().backward()
    return {**{k: getattr(ref, k).grad for k in GRADS}, "x": xr.grad}


def _kernel_grads(lstm, x, h0, c0, dhs, x_grad=True):
    lstm.zero_grad()
    xk = x.detach().clone().requires_grad_(x_grad)
    out = fused_lstm.lstm_forward(lstm, xk, h0, c0)
    assert out is not None
    (out[0] * dhs).sum().backward()
    return {**{k: getattr(lstm, k).grad.clone() for k in GRADS}, "x": xk.grad}


@HIDDEN
@pytest.mark.parametrize("b,l,d_in", [(1, 1, 17), (33, 3, 20), (64, 1, 33), (257, 8, 127), (4097, 2, 128)])
@pytest.mark.parametrize("where", ["every_step", "h_n_only"])
def test_gradients_match_fp64_autograd(hidden, b, l, d_in, where, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(b, l, d_in, hidden)
    dhs = torch.randn(b, l, hidden, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    if where == "h_n_only":
        dhs[:, :-1] = 0
    ours, names = _timed(lambda: _kernel_grads(lstm, x, h0, c0, dhs))
    assert NEW | {"lstm_narrow_wide_in_dx"} <= names, sorted(names)
    want, t32 = _module_grads(lstm, x, h0, c0, dhs, torch.float64), _module_grads(lstm, x, h0, c0, dhs, torch.float32)
    for k in (*GRADS, "x"):
        scale = float(want[k].abs().max())
        err = float((ours[k].double() - want[k]).abs().max())
        err32 = float((t32[k].double() - want[k]).abs().max())
        print(f"{k}: err {err:.3e}, torch fp32 {err32:.3e}, scale {scale:.3e}")
        assert torch.isfinite(ours[k]).all() and ours[k].shape == want[k].shape, k
        assert err / scale < 2e-5, (k, err, scale)
        assert err <= max(3 * err32, 1e-6 * scale), (k, err, err32, scale)


@HIDDEN
def test_gradients_repeat_and_dx_runs_only_where_x_wants_it(hidden, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    lstm = _lstm(hidden, 24)
    x, h0, c0 = _inputs(3000, 4, 24, hidden)
    dhs = torch.randn(3000, 4, hidden, device=DEV)
    first, second = _kernel_grads(lstm, x, h0, c0, dhs), _kernel_grads(lstm, x, h0, c0, dhs)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    without, names = _timed(lambda: _kernel_grads(lstm, x, h0, c0, dhs, x_grad=False))
    assert NEW <= names and "lstm_narrow_wide_in_dx" not in names, sorted(names)
    assert without["x"] is None and all(torch.equal(without[k], first[k]) for k in GRADS)


@HIDDEN
@pytest.mark.parametrize("d_in", [17, 128])
def test_switch_on_routes_to_the_kernels(hidden, d_in, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    calls = _count_module_calls(monkeypatch)
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(50, 3, d_in, hidden)

    def run():
        out = fused_lstm.lstm_forward(lstm, x, h0, c0)
        assert out is not None
        out[0].sum().backward()

    _, names = _timed(run)
    assert NEW <= names and not calls, sorted(names)
    assert fused_lstm.lstm_forward(lstm, x, h0.clone().requires_grad_(), c0) is None
    for value in (None, "0", "true", "2"):
        monkeypatch.delenv(SWITCH) if value is None else monkeypatch.setenv(SWITCH, value)
        assert fused_lstm.lstm_forward(lstm, x, h0, c0) is None, value
        monkeypatch.setenv(SWITCH, "1")


@pytest.mark.parametrize("case", ["h96", "d129", "layers2", "nobias", "fp64", "cpu"])
def test_switch_on_leaves_other_lstms_to_the_module(case, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    hidden = 96 if case == "h96" else 64
    d_in = 129 if case == "d129" else 24
    kw = {"layers2": {"num_layers": 2}, "nobias": {"bias": False}}.get(case, {})
    dev, dtype = ("cpu" if case == "cpu" else DEV), (torch.float64 if case == "fp64" else torch.float32)
    lstm = nn.LSTM(d_in, hidden, batch_first=True, **kw).to(dev, dtype)
    x = torch.randn(8, 3, d_in, device=dev, dtype=dtype)
    h0 = torch.zeros(8, hidden, device=dev, dtype=dtype)
    assert fused_lstm.lstm_forward(lstm, x, h0, h0) is None
    assert fused_lstm.lstm_heads_forward(lstm, [nn.Linear(hidden, 2).to(dev, dtype)], x, h0, h0) is None
    if case == "layers2":  # (a stack whose layer 0 is this wide stays on the module)
        states = torch.zeros(8, 2, hidden, device=dev)
        assert fused_lstm.lstm_stack_forward(lstm, x, states, states) is None


@HIDDEN
@pytest.mark.parametrize("model_name", ["DefaultDiscreteRecurrentModel", "DefaultContinuousRecurrentModel"])
def test_default_models_match_the_eager_modules(model_name, hidden, monkeypatch):
    """Two heads (2 + 1 outputs) behind 24 floats through ``lstm_heads_forward``, against the same model with
    ``fused_lstm.ENABLED = False``, at the bars of
    tests/test_lstm_narrow_gpu.py::test_default_recurrent_models_match_the_eager_modules."""
    monkeypatch.setenv(SWITCH, "1")
    b, l, d_in = 300, 4, 24
    obs_spec = Unbounded(shape=torch.Size([d_in]), device=DEV)
    act_spec = (CategoricalSpec(2, shape=torch.Size([1]), device=DEV) if "Discrete" in model_name
                else Unbounded(shape=torch.Size([1]), device=DEV))
    torch.manual_seed(2)
    model = getattr(models_recurrent, model_name)(obs_spec, act_spec, hidden_size=hidden).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.randn(b, l, d_in, device=DEV, generator=g) * 3
    states = TensorDict({DataKeys.HIDDEN_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g) * 0.3,
                         DataKeys.CELL_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g)}, batch_size=[b, l])
    weights = {}

    def run(enabled):
        monkeypatch.setattr(fused_lstm, "ENABLED", enabled)
        model.zero_grad()
        feats, new_states = model(TensorDict({DataKeys.OBS: obs}, batch_size=[b, l]), states)
        outs = {k: v for k, v in feats.items() if torch.is_tensor(v)}
        outs["value"] = model.value_function()
        for k, v in outs.items():
            weights.setdefault(k, torch.randn(v.shape, device=DEV, generator=g))
        sum((v * weights[k]).sum() for k, v in outs.items()).backward()
        return ([v.detach().clone() for v in outs.values()]
                + [new_states[DataKeys.HIDDEN_STATES].detach().clone(), new_states[DataKeys.CELL_STATES].detach().clone()],
                {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})

    calls = _count_module_calls(monkeypatch)
    (fused, fgrads), names = _timed(lambda: run(True))
    assert NEW <= names and not calls, sorted(names)
    eager, egrads = run(False)
    assert calls == [1]
    for a, e in zip(fused, eager):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)
    assert set(fgrads) == set(egrads) and any("lstm" in k for k in egrads)
    for k in egrads:
        scale = float(egrads[k].abs().max()) + 1e-12
        assert float((fgrads[k] - egrads[k]).abs().max()) / scale < 5e-5, k


def test_recurrent_algorithm_on_a_24_float_walk_env(monkeypatch):
    """One collect() + step() at hidden_size 64 on a 24-float walk environment against the same seeded run with the
    switch unset (torch's LSTM): returns to 1e-4, losses to 2e-3 relative and 2e-6 absolute (the bars of
    tests/test_lstm_wide_input_gpu.py's algorithm test); the timers name the new kernels only with the switch on."""
    def run(switch):
        monkeypatch.setenv(SWITCH, "1") if switch else monkeypatch.delenv(SWITCH, raising=False)
        torch.manual_seed(13)
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=16, seqs_per_state_reset=4,
                                        model_config={"hidden_size": 64}).build(walk_env(24, 3))
        return _timed(lambda: (algo.collect(), algo.step()))

    (c1, s1), on = run(True)
    (c0, s0), off = run(False)
    assert NEW <= on, sorted(on)
    assert not any(name.startswith("lstm_narrow_wide_in") for name in off), sorted(off)
    print(c0["returns/mean"], c1["returns/mean"], {k: (s0[k], s1[k]) for k in ("losses/policy", "losses/vf", "losses/total")})
    assert c1["returns/mean"] == pytest.approx(c0["returns/mean"], rel=1e-4)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s1[k] == pytest.approx(s0[k], rel=2e-3, abs=2e-6), k
