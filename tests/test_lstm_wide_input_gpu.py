"""The width-256 LSTM behind 8 to 128 input floats (rl8_amd/csrc/lstm_wide_in_kernels.hip) on the GPU, against
``torch.nn.LSTM`` in float64 on the same fp32 inputs and parameters.

Yardstick: with ``ref64`` the float64 module and ``ref32`` the float32 one (cudnn flags off), a kernel result ``k``
passes when ``max|k - ref64| <= 3 max|ref32 - ref64| + 2^-23 max|ref64|`` over ALL elements -- three times what
torch's own fp32 evaluation is off (the project's bar for its fp32-MFMA kernels, tests/test_mlp_split_gpu.py) plus one
rounding of the output."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402

DEV = "cuda:0"
ULP = 2.0 ** -23


def reference_lstm(d_in, seed):
    torch.manual_seed(seed)
    return torch.nn.LSTM(d_in, 256, num_layers=1, batch_first=True).to(DEV)


def pack(lstm):
    return hip.lstm_wide_in_pack(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)


def inputs(b, l, d_in, seed, with_dhs=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, l, d_in, device=DEV, generator=g) * 3
    h0 = torch.randn(b, 256, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, 256, device=DEV, generator=g)
    if with_dhs:
        return x, h0, c0, torch.randn(b, l, 256, device=DEV, generator=g) / (b * l)
    return x, h0, c0


def holds(name, k, ref32, ref64):
    """The yardstick of the module docstring; prints its figures before it asserts."""
    err = float((k.double() - ref64).abs().max())
    own = float((ref32.double() - ref64).abs().max())
    bound = 3.0 * own + ULP * float(ref64.abs().max())
    print(f"{name}: |k - ref64| = {err:.3e}, |ref32 - ref64| = {own:.3e}, bound = {bound:.3e}")
    assert err <= bound, (name, err, own, bound)


def run_module(lstm, x, h0, c0, dhs=None):
    """(hs, h_n, c_n[, parameter gradients]) of ``lstm`` in its own dtype."""
    dt = lstm.weight_hh_l0.dtype
    lstm.zero_grad()
    with torch.backends.cudnn.flags(enabled=False), torch.set_grad_enabled(dhs is not None):
        out, (hn, cn) = lstm(x.to(dt), (h0.to(dt).unsqueeze(0), c0.to(dt).unsqueeze(0)))
        if dhs is None:
            return out, hn[0], cn[0]
        out.backward(dhs.to(dt))
    return {"w_ih": lstm.weight_ih_l0.grad, "w_hh": lstm.weight_hh_l0.grad, "b": lstm.bias_ih_l0.grad}


FORWARD_SHAPES = [(1, 1, 8), (31, 3, 9), (32, 4, 15), (33, 2, 16), (100, 5, 17), (257, 3, 40), (64, 2, 64), (1000, 3, 127),
                  (4097, 2, 128), (16417, 1, 24)]


@pytest.mark.parametrize("b,l,d_in", FORWARD_SHAPES)
def test_forward_holds_to_fp64(b, l, d_in):
    """A lone row, the 32-row tile edge, the k-group edge (15 -> 16 columns, 16 -> 17), every compiled class of extra
    k-groups, both ends of the envelope, and more tiles than the grid has workgroups."""
    lstm = reference_lstm(d_in, b + l)
    x, h0, c0 = inputs(b, l, d_in, b)
    ref32 = run_module(lstm, x, h0, c0)
    ref64 = run_module(copy.deepcopy(lstm).double(), x, h0, c0)
    packed = pack(lstm)
    assert packed.numel() == 1024 * (256 + 8 * math.ceil((d_in + 1) / 8))
    hs, hn, cn, gates, cs = hip.lstm_wide_in_forward(x, h0, c0, packed, save=True)
    for name, k, r32, r64 in zip(("hs", "h_n", "c_n"), (hs, hn, cn), ref32, ref64):
        holds(name, k, r32, r64)
    assert torch.equal(hs[:, -1], hn) and torch.equal(cs[:, -1], cn)
    # saved gates reproduce the cell update: c_t = f c_{t-1} + i g, h_t = o tanh(c_t)
    i, f, gg, o = gates.unbind(2)
    c_prev = torch.cat([c0.unsqueeze(1), cs[:, :-1]], 1)
    torch.testing.assert_close(cs, f * c_prev + i * gg, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(hs, o * torch.tanh(cs), rtol=1e-5, atol=2e-6)
    # inference launch: same bits, nothing saved
    hs2, hn2, cn2, none_g, none_c = hip.lstm_wide_in_forward(x, h0, c0, packed)
    assert none_g is None and none_c is None
    assert torch.equal(hs2, hs) and torch.equal(hn2, hn) and torch.equal(cn2, cn)


def test_weights_changed_in_place_are_repacked():
    from rl8_amd.nn import fused_lstm

    lstm = reference_lstm(24, 1)
    x, h0, c0 = inputs(40, 3, 24, 2)
    with torch.no_grad():
        first = fused_lstm.lstm_forward(lstm, x, h0, c0)
        kept = fused_lstm._packs(lstm, "wide")
        assert fused_lstm._packs(lstm, "wide") is kept  # cached while nothing changes
        lstm.weight_ih_l0.mul_(0.5)
        lstm.bias_hh_l0.add_(0.25)
        second = fused_lstm.lstm_forward(lstm, x, h0, c0)
        assert fused_lstm._packs(lstm, "wide") is not kept
        ref32 = run_module(lstm, x, h0, c0)
        ref64 = run_module(copy.deepcopy(lstm).double(), x, h0, c0)
    assert not torch.equal(first[0], second[0])
    for name, k, r32, r64 in zip(("hs", "h_n", "c_n"), second, ref32, ref64):
        holds(name, k, r32, r64)


def test_argument_checks():
    assert [hip.lstm_wide_in_supports(d) for d in (7, 8, 128, 129)] == [False, True, True, False]
    lstm = reference_lstm(24, 0)
    packed = pack(lstm)
    x = torch.zeros(4, 2, 24, device=DEV)
    state = torch.zeros(4, 256, device=DEV)
    with pytest.raises(ValueError):
        hip.lstm_wide_in_forward(x, torch.zeros(4, 128, device=DEV), state, packed)
    with pytest.raises(ValueError):
        hip.lstm_wide_in_forward(torch.zeros(4, 2, 40, device=DEV), state, state, packed)  # a pack of another depth
    with pytest.raises(ValueError):
        hip.lstm_wide_in_forward(torch.zeros(4, 2, 7, device=DEV), state, state, packed)
    with pytest.raises(ValueError):
        hip.lstm_wide_in_pack(lstm.weight_ih_l0[:, :7].contiguous(), lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
    with pytest.raises(ValueError):
        hip.lstm_wide_in_wgrad(torch.zeros(8, 1024, device=DEV), torch.zeros(9, 24, device=DEV))


# (700, 3, 24): 2100 rows, just past the 64 x 32 rows one pass of the weight-gradient kernel's slabs covers
BACKWARD_SHAPES = [(1, 1, 8), (33, 3, 16), (300, 5, 17), (2000, 4, 40), (4097, 2, 128), (700, 3, 24)]


@pytest.mark.parametrize("b,l,d_in", BACKWARD_SHAPES)
def test_weight_gradients_on_both_routes(b, l, d_in):
    """The all-fp32 route (rl8_lstm_backward_dgates_f32 + "f32") to the yardstick; the default plane route (rows kernel,
    fp16-plane W_hh gradient) to the bars tests/test_lstm_gpu.py::test_lstm_backward_on_planes_matches_autograd sets at
    d_in <= 7: 2e-5 of the largest entry off torch's autograd, 5e-6 off the fp32 route."""
    lstm = reference_lstm(d_in, b + 7 * l)
    x, h0, c0, dhs = inputs(b, l, d_in, b + 1, with_dhs=True)
    ref64 = {k: v.clone() for k, v in run_module(copy.deepcopy(lstm).double(), x, h0, c0, dhs).items()}
    ref32 = {k: v.clone() for k, v in run_module(lstm, x, h0, c0, dhs).items()}
    hs, hn, cn, gates, cs = hip.lstm_wide_in_forward(x, h0, c0, pack(lstm), save=True)
    f32 = hip.lstm_backward(x, h0, c0, hs, gates, cs, dhs, hip.lstm_pack_transposed(lstm.weight_hh_l0), wgrad="f32",
                            wide_in=True)
    planes = hip.lstm_backward(x, h0, c0, hs, gates, cs, dhs, None, rows_packed=hip.lstm_rows_backward_pack(lstm.weight_hh_l0),
                               wide_in=True)
    for name in ("w_ih", "w_hh", "b"):
        assert f32[name].shape == ref32[name].shape and planes[name].shape == ref32[name].shape
        scale = float(ref32[name].abs().max()) + 1e-12
        off_autograd = float((planes[name] - ref32[name]).abs().max()) / scale
        off_f32 = float((planes[name] - f32[name]).abs().max()) / scale
        print(f"{name}: planes off autograd {off_autograd:.3e}, off the fp32 route {off_f32:.3e}")
    for name in ("w_ih", "w_hh", "b"):
        holds(name, f32[name], ref32[name], ref64[name])
    for name in ("w_ih", "w_hh", "b"):
        scale = float(ref32[name].abs().max()) + 1e-12
        assert float((planes[name] - ref32[name]).abs().max()) / scale < 2e-5, name
        assert float((planes[name] - f32[name]).abs().max()) / scale < 5e-6, name
    with pytest.raises(ValueError, match="wide_in"):
        hip.lstm_backward(x[:, :, :7].contiguous(), h0, c0, hs, gates, cs, dhs, None, wide_in=True,
                          rows_packed=hip.lstm_rows_backward_pack(lstm.weight_hh_l0))


@pytest.mark.parametrize("m,d_in", [(1, 8), (33, 15), (2049, 16), (5000, 17), (100, 127), (20001, 128), (4096, 24)])
def test_input_weight_gradient_alone(m, d_in):
    """dW_ih = dG^T x and db = the column sums of dG on random operands against the fp64 product: the padding widths
    around a k-group and a column tile (15, 16, 17; 127, 128), one tile, a partial tile, more tiles than slabs."""
    g = torch.Generator(device=DEV).manual_seed(m + d_in)
    dgates = torch.randn(m, 1024, device=DEV, generator=g)
    x = torch.randn(m, d_in, device=DEV, generator=g) * 3
    dw, db = hip.lstm_wide_in_wgrad(dgates, x)
    assert tuple(dw.shape) == (1024, d_in) and tuple(db.shape) == (1024,)
    holds("dw_ih", dw, dgates.t() @ x, dgates.double().t() @ x.double())
    holds("db", db, dgates.sum(0), dgates.double().sum(0))
    dw2, db2 = hip.lstm_wide_in_wgrad(dgates, x)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_forward_and_backward_repeat_bit_for_bit():
    b, l, d_in = 8192, 4, 24
    lstm = reference_lstm(d_in, 3)
    x, h0, c0, dhs = inputs(b, l, d_in, 17, with_dhs=True)
    packed, rows = pack(lstm), hip.lstm_rows_backward_pack(lstm.weight_hh_l0)

    def run():
        hs, hn, cn, gates, cs = hip.lstm_wide_in_forward(x, h0, c0, packed, save=True)
        grads = hip.lstm_backward(x, h0, c0, hs, gates, cs, dhs, None, rows_packed=rows, hs_bound=1.0, wide_in=True)
        return [hs, hn, cn, gates, cs, grads["w_hh"], grads["w_ih"], grads["b"]]

    first = run()
    for trial in range(10):
        for a, c in zip(first, run()):
            assert torch.equal(a, c), trial


# --- model level ---------------------------------------------------------------------------------------------------------
def _model_and_batch(model_cls, d_in, b, l):
    from rl8_amd.data import DataKeys
    from rl8_amd.specs import Categorical as CategoricalSpec, Unbounded
    from rl8_amd.tensordict import TensorDict

    obs_spec = Unbounded(shape=torch.Size([d_in]), device=DEV)
    discrete = "Discrete" in model_cls.__name__
    act_spec = CategoricalSpec(2, shape=torch.Size([1]), device=DEV) if discrete else Unbounded(shape=torch.Size([1]), device=DEV)
    torch.manual_seed(2)
    model = model_cls(obs_spec, act_spec).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.randn(b, l, d_in, device=DEV, generator=g) * 3
    states = TensorDict(
        {DataKeys.HIDDEN_STATES: torch.randn(b, l, 1, 256, device=DEV, generator=g) * 0.3,
         DataKeys.CELL_STATES: torch.randn(b, l, 1, 256, device=DEV, generator=g)}, batch_size=[b, l])
    return model, obs, states


@pytest.mark.parametrize("fuse_heads", [True, False])
@pytest.mark.parametrize("model_name", ["DefaultDiscreteRecurrentModel", "DefaultContinuousRecurrentModel"])
def test_default_models_match_the_eager_modules(model_name, fuse_heads, monkeypatch):
    """Body and bars of tests/test_lstm_gpu.py::test_fused_recurrent_model_matches_the_eager_modules on a 24-float
    observation; a spy shows the new forward ran and ``nn.LSTM.forward`` did not."""
    from rl8_amd import models_recurrent
    from rl8_amd.data import DataKeys
    from rl8_amd.nn import fused_lstm
    from rl8_amd.tensordict import TensorDict

    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM", raising=False)
    monkeypatch.setattr(fused_lstm, "FUSE_HEADS", fuse_heads)
    b, l, d_in = 300, 4, 24
    model, obs, states = _model_and_batch(getattr(models_recurrent, model_name), d_in, b, l)
    g = torch.Generator(device=DEV).manual_seed(1)
    weights = {}
    kernel_calls, module_calls = [], []
    real_forward, real_module = hip.lstm_wide_in_forward, torch.nn.LSTM.forward
    monkeypatch.setattr(hip, "lstm_wide_in_forward", lambda *a, **kw: kernel_calls.append(a[0].shape) or real_forward(*a, **kw))
    monkeypatch.setattr(torch.nn.LSTM, "forward", lambda self, *a, **kw: module_calls.append(1) or real_module(self, *a, **kw))

    def run(enabled):
        fused_lstm.ENABLED = enabled
        try:
            model.zero_grad()
            feats, new_states = model(TensorDict({DataKeys.OBS: obs}, batch_size=[b, l]), states)
            outs = {k: v for k, v in feats.items() if torch.is_tensor(v)}
            outs["value"] = model.value_function()
            loss = 0.0
            for k, v in outs.items():
                if k not in weights:
                    weights[k] = torch.randn(v.shape, device=DEV, generator=g)
                loss = loss + (v * weights[k]).sum()
            loss.backward()
            return ([v.detach().clone() for v in outs.values()]
                    + [new_states[DataKeys.HIDDEN_STATES].detach().clone(), new_states[DataKeys.CELL_STATES].detach().clone()],
                    {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        finally:
            fused_lstm.ENABLED = True

    fused = run(True)
    assert kernel_calls == [(b, l, d_in)] and not module_calls
    eager = run(False)
    assert len(kernel_calls) == 1 and module_calls == [1]
    for a, e in zip(fused[0], eager[0]):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=2e-6)
    assert set(fused[1]) == set(eager[1]) and any("lstm" in k for k in eager[1])
    for k in eager[1]:
        scale = float(eager[1][k].abs().max()) + 1e-12
        assert float((fused[1][k] - eager[1][k]).abs().max()) / scale < 5e-5, k


def test_entries_decline_what_the_family_does_not_take(monkeypatch):
    from rl8_amd.nn import fused_lstm

    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM", raising=False)
    lstm, heads = reference_lstm(24, 0), [torch.nn.Linear(256, 2).to(DEV), torch.nn.Linear(256, 1).to(DEV)]
    x, h0, c0 = inputs(8, 2, 24, 0)
    assert fused_lstm.lstm_forward(lstm, x, h0, c0) is not None
    assert fused_lstm.lstm_heads_forward(lstm, heads, x, h0, c0) is not None
    # an x that requires a gradient under grad mode: the family forms none and must not drop it
    xg = x.clone().requires_grad_()
    assert fused_lstm.lstm_forward(lstm, xg, h0, c0) is None and fused_lstm.lstm_heads_forward(lstm, heads, xg, h0, c0) is None
    with torch.no_grad():
        assert fused_lstm.lstm_forward(lstm, xg, h0, c0) is not None
    for state in ("h0", "c0"):
        kw = {"h0": h0, "c0": c0, state: (h0 if state == "h0" else c0).clone().requires_grad_()}
        assert fused_lstm.lstm_forward(lstm, x, **kw) is None
    # outside the envelope: 7 floats are the "256" family's, 129 nobody's
    assert fused_lstm._wide_input_family(reference_lstm(7, 0)) is None and fused_lstm._family(reference_lstm(7, 0)) == "256"
    wide = reference_lstm(129, 0)
    assert fused_lstm.lstm_forward(wide, torch.zeros(8, 2, 129, device=DEV), h0, c0) is None
    # the switch, read per call
    monkeypatch.setenv("RL8_AMD_WIDE_INPUT_LSTM", "0")
    assert fused_lstm.lstm_forward(lstm, x, h0, c0) is None and fused_lstm.lstm_heads_forward(lstm, heads, x, h0, c0) is None
    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM")
    assert fused_lstm.lstm_forward(lstm, x, h0, c0) is not None


# --- algorithm level -----------------------------------------------------------------------------------------------------
def test_recurrent_algorithm_on_a_24_float_walk_env_runs_the_kernels(monkeypatch):
    """One collect() + step() of the recurrent algorithm on a 24-float walk environment against the SAME seeded run with
    ``RL8_AMD_WIDE_INPUT_LSTM=0`` (torch's LSTM): the rollout's returns to 1e-4, the losses to 2e-3 -- the bars of
    test_recurrent_walk_env_of_four_six_seven_observations_runs_the_plane_lstm -- and the kernel timers name the new
    forward and weight-gradient kernels.  (``seqs_per_state_reset=4``: the default of 8 sequences of 4 steps asks for a
    horizon that 32 divides, which 16 is not; every other setting is the default.)"""
    from rl8_amd import RecurrentAlgorithmConfig

    from ._envs import walk_env

    def run(switch):
        if switch is None:
            monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM", raising=False)
        else:
            monkeypatch.setenv("RL8_AMD_WIDE_INPUT_LSTM", switch)
        torch.manual_seed(13)
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=16, seqs_per_state_reset=4).build(walk_env(24, 3))
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            out = algo.collect(), algo.step()
            return out, hip.timer.summary()
        finally:
            hip.timer.enabled = False
            hip.timer.reset()

    (c1, s1), timed = run(None)
    (c0, s0), timed_off = run("0")
    assert {"lstm_wide_in_forward", "lstm_wide_in_forward_save", "lstm_wide_in_wgrad"} <= set(timed), sorted(timed)
    assert not any(name.startswith("lstm_wide_in") for name in timed_off), sorted(timed_off)
    print(c0["returns/mean"], c1["returns/mean"], {k: (s0[k], s1[k]) for k in ("losses/policy", "losses/vf", "losses/total")})
    assert c1["returns/mean"] == pytest.approx(c0["returns/mean"], rel=1e-4)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s1[k] == pytest.approx(s0[k], rel=2e-3, abs=2e-6), k
