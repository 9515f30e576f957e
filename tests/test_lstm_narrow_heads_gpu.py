"""The narrow recurrent models' output heads and lean rollout (hidden width 64 / 128): heads forward / backward against
fp64 at the bars of tests/test_lstm_gpu.py; single, pair and in-rollout forms bit for bit; the backward through time
with the heads inside against the array form and fp64 autograd; the default models with and without the one-node
training pass; lean against plumbed rollout; one update against the eager modules; and what runs where."""

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
NEW_TIMERS = ("linear_heads_narrow_forward", "linear_heads_narrow_backward", "rollout_step_dummy_heads_narrow")


def _timed(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        out = fn()
    finally:
        hip.timer.enabled = False
    return out, set(hip.timer.summary())


# --- heads forward / backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("m,n", [(1, 1), (67, 3), (5000, 2), (100_001, 8)])
def test_narrow_heads_match_torch(hidden, m, n):
    """Inputs and bars of tests/test_lstm_gpu.py::test_linear_heads_match_torch (the dots are a quarter or half as
    long); the parameter gradients do not depend on whether dh is written, and repeat bit for bit."""
    g = torch.Generator(device=DEV).manual_seed(m)
    h = torch.randn(m, hidden, device=DEV, generator=g)
    w = (torch.randn(n, hidden, device=DEV, generator=g) / 16).requires_grad_(True)
    b = torch.randn(n, device=DEV, generator=g).requires_grad_(True)
    dout = torch.randn(m, n, device=DEV, generator=g) / m
    hr = h.clone().requires_grad_(True)
    want = torch.nn.functional.linear(hr.double(), w.double(), b.double())
    want.backward(dout.double())
    out = hip.linear_heads_narrow_forward(h, w, b)
    print(f"out max err {float((out.double() - want).abs().max()):.3e}")
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-5)
    dh, dw, db = hip.linear_heads_narrow_backward(h, dout, w)
    for name, ours, ref in (("dh", dh, hr.grad), ("dw", dw, w.grad), ("db", db, b.grad)):
        print(f"{name} max err {float((ours.double() - ref.double()).abs().max()):.3e} of {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(dh.double(), hr.grad.double(), rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(dw.double(), w.grad.double(), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(db.double(), b.grad.double(), rtol=1e-4, atol=1e-7)
    none, dw2, db2 = hip.linear_heads_narrow_backward(h, dout, w, need_dh=False)
    assert none is None and torch.equal(dw2, dw) and torch.equal(db2, db)
    assert torch.equal(hip.linear_heads_narrow_forward(h, w, b), out)
    dh3, dw3, db3 = hip.linear_heads_narrow_backward(h, dout, w)
    assert torch.equal(dh3, dh) and torch.equal(dw3, dw) and torch.equal(db3, db)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("m,n_a,n_b", [(1, 1, 1), (67, 2, 1), (8192, 2, 1), (100_001, 5, 3)])
def test_narrow_heads_pair_is_the_two_single_launches(hidden, m, n_a, n_b):
    """Shapes of tests/test_lstm_gpu.py::test_linear_heads_pair_is_the_two_single_launches; also against the stacked
    single launch the models' forward makes: one output's arithmetic depends on the width alone."""
    g = torch.Generator(device=DEV).manual_seed(m + n_a)
    h = torch.randn(m, hidden, device=DEV, generator=g)
    w_a, w_b = (torch.randn(n, hidden, device=DEV, generator=g) / 16 for n in (n_a, n_b))
    b_a, b_b = torch.randn(n_a, device=DEV, generator=g), torch.randn(n_b, device=DEV, generator=g)
    out_a, out_b = hip.linear_heads_narrow_forward_pair(h, w_a, b_a, w_b, b_b)
    assert torch.equal(out_a, hip.linear_heads_narrow_forward(h, w_a, b_a))
    assert torch.equal(out_b, hip.linear_heads_narrow_forward(h, w_b, b_b))
    both = hip.linear_heads_narrow_forward(h, torch.cat([w_a, w_b]), torch.cat([b_a, b_b]))
    assert torch.equal(both[:, :n_a], out_a) and torch.equal(both[:, n_a:], out_b)


# --- the backward through time with the heads inside ----------------------------------------------------------------
def _lstm(hidden, d_in, seed=0):
    torch.manual_seed(seed)
    return nn.LSTM(d_in, hidden, batch_first=True).to(DEV)


def _inputs(b, l, d_in, hidden, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, l, d_in, device=DEV, generator=g)
    h0 = torch.randn(b, hidden, device=DEV, generator=g) * 0.5
    c0 = torch.randn(b, hidden, device=DEV, generator=g)
    return x, h0, c0


def _torch_grads(lstm, x, h0, c0, dhs, dtype):
    ref = nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True).to(DEV, dtype)
    ref.load_state_dict(lstm.state_dict())
    with torch.backends.cudnn.flags(enabled=False):
        hs, _ = ref(x.to(dtype), (h0[None].to(dtype), c0[None].to(dtype)))
        (hs * dhs.to(dtype)).sum().backward()
    return {k: getattr(ref, k).grad for k in GRADS}


def _check_grads(ours, want, t32):
    """The bars of tests/test_lstm_narrow_gpu.py::_check_grads."""
    for k, ok in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b"), ("bias_hh_l0", "b")):
        g = ours[ok].double()
        scale = float(want[k].abs().max())
        err = float((g - want[k]).abs().max())
        err32 = float((t32[k].double() - want[k]).abs().max())
        print(f"{k}: err {err:.3e}, torch fp32 err {err32:.3e}, scale {scale:.3e}")
        assert torch.isfinite(ours[ok]).all(), k
        assert err / scale < 2e-5, (k, err, scale)
        assert err <= max(3 * err32, 1e-6 * scale), (k, err, err32, scale)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("b,l,d_in", [(1, 1, 1), (31, 3, 4), (257, 8, 16), (4097, 2, 3)])
def test_backward_with_the_heads_inside_matches_the_array_form(hidden, b, l, d_in, n):
    lstm = _lstm(hidden, d_in)
    x, h0, c0 = _inputs(b, l, d_in, hidden)
    g = torch.Generator(device=DEV).manual_seed(7 + n)
    dout = torch.randn(b * l, n, device=DEV, generator=g)
    w = torch.randn(n, hidden, device=DEV, generator=g) / 8
    params = [getattr(lstm, k).detach() for k in GRADS]
    hs, _, _, gates, cs = hip.lstm_narrow_forward(x, h0, c0, *params, save=True)
    w_hh = lstm.weight_hh_l0.detach()
    inside = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, None, heads=(dout, w))
    dhs = (dout @ w).view(b, l, hidden)
    array = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dhs)
    for k in array:
        scale = float(array[k].abs().max()) + 1e-30
        err = float((inside[k] - array[k]).abs().max())
        print(f"{k}: heads inside against dhs = dout @ w: {err / scale:.3e} of the largest entry")
        assert err / scale < 2e-6, (k, err, scale)
    dhs64 = (dout.double() @ w.double()).view(b, l, hidden)
    _check_grads(inside, _torch_grads(lstm, x, h0, c0, dhs64, torch.float64),
                 _torch_grads(lstm, x, h0, c0, dhs64.float(), torch.float32))
    again = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, None, heads=(dout, w))
    for k in inside:
        assert torch.equal(inside[k], again[k]), k
    # with dhs formed by the heads' own backward kernel the two forms are the same sums in the same order
    dh, _, _ = hip.linear_heads_narrow_backward(hs.view(-1, hidden), dout, w)
    same = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dh.view(b, l, hidden))
    for k in inside:
        assert torch.equal(inside[k], same[k]), k


# --- the rollout tail with the heads inside -------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("n,with_noise,deterministic", [(1, False, 0), (67, True, 0), (8192, False, 0), (10_001, False, 1),
                                                       (10_001, True, 0)])
def test_narrow_rollout_step_with_the_heads_inside_is_the_three_launches(hidden, n, with_noise, deterministic):
    """Cases of tests/test_lstm_gpu.py::test_rollout_step_with_the_heads_inside_is_the_three_launches."""
    g = torch.Generator(device=DEV).manual_seed(n)
    h = torch.randn(n, hidden, device=DEV, generator=g)
    w_pol, b_pol = torch.randn(2, hidden, device=DEV, generator=g) / 16, torch.randn(2, device=DEV, generator=g)
    w_vf, b_vf = torch.randn(1, hidden, device=DEV, generator=g) / 16, torch.randn(1, device=DEV, generator=g)
    noise = torch.rand(n, 2, device=DEV, generator=g) + 0.01 if with_noise else None
    state0 = (torch.rand(n, device=DEV, generator=g) * 2 - 1) * 100
    rdr_t = torch.randn(n, device=DEV, generator=g)
    lib = hip.load()

    def outputs():
        return dict(state=state0.clone(), action=torch.zeros(n, dtype=torch.int64, device=DEV),
                    logp=torch.zeros(n, device=DEV), value=torch.zeros(n, device=DEV), reward=torch.zeros(n, device=DEV),
                    obs=torch.zeros(n, device=DEV), rdr=torch.zeros(n, device=DEV))

    a, b = outputs(), outputs()
    hip.rollout_step_dummy_heads_narrow(h, w_pol, b_pol, w_vf, b_vf, noise, a["state"], a["action"], a["logp"],
                                        a["value"], a["reward"], a["obs"], rdr_t, a["rdr"], 0.95, 1234, 7, 5,
                                        bool(deterministic))
    logits = hip.linear_heads_narrow_forward(h, w_pol, b_pol)
    value = hip.linear_heads_narrow_forward(h, w_vf, b_vf)
    hip._check(lib.rl8_rollout_step_dummy_f32(
        1, 0, hip._ptr(logits), None, hip._ptr(value), hip._ptr(noise), hip._ptr(b["state"]), hip._ptr(b["action"]),
        hip._ptr(b["logp"]), hip._ptr(b["value"]), hip._ptr(b["reward"]), hip._ptr(b["obs"]), hip._ptr(rdr_t),
        hip._ptr(b["rdr"]), 0.95, n, 1234, 7, 5, deterministic, hip._stream()), "rl8_rollout_step_dummy_f32")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["action"].min()) >= 0 and int(a["action"].max()) <= 1
    assert torch.equal(a["value"], value.view(-1))


# --- the default models ---------------------------------------------------------------------------------------------
MODELS = [(DefaultDiscreteRecurrentModel, DiscreteDummyEnv), (DefaultContinuousRecurrentModel, ContinuousDummyEnv)]


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("model_cls,env_cls", MODELS)
def test_narrow_models_with_and_without_the_one_node_training_pass(model_cls, env_cls, hidden, monkeypatch):
    """Protocol and bars of tests/test_lstm_gpu.py::test_recurrent_model_with_and_without_the_fused_heads_node."""
    b, l = 517, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    obs = torch.randn(b, l, 1, device=DEV, generator=g) * 10
    states = TensorDict(
        {DataKeys.HIDDEN_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g) * 0.3,
         DataKeys.CELL_STATES: torch.randn(b, l, 1, hidden, device=DEV, generator=g)}, batch_size=[b, l])
    env = env_cls(4, 8, device=DEV)
    torch.manual_seed(5)
    model = model_cls(env.observation_spec, env.action_spec, hidden_size=hidden).to(DEV)
    w_value = torch.randn(b * l, 1, device=DEV, generator=g) / (b * l)
    w_state = torch.randn(b, 1, hidden, device=DEV, generator=g) / b
    forms = []
    real = hip.lstm_narrow_backward
    monkeypatch.setattr(hip, "lstm_narrow_backward",
                        lambda *a, heads=None: forms.append("heads" if heads is not None else "array") or real(*a, heads=heads))
    for use_state in (False, True):
        def run(fuse):
            monkeypatch.setattr(fused_lstm, "FUSE_HEADS", fuse)
            model.zero_grad()
            feats, new_states = model(TensorDict({DataKeys.OBS: obs}, batch_size=[b, l]), states)
            loss = (sum((v * (i + 1)).sum() for i, v in enumerate(feats.values())) / (b * l)
                    + (model.value_function() * w_value).sum())
            if use_state:
                loss = loss + (new_states[DataKeys.HIDDEN_STATES] * w_state).sum()
            loss.backward()
            return ([v.detach().clone() for v in feats.values()] + [model.value_function().detach().clone()],
                    {k: p.grad.clone() for k, p in model.named_parameters()})

        forms.clear()
        one, two = run(True), run(False)
        assert forms == ["array" if use_state else "heads", "array"]  # (the node falls back inside when h_n is read)
        for a, e in zip(one[0], two[0]):
            assert torch.equal(a, e)
        for k in two[1]:
            scale = float(two[1][k].abs().max()) + 1e-30
            err = float((one[1][k] - two[1][k]).abs().max()) / scale
            print(f"{model_cls.__name__} H={hidden} state={use_state} {k}: {err:.3e}")
            assert err < 2e-6, (model_cls.__name__, use_state, k)


def _count_linear_calls(monkeypatch):
    calls = []
    real = nn.Linear.forward
    monkeypatch.setattr(nn.Linear, "forward", lambda self, *a, **k: calls.append(self) or real(self, *a, **k))
    return calls


def _run_algo(env_cls, hidden, enabled, layers=1, **config):
    before = fused_lstm.ENABLED
    fused_lstm.ENABLED = enabled
    try:
        torch.manual_seed(11)
        algo = RecurrentAlgorithmConfig(num_envs=256, horizon=32, model_config={"hidden_size": hidden, "num_layers": layers},
                                        **config).build(env_cls)
        collect = algo.collect()
        step = algo.step()
        params = torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])
    finally:
        fused_lstm.ENABLED = before
    return collect, step, params


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_no_module_head_runs_in_collect_and_step(env, hidden, layers, monkeypatch):
    env_cls, config = (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv,
                                                                          {"distribution_cls": SquashedNormal})
    calls = _count_linear_calls(monkeypatch)
    _, names = _timed(lambda: _run_algo(env_cls, hidden, True, layers=layers, **config))
    assert not calls, f"{len(calls)} nn.Linear forward calls"
    assert {"linear_heads_narrow_forward", "linear_heads_narrow_backward"} <= names
    if env == "discrete" and layers == 1:  # the lean rollout, its heads inside the timestep's last kernel
        assert "rollout_step_dummy_heads_narrow" in names


# --- lean against plumbed rollout -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_heads", [None, "0"])
@pytest.mark.parametrize("hidden", [64, 128])
def test_narrow_lean_and_plumbed_rollouts_agree(hidden, fuse_heads, monkeypatch):
    """tests/test_algorithm_gpu.py::test_recurrent_lean_and_plumbed_rollouts_agree's protocol: buffers, states,
    statistics and the losses of the following update equal, with the heads inside the rollout's last kernel and with
    RL8_AMD_ROLLOUT_FUSE_HEADS=0 (pair form + the plain kernel)."""
    from rl8_amd.algorithms._recurrent import _LeanRollout

    if fuse_heads is None:
        monkeypatch.delenv("RL8_AMD_ROLLOUT_FUSE_HEADS", raising=False)
    else:
        monkeypatch.setenv("RL8_AMD_ROLLOUT_FUSE_HEADS", fuse_heads)

    def run(lean):
        torch.manual_seed(9)
        algo = RecurrentAlgorithmConfig(horizon=32, num_envs=300, seq_len=4, seqs_per_state_reset=4,
                                        horizons_per_env_reset=2,
                                        model_config={"hidden_size": hidden}).build(DiscreteDummyEnv)
        assert _LeanRollout.available(algo)
        algo.lean_rollout = lean
        out = []
        for _ in range(2):
            stats = algo.collect()
            buf = {k: v.clone() for k, v in algo.buffer.items() if torch.is_tensor(v)}
            states = {k: v.clone() for k, v in algo.buffer[DataKeys.STATES].items()}
            out.append((stats, buf, states, algo.step()))
        return out, algo.state.seqs

    ((a, seqs_a), names_a), ((b, seqs_b), names_b) = _timed(lambda: run(True)), _timed(lambda: run(False))
    assert ("rollout_step_dummy_heads_narrow" in names_a) == (fuse_heads is None)
    assert "rollout_step_dummy_heads_narrow" not in names_b
    assert seqs_a == seqs_b
    for (s0, b0, st0, u0), (s1, b1, st1, u1) in zip(a, b):
        for k in b0:
            assert torch.equal(b0[k], b1[k]), k
        for k in st0:
            assert torch.equal(st0[k], st1[k]), k
        for k in s0:
            if not k.startswith("profiling"):
                assert s0[k] == s1[k], k
        for k in ("losses/policy", "losses/vf", "losses/total", "monitors/kl_div"):
            assert u0[k] == u1[k], k


# --- one update against the eager modules ---------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,env", [(64, "discrete"), (128, "continuous")])
def test_one_update_with_the_narrow_heads_matches_the_eager_modules(hidden, env):
    """Bars of tests/test_lstm_narrow_gpu.py::test_one_update_matches_the_eager_modules."""
    env_cls, config = (DiscreteDummyEnv, {}) if env == "discrete" else (ContinuousDummyEnv,
                                                                          {"distribution_cls": SquashedNormal})
    (_, s0, p0), names = _timed(lambda: _run_algo(env_cls, hidden, True, **config))
    assert {"linear_heads_narrow_forward", "linear_heads_narrow_backward"} <= names
    _, s1, p1 = _run_algo(env_cls, hidden, False, **config)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        print(f"{k}: {s0[k]!r} against {s1[k]!r}")
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    print(f"parameters: max difference {float((p0 - p1).abs().max()):.3e}")
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


# --- what runs where ------------------------------------------------------------------------------------------------
def test_width_256_runs_none_of_the_narrow_heads_kernels():
    _, names = _timed(lambda: _run_algo(DiscreteDummyEnv, 256, True))
    assert not any(n in names for n in NEW_TIMERS) and not any(n.startswith("lstm_narrow") for n in names), names
    assert "linear_heads_forward" in names or "rollout_step_dummy" in names


def test_width_96_runs_the_modules(monkeypatch):
    calls = _count_linear_calls(monkeypatch)
    _, names = _timed(lambda: _run_algo(DiscreteDummyEnv, 96, True))
    assert calls, "the heads of a width-96 model are the modules"
    assert not any(n in names for n in NEW_TIMERS) and not any(n.startswith("lstm_narrow") for n in names), names
    h = torch.zeros(4, 96, device=DEV)
    assert fused_lstm.heads_forward([nn.Linear(96, 2).to(DEV)], h) is None
    with pytest.raises(ValueError):
        hip.linear_heads_narrow_forward(h, torch.zeros(2, 96, device=DEV), torch.zeros(2, device=DEV))
