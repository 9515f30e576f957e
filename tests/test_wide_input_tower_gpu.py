"""Wide-input towers (width 256 behind 17 to 128 inputs, rl8_amd/csrc/mlp_wide_in_kernels.hip): forward and all six
parameter gradients against fp64 torch, beside torch's own fp32 at the same inputs (the helpers and bars of
tests/test_mlp_narrow_gpu.py::_check, restated); ReLU'(0) = 0; run-to-run bit equality, also across the backward's row
segments; the routing of ``fused_mlp.tower_forward``; and one collect() + step() of PPO on a 24-float observation
against the same run on the torch modules."""

import functools
import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.models import DefaultContinuousModel  # noqa: E402
from rl8_amd.nn import fused_mlp  # noqa: E402
from rl8_amd.specs import Unbounded  # noqa: E402

from ._envs import walk_env  # noqa: E402

DEV = "cuda:0"
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
HIDDEN = 256
SWITCH = "RL8_AMD_WIDE_INPUT_TOWERS"


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


def _modules(p):
    """The tower as the modules ``tower_forward`` classifies, holding clones of ``p`` (one head)."""
    d_in, n_out = p["w1"].shape[1], p["w3"].shape[0]
    trunk = nn.Sequential(nn.Sequential(nn.Linear(d_in, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN)), nn.ReLU()).to(DEV)
    head = nn.Linear(HIDDEN, n_out).to(DEV)
    with torch.no_grad():
        for layer, w, b in ((trunk[0][0], "w1", "b1"), (trunk[0][2], "w2", "b2"), (head, "w3", "b3")):
            layer.weight.copy_(p[w])
            layer.bias.copy_(p[b])
    return trunk, head


def _fused(x, p, dout=None):
    """(out, gradients or None) through ``fused_mlp.tower_forward``: the route under test, segment walk included."""
    trunk, head = _modules(p)
    if dout is None:
        with torch.no_grad():
            out = fused_mlp.tower_forward(trunk, [head], x)
        assert out is not None
        return out, None
    out = fused_mlp.tower_forward(trunk, [head], x)
    assert out is not None and out.requires_grad
    out.backward(dout)
    layers = {"w1": trunk[0][0].weight, "b1": trunk[0][0].bias, "w2": trunk[0][2].weight, "b2": trunk[0][2].bias,
              "w3": head.weight, "b3": head.bias}
    return out.detach(), {k: layers[k].grad for k in NAMES}


def _terms(x, p):
    """The size of the head's terms, |h2| |w3|^T + |b3|: a single output that cancels to nearly zero -- m = 1,
    n_out = 1 -- would otherwise measure luck."""
    q = {k: v.double() for k, v in p.items()}
    return float((torch.relu(torch.relu(x.double() @ q["w1"].T + q["b1"]) @ q["w2"].T + q["b2"]) @ q["w3"].abs().T
                  + q["b3"].abs()).max())


def _check_forward(out, x, p, want, eager):
    assert torch.isfinite(out).all()
    terms = _terms(x, p)
    err, err32 = (float((o.double() - want).abs().max()) / terms for o in (out, eager))
    print(f"forward d_in={x.shape[1]} m={x.shape[0]} n_out={out.shape[1]}: err {err:.3e} torch-fp32 {err32:.3e}")
    assert err <= max(2 * err32, 1e-6), (err, err32)


def _check_gradients(g, p, gwant, geager, what=""):
    for k in NAMES:
        assert g[k].shape == p[k].shape and torch.isfinite(g[k]).all(), k
        rel, rel32 = _rel(g[k], gwant[k]), _rel(geager[k], gwant[k])
        print(f"gradient {what} {k}: rel {rel:.3e} torch-fp32 {rel32:.3e}")
        assert rel <= max(3 * rel32, 5e-6), (k, rel, rel32)


def _check(x, p, dout):
    want, gwant = _autograd(x, p, dout, torch.float64)
    eager, geager = _autograd(x, p, dout, torch.float32)
    out, g = _fused(x, p, dout)
    _check_forward(out, x, p, want, eager)
    _check_gradients(g, p, gwant, geager, f"d_in={x.shape[1]} m={x.shape[0]} n_out={dout.shape[1]}")
    return out, g


# first width past the old limit, both sides of a 32-column tile (and of the k-granule of 8: 24, 31 / 32, 33), the maximum
D_INS = (17, 24, 31, 32, 33, 64, 100, 128)
MS = (1, 63, 64, 65, 4097, 70_001)
N_OUTS = (1, 2, 3, 8)
_BACKWARD_N_OUT = dict(zip(itertools.product(D_INS, MS), itertools.cycle(N_OUTS)))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("d_in", D_INS)
def test_forward_and_gradients_against_fp64(d_in, m):
    for n_out in N_OUTS:
        g = torch.Generator(device=DEV).manual_seed(1000 * d_in + 10 * n_out + m % 997)
        x = torch.randn(m, d_in, device=DEV, generator=g)
        p = _params(g, HIDDEN, d_in, n_out)
        if n_out == _BACKWARD_N_OUT[d_in, m]:
            _check(x, p, _away_from_kinks(x, p, torch.randn(m, n_out, device=DEV, generator=g)))
        else:
            with torch.no_grad():
                want = _tower(x.double(), {k: v.double() for k, v in p.items()})
                eager = _tower(x, p)
            _check_forward(_fused(x, p)[0], x, p, want, eager)


@pytest.mark.parametrize("d_in,m,n_out", [(24, 70_001, 4), (128, 4097, 1), (33, 65, 8)])
def test_dw2_on_fp32_mfma_holds_the_same_bars(d_in, m, n_out, monkeypatch):
    """The default forms dW2 on bf16 planes (``fused_mlp.WIDE_INPUT_DW2_PLANES``); ``rl8_mlp_wgrad_f32`` behind the same
    backward holds the same bars, and only dW2 differs between the two."""
    g = torch.Generator(device=DEV).manual_seed(d_in + m)
    x = torch.randn(m, d_in, device=DEV, generator=g)
    p = _params(g, HIDDEN, d_in, n_out)
    dout = _away_from_kinks(x, p, torch.randn(m, n_out, device=DEV, generator=g))
    planes = _fused(x, p, dout)[1]
    monkeypatch.setattr(fused_mlp, "WIDE_INPUT_DW2_PLANES", False)
    _, fp32 = _check(x, p, dout)
    for k in NAMES:
        assert torch.equal(planes[k], fp32[k]) or k == "w2", k


@pytest.mark.parametrize("d_in", [24, 33])
def test_relu_derivative_at_zero_is_zero(d_in):
    """Rows of x = 0 with b1 = 0 on half the units and b2 = 0 on half: z1 and z2 are exactly 0 there, and the
    gradients must take ReLU'(0) = 0 as torch does."""
    g = torch.Generator(device=DEV).manual_seed(7)
    m, n_out = 4099, 3
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
    m, d_in, n_out = 70_001, 33, 3
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
    launches: dict = {}
    monkeypatch.setattr(fused_mlp, "WIDE_INPUT_SEGMENT_ROWS", 4096)
    m, d_in, n_out = 3 * 4096 + 5, 31, 2
    g = torch.Generator(device=DEV).manual_seed(m)
    p = _params(g, HIDDEN, d_in, n_out)
    x = torch.randn(m, d_in, device=DEV, generator=g)
    dout = _away_from_kinks(x, p, torch.randn(m, n_out, device=DEV, generator=g))
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        _, a = _check(x, p, dout)
        launches.update(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    assert launches["mlp_wide_in_backward"]["launches"] == 4 and launches["mlp_wide_in_wgrad"]["launches"] == 4
    assert launches["mlp_wgrad"]["launches"] == 4
    b = _fused(x, p, dout)[1]
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("d_in", [17, 100])
def test_the_weight_gradients_accumulate_into_out(d_in):
    """``accumulate`` adds a launch's product to what ``out`` holds, for dW1 and (``hip.mlp_wgrad``, fp32 MFMA or bf16
    planes) for dW2; without it ``out`` is overwritten, whatever it held."""
    g = torch.Generator(device=DEV).manual_seed(d_in)
    m = 5000
    dz, h1 = torch.randn(m, HIDDEN, device=DEV, generator=g), torch.randn(m, HIDDEN, device=DEV, generator=g)
    x = torch.randn(m, d_in, device=DEV, generator=g)
    for product, right in ((hip.mlp_wide_in_wgrad, x), (hip.mlp_wgrad, h1),
                           (functools.partial(hip.mlp_wgrad, planes=True), h1)):
        whole = product(dz, right)
        want = dz.double().T @ right.double()
        assert _rel(whole, want) <= 5e-6
        out = torch.full_like(whole, float("nan"))
        assert product(dz[:3000], right[:3000], out=out) is out
        first = out.clone()
        product(dz[3000:], right[3000:], out=out, accumulate=True)
        # (the same <= 160 fp32 terms -- one per workgroup slab and the first product -- in another association: at
        # most 160 roundings of 2^-24 apart, relative to the largest entry's terms)
        assert _rel(out, first + product(dz[3000:], right[3000:])) <= 160 * 2.0 ** -24
        assert not torch.equal(out, first) and _rel(out, want) <= 5e-6


def _trunk(d_in, width):
    return nn.Sequential(nn.Sequential(nn.Linear(d_in, width), nn.ReLU(), nn.Linear(width, width)), nn.ReLU()).to(DEV)


def test_routing(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    trunk, head = _trunk(24, HIDDEN), nn.Linear(HIDDEN, 4).to(DEV)
    x = torch.randn(100, 24, device=DEV)
    out = fused_mlp.tower_forward(trunk, [head], x)
    assert out is not None and out.shape == (100, 4) and out.requires_grad
    torch.testing.assert_close(out, head(trunk(x)), rtol=1e-4, atol=1e-5)
    two = fused_mlp.tower_forward(trunk, [head, nn.Linear(HIDDEN, 1).to(DEV)], x)
    assert two is not None and two.shape == (100, 5)
    with torch.no_grad():
        assert fused_mlp.tower_forward(trunk, [head], x.clone().requires_grad_(True)) is not None  # (no gradient can follow)
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
        assert fused_mlp.tower_forward(_trunk(24, width), [nn.Linear(width, 4).to(DEV)], x) is None
    monkeypatch.setenv(SWITCH, "0")
    assert fused_mlp.tower_forward(trunk, [head], x) is None
    monkeypatch.setenv(SWITCH, "1")
    assert fused_mlp.tower_forward(trunk, [head], x) is not None


def test_a_weight_changed_in_place_is_repacked():
    trunk, head = _trunk(40, HIDDEN), nn.Linear(HIDDEN, 2).to(DEV)
    x = torch.randn(300, 40, device=DEV)
    with torch.no_grad():
        fused_mlp.tower_forward(trunk, [head], x)
        trunk[0][0].weight.mul_(-1.5)
        trunk[0][2].weight.add_(0.01)
        out = fused_mlp.tower_forward(trunk, [head], x)
        torch.testing.assert_close(out, head(trunk(x)), rtol=1e-4, atol=1e-5)


def _run_algo(kernels=None):
    torch.manual_seed(11)
    algo = AlgorithmConfig(num_envs=256, horizon=16).build(walk_env(24, 4))
    if kernels is not None:
        hip.timer.reset()
        hip.timer.enabled = True
    try:
        algo.collect()
        step = algo.step()
        if kernels is not None:
            kernels.update(hip.timer.summary())
    finally:
        hip.timer.enabled = False
    return step, torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])


def test_default_models_on_a_24_float_observation_run_the_kernels(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    calls = []
    real = torch.nn.functional.linear
    monkeypatch.setattr(torch.nn.functional, "linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    kernels: dict = {}
    _run_algo(kernels)
    assert {"mlp_wide_in_forward", "mlp_wide_in_backward", "mlp_wide_in_wgrad", "mlp_wgrad"} <= set(kernels), sorted(kernels)
    assert not calls, "an eager nn.Linear ran"


def test_one_update_matches_the_torch_modules(monkeypatch):
    """Losses at rel 1e-5 / abs 1e-8; parameters at rtol 1e-4 and atol 1e-5 (1 % of Adam's first step, lr = 1e-3): the
    fused and eager towers round differently, and a ReLU that rounding decides the other way for one sample moves a
    few weights by ~2e-6 (the bars and the reasoning of test_mlp_narrow_gpu.py::test_one_update_matches_the_eager_modules)."""
    monkeypatch.delenv(SWITCH, raising=False)
    s0, p0 = _run_algo()
    monkeypatch.setenv(SWITCH, "0")
    kernels: dict = {}
    s1, p1 = _run_algo(kernels)
    assert not any(k.startswith("mlp_wide_in") for k in kernels)
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)


def test_the_continuous_models_two_head_tower():
    """``DefaultContinuousModel``'s policy tower (mean and log-std heads as one [2a, 256] head) on a [512, 24] input."""
    torch.manual_seed(5)
    model = DefaultContinuousModel(Unbounded(24, device=DEV), Unbounded(shape=torch.Size([2]), device=DEV)).to(DEV)
    heads = [model.action_mean, model.action_log_std]
    with torch.no_grad():  # (the model's own heads start at 1e-3 and zero bias: give the bars something to measure)
        for h in heads:
            h.weight.normal_(0.0, HIDDEN ** -0.5)
            h.bias.normal_()
    l1, l2 = model.latent_model[0][0], model.latent_model[0][-1]
    p = {"w1": l1.weight, "b1": l1.bias, "w2": l2.weight, "b2": l2.bias,
         "w3": torch.cat([h.weight for h in heads], 0), "b3": torch.cat([h.bias for h in heads], 0)}
    p = {k: v.detach().clone() for k, v in p.items()}
    g = torch.Generator(device=DEV).manual_seed(512)
    x = torch.randn(512, 24, device=DEV, generator=g)
    dout = _away_from_kinks(x, p, torch.randn(512, 4, device=DEV, generator=g))
    want, gwant = _autograd(x, p, dout, torch.float64)
    eager, geager = _autograd(x, p, dout, torch.float32)
    out = fused_mlp.tower_forward(model.latent_model, heads, x)
    assert out is not None and out.shape == (512, 4)
    out.backward(dout)
    _check_forward(out.detach(), x, p, want, eager)
    got = {"w1": l1.weight.grad, "b1": l1.bias.grad, "w2": l2.weight.grad, "b2": l2.bias.grad,
           "w3": torch.cat([h.weight.grad for h in heads], 0), "b3": torch.cat([h.bias.grad for h in heads], 0)}
    _check_gradients(got, p, gwant, geager, "continuous model")
