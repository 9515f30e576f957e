"""Narrow towers behind wide inputs and wide heads (width 64 / 128, up to 128 inputs and 128 outputs,
rl8_amd/csrc/mlp_narrow_wide_kernels.hip, opt-in): forward, all six parameter gradients and dx against fp64 torch at the
bars of tests/test_mlp_narrow_gpu.py (its helpers, imported); ReLU'(0) = 0; bit-repeatability and 0xA5 guards around
every output at a partial tile; the routing of ``fused_mlp.tower_forward`` under the switch; and one collect() + step()
of PPO with the switch on against the same run with it off."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.nn import fused_mlp  # noqa: E402

from ._envs import walk_env  # noqa: E402
from .test_mlp_narrow_gpu import DEV, NAMES, _autograd, _away_from_kinks, _rel, _trunk  # noqa: E402
from .test_wide_head_tower_gpu import push_env  # noqa: E402

SWITCH = "RL8_AMD_NARROW_WIDE_TOWERS"
# each side alone, both sides, the 32 / 64 / 128 classes' boundaries, a non-multiple of every padding
SHAPES = [(17, 1), (23, 2), (128, 8), (1, 9), (16, 128), (24, 12), (128, 128), (33, 34)]
# (32 833 rows are 514 tiles: more than the 512 workgroups of the widest grid, so some workgroup takes a second tile)
MS = [1, 63, 64, 65, 4097, 32_833]


def _inputs(seed, hidden, m, d_in, n_out):
    """x, parameters and dout from a CPU generator: the same values wherever the test runs."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(DEV)  # noqa: E731
    x = r(m, d_in)
    p = {"w1": r(hidden, d_in) * 0.5, "b1": r(hidden) * 0.1, "w2": r(hidden, hidden) / hidden ** 0.5,
         "b2": r(hidden) * 0.1, "w3": r(n_out, hidden) / hidden ** 0.5, "b3": r(n_out)}
    return x, p, r(m, n_out)


def _case(seed, hidden, m, d_in, n_out):
    """dout away from the kinks; the zeroed rows stay under 5 % of the rows (checked for every seed used below with
    the fp64 expression on the CPU before the seeds were fixed)."""
    x, p, dout = _inputs(seed, hidden, m, d_in, n_out)
    dout = _away_from_kinks(x, p, dout)
    assert int((dout == 0).all(1).sum()) <= 0.05 * m
    return x, p, dout


def _check(x, p, dout):
    """The bars of tests/test_mlp_narrow_gpu.py::_check, with dx held like a parameter gradient."""
    xd = x.double().requires_grad_(True)
    xf = x.clone().requires_grad_(True)
    want, gwant = _autograd(xd, p, dout, torch.float64)
    eager, geager = _autograd(xf, p, dout, torch.float32)
    gwant["x"], geager["x"] = xd.grad, xf.grad
    out = hip.mlp_narrow_wide_forward(x, *(p[k] for k in NAMES))
    assert out.shape == want.shape and torch.isfinite(out).all()
    q = {k: v.double() for k, v in p.items()}
    terms = float((torch.relu(torch.relu(x.double() @ q["w1"].T + q["b1"]) @ q["w2"].T + q["b2"]) @ q["w3"].abs().T
                   + q["b3"].abs()).max())
    err, err32 = (float((o.double() - want).abs().max()) / terms for o in (out, eager))
    print(f"out {err:.3g} (torch fp32 {err32:.3g})")
    assert err <= max(2 * err32, 1e-6), (err, err32)
    g = hip.mlp_narrow_wide_backward(x, dout, *(p[k] for k in NAMES[:5]), want_dx=True)
    for k in (*NAMES, "x"):
        assert g[k].shape == gwant[k].shape and torch.isfinite(g[k]).all(), k
        got, ref = _rel(g[k], gwant[k]), _rel(geager[k], gwant[k])
        print(f"{k} {got:.3g} (torch fp32 {ref:.3g})")
        assert got <= max(3 * ref, 5e-6), (k, got, ref)
    return out, g


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_and_gradients_against_fp64(hidden, m, shape):
    _check(*_case(1000 * hidden + 10 * shape[0] + shape[1] + m % 997, hidden, m, *shape))


@pytest.mark.parametrize("hidden", [64, 128])
def test_relu_derivative_at_zero_is_zero(hidden):
    """Rows of x = 0 with b1 = 0 on half the units and b2 = 0 on half: z1 and z2 are exactly 0 there, and the
    gradients must take ReLU'(0) = 0 as torch does (tests/test_mlp_narrow_gpu.py, at a wide shape)."""
    x, p, dout = _inputs(7, hidden, 4099, 33, 34)
    p["b1"][: hidden // 2] = 0.0
    p["b1"][hidden // 2:] = -0.5
    p["b2"][: hidden // 2] = 0.0
    x[::2] = 0.0
    _check(x, p, dout)
    ones = _autograd(x[::2], p, dout[::2], torch.float64)[1]
    assert float(ones["b1"][: hidden // 2].abs().max()) == 0.0 and float(ones["b2"][: hidden // 2].abs().max()) == 0.0


@pytest.mark.parametrize("hidden", [64, 128])
def test_repeats_bit_for_bit_and_stays_inside_its_buffers(hidden):
    """At a partial tile (m = 65) and a partial class (33 x 34): the same calls twice give equal bits, with dx and
    without; and the raw entries, handed buffers inside 0xA5 guards, leave every guard byte as it was."""
    m, d_in, n_out = 65, 33, 34
    x, p, dout = _case(65, hidden, m, d_in, n_out)
    args = [p[k] for k in NAMES]
    assert torch.equal(hip.mlp_narrow_wide_forward(x, *args), hip.mlp_narrow_wide_forward(x, *args))
    a = hip.mlp_narrow_wide_backward(x, dout, *args[:5], want_dx=True)
    b = hip.mlp_narrow_wide_backward(x, dout, *args[:5], want_dx=True)
    c = hip.mlp_narrow_wide_backward(x, dout, *args[:5])
    assert "x" not in c
    for k in (*NAMES, "x"):
        assert torch.equal(a[k], b[k]) and (k == "x" or torch.equal(a[k], c[k])), k
    lib, guard, stream = hip.load(), 4096, torch.cuda.current_stream().cuda_stream
    grads = hidden * d_in + hidden + hidden * hidden + hidden + n_out * hidden + n_out
    sizes = {"out": 4 * m * n_out, "dx": 4 * m * d_in, "grads": 4 * grads,
             "fws": lib.rl8_mlp_narrow_wide_workspace_bytes(m, hidden, d_in, n_out, 0),
             "bws": lib.rl8_mlp_narrow_wide_workspace_bytes(m, hidden, d_in, n_out, 1)}
    bufs = {k: torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    at = {k: v.data_ptr() + guard for k, v in bufs.items()}
    ptr = [t.data_ptr() for t in (p["w1"], p["b1"], p["w2"], p["b2"], p["w3"])]
    assert lib.rl8_mlp_narrow_wide_forward_f32(x.data_ptr(), m, d_in, *ptr, p["b3"].data_ptr(), n_out, hidden, at["fws"],
                                               at["out"], stream) == 0
    assert lib.rl8_mlp_narrow_wide_backward_f32(x.data_ptr(), dout.data_ptr(), m, d_in, *ptr, n_out, hidden, at["bws"],
                                                at["dx"], stream) == 0
    assert lib.rl8_mlp_narrow_wide_reduce_f32(at["bws"], m, hidden, d_in, n_out, at["grads"], stream) == 0
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v[:guard] == 0xA5).all()) and bool((v[-guard:] == 0xA5).all()), k
    inner = lambda k: bufs[k][guard:-guard].view(torch.float32)  # noqa: E731
    assert torch.equal(inner("dx").view(m, d_in), a["x"]) and torch.equal(inner("grads"), torch.cat([a[k].flatten() for k in NAMES]))


def _launched(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        fn()
        return set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()


@pytest.mark.parametrize("hidden", [64, 128])
def test_routing(hidden, monkeypatch):
    torch.manual_seed(5)
    trunk = _trunk(24, hidden, hidden)
    heads = [nn.Linear(hidden, 6).to(DEV), nn.Linear(hidden, 6).to(DEV)]
    x = torch.randn(100, 24, device=DEV)
    for value in (None, "0", "on"):  # the switch unset, off, or anything but "1": the modules
        monkeypatch.delenv(SWITCH, raising=False) if value is None else monkeypatch.setenv(SWITCH, value)
        assert fused_mlp.tower_forward(trunk, heads, x) is None
    monkeypatch.setenv(SWITCH, "1")
    out = fused_mlp.tower_forward(trunk, heads, x)
    assert out is not None and out.shape == (100, 12) and out.requires_grad
    xg = x.clone().requires_grad_(True)
    got: list = []
    names = _launched(lambda: got.append(fused_mlp.tower_forward(trunk, heads, xg)))
    assert got[0] is not None and got[0].requires_grad and names == {"mlp_narrow_wide_forward"}
    dout = torch.randn(100, 12, device=DEV)
    names = _launched(lambda: got[0].backward(dout))
    assert names == {"mlp_narrow_wide_backward_dx", "mlp_narrow_wide_reduce"}
    xd = x.double().requires_grad_(True)
    w = [q.detach().double() for q in (*trunk.parameters(), *[q for h in heads for q in (h.weight, h.bias)])]
    h2 = torch.relu(torch.relu(xd @ w[0].T + w[1]) @ w[2].T + w[3])
    torch.cat([h2 @ w[4].T + w[5], h2 @ w[6].T + w[7]], -1).backward(dout.double())
    assert _rel(xg.grad, xd.grad) <= 5e-6
    assert all(q.grad is not None for q in trunk.parameters())
    # declined with the switch on: the caller runs the modules
    head = nn.Linear(hidden, 12).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert fused_mlp.tower_forward(trunk, [head], x) is None
    assert fused_mlp.tower_forward(_trunk(24, hidden, hidden).double(), [nn.Linear(hidden, 12).to(DEV).double()], x.double()) is None
    # (parameters that are not float32, or not on x's device)
    assert fused_mlp.tower_forward(_trunk(24, hidden, hidden).double(), [nn.Linear(hidden, 12).to(DEV).double()], x) is None
    assert fused_mlp.tower_forward(_trunk(24, hidden, hidden).cpu(), [nn.Linear(hidden, 12)], x) is None
    assert fused_mlp.tower_forward(trunk, [head], torch.randn(24, 100, device=DEV).T) is None
    assert fused_mlp.tower_forward(trunk, [head], x[:0]) is None
    assert fused_mlp.tower_forward(trunk, [head], x[:, :23].contiguous()) is None
    assert fused_mlp.tower_forward(_trunk(24, 96, 96), [nn.Linear(96, 12).to(DEV)], x) is None
    assert fused_mlp.tower_forward(_trunk(24, hidden, hidden, act=nn.Tanh), [head], x) is None
    assert fused_mlp.tower_forward(_trunk(24, hidden, hidden, bias=False), [nn.Linear(hidden, 12, bias=False).to(DEV)], x) is None
    assert fused_mlp.tower_forward(_trunk(129, hidden, hidden), [head], torch.randn(100, 129, device=DEV)) is None
    assert fused_mlp.tower_forward(trunk, [nn.Linear(hidden, 129).to(DEV)], x) is None
    # width 256 is untouched: (24, 12) launches the wide-head kernels as before
    names = _launched(lambda: fused_mlp.tower_forward(_trunk(24, 256, 256), [nn.Linear(256, 12).to(DEV)], x))
    assert "mlp_wide_out_forward_save" in names and not any(k.startswith("mlp_narrow") for k in names), names


def _run_algo(env, hidden):
    got: list = []

    def run():
        torch.manual_seed(11)
        algo = AlgorithmConfig(num_envs=256, horizon=16, model_config={"hiddens": (hidden, hidden)}).build(env)
        algo.collect()
        got.append({k: algo.buffer[k].clone() for k in (DataKeys.OBS, DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.VALUES)})
        got.extend([algo.step(), torch.cat([p.detach().flatten() for p in algo.policy.model.parameters()])])

    return (_launched(run), *got)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("env", ["discrete", "continuous"])
def test_one_update_matches_the_torch_modules(env, hidden, monkeypatch):
    """The bars of tests/test_mlp_narrow_gpu.py::test_one_update_matches_the_eager_modules.  Discrete: policy tower
    24 -> H -> H -> 12; continuous: 24 -> H -> H -> [6 | 6]; the value towers 24 -> H -> H -> 1."""
    cls = walk_env(24, 12) if env == "discrete" else push_env(24, 6)
    monkeypatch.setenv(SWITCH, "0")
    off, c1, s1, p1 = _run_algo(cls, hidden)
    assert not any(k.startswith("mlp_narrow") for k in off), sorted(off)
    monkeypatch.setenv(SWITCH, "1")
    calls = []
    real = torch.nn.functional.linear
    monkeypatch.setattr(torch.nn.functional, "linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    on, c0, s0, p0 = _run_algo(cls, hidden)
    assert {"mlp_narrow_wide_forward", "mlp_narrow_wide_backward", "mlp_narrow_wide_reduce"} <= on, sorted(on)
    assert not calls, "an eager nn.Linear ran"
    for k in ("losses/policy", "losses/vf", "losses/total"):
        assert s0[k] == pytest.approx(s1[k], rel=1e-5, abs=1e-8), (k, s0[k], s1[k])
    torch.testing.assert_close(p0, p1, rtol=1e-4, atol=1e-5)
    for k in c0:  # (the rollout: the same observations and actions, log-probabilities and values at the parameters' bar)
        torch.testing.assert_close(c0[k], c1[k], rtol=1e-4, atol=1e-5, msg=k)
