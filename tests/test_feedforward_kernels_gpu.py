"""The fused feedforward kernels (``rl8_feedforward_f32`` / ``rl8_feedforward_backward_f32``) on the GPU, and the
modules that run on them.

Yardsticks.  ``ref64``: ``rl8_amd.nn.fused_feedforward.feedforward_reference`` in float64 on the CPU (pinned to the
modules at 1e-12 by ``tests/test_feedforward_host.py``).  ``torch32``: what the modules ran before these kernels --
``layer_norm``, ``linear``, ``relu``, ``linear`` and the sum as eager torch ops -- on the same device tensors in float32,
forward and autograd.

Inputs are seeded on the CPU: standard-normal ``x`` and ``dout``, default-initialised Linears, ``gamma`` uniform in
[0.5, 1.5], ``beta`` standard normal.  Every case is made tie-free before it is used: the pre-activations are formed in
float64 and every row that has a ``|z| < 1e-4`` is drawn again until none is left, so that no ReLU gate differs between
float32 and float64 (a gate that does moves a parameter gradient by one whole token's contribution, which says nothing
about a kernel).  With that, 100 % of the elements are compared.  A case whose draw leaves every gate closed (F = 2 and
H = 1 allow it: a normalised row of two features takes one of two values) is drawn again, so that no case compares zeros.

Bars (the "3x the yardstick's own error + floor" rule of DESIGN.md §5 / §8):
* forward, elementwise: ``|got - ref64| <= 3 max|torch32 - ref64| + 1e-6 + 1e-5 |ref64|``;
* dx and each parameter gradient: ``|got - ref64| <= 3 max|torch32 - ref64| + 2e-5 max|ref64| + 1e-9``.
Each case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor before it asserts (measured on an MI355X: out
0.65 .. 1.63, dx 0.71 .. 1.26, dgamma 0.31 .. 4.12, dbeta 0.24 .. 1.45, dw1 0.11 .. 2.80, db1 0.27 .. 3.21, dw2 0.10 .. 1.76,
db2 0.48 .. 4.45, the ratios above 3 at R <= 256 where the floor carries the bar).  Every kernel output lies
between guard words.
"""

import functools
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402
from rl8_amd.nn import CrossAttention, SelfAttention, SelfAttentionStack  # noqa: E402
from rl8_amd.nn.fused_feedforward import feedforward_reference  # noqa: E402

DEV = "cuda"
GUARD = 64  # elements in front of and behind every kernel output
EPS = 1e-5
NAMES = ("out", "dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")


def limits() -> hip.FeedforwardLimits:
    return hip.feedforward_limits()


def cases() -> list[tuple[int, int, int, bool, float, int]]:
    """(R, F, H, residual, offset added to x, elements every base pointer sits into its allocation).  The sizes that
    depend on the kernels' launch shapes take them from the library."""
    lim = limits()
    stride = lim.grid_cap * lim.block + 77  # (beyond one pass of all three kernels: the weight-gradient kernel's is less)
    assert stride > lim.wgrad_grid_cap * lim.wgrad_rows
    return [
        (1, 1, 1, True, 0.0, 0), (1, 1, 1, False, 0.0, 0),
        (63, 2, 1, True, 0.0, 0), (64, 2, 1, False, 0.0, 0), (65, 2, 1, True, 0.0, 0),
        (257, 3, 63, False, 0.0, 0),
        (20495, 8, 64, True, 30.0, 0),  # rows of mean 30: the two-pass variance
        (20495, 8, 64, False, 0.0, 0),
        (4099, 16, 65, True, 0.0, 0),
        (4099, 31, 128, False, 0.0, 0),
        (4099, 32, 256, True, 0.0, 0),  # the envelope's corner
        (67, 12, 128, True, 0.0, 1),
        (stride, 2, 1, True, 0.0, 0),
        (lim.wgrad_rows - 1, 8, 64, True, 0.0, 0), (lim.wgrad_rows, 8, 64, False, 0.0, 0),
        (lim.wgrad_rows + 1, 8, 64, True, 0.0, 0),
    ]


NUM_CASES = 16
MEAN_30, PLAIN_8_64, CORNER = 6, 7, 10


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def parameters(f: int, h: int, seed: int) -> dict[str, torch.Tensor]:
    """CPU float32 parameters of the block: default-initialised Linears, gamma in [0.5, 1.5], beta standard normal."""
    g = gen(seed)
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        up, down = nn.Linear(f, h), nn.Linear(h, f)
    return dict(gamma=torch.rand(f, generator=g) + 0.5, beta=torch.randn(f, generator=g), w1=up.weight.detach().clone(),
                b1=up.bias.detach().clone(), w2=down.weight.detach().clone(), b2=down.bias.detach().clone())


def pre_activations(x: torch.Tensor, p: dict) -> torch.Tensor:
    """``z [R, H]`` in float64."""
    n = torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), p["gamma"].double(), p["beta"].double(), EPS)
    return n @ p["w1"].double().t() + p["b1"].double()


def tie_free(x: torch.Tensor, p: dict, g: torch.Generator, offset: float) -> torch.Tensor:
    """``x`` with every row drawn again that has a pre-activation nearer to 0 than 1e-4 in float64."""
    for _ in range(64):
        close = (pre_activations(x, p).abs() < 1e-4).any(dim=-1)
        if not bool(close.any()):
            return x
        x = x.clone()
        x[close] = torch.randn(int(close.sum()), x.shape[-1], generator=g) + offset
    raise AssertionError("rows with a pre-activation at 0 after 64 rounds")


def with_grads(x, p, dout, residual):
    """``(out, dx, dgamma, dbeta, dw1, db1, dw2, db2)`` of ``feedforward_reference`` on ``x`` and ``p`` as they come."""
    x = x.clone().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = feedforward_reference(x, leaves["gamma"], leaves["beta"], EPS, leaves["w1"], leaves["b1"], leaves["w2"],
                                leaves["b2"], residual)
    out.backward(dout)
    return (out.detach(), x.grad) + tuple(leaves[k].grad for k in ("gamma", "beta", "w1", "b1", "w2", "b2"))


@functools.lru_cache(maxsize=None)
def case(index: int) -> dict:
    """Inputs (CPU, float32), ``ref64`` and ``torch32`` of ``cases()[index]``: computed once, shared, never modified."""
    r, f, h, residual, offset, shift = cases()[index]
    for draw in range(32):  # (the first draw that opens a gate and, where there is more than one, leaves one closed)
        g = gen(100 + index + 1000 * draw)
        p = parameters(f, h, 200 + index + 1000 * draw)
        x = tie_free(torch.randn(r, f, generator=g) + offset, p, g, offset)
        is_open = pre_activations(x, p) > 0
        if bool(is_open.any()) and (r * h == 1 or not bool(is_open.all())):
            break
    else:
        raise AssertionError("no draw with an open and a closed gate")
    dout = torch.randn(r, f, generator=g)
    ref64 = with_grads(x.double(), {k: v.double() for k, v in p.items()}, dout.double(), residual)
    torch32 = with_grads(x.to(DEV), {k: v.to(DEV) for k, v in p.items()}, dout.to(DEV), residual)
    return dict(x=x, dout=dout, p=p, residual=residual, shift=shift, ref64=ref64,
                torch32=tuple(t.double().cpu() for t in torch32))


def guarded(numel: int, shift: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """A sentinel-filled float32 buffer and the ``numel`` elements ``GUARD + shift`` into it that a kernel may write."""
    buf = torch.full((numel + shift + 2 * GUARD,), -77.0, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + numel]


def assert_guards(buf: torch.Tensor, inner: torch.Tensor, what: str) -> None:
    front = (inner.data_ptr() - buf.data_ptr()) // 4
    assert bool((buf[:front] == -77).all()) and bool((buf[front + inner.numel():] == -77).all()), \
        f"{what}: wrote outside its output"


def placed(t: torch.Tensor, shift: int) -> torch.Tensor:
    """A device copy of ``t`` whose base pointer sits ``shift`` elements into its allocation."""
    buf = torch.empty(t.numel() + shift, dtype=torch.float32, device=DEV)
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


def ptr(t: None | torch.Tensor) -> None | int:
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def run_kernels(x, dout, p, residual, shift=0, *, want_dx=True, want_params=True):
    """The raw entries on device copies of CPU tensors: ``(out, dx, dgamma, dbeta, dw1, db1, dw2, db2)``, a piece
    that was not asked for ``None``; every output, and the workspace, between guard words that are checked."""
    r, f = x.shape
    h = p["w1"].shape[0]
    lib = hip.load()
    xd, gd = placed(x, shift), placed(dout, shift)
    d = {k: placed(v, shift) for k, v in p.items()}
    obuf, out = guarded(r * f, shift)
    assert lib.rl8_feedforward_f32(ptr(xd), ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(d["w1"]), ptr(d["b1"]),
                                   ptr(d["w2"]), ptr(d["b2"]), r, f, h, int(residual), ptr(out), stream()) == 0
    assert_guards(obuf, out, "out")
    assert not bool((out == -77).any()), "out: an element was not written"
    sizes = dict(dx=r * f, dgamma=f, dbeta=f, dw1=h * f, db1=h, dw2=f * h, db2=f)
    wanted = {name: (want_dx if name == "dx" else want_params) for name in sizes}
    grads = {name: guarded(numel, shift) for name, numel in sizes.items()}
    wbuf, workspace = guarded(hip.feedforward_workspace_floats(r, f, h), shift)
    args = [ptr(grads[name][1]) if wanted[name] else None for name in sizes]
    assert lib.rl8_feedforward_backward_f32(ptr(xd), ptr(gd), ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(d["w1"]),
                                            ptr(d["b1"]), ptr(d["w2"]), r, f, h, int(residual), *args,
                                            ptr(workspace) if want_params else None, stream()) == 0
    assert_guards(wbuf, workspace, "workspace")
    results = [out.view(r, f)]
    for name, (buf, inner) in grads.items():
        assert_guards(buf, inner, name)
        if wanted[name]:
            assert not bool((inner == -77).any()), f"{name}: an element was not written"
        else:
            assert bool((buf == -77).all()), f"{name}: written though it was not asked for"
        results.append(inner if wanted[name] else None)
    if not want_params:
        assert bool((wbuf == -77).all()), "workspace: written though no parameter gradient was asked for"
    shapes = dict(dx=(r, f), dgamma=(f,), dbeta=(f,), dw1=(h, f), db1=(h,), dw2=(f, h), db2=(f,))
    return tuple(t if t is None or n == "out" else t.view(shapes[n]) for n, t in zip(NAMES, results))


def run_case(c: dict, **kwargs):
    return run_kernels(c["x"], c["dout"], c["p"], c["residual"], c["shift"], **kwargs)


@pytest.mark.parametrize("index", range(NUM_CASES))
def test_kernels_against_float64_within_three_times_torch_s_own_error(index):
    assert len(cases()) == NUM_CASES
    c = case(index)
    got = [t.double().cpu() for t in run_case(c)]
    figures = []
    for name, g, want, t32 in zip(NAMES, got, c["ref64"], c["torch32"]):
        assert g.shape == want.shape, name
        assert not torch.isnan(g).any() and not torch.isnan(t32).any(), name
        torch_err, err = float((t32 - want).abs().max()), float((g - want).abs().max())
        figures.append((name, err, torch_err))
    print(f"{cases()[index]}: " + "  ".join(f"{n} {err:.2e} / {te:.2e} = {err / te if te else math.nan:.2f}"
                                            for n, err, te in figures))
    for (name, _, torch_err), g, want in zip(figures, got, c["ref64"]):
        if name == "out":
            bar = 3 * torch_err + 1e-6 + 1e-5 * want.abs()
        else:
            bar = torch.full_like(want, 3 * torch_err + 2e-5 * float(want.abs().max()) + 1e-9)
        assert bool(((g - want).abs() <= bar).all()), (name, float(((g - want).abs() - bar).max()))


# --- edges ----------------------------------------------------------------------------------------------------------
def test_a_hidden_unit_at_exactly_zero_takes_and_gives_no_gradient():
    r, f, h, j = 257, 8, 64, 17
    g = gen(31)
    p = parameters(f, h, 32)
    p["w1"][j] = 0.0
    p["b1"][j] = 0.0  # z_j = +0 exactly on every row: the gate is closed
    x, dout = torch.randn(r, f, generator=g), torch.randn(r, f, generator=g)
    out, dx, _, _, dw1, db1, dw2, _ = run_kernels(x, dout, p, True)
    assert not bool(dw1[j].any()) and float(db1[j]) == 0.0 and not bool(dw2[:, j].any())
    assert bool(dw1[j - 1].any()) and float(db1[j - 1]) != 0.0 and bool(dw2[:, j - 1].any())
    other = {k: v.clone() for k, v in p.items()}
    other["w2"][:, j] = 1000.0 * torch.randn(f, generator=g)  # what the unit would pass on changes ...
    out2, dx2, *_ = run_kernels(x, dout, other, True)
    assert torch.equal(dx2, dx) and torch.equal(out2, out)  # ... and its share of out and dx stays exactly 0


@pytest.mark.parametrize("residual", [True, False])
def test_a_constant_row_has_variance_zero_and_a_finite_gradient(residual):
    r, f, h = 67, 8, 64
    g = gen(41)
    p = parameters(f, h, 42)
    x, dout = torch.randn(r, f, generator=g), torch.randn(r, f, generator=g)
    x[5] = 3.5
    out, dx, *params = run_kernels(x, dout, p, residual)
    d = {k: v.double() for k, v in p.items()}
    want = d["w2"] @ torch.relu(d["w1"] @ d["beta"] + d["b1"]) + d["b2"] + (3.5 if residual else 0.0)
    assert bool(((out[5].double().cpu() - want).abs() <= 1e-6 + 1e-5 * want.abs()).all())
    assert bool(torch.isfinite(dx).all()) and all(bool(torch.isfinite(t).all()) for t in params)


def test_a_nan_and_an_infinity_stay_in_their_rows():
    r, f, h = 321, 8, 64
    g = gen(51)
    p = parameters(f, h, 52)
    x, dout = torch.randn(r, f, generator=g), torch.randn(r, f, generator=g)
    clean_out, clean_dx, *_ = run_kernels(x, dout, p, True)
    bad = x.clone()
    bad[7, 3] = math.nan
    bad[200, 0] = math.inf
    out, dx, *_ = run_kernels(bad, dout, p, True)
    t_out, t_dx, *_ = with_grads(bad.to(DEV), {k: v.to(DEV) for k, v in p.items()}, dout.to(DEV), True)
    for row in (7, 200):
        assert bool(torch.isnan(t_out[row]).any()) and bool(torch.isnan(t_dx[row]).any())
        assert bool(torch.isnan(out[row])[torch.isnan(t_out[row])].all()), f"out, row {row}"
        assert bool(torch.isnan(dx[row])[torch.isnan(t_dx[row])].all()), f"dx, row {row}"
    rest = torch.ones(r, dtype=torch.bool)
    rest[[7, 200]] = False
    assert torch.equal(out[rest.to(DEV)], clean_out[rest.to(DEV)]) and torch.equal(dx[rest.to(DEV)], clean_dx[rest.to(DEV)])


@pytest.mark.parametrize("index", [MEAN_30, CORNER])
def test_parameter_gradients_are_bit_reproducible(index):
    first, second = run_case(case(index)), run_case(case(index))
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), name


def test_an_output_that_is_not_wanted_is_skipped():
    c = case(PLAIN_8_64)
    everything = run_case(c)
    only_dx = run_case(c, want_params=False)  # (run_kernels checks that the rest and the workspace stay untouched)
    only_params = run_case(c, want_dx=False)
    assert torch.equal(only_dx[1], everything[1]) and all(t is None for t in only_dx[2:])
    assert only_params[1] is None
    for name, a, b in zip(NAMES[2:], only_params[2:], everything[2:]):
        assert torch.equal(a, b), name
    run_case(c, want_dx=False, want_params=False)


# --- the modules through the public route -------------------------------------------------------------------------
def launches() -> dict[str, int]:
    return {name: int(s["launches"]) for name, s in hip.timer.summary().items() if name.startswith("feedforward")}


def module_runs(monkeypatch, module, inputs, kwargs, dout):
    """``(outputs, gradients of inputs and parameters, feedforward launches)`` with the kernels on and off."""
    runs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", switch)
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            xs = [x.clone().requires_grad_(True) for x in inputs]
            module.zero_grad()
            out = module(*xs, **kwargs)
            out.backward(dout)
            ran = launches()
        finally:
            hip.timer.enabled = False
        grads = {f"input {i}": x.grad for i, x in enumerate(xs)}
        grads.update({name: p.grad.clone() for name, p in module.named_parameters()})
        runs.append((out.detach(), grads, ran))
    return runs


def assert_module_runs_agree(runs, passes: int = 1) -> None:
    (out1, grads1, ran1), (out0, grads0, ran0) = runs
    assert ran1 == {"feedforward": passes, "feedforward_backward": passes} and ran0 == {}
    assert set(grads1) == set(grads0)
    for name, got, want in [("out", out1, out0)] + [(n, grads1[n], grads0[n]) for n in grads0]:
        diff, top = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name}: max|on - off| {diff:.2e}, largest entry {top:.2e}")
        if name == "out":
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6, msg=lambda m, n=name: f"{n}: {m}")
        else:
            assert diff <= 2e-5 * top, name


def window_padding(b: int, t: int) -> torch.Tensor:
    """Row i has ``i % t`` leading cells padded (a rolling window that is still filling)."""
    return (torch.arange(t).expand(b, t) < (torch.arange(b) % t).unsqueeze(1)).to(DEV)


def test_self_attention_residual_on_the_kernels_and_with_the_switch_off(monkeypatch):
    torch.manual_seed(5)
    b, t, e = 67, 5, 8
    layer = SelfAttention(e, num_heads=4, hidden_dim=64, skip_kind="residual").to(DEV)
    x = torch.randn(b, t, e, generator=gen(61)).to(DEV)
    dout = torch.randn(b, t, e, generator=gen(62)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, layer, [x], dict(key_padding_mask=window_padding(b, t)), dout))
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "1")
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        with torch.no_grad():
            layer(x)
        assert launches() == {"feedforward": 1}
    finally:
        hip.timer.enabled = False


def test_cross_attention_cat_on_the_kernels_and_with_the_switch_off(monkeypatch):
    torch.manual_seed(6)
    b, tq, tk, e = 67, 2, 5, 12
    layer = CrossAttention(e, num_heads=4, hidden_dim=128, skip_kind="cat").to(DEV)
    q = torch.randn(b, tq, e, generator=gen(63)).to(DEV)
    kv = torch.randn(b, tk, e, generator=gen(64)).to(DEV)
    dout = torch.randn(b, tq, e, generator=gen(65)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, layer, [q, kv], {}, dout))


def test_self_attention_without_a_skip_connection_on_the_kernels_and_with_the_switch_off(monkeypatch):
    torch.manual_seed(7)
    b, t, e = 67, 5, 8
    layer = SelfAttention(e, skip_kind=None).to(DEV)
    x = torch.randn(b, t, e, generator=gen(66)).to(DEV)
    dout = torch.randn(b, t, e, generator=gen(67)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, layer, [x], {}, dout))


def test_a_shared_layer_s_gradients_accumulate_over_both_passes(monkeypatch):
    torch.manual_seed(8)
    b, t, e = 67, 5, 8
    stack = SelfAttentionStack(SelfAttention(e, num_heads=4, hidden_dim=64, skip_kind="residual"), 2,
                               share_parameters=True).to(DEV)
    x = torch.randn(b, t, e, generator=gen(68)).to(DEV)
    dout = torch.randn(b, t, e, generator=gen(69)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, stack, [x], dict(key_padding_mask=window_padding(b, t)), dout),
                             passes=2)


def test_transformer_trader_collects_and_steps_on_the_kernels(monkeypatch):
    num_envs, horizon, num_layers = 64, 32, 2
    runs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", switch)
        torch.manual_seed(0)
        algo = AlgorithmConfig(num_envs=num_envs, horizon=horizon, model_cls=TransformerTrader,
                               model_config={"seq_len": 4}, num_sgd_iters=1).build(AlgoTrading)
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            algo.collect()
            collected = launches()
            buf = algo.buffer
            record = [buf[key].clone() for key in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.VALUES)]
            hip.timer.reset()
            stats = algo.step()
            stepped = launches()
        finally:
            hip.timer.enabled = False
        assert math.isfinite(stats["losses/total"])
        runs.append((record, collected, stepped, stats))
    (on, collected, stepped, stats_on), (off, collected_off, stepped_off, stats_off) = runs
    assert collected == {"feedforward": (horizon + 1) * num_layers}  # (one per pass through the shared layer)
    assert stepped == {"feedforward": num_layers, "feedforward_backward": num_layers}
    assert collected_off == {} and stepped_off == {}
    assert torch.equal(on[0], off[0]), "actions differ"
    for name, got, want in (("logp", on[1], off[1]), ("values", on[2], off[2])):
        print(f"{name}: max|on - off| {float((got - want).abs().max()):.2e}")
        torch.testing.assert_close(got, want, rtol=1e-5, atol=2e-6, msg=lambda m, n=name: f"{n}: {m}")
    print(f"losses/total on {stats_on['losses/total']:.8f} off {stats_off['losses/total']:.8f}")
