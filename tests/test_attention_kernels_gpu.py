"""The short-sequence attention kernels (``rl8_attention_f32`` / ``rl8_attention_backward_f32``) on the GPU, and the
modules that run on them.

Yardsticks.  ``ref64``: ``rl8_amd.nn.fused_attention.attention_reference`` in float64 on the CPU (pinned to
``nn.MultiheadAttention`` at 1e-12 by ``tests/test_attention_host.py``).  ``torch32``: what the modules ran before these
kernels -- ``scaled_dot_product_attention`` on torch's math backend with the two masks merged into one float mask, as
``nn.MultiheadAttention`` calls it -- on the same device tensors in float32, forward and autograd.

Bars (the "3x the yardstick's own error + floor" rule of DESIGN.md §5 / §8), on 100 % of the elements:
* forward, elementwise: ``|got - ref64| <= 3 max|torch32 - ref64| + 1e-6 + 1e-5 |ref64|`` (the floor is the masked
  log-softmax bars');
* each of dq, dk, dv: ``|got - ref64| <= 3 max|torch32 - ref64| + 2e-5 max|ref64| + 1e-9`` (the floor is the loss
  kernels' gradient bars').
Each case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor before it asserts (measured on an MI355X: out
0.71 .. 2.03, dq 0.96 .. 2.04, dk 0.98 .. 2.99, dv 0.49 .. 2.46).

A query without an admissible key -- every key padded, or at ``-inf`` in the bias -- has output 0, ``lse = +inf`` and
gradient 0, and adds exactly nothing to dk and dv.  Every kernel output lies between guard words.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402
from rl8_amd.nn import CrossAttention, SelfAttention  # noqa: E402
from rl8_amd.nn.fused_attention import attention_reference  # noqa: E402

DEV = "cuda"
GUARD = 64  # elements in front of and behind every kernel output
#: (B, Tq, Tk, H, D, layout, masks): every B in {1, 3, 64, 67, 4099}, T in {1, 2, 5, 33, 64}, D in {1, 2, 3, 8, 16} and H
#: in {1, 4} at least twice, Tq != Tk five times.  Layouts: ``packed`` one [B, T, 3E] projection and one gradient buffer
#: of that shape; ``cross`` q dense, k and v in one [B, Tk, 2E]; ``separate`` three dense tensors; ``offset`` three
#: dense tensors whose base pointers sit one element into their allocations.
CASES = [
    (4099, 5, 5, 4, 2, "packed", "window"),
    (67, 1, 1, 1, 1, "separate", "none"),
    (3, 64, 64, 1, 16, "packed", "causal"),
    (64, 2, 33, 4, 3, "cross", "random"),
    (67, 33, 5, 4, 8, "separate", "both"),
    (1, 5, 5, 4, 2, "offset", "bias"),
    (1, 64, 1, 1, 16, "separate", "bias"),
    (3, 2, 2, 4, 1, "packed", "none"),
    (64, 33, 33, 1, 3, "packed", "window"),
    (4099, 1, 2, 4, 8, "cross", "random"),
    (4099, 2, 64, 1, 1, "cross", "window"),
]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def make_masks(kind: str, b: int, tq: int, tk: int, seed: int) -> tuple[None | torch.Tensor, None | torch.Tensor]:
    """CPU ``(key_padding [b, tk] bool, True = PADDED; bias [tq, tk] float32)``.  ``window``: row i has ``i % tk`` leading
    keys padded.  ``random``: 0.4 of the keys, batch row 0 entirely.  ``causal``: a bool mask as 0 / -inf.  ``bias``:
    random floats, 0.3 of them -inf.  ``both``: the random padding and the random bias together."""
    g = gen(seed)
    window = torch.arange(tk).expand(b, tk) < (torch.arange(b) % tk).unsqueeze(1)
    random = torch.rand(b, tk, generator=g) < 0.4
    random[0] = True
    causal = torch.zeros(tq, tk).masked_fill(torch.arange(tk).expand(tq, tk) > torch.arange(tq).unsqueeze(1), -math.inf)
    bias = torch.randn(tq, tk, generator=g).masked_fill(torch.rand(tq, tk, generator=g) < 0.3, -math.inf)
    return {"none": (None, None), "window": (window, None), "random": (random, None), "causal": (None, causal),
            "bias": (None, bias), "both": (random, bias)}[kind]


def guarded(numel: int) -> tuple[torch.Tensor, torch.Tensor]:
    """A sentinel-filled float32 buffer and the ``numel`` elements in its middle that a kernel may write."""
    buf = torch.full((numel + 2 * GUARD,), -77.0, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def assert_guards(buf: torch.Tensor, what: str) -> None:
    assert bool((buf[:GUARD] == -77).all()) and bool((buf[-GUARD:] == -77).all()), f"{what}: wrote outside its output"


def lay_out(layout: str, b: int, tq: int, tk: int, e: int, fill=None):
    """Device views ``(q, k, v)`` in ``layout`` and the guarded buffers they live in; ``fill`` = CPU (q, k, v) to copy in,
    or nothing for gradient outputs (left at the sentinel)."""
    if layout == "packed":
        assert tq == tk
        buf, flat = guarded(b * tq * 3 * e)
        qkv = flat.view(b, tq, 3 * e)
        views, bufs = (qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:]), [buf]
    elif layout == "cross":
        qbuf, qflat = guarded(b * tq * e)
        kvbuf, kvflat = guarded(b * tk * 2 * e)
        kv = kvflat.view(b, tk, 2 * e)
        views, bufs = (qflat.view(b, tq, e), kv[..., :e], kv[..., e:]), [qbuf, kvbuf]
    else:
        shift = 1 if layout == "offset" else 0  # (GUARD + 1 elements, 4 bytes past a 256-byte boundary)
        views, bufs = [], []
        for t in (tq, tk, tk):
            buf, flat = guarded(b * t * e + shift)
            views.append(flat[shift:].view(b, t, e))
            bufs.append(buf)
    if fill is not None:
        for view, x in zip(views, fill):
            view.copy_(x)
    return tuple(views), bufs


def ptr(t: None | torch.Tensor) -> None | int:
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def raw_forward(q, k, v, padding, bias, heads):
    """``rl8_attention_f32`` on device views: ``(out [B, Tq, E], lse [B, H, Tq])`` between guard words."""
    (b, tq, e), tk = q.shape, k.shape[1]
    obuf, out = guarded(b * tq * e)
    lbuf, lse = guarded(b * heads * tq)
    status = hip.load().rl8_attention_f32(ptr(q), hip._rows(q, (b, tq, e), "q"), ptr(k), ptr(v),
                                          hip._rows(k, (b, tk, e), "k"), ptr(padding), ptr(bias), b, tq, tk, heads,
                                          e // heads, ptr(out), ptr(lse), stream())
    assert status == 0
    assert_guards(obuf, "out")
    assert_guards(lbuf, "lse")
    return out.view(b, tq, e), lse.view(b, heads, tq)


def raw_backward(layout, q, k, v, padding, bias, out, lse, dout, heads):
    """``rl8_attention_backward_f32`` writing gradients laid out as the operands are: ``(dq, dk, dv)``."""
    (b, tq, e), tk = q.shape, k.shape[1]
    (dq, dk, dv), bufs = lay_out(layout, b, tq, tk, e)
    wbuf, delta = guarded(b * heads * tq)
    status = hip.load().rl8_attention_backward_f32(
        ptr(q), hip._rows(q, (b, tq, e), "q"), ptr(k), ptr(v), hip._rows(k, (b, tk, e), "k"), ptr(padding), ptr(bias),
        ptr(out), ptr(lse), ptr(dout), b, tq, tk, heads, e // heads, ptr(dq), hip._rows(dq, (b, tq, e), "dq"), ptr(dk),
        ptr(dv), hip._rows(dk, (b, tk, e), "dk"), ptr(delta), stream())
    assert status == 0
    for buf in bufs + [wbuf]:
        assert_guards(buf, "gradients")
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert not bool((g == -77).any()), f"{name}: an element was not written"
    return dq, dk, dv


def torch_math(q, k, v, padding, bias, heads):
    """The route before these kernels, on device tensors: the math backend under the merged float mask."""
    (b, tq, e), tk = q.shape, k.shape[1]
    d = e // heads
    mask = None
    if padding is not None or bias is not None:
        mask = torch.zeros(b, 1, tq, tk, dtype=q.dtype, device=q.device)
        if bias is not None:
            mask = mask + bias
        if padding is not None:
            mask = mask.masked_fill(padding[:, None, None, :], -math.inf)
    split = lambda x, t: x.reshape(b, t, heads, d).transpose(1, 2)  # noqa: E731
    with sdpa_kernel(SDPBackend.MATH):
        out = F.scaled_dot_product_attention(split(q, tq), split(k, tk), split(v, tk), attn_mask=mask)
    return out.transpose(1, 2).reshape(b, tq, e)


def with_grads(fn, q, k, v, dout):
    q, k, v = (x.clone().requires_grad_(True) for x in (q, k, v))
    out = fn(q, k, v)
    out.backward(dout)
    return out.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def case(index: int) -> dict:
    """Inputs (CPU, float32), ``ref64`` and ``torch32`` of ``CASES[index]``: computed once, shared, never modified."""
    b, tq, tk, heads, d, layout, kind = CASES[index]
    e = heads * d
    g = gen(100 + index)
    q, k, v = (torch.randn(b, t, e, generator=g) for t in (tq, tk, tk))
    dout = torch.randn(b, tq, e, generator=g)
    padding, bias = make_masks(kind, b, tq, tk, 200 + index)
    ref64 = with_grads(lambda a, c, w: attention_reference(a, c, w, padding, None if bias is None else bias.double(),
                                                           heads), q.double(), k.double(), v.double(), dout.double())
    dp, db = (None if m is None else m.to(DEV) for m in (padding, bias))
    torch32 = with_grads(lambda a, c, w: torch_math(a, c, w, dp, db, heads), q.to(DEV), k.to(DEV), v.to(DEV),
                         dout.to(DEV))
    return dict(q=q, k=k, v=v, dout=dout, padding=padding, bias=bias, heads=heads, layout=layout,
                ref64=ref64, torch32=tuple(x.double().cpu() for x in torch32))


def run_kernels(c: dict, dout: None | torch.Tensor = None):
    """``(out, lse, dq, dk, dv)`` of the kernels on a case, its operands and gradients in the case's layout."""
    (b, tq, e), tk = c["q"].shape, c["k"].shape[1]
    (q, k, v), _ = lay_out(c["layout"], b, tq, tk, e, fill=(c["q"], c["k"], c["v"]))
    padding, bias = (None if m is None else m.to(DEV) for m in (c["padding"], c["bias"]))
    out, lse = raw_forward(q, k, v, padding, bias, c["heads"])
    dout = (c["dout"] if dout is None else dout).to(DEV)
    dq, dk, dv = raw_backward(c["layout"], q, k, v, padding, bias, out, lse, dout, c["heads"])
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("index", range(len(CASES)), ids=lambda i: "-".join(map(str, CASES[i])))
def test_kernels_against_float64_within_three_times_torch_s_own_error(index):
    c = case(index)
    out, lse, dq, dk, dv = run_kernels(c)
    got = [x.double().cpu() for x in (out, dq, dk, dv)]
    names = ("out", "dq", "dk", "dv")
    figures = []
    for name, g, want, t32 in zip(names, got, c["ref64"], c["torch32"]):
        assert not torch.isnan(g).any() and not torch.isnan(t32).any(), name
        torch_err, err = float((t32 - want).abs().max()), float((g - want).abs().max())
        figures.append((name, err, torch_err))
    print(f"{CASES[index]}: " + "  ".join(f"{n} {err:.2e} / {te:.2e} = {err / te if te else math.nan:.2f}"
                                           for n, err, te in figures))
    for (name, _, torch_err), g, want in zip(figures, got, c["ref64"]):
        if name == "out":
            bar = 3 * torch_err + 1e-6 + 1e-5 * want.abs()
        else:
            bar = torch.full_like(want, 3 * torch_err + 2e-5 * float(want.abs().max()) + 1e-9)
        assert bool(((g - want).abs() <= bar).all()), (name, float(((g - want).abs() - bar).max()))
    # lse: log-sum-exp of the admissible scores, +inf where there is none
    heads = c["heads"]
    (b, tq, e), tk = c["q"].shape, c["k"].shape[1]
    qh, kh = (x.double().reshape(b, t, heads, e // heads).transpose(1, 2) for x, t in ((c["q"], tq), (c["k"], tk)))
    scores = qh @ kh.transpose(-1, -2) / math.sqrt(e // heads)
    if c["bias"] is not None:
        scores = scores + c["bias"].double()
    if c["padding"] is not None:
        scores = scores.masked_fill(c["padding"][:, None, None, :], -math.inf)
    want_lse = torch.logsumexp(scores, dim=-1)
    dead = want_lse == -math.inf
    got_lse = lse.double().cpu()
    assert bool((got_lse[dead] == math.inf).all())
    assert bool(((got_lse - want_lse)[~dead].abs() <= 1e-6 + 1e-5 * want_lse[~dead].abs()).all())


def test_a_fully_padded_batch_row_gives_zeros_and_no_nan():
    index = 3  # (64, 2, 33, 4, 3) under random padding: batch row 0 has no key at all
    c = case(index)
    assert bool(c["padding"][0].all()) and not bool(c["padding"][1:].all(dim=1).any())
    out, lse, dq, dk, dv = run_kernels(c)
    for name, x in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert not bool(torch.isnan(x).any()), name
        assert not bool(x[0].any()), f"{name} of the padded batch row is not exactly 0"
    assert bool((lse[0] == math.inf).all()) and bool(torch.isfinite(lse[1:]).all())
    # padded keys of the other rows take no gradient either
    padded = c["padding"].to(DEV)
    assert not bool(dk[padded].any()) and not bool(dv[padded].any())


def test_a_query_without_a_key_adds_exactly_nothing_to_dk_and_dv():
    b, tq, tk, heads, d = 67, 5, 7, 4, 2
    e = heads * d
    g = gen(31)
    bias = torch.randn(tq, tk, generator=g)
    bias[1] = -math.inf  # query 1 of every batch row may attend to nothing
    bias[3, :4] = -math.inf
    c = dict(q=torch.randn(b, tq, e, generator=g), k=torch.randn(b, tk, e, generator=g),
             v=torch.randn(b, tk, e, generator=g), dout=torch.randn(b, tq, e, generator=g), padding=None, bias=bias,
             heads=heads, layout="cross")
    out, lse, dq, dk, dv = run_kernels(c)
    assert not bool(out[:, 1].any()) and not bool(dq[:, 1].any()) and bool((lse[:, :, 1] == math.inf).all())
    assert bool(out[:, 0].any()) and bool(dq[:, 0].any())
    other = c["dout"].clone()
    other[:, 1] = 1000.0 * torch.randn(b, e, generator=g)  # what flows into the dead query changes ...
    _, _, dq2, dk2, dv2 = run_kernels(c, dout=other)
    assert torch.equal(dk2, dk) and torch.equal(dv2, dv) and torch.equal(dq2, dq)  # ... and nothing else does
    for x in (out, dq, dk, dv):
        assert not bool(torch.isnan(x).any())


@pytest.mark.parametrize("index", [0, 4])
def test_backward_is_bit_reproducible(index):
    first = run_kernels(case(index))
    second = run_kernels(case(index))
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# --- the modules through the public route -------------------------------------------------------------------------
def launches() -> dict[str, int]:
    return {name: int(s["launches"]) for name, s in hip.timer.summary().items() if name.startswith("attention")}


def module_runs(monkeypatch, module, inputs, kwargs, dout):
    """``(outputs, gradients of inputs and parameters, attention launches)`` with the kernels on and off."""
    runs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", switch)
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


def assert_module_runs_agree(runs) -> None:
    (out1, grads1, ran1), (out0, grads0, ran0) = runs
    assert ran1 == {"attention": 1, "attention_backward": 1} and ran0 == {}
    assert set(grads1) == set(grads0)
    for name, got, want in [("out", out1, out0)] + [(n, grads1[n], grads0[n]) for n in grads0]:
        diff, top = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name}: max|on - off| {diff:.2e}, largest entry {top:.2e}")
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6, msg=lambda m, n=name: f"{n}: {m}")
        assert diff <= 2e-5 * top, name


def test_self_attention_on_the_kernels_and_with_the_switch_off(monkeypatch):
    torch.manual_seed(5)
    b, t, e = 5, 5, 8
    layer = SelfAttention(e, num_heads=4, hidden_dim=64, skip_kind="residual").to(DEV)
    x = torch.randn(b, t, e, generator=gen(51)).to(DEV)
    dout = torch.randn(b, t, e, generator=gen(52)).to(DEV)
    padding = make_masks("window", b, t, t, 0)[0].to(DEV)
    causal = (torch.arange(t).expand(t, t) > torch.arange(t).unsqueeze(1)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, layer, [x], dict(key_padding_mask=padding), dout))
    assert_module_runs_agree(module_runs(monkeypatch, layer, [x], dict(attention_mask=causal), dout))
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        with torch.no_grad():
            layer(x, key_padding_mask=padding)
        assert launches() == {"attention": 1}
    finally:
        hip.timer.enabled = False


def test_cross_attention_on_the_kernels_and_with_the_switch_off(monkeypatch):
    torch.manual_seed(6)
    b, tq, tk, e = 5, 2, 5, 12
    layer = CrossAttention(e, num_heads=4).to(DEV)
    q = torch.randn(b, tq, e, generator=gen(61)).to(DEV)
    kv = torch.randn(b, tk, e, generator=gen(62)).to(DEV)
    padding = make_masks("window", b, tq, tk, 0)[0].to(DEV)
    with torch.no_grad():
        shape = layer(q, kv, key_padding_mask=padding).shape
    dout = torch.randn(shape, generator=gen(63)).to(DEV)
    assert_module_runs_agree(module_runs(monkeypatch, layer, [q, kv], dict(key_padding_mask=padding), dout))


def test_attention_dropout_in_training_stays_on_torch(monkeypatch):
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    torch.manual_seed(7)
    layer = SelfAttention(8, num_heads=4, hidden_dim=64, attention_dropout=0.1, skip_kind="residual").to(DEV)
    x = torch.randn(5, 5, 8, generator=gen(71)).to(DEV)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        layer.train()(x).sum().backward()
        assert launches() == {}
        layer.eval()(x).sum().backward()
        assert launches() == {"attention": 1, "attention_backward": 1}
    finally:
        hip.timer.enabled = False


def test_transformer_trader_collects_and_steps_on_the_kernels(monkeypatch):
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    num_envs, horizon = 64, 32
    torch.manual_seed(0)
    algo = AlgorithmConfig(num_envs=num_envs, horizon=horizon, model_cls=TransformerTrader, model_config={"seq_len": 4},
                           num_sgd_iters=1).build(AlgoTrading)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        algo.collect()
        assert launches() == {"attention": 2 * (horizon + 1)}  # (two passes through the shared layer per forward)
        hip.timer.reset()
        stats = algo.step()
        assert launches() == {"attention": 2, "attention_backward": 2}
    finally:
        hip.timer.enabled = False
    assert math.isfinite(stats["losses/total"])
