"""The streaming attention kernels (``rl8_attention_long_f32`` / ``rl8_attention_long_backward_f32``) on the GPU, and
the modules that reach them with ``RL8_AMD_LONG_ATTENTION=1``.

Yardsticks, bars and helpers are those of ``tests/test_attention_kernels_gpu.py`` (its docstring has the two bars): each
case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor before it asserts (measured on an MI355X: out 0.73 ..
1.47, dq 0.81 .. 1.97, dk 0.46 .. 2.67, dv 0.85 .. 2.44).
"""

import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402
from rl8_amd.nn import PerceiverLayer, SelfAttention  # noqa: E402
from rl8_amd.nn.fused_attention import attention_reference  # noqa: E402

from .test_attention_kernels_gpu import (DEV, assert_guards, gen, guarded, launches, lay_out, make_masks, ptr,  # noqa: E402
                                         stream, torch_math, with_grads)

#: (B, Tq, Tk, H, D, layout, masks): the smallest shapes at which each mechanism can go wrong.  Chunks are 64 rows of the
#: streamed sequence; 1 / 2 / >= 3 strips of 16 rows give 4 / 2 / 1 lanes over a chunk's tiles.
CASES = [
    (67, 5, 130, 2, 17, "cross", "window"),  # one strip, four lanes, three chunks; rows 64 .. 66: first chunk all padded
    (3, 17, 129, 4, 8, "cross", "random"),  # two strips, two lanes; a chunk of one key; batch row 0 dead
    (3, 129, 129, 1, 64, "packed", "causal"),  # smallest outside the wide family; NF = 4; later chunks all -inf
    (1, 65, 192, 2, 32, "cross", "both"),  # five strips: no lane split; chunk-exact Tk (packed needs Tq = Tk)
    (3, 16, 193, 1, 33, "offset", "bias"),  # strip-exact Tq; one key past a chunk edge; column padding; unaligned bases
    (3, 300, 5, 2, 20, "separate", "window"),  # dK/dV streams five query chunks with its split on
    (1, 2048, 17, 1, 8, "separate", "none"),  # the envelope's edge, one side at a time
    (1, 3, 2048, 2, 64, "cross", "random"),
    (67, 5, 5, 2, 1, "packed", "none"),  # inside every family: D = 1, one chunk, three lanes without a tile
    # ``random`` and ``both`` pad batch row 0 entirely, so the two B = 1 cases above are dead throughout (every chunk
    # without a key): the same shapes with live batch rows behind it
    (3, 65, 192, 2, 32, "cross", "both"),
    (2, 3, 2048, 2, 64, "cross", "random"),
]


@functools.lru_cache(maxsize=None)
def case(index: int) -> dict:
    """Inputs (CPU, float32), ``ref64`` and ``torch32`` of ``CASES[index]``: computed once, shared, never modified."""
    b, tq, tk, heads, d, layout, kind = CASES[index]
    e = heads * d
    g = gen(500 + index)
    q, k, v = (torch.randn(b, t, e, generator=g) for t in (tq, tk, tk))
    dout = torch.randn(b, tq, e, generator=g)
    padding, bias = make_masks(kind, b, tq, tk, 600 + index)
    ref64 = with_grads(lambda a, c, w: attention_reference(a, c, w, padding, None if bias is None else bias.double(),
                                                           heads), q.double(), k.double(), v.double(), dout.double())
    dp, db = (None if m is None else m.to(DEV) for m in (padding, bias))
    torch32 = with_grads(lambda a, c, w: torch_math(a, c, w, dp, db, heads), q.to(DEV), k.to(DEV), v.to(DEV),
                         dout.to(DEV))
    return dict(q=q, k=k, v=v, dout=dout, padding=padding, bias=bias, heads=heads, layout=layout, ref64=ref64,
                torch32=tuple(x.double().cpu() for x in torch32))


def run_kernels(c: dict):
    """``(out, lse, dq, dk, dv)`` of the long entries, operands and gradients in the case's layout, every output
    between guard words."""
    (b, tq, e), tk, heads, lib = c["q"].shape, c["k"].shape[1], c["heads"], hip.load()
    (q, k, v), _ = lay_out(c["layout"], b, tq, tk, e, fill=(c["q"], c["k"], c["v"]))
    padding, bias = (None if m is None else m.to(DEV) for m in (c["padding"], c["bias"]))
    (obuf, out), (lbuf, lse), (wbuf, delta) = guarded(b * tq * e), guarded(b * heads * tq), guarded(b * heads * tq)
    strides = hip._rows(q, (b, tq, e), "q"), hip._rows(k, (b, tk, e), "k")
    assert lib.rl8_attention_long_f32(ptr(q), strides[0], ptr(k), ptr(v), strides[1], ptr(padding), ptr(bias), b, tq, tk,
                                      heads, e // heads, ptr(out), ptr(lse), stream()) == 0
    (dq, dk, dv), bufs = lay_out(c["layout"], b, tq, tk, e)
    dout = c["dout"].to(DEV)
    assert lib.rl8_attention_long_backward_f32(
        ptr(q), strides[0], ptr(k), ptr(v), strides[1], ptr(padding), ptr(bias), ptr(out), ptr(lse), ptr(dout), b, tq, tk,
        heads, e // heads, ptr(dq), hip._rows(dq, (b, tq, e), "dq"), ptr(dk), ptr(dv), hip._rows(dk, (b, tk, e), "dk"),
        ptr(delta), stream()) == 0
    for buf in bufs + [obuf, lbuf, wbuf]:
        assert_guards(buf, "a kernel output")
    for name, x in (("out", out), ("lse", lse), ("delta", delta), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert not bool((x == -77).any()), f"{name}: an element was not written"
    return out.view(b, tq, e), lse.view(b, heads, tq), dq, dk, dv


@pytest.mark.parametrize("index", range(len(CASES)), ids=lambda i: "-".join(map(str, CASES[i])))
def test_long_kernels_against_float64_within_three_times_torch_s_own_error(index):
    c = case(index)
    out, lse, dq, dk, dv = run_kernels(c)
    got = [x.double().cpu() for x in (out, dq, dk, dv)]
    figures = []
    for name, g, want, t32 in zip(("out", "dq", "dk", "dv"), got, c["ref64"], c["torch32"]):
        assert not torch.isnan(g).any() and not torch.isnan(t32).any(), name
        figures.append((name, float((g - want).abs().max()), float((t32 - want).abs().max())))
    print(f"{CASES[index]}: " + "  ".join(f"{n} {err:.2e} / {te:.2e} = {err / te if te else math.nan:.2f}"
                                           for n, err, te in figures))
    for (name, _, torch_err), g, want in zip(figures, got, c["ref64"]):
        floor = 1e-6 + 1e-5 * want.abs() if name == "out" else 2e-5 * float(want.abs().max()) + 1e-9
        excess = (g - want).abs() - (3 * torch_err + floor)
        assert bool((excess <= 0).all()), (name, float(excess.max()))
    # a query without an admissible key: out and dq exactly 0, lse = +inf (and finite for every other query)
    (b, tq, _), tk = c["q"].shape, c["k"].shape[1]
    masked = torch.zeros(b, tq, tk, dtype=torch.bool)
    if c["bias"] is not None:
        masked |= c["bias"] == -math.inf
    if c["padding"] is not None:
        masked |= c["padding"][:, None, :]
    dead = masked.all(dim=-1)  # [B, Tq]
    by_query = lse.cpu().transpose(1, 2)  # [B, Tq, H]
    assert bool((by_query[dead] == math.inf).all()) and bool(torch.isfinite(by_query[~dead]).all())
    assert not bool(got[0][dead].any()) and not bool(got[1][dead].any())
    if CASES[index][6] in ("random", "both"):
        assert bool(dead[0].all())  # (batch row 0 has every key padded)
    if c["padding"] is not None:  # padded keys take no gradient
        assert not bool(got[2][c["padding"]].any()) and not bool(got[3][c["padding"]].any())
    for first, second in zip((out, lse, dq, dk, dv), run_kernels(c)):  # a second run: the same bits
        assert torch.equal(first, second)


# --- the modules through the public route -------------------------------------------------------------------------
def module_run(monkeypatch, module, inputs, padding, dout, switch):
    """``([output, input gradients ..., parameter gradients ...], attention launches)`` of one forward + backward."""
    monkeypatch.setenv("RL8_AMD_LONG_ATTENTION", switch)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        xs = [x.clone().requires_grad_(True) for x in inputs]
        module.zero_grad()
        out = module(*xs, key_padding_mask=padding)
        out.backward(dout)
        ran = launches()
    finally:
        hip.timer.enabled = False
    return [out.detach()] + [x.grad for x in xs] + [p.grad.clone() for p in module.parameters()], ran


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_modules_on_the_long_kernels_against_float64(monkeypatch, kind):
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    monkeypatch.delenv("RL8_AMD_WIDE_ATTENTION", raising=False)
    torch.manual_seed(8)
    if kind == "self":
        b, tq, tk, e = 5, 130, 130, 64
        layer = SelfAttention(e, num_heads=2, hidden_dim=128, skip_kind="residual")
    else:
        # (the self-attention over the 8 latents has heads of 32 floats: the wide family's, which this switch leaves
        # on the module)
        b, tq, tk, e = 5, 8, 200, 64
        layer = PerceiverLayer(e, num_heads=2, num_layers=1)
    inputs = [torch.randn(b, t, e, generator=gen(91 + i)) for i, t in enumerate((tq,) if kind == "self" else (tq, tk))]
    padding = make_masks("window", b, tq, tk, 0)[0]
    reference = copy.deepcopy(layer).double()
    with torch.no_grad():
        dout = torch.randn(reference(*[x.double() for x in inputs], key_padding_mask=padding).shape, generator=gen(93))
    want, _ = module_run(monkeypatch, reference, [x.double() for x in inputs], padding, dout.double(), "0")
    layer = layer.to(DEV)
    device_args = ([x.to(DEV) for x in inputs], padding.to(DEV), dout.to(DEV))
    off, ran_off = module_run(monkeypatch, layer, *device_args, "0")
    on, ran_on = module_run(monkeypatch, layer, *device_args, "1")
    assert ran_on == {"attention_long": 1, "attention_long_backward": 1} and ran_off == {}
    names = ["out"] + [f"input {i}" for i in range(len(inputs))] + [n for n, _ in layer.named_parameters()]
    for name, got, base, ref in zip(names, on, off, want):
        diff, off_err = (got.double().cpu() - ref).abs(), float((base.double().cpu() - ref).abs().max())
        print(f"{name}: on {float(diff.max()):.2e}, off {off_err:.2e}")
        floor = 1e-6 + 1e-5 * ref.abs() if name == "out" else 2e-5 * float(ref.abs().max()) + 1e-9
        assert bool((diff <= 3 * off_err + floor).all()), name


def test_transformer_trader_over_160_steps_collects_and_steps_on_the_long_kernels(monkeypatch):
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    monkeypatch.setenv("RL8_AMD_LONG_ATTENTION", "1")
    torch.manual_seed(0)
    algo = AlgorithmConfig(num_envs=64, horizon=8, model_cls=TransformerTrader,
                           model_config={"seq_len": 160}).build(AlgoTrading)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = dict(algo.collect())
        stats.update(algo.step())
        ran = launches()
    finally:
        hip.timer.enabled = False
    assert ran.get("attention_long", 0) > 0 and ran.get("attention_long_backward", 0) > 0
    for name, value in stats.items():
        assert math.isfinite(float(value)), name
