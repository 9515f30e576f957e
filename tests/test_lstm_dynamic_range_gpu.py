"""The width-256 LSTM on fp16 planes over the range of its states: the forward against the magnitude of ``h0``
(``hip.lstm_forward_split``, ``fused_lstm.lstm_forward`` under autograd, ``fused_lstm.lstm_heads_forward``), against
the weights, ``c0`` and ``x``, and the heads form of the backward through time at and past its documented limit on
``|c|`` (``include/rl8_amd.h``, beside ``rl8_lstm_rows_backward_heads_f32``).

Yardsticks.  ``ref64``: ``torch.nn.LSTM(d_in, 256)`` in float64 on the same fp32 inputs (no MIOpen); a float64
recurrence written out with torch ops, pinned to that module at 1e-12, supplies what the module does not return (the
cell state of every step, the gates, the step-0 pre-activations).  ``torch32``: the same module in float32, eager, on
the device.  Beside it, printed only, the project's fp32-MFMA kernel ``hip.lstm_forward``, which has no planes and no
scale.

Bars (DESIGN.md sections 5 and 8): ``|got - ref64| <= 3 max|torch32 - ref64| + floor``, taken row by row (a global
maximum would hide the small rows beside a large one).  Floors: 2e-6 for ``hs`` (``|h| < 1``), ``2e-6 max(1, the
row's max |c0|)`` for ``cs`` / ``cn`` and the saved gates; a head output ``hs . w + b`` inherits ``2e-6 (1 + sum |w|)``;
a gradient ``2e-5`` of its largest entry (the bar of ``test_lstm_backward_on_planes_matches_autograd``).

What the big-row cases hold and what they do not.  With ``W_hh / (16 * 2^10)``, as the sensitivity rule below
prescribes, the small rows' recurrent term is ~1e-4 of a pre-activation, so the 2e-6 floor resolves it to a few per
cent: these cases catch a dropped, mis-scaled or misplaced product of the rows beside the large one, not lost plane
bits -- the header's claim that such rows keep both planes' bits is arithmetic (stated there), not something this
module measures; plane bits are measured by the product test of group 2.  At b = 1 the three ``big_row_*`` ids are
the same single row with no neighbour (kept so that every case runs at every shape).

Sensitivity.  With a large ``h0`` and ordinary weights every gate saturates and a wrong product still gives h = +-1,
so ``W_hh`` is ``U(-1, 1) / (16 max(1, s))`` for an ``h0`` of magnitude ``s`` (step-0 recurrent pre-activations of
standard deviation ~1/3), and every case asserts, in float64, that at least 90 % of the step-0 gate pre-activations lie
in (-6, 6).  Everything is drawn on the CPU with a seeded generator.

Non-finite rows.  A NaN in a row of ``h0`` gives NaN in that row of ``hs`` / ``cs``, here as in torch.  One infinity
saturates torch's gates (its row stays finite there); its planes are (inf, NaN), so that row is NaN here: loud, in that
row only, and stated in the header.

Before the fix that came with this module the state planes were those of ``h0 * 2^14`` whatever ``h0``: from
``|h0| = 4.0`` up every case of the first group failed with NaN rows (the assertion's text is under MEASURED).

Each case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor, and the same ratio of the fp32-MFMA kernel,
before it asserts.  Measured on an MI355X: see MEASURED below.
"""

import functools
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402
from rl8_amd.nn import fused_lstm  # noqa: E402

DEV = "cuda:0"
H = 256

#: ``got / yardstick`` as printed, over all shapes (filled in from a run on an MI355X)
MEASURED = """
group 1, forward (a):   hs 0.64 .. 2.80, cn 0.64 .. 2.06, cs 0.48 .. 1.84, gates 0.34 .. 2.61
   (fp32-MFMA kernel:   hs 0.79 .. 2.80, cn 0.71 .. 2.86, cs 0.65 .. 2.49, gates 0.71 .. 3.43)
group 1, autograd (b):  w_ih 0.49 .. 2.60, w_hh 0.27 .. 12.85 (h0 = 0 and 1e-30: the yardstick's error is ~0 there and
                        the floor of 2e-5 of the largest entry carries the bar), b 0.57 .. 2.54
group 1, heads (c):     out 0.23 .. 5.22 (under its floor), w_ih 0.42 .. 1.93, w_hh 0.23 .. 10.22, b 0.50 .. 2.17,
                        w_heads 0.14 .. 3.67
group 2:                hs 0.61 .. 3.88, cn 0.52 .. 4.86, cs 0.52 .. 2.27, gates 0.55 .. 4.59
   (fp32-MFMA kernel:   hs 0.74 .. 3.77, cn 0.68 .. 5.15, cs 0.56 .. 3.08, gates 0.75 .. 5.86; the ratios above 3 are
                        b = 1 rows whose yardstick error is below 1e-7, under the floor for both kernels)
group 2, the product:   per gate row, relative to sum |h| |w|, on the rows under test: planes 1.1e-07 .. 4.9e-07,
                        torch32 0.96e-07 .. 6.4e-07 (planes / torch32 0.64 .. 1.72), bar 5.4e-06 .. 7.5e-06; the same
                        product without its low planes 5.1e-05 .. 1.6e-03, seven to two hundred times the bar
group 3, |c| <= 4000:   err16 / (3 err_bf + 2e-7) 0.11 .. 0.84
group 3, past it:       |c| = 5000 loses no sequence (the kernel's bound is conservative); |c| = 1e5 at l = 3 loses
                        exactly the sequences that hold it (first and last of a wave, the last of the ragged wave) and
                        returns a NaN bound; before this module's fix to the maximum the bound came back finite there
                        (``assert not True`` on ``math.isfinite(bound)``).
Before the fix to the state split, from |h0| = 4.0 up (s = 4, 17, 1e4, 1e30 and every big-row case):
``AssertionError: hs: 300 of 300 rows not finite whose reference is (['hs nan / 2.59e-07 = nan (fp32-MFMA 0.79)'])``.
"""

BS, LS, DS, NS = (1, 129, 300), (1, 3), (1, 5), (1, 3)
H0_SCALES = (0.0, 1e-30, 0.999, 1.5, 3.99, 4.0, 17.0, 1e4, 1e30)
BIG = 2.0 ** 10


def _h0_cases():
    """(case id, b, l, d_in) for the first group: every magnitude at every shape; the big-row cases where the row exists."""
    out = []
    for b in BS:
        for l in LS:
            for d in DS:
                out += [(f"s={s:g}", b, l, d) for s in H0_SCALES]
                out += [("big_row_middle", b, l, d), ("big_row_first", b, l, d), ("big_row_last", b, l, d)]
                if b > 128:
                    out += [("big_row_128", b, l, d), ("nonfinite_rows", b, l, d)]
    return out


WEIGHT_CASES = ("outlier_weights", "six_decades", "zero_w_hh", "tiny_everything", "c0_1e4", "c0_1e-30", "x_1e5")


def _u(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1


@functools.lru_cache(maxsize=None)
def _case(case: str, b: int, l: int, d: int):
    """Inputs (seeded, CPU-drawn), the float64 reference and the float32 yardsticks of one case: computed once, shared
    by the tests that read them, never written."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{case} {b} {l} {d}".encode()))
    s, rows_big, rows_bad = 0.5, [], []
    x = torch.randn(b, l, d, generator=g) * 2
    w_ih, b_ih, b_hh = _u(g, 4 * H, d) * 0.2, _u(g, 4 * H) * 0.1, _u(g, 4 * H) * 0.1
    c0 = torch.randn(b, H, generator=g)
    h0 = _u(g, b, H) * 0.5
    if case.startswith("s="):
        s = float(case[2:])
        h0 = _u(g, b, H) * s
        h0[b // 2, 7] = s
        h0[0, 3] = -s
    elif case.startswith("big_row") or case == "nonfinite_rows":
        s = BIG
        r = {"big_row_middle": b // 2, "big_row_first": 0, "big_row_last": b - 1, "big_row_128": 128, "nonfinite_rows": 5}[case]
        h0 = _u(g, b, H) * 0.3
        h0[r] = _u(g, H) * BIG
        h0[r, 11] = -BIG
        rows_big = [r]
        if case == "nonfinite_rows":
            rows_bad = [2, b - 1]
            h0[2, 100] = float("nan")
            h0[b - 1, 0] = float("inf")
    w_hh = _u(g, 4 * H, H) / (16 * max(1.0, s))
    if case == "outlier_weights":
        at = torch.randperm(4 * H * H, generator=g)[:20]
        w_hh.view(-1)[at] *= 1000.0
    elif case == "six_decades":
        # rows over six decades, the largest rows where the plain matrix is: the pre-activation condition still holds
        w_hh *= (10.0 ** (torch.arange(4 * H) % 6 - 3).float() / 100.0)[:, None]
    elif case == "zero_w_hh":
        w_hh.zero_()
    elif case == "tiny_everything":
        w_ih, w_hh, b_ih, b_hh, h0 = w_ih * 1e-12, w_hh * 1e-12, b_ih * 1e-12, b_hh * 1e-12, h0 * 1e-12
    elif case == "c0_1e4":
        c0 = _u(g, b, H) * 1e4
    elif case == "c0_1e-30":
        c0 = _u(g, b, H) * 1e-30
    elif case == "x_1e5":
        x, w_ih = x * 1e5, w_ih * 1e-5
    t = dict(x=x, h0=h0, c0=c0, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh)
    t = {k: v.to(DEV).contiguous() for k, v in t.items()}
    ref = _recurrence(t, torch.float64)
    y32 = _recurrence(t, torch.float32)
    # the float64 recurrence IS the float64 module; the float32 module is the yardstick of what it returns
    m64, m32 = _module(t, torch.float64), _module(t, torch.float32)
    good = torch.ones(b, dtype=torch.bool, device=DEV)
    good[rows_bad] = False
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        hs_m, (_, cn_m) = m64(t["x"].double(), (t["h0"].double()[None], t["c0"].double()[None]))
        hs_32, (_, cn_32) = m32(t["x"], (t["h0"][None], t["c0"][None]))
    assert float((hs_m - ref["hs"])[good].abs().max()) < 1e-12 and float(((cn_m[0] - ref["cs"][:, -1])[good] / (1 + ref["cs"][:, -1][good].abs())).abs().max()) < 1e-12
    y32["hs"], y32["cn"] = hs_32, cn_32[0]
    ref["cn"] = ref["cs"][:, -1]
    # the condition on the inputs: the step-0 gates are not saturated, so a wrong product moves the outputs
    pre0 = ref["pre0"][good]
    inside = float(((pre0 > -6) & (pre0 < 6)).double().mean())
    assert inside >= 0.9, (case, inside)
    mfma = hip.lstm_forward(t["x"], t["h0"], t["c0"], hip.lstm_pack(t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"]), save=True)
    return dict(t=t, ref=ref, y32=y32, good=good, bad=rows_bad, big=rows_big, m64=m64, m32=m32,
                mfma=dict(hs=mfma[0], cn=mfma[2], gates=mfma[3], cs=mfma[4]))


def _module(t, dtype):
    m = torch.nn.LSTM(t["x"].shape[2], H, batch_first=True).to(DEV, dtype)
    with torch.no_grad():
        for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(m, name).copy_(t[key].to(dtype))
    return m


def _recurrence(t, dtype):
    """The LSTM's recurrences with torch ops in ``dtype``: hs, cs [B, L, 256], gates [B, L, 4, 256], pre0 [B, 1024]."""
    x, h, c, w_ih, w_hh, b_ih, b_hh = (t[k].to(dtype) for k in ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh"))
    bias = b_ih + b_hh
    hs, cs, gates, pre0 = [], [], [], None
    for step in range(x.shape[1]):
        pre = x[:, step] @ w_ih.T + h @ w_hh.T + bias
        pre0 = pre if pre0 is None else pre0
        i, f, gg, o = pre.view(-1, 4, H).unbind(1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c), gates.append(torch.stack([i, f, gg, o], 1))
    return dict(hs=torch.stack(hs, 1), cs=torch.stack(cs, 1), gates=torch.stack(gates, 1), pre0=pre0)


def _rows(v: torch.Tensor) -> torch.Tensor:
    """max over everything but the leading (row) dimension; NaN where a row holds one."""
    flat = v.reshape(v.shape[0], -1)
    return torch.where(torch.isnan(flat).any(1), torch.full_like(flat[:, 0], math.nan), flat.abs().amax(1))


def _hold(name, got, want, t32, floor, good, figures, also=None):
    """Row by row: |got - ref64| <= 3 max|torch32 - ref64| + floor on the rows of ``good``; the figures first."""
    err, yard = _rows(got.double() - want)[good], _rows(t32.double() - want)[good]
    floor = floor[good] if isinstance(floor, torch.Tensor) and floor.ndim else floor
    ratio = float(err.max()) / float(yard.max()) if float(yard.max()) else math.nan
    text = f"{name} {float(err.max()):.2e} / {float(yard.max()):.2e} = {ratio:.2f}"
    if also is not None:
        e2 = _rows(also.double() - want)[good]
        text += f" (fp32-MFMA {float(e2.max()) / float(yard.max()) if float(yard.max()) else math.nan:.2f})"
    figures.append(text)
    bad = int(torch.isnan(err).sum())
    assert bad == 0, f"{name}: {bad} of {err.numel()} rows not finite whose reference is ({figures})"
    assert bool((err <= 3 * yard + floor).all()), (name, float((err - 3 * yard - floor).max()), figures)


def _c_floor(c0: torch.Tensor) -> torch.Tensor:
    return 2e-6 * torch.nan_to_num(c0.abs().amax(1), nan=1.0, posinf=1.0).clamp_min(1.0).double()


def _check_forward(k, got, figures, gates=True):
    ref, y32, good, mfma = k["ref"], k["y32"], k["good"], k["mfma"]
    cf = _c_floor(k["t"]["c0"])
    _hold("hs", got["hs"], ref["hs"], y32["hs"], 2e-6, good, figures, mfma["hs"])
    _hold("cn", got["cn"], ref["cn"], y32["cn"], cf, good, figures, mfma["cn"])
    if gates:
        _hold("cs", got["cs"], ref["cs"], y32["cs"], cf, good, figures, mfma["cs"])
        _hold("gates", got["gates"], ref["gates"], y32["gates"], cf, good, figures, mfma["gates"])
    for r in k["bad"]:  # non-finite, and in those rows only
        assert not bool(torch.isfinite(got["hs"][r]).any()) and not bool(torch.isfinite(got["cn"][r]).any()), r
    if k["bad"]:
        assert bool(torch.isnan(ref["hs"][k["bad"][0]]).all())  # (the NaN row: as in torch)


def _split_forward(k, save):
    t = k["t"]
    packed, wb = hip.lstm_pack_split(t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"])
    hs, hn, cn, gates, cs = hip.lstm_forward_split(t["x"], t["h0"], t["c0"], packed, wb, save=save)
    assert torch.equal(hn, hs[:, -1])
    return dict(hs=hs, cn=cn, gates=gates, cs=cs)


@pytest.mark.parametrize("case,b,l,d", _h0_cases())
def test_plane_forward_holds_for_any_h0(case, b, l, d):
    """(a) ``hip.lstm_forward_split`` with and without the saved gates."""
    k, figures = _case(case, b, l, d), []
    got = _split_forward(k, True)
    try:
        _check_forward(k, got, figures)
    finally:
        print(f"[forward {case} b={b} l={l} d={d}]", "; ".join(figures))
    lean = _split_forward(k, False)
    assert lean["gates"] is None and lean["cs"] is None
    good = k["good"]
    assert torch.equal(lean["hs"][good], got["hs"][good]) and torch.equal(lean["cn"][good], got["cn"][good])


def _grad_hold(name, got, want, t32, figures):
    err, yard, top = float((got.double() - want).abs().max()), float((t32.double() - want).abs().max()), float(want.abs().max())
    figures.append(f"{name} {err:.2e} / {yard:.2e} = {err / yard if yard else math.nan:.2f}")
    assert math.isfinite(err), (name, figures)
    assert err <= 3 * yard + 2e-5 * top, (name, err, yard, top, figures)


@functools.lru_cache(maxsize=None)
def _head_modules():
    g = torch.Generator().manual_seed(3)
    heads = [torch.nn.Linear(H, n) for n in (2, 1)]
    with torch.no_grad():
        for head in heads:
            head.weight.copy_(_u(g, *head.weight.shape) / 16), head.bias.copy_(_u(g, *head.bias.shape))
    return [head.to(DEV) for head in heads]


def _stacked_heads():
    heads = _head_modules()
    return torch.cat([h.weight for h in heads]).detach(), torch.cat([h.bias for h in heads]).detach()


@functools.lru_cache(maxsize=None)
def _autograd_reference(case, b, l, d, with_heads=False):
    """Gradients of sum(hs * dhs), or of sum(heads(hs) * dout), in the float64 and the float32 module, once per case."""
    k, heads = _case(case, b, l, d), (_stacked_heads() if with_heads else None)
    t = k["t"]
    b, l = t["x"].shape[:2]
    g = torch.Generator().manual_seed(b + 10 * l)
    dhs = (torch.randn(b, l, H, generator=g) / (b * l)).to(DEV)
    out = {"dhs": dhs}
    if heads is not None:
        out["dout"] = (torch.randn(b * l, heads[0].shape[0], generator=g) / (b * l)).to(DEV)
    for tag, m, dt in (("ref", k["m64"], torch.float64), ("y32", k["m32"], torch.float32)):
        m.zero_grad()
        with torch.backends.cudnn.flags(enabled=False):
            hs, _ = m(t["x"].to(dt), (t["h0"].to(dt)[None], t["c0"].to(dt)[None]))
        if heads is None:
            loss = (hs * dhs.to(dt)).sum()
        else:
            w, bias = (p.detach().to(dt).requires_grad_(True) for p in heads)
            y = hs.reshape(-1, H) @ w.T + bias
            loss = (y * out["dout"].to(dt)).sum()
            out[tag + "_out"] = y.detach()
        loss.backward()
        out[tag] = {"w_ih": m.weight_ih_l0.grad.clone(), "w_hh": m.weight_hh_l0.grad.clone(), "b": m.bias_ih_l0.grad.clone()}
        if heads is not None:
            out[tag].update(w_heads=w.grad.clone(), b_heads=bias.grad.clone())
    return out


@pytest.mark.parametrize("case,b,l,d", _h0_cases())
def test_fused_lstm_under_autograd_holds_for_any_h0(case, b, l, d):
    """(b) ``fused_lstm.lstm_forward`` under autograd: outputs, ``cn`` and the gradients of ``w_ih``, ``w_hh`` and the
    bias -- the fp16-plane weight gradient scales step 0 by max |h0|.  With a NaN and an infinity in ``h0`` the
    gradients are NaN in torch too: that case holds the training forward (saved gates, shared planes) on the other rows."""
    k, figures = _case(case, b, l, d), []
    t = k["t"]
    lstm = _module(t, torch.float32)
    assert fused_lstm._plan(d, b).forward_planes
    hs, hn, cn = fused_lstm.lstm_forward(lstm, t["x"], t["h0"], t["c0"])
    assert hs.requires_grad
    if k["bad"]:
        try:
            _check_forward(k, dict(hs=hs.detach(), cn=cn), figures, gates=False)
        finally:
            print(f"[autograd {case} b={b} l={l} d={d}]", "; ".join(figures))
        return
    want = _autograd_reference(case, b, l, d)
    (hs * want["dhs"]).sum().backward()
    try:
        _check_forward(k, dict(hs=hs.detach(), cn=cn), figures, gates=False)
        _grad_hold("w_ih", lstm.weight_ih_l0.grad, want["ref"]["w_ih"], want["y32"]["w_ih"], figures)
        _grad_hold("w_hh", lstm.weight_hh_l0.grad, want["ref"]["w_hh"], want["y32"]["w_hh"], figures)
        _grad_hold("b_ih", lstm.bias_ih_l0.grad, want["ref"]["b"], want["y32"]["b"], figures)
        _grad_hold("b_hh", lstm.bias_hh_l0.grad, want["ref"]["b"], want["y32"]["b"], figures)
    finally:
        print(f"[autograd {case} b={b} l={l} d={d}]", "; ".join(figures))


@pytest.mark.parametrize("case,b,l,d", _h0_cases())
def test_fused_lstm_heads_node_holds_for_any_h0(case, b, l, d):
    """(c) ``fused_lstm.lstm_heads_forward``: LSTM + heads as one node, the heads' data gradient formed inside the
    backward through time."""
    k, figures = _case(case, b, l, d), []
    t = k["t"]
    heads, stacked = _head_modules(), _stacked_heads()
    for head in heads:
        head.zero_grad()
    lstm = _module(t, torch.float32)
    res = fused_lstm.lstm_heads_forward(lstm, heads, t["x"], t["h0"], t["c0"])
    assert res is not None
    outs, hs, hn, cn = res
    out = torch.cat(outs, 1)
    if k["bad"]:  # (gradients are NaN in torch too: the node's forward on the other rows)
        try:
            _check_forward(k, dict(hs=hs.detach(), cn=cn), figures, gates=False)
            assert bool(torch.isfinite(out.detach().view(b, -1)[k["good"]]).all())
        finally:
            print(f"[heads {case} b={b} l={l} d={d}]", "; ".join(figures))
        return
    want = _autograd_reference(case, b, l, d, True)
    (out * want["dout"]).sum().backward()
    try:
        _check_forward(k, dict(hs=hs.detach(), cn=cn), figures, gates=False)
        floor = 2e-6 * (1 + stacked[0].abs().sum(1).max().double())
        rows = lambda v: v.view(t["x"].shape[0], -1)  # noqa: E731
        _hold("out", rows(out.detach()), rows(want["ref_out"]), rows(want["y32_out"]), floor, k["good"], figures)
        _grad_hold("w_hh", lstm.weight_hh_l0.grad, want["ref"]["w_hh"], want["y32"]["w_hh"], figures)
        _grad_hold("w_ih", lstm.weight_ih_l0.grad, want["ref"]["w_ih"], want["y32"]["w_ih"], figures)
        _grad_hold("b_ih", lstm.bias_ih_l0.grad, want["ref"]["b"], want["y32"]["b"], figures)
        _grad_hold("b_hh", lstm.bias_hh_l0.grad, want["ref"]["b"], want["y32"]["b"], figures)
        _grad_hold("w_heads", torch.cat([h.weight.grad for h in heads]), want["ref"]["w_heads"], want["y32"]["w_heads"], figures)
        _grad_hold("b_heads", torch.cat([h.bias.grad for h in heads]), want["ref"]["b_heads"], want["y32"]["b_heads"], figures)
    finally:
        print(f"[heads {case} b={b} l={l} d={d}]", "; ".join(figures))


@pytest.mark.parametrize("b,l,d", [(b, l, d) for b in BS for l in LS for d in DS])
@pytest.mark.parametrize("case", WEIGHT_CASES)
def test_plane_forward_holds_over_weights_c0_and_x(case, b, l, d):
    """Group 2: ordinary ``h0``; outlier and spread weights, no recurrent weights, everything tiny, cell states of
    1e4 and 1e-30, observations of 1e5.  (The recurrent product itself, row by row:
    test_recurrent_product_per_gate_row_holds_under_outliers_and_decades.)"""
    k, figures = _case(case, b, l, d), []
    got = _split_forward(k, True)
    try:
        _check_forward(k, got, figures)
    finally:
        print(f"[weights {case} b={b} l={l} d={d}]", "; ".join(figures))
    lean = _split_forward(k, False)
    assert torch.equal(lean["hs"], got["hs"]) and torch.equal(lean["cn"], got["cn"])


PRODUCT_CASES = ("outliers",) + tuple(f"decade{k:+d}" for k in range(-3, 3))
PRE_USABLE = 1.0                      # |pre-activation| below which a gate is inverted
INVERSE_SLOPE = 0.19661193324148185   # sigma'(1), the smallest slope of a gate on (-1, 1) (tanh'(1) = 0.42)


@functools.lru_cache(maxsize=None)
def _product_case(case: str, b: int, d: int):
    g = torch.Generator().manual_seed(zlib.crc32(f"product {case} {b} {d}".encode()))
    x, c0, h0 = torch.randn(b, 1, d, generator=g) * 2, torch.randn(b, H, generator=g), _u(g, b, H) * 0.5
    w_hh = _u(g, 4 * H, H) / 16
    decade = torch.zeros(4 * H, dtype=torch.long)
    if case == "outliers":
        w_hh.view(-1)[torch.randperm(4 * H * H, generator=g)[:20]] *= 1000.0
    else:
        k0 = int(case[len("decade"):])
        decade = torch.arange(4 * H) % 6 - 3 - k0
        w_hh *= (10.0 ** decade.double()).float()[:, None]
    zeros = torch.zeros(4 * H)
    t = dict(x=x, h0=h0, c0=c0, w_ih=torch.zeros(4 * H, d), w_hh=w_hh, b_ih=zeros, b_hh=zeros.clone())
    t = {k: v.to(DEV).contiguous() for k, v in t.items()}
    return t, _recurrence(t, torch.float64), _recurrence(t, torch.float32), (decade == 0).to(DEV), (decade <= 0).to(DEV)


def _pre_of(gates):
    """Step-0 pre-activations from saved post-activation gates [B, L, 4, 256], in float64."""
    i, f, gg, o = gates[:, 0].double().unbind(1)
    return torch.cat([torch.logit(i), torch.logit(f), torch.atanh(gg), torch.logit(o)], 1)


def _f16_high_planes_only(t):
    """What the recurrent product would be with the low planes dropped (the kernel's scaling, fp16 rounding): the
    wrong answer this test has to be able to see."""
    w, h = t["w_hh"].double(), t["h0"].double()
    sw = 2.0 ** (14 - math.frexp(float(w.abs().max()))[1])
    return ((h * 2.0 ** 14).half().double() / 2.0 ** 14) @ ((w * sw).half().double() / sw).T


@pytest.mark.parametrize("b,d", [(b, d) for b in BS for d in DS])
@pytest.mark.parametrize("case", PRODUCT_CASES)
def test_recurrent_product_per_gate_row_holds_under_outliers_and_decades(case, b, d):
    """The recurrent product alone (``w_ih`` and the biases are zero), gate row by gate row against the row's
    ``sum |h| |w|``, as test_lstm_weight_gradient_planes_hold_over_the_dynamic_range measures the weight gradient.
    ``outliers``: twenty entries of ``W_hh`` at 1000 times the rest.  ``decade-3 .. decade+2``: the six_decades matrix
    (rows scaled by 10^k, k = -3 .. 2) times the power of ten that puts decade k's rows at pre-activations of ~0.17:
    the rows above saturate, and each decade in its turn is observable through its gates while W_hh's one power of
    two is set by rows up to 10^5 larger.  Held: the rows of that decade and of the decades below it; a row of a
    decade above shows at most a stray entry or two with |pre| < 1 among pre-activations of 10 to 10^4 times that,
    and a maximum over one entry against a maximum over one entry is no comparison -- it has its own case.  (In six_decades as group 2 runs it the small rows' whole product is 1e-5 of
    a pre-activation, which no fp32 gate resolves.)  The step-0 pre-activation is recovered from the saved gate (logit
    / atanh in float64) where |pre| < 1; the yardstick is torch's float32 gate through the same inverse; the floor is
    the saved gates' 2e-6 through the inverse's largest slope, 2e-6 / sigma'(1) = 1.02e-5 of a pre-activation --
    5e-6 of ``sum |h| |w|`` ~ 2 on the rows under test.  A product without its low planes is 1e-4 of a
    pre-activation off on those rows, and the test asserts that it would not pass."""
    t, ref, y32, rows, held = _product_case(case, b, d)
    packed, wb = hip.lstm_pack_split(t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"])
    got = hip.lstm_forward_split(t["x"], t["h0"], t["c0"], packed, wb, save=True)[3]
    mfma = hip.lstm_forward(t["x"], t["h0"], t["c0"], hip.lstm_pack(t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"]), save=True)[3]
    pre64 = ref["pre0"]
    usable = pre64.abs() < PRE_USABLE
    assert float(usable[:, rows].double().mean()) > 0.9   # the rows under test are observable
    zero, inf = torch.zeros_like(pre64), torch.full_like(pre64, math.inf)
    size = torch.where(usable, t["h0"].double().abs() @ t["w_hh"].double().abs().T, inf).amin(0)   # per gate row
    worst = lambda pre: torch.where(usable, (pre - pre64).abs(), zero).amax(0)  # noqa: E731
    err, yard, err_mfma, err_high = worst(_pre_of(got)), worst(_pre_of(y32["gates"])), worst(_pre_of(mfma)), worst(_f16_high_planes_only(t))
    seen = usable.any(0) & held
    floor = 2e-6 / INVERSE_SLOPE
    rel = lambda e: float((e / size)[seen & rows].max())  # noqa: E731
    print(f"[product {case} b={b} d={d}] rows under test, err / sum|h||w|: planes {rel(err):.2e}, torch32 {rel(yard):.2e},"
          f" fp32-MFMA {rel(err_mfma):.2e}, bar {rel(3 * yard + floor):.2e}; without the low planes {rel(err_high):.2e};"
          f" planes / torch32 = {float(err[seen].max()) / float(yard[seen].max()):.2f}")
    assert bool(((err / size)[seen] <= (3 * yard / size + floor / size)[seen]).all()), rel(err)
    # the measure is sensitive: the product without its low planes misses the same bar on the rows under test
    assert bool(((err_high / size) > (3 * yard / size + floor / size))[seen & rows].any())


# ---- group 3: the heads form of the backward through time at its limit -------------------------------------------


def _bptt_fp64(c0, gates, cs, dhs, w_hh):
    """The recurrences of the backward through time in float64 (as in tests/test_lstm_gpu.py)."""
    b, l = dhs.shape[:2]
    c0, gates, cs, dhs, w = (v.double() for v in (c0, gates, cs, dhs, w_hh))
    dg = torch.zeros(b, l, 4, H, dtype=torch.float64, device=DEV)
    dh_carry = torch.zeros(b, H, dtype=torch.float64, device=DEV)
    dc_carry = torch.zeros_like(dh_carry)
    for t in range(l - 1, -1, -1):
        i, f, g, o = gates[:, t].unbind(1)
        c_prev = cs[:, t - 1] if t > 0 else c0
        dh = dhs[:, t] + dh_carry
        tc = torch.tanh(cs[:, t])
        dg[:, t, 3] = dh * tc * o * (1 - o)
        dc = dh * o * (1 - tc * tc) + dc_carry
        dg[:, t, 0] = dc * g * i * (1 - i)
        dg[:, t, 2] = dc * i * (1 - g * g)
        dg[:, t, 1] = dc * c_prev * f * (1 - f)
        dc_carry = dc * f
        dh_carry = dg[:, t].reshape(b, 4 * H) @ w
    return dg


def _heads_backward_inputs(b, l, n, magnitude, beyond=None):
    """Free inputs: f in (0.2, 0.8); half of the cell states of size ``magnitude``, the rest below 1.5 (a saturated tanh
    passes no dL/dc: the small ones let it through, the forget gate carries it to the large ones).  ``beyond``: the size
    of the large cell states in a few sequences (first and last of the first wave, the last of all)."""
    g = torch.Generator().manual_seed(1000 * b + 10 * l + n + int(magnitude))
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    gates = r(b, l, 4, H)
    gates[:, :, 2] = gates[:, :, 2] * 2 - 1
    gates[:, :, 1] = 0.2 + 0.6 * gates[:, :, 1]
    small, sign, large = (r(b, l + 1, H) * 2 - 1) * 1.5, torch.sign(r(b, l + 1, H) - 0.5), r(b, l + 1, H) < 0.5
    size = torch.full((b, 1, 1), float(magnitude))
    hit = sorted({0, min(31, b - 1), b - 1}) if beyond else []
    if beyond:
        size[hit] = float(beyond)
    c = torch.where(large, sign * size * (0.5 + 0.5 * r(b, l + 1, H)), small)
    dout = (r(b * l, n) * 2 - 1) * torch.exp(-12 * r(b, 1)).repeat_interleave(l, 0) * 1e-3
    w, w_hh = (r(n, H) * 2 - 1) / 16, (r(4 * H, H) * 2 - 1) / 16
    dev = lambda v: v.to(DEV).contiguous()  # noqa: E731
    return dev(c[:, 0]), dev(gates), dev(c[:, 1:]), dev(dout), dev(w), dev(w_hh), hit


def _both_plane_schemes(c0, gates, cs, dout, w, packed, monkeypatch):
    monkeypatch.delenv("RL8_AMD_LSTM_BACKWARD_PLANES", raising=False)
    f16, bound = hip.lstm_rows_backward(c0, gates, cs, None, packed, with_bound=True, heads=(dout, w))
    monkeypatch.setenv("RL8_AMD_LSTM_BACKWARD_PLANES", "bf16")
    bf16 = hip.lstm_rows_backward(c0, gates, cs, None, packed, heads=(dout, w))
    monkeypatch.delenv("RL8_AMD_LSTM_BACKWARD_PLANES")
    return f16, bound, bf16


HEADS_SHAPES = [(b, l, n) for b in BS for l in LS for n in NS]


@pytest.mark.parametrize("b,l,n", HEADS_SHAPES)
@pytest.mark.parametrize("magnitude", [1000, 4000])
def test_heads_backward_inside_its_limit(b, l, n, magnitude, monkeypatch):
    """|c| up to 1000 and 4000 (the limit is 4094) with an open forget gate: per sequence, relative to the sequence's
    largest gate gradient, err16 <= 3 err_bf + 2e-7; everything finite; the bound is max |dG|."""
    c0, gates, cs, dout, w, w_hh, _ = _heads_backward_inputs(b, l, n, magnitude)
    f16, bound, bf16 = _both_plane_schemes(c0, gates, cs, dout, w, hip.lstm_rows_backward_pack(w_hh), monkeypatch)
    want = _bptt_fp64(c0, gates, cs, (dout.double() @ w.double()).view(b, l, H), w_hh)
    scale = want.abs().amax(dim=(1, 2, 3)).clamp_min(1e-300)
    err16, err_bf = (f16.double() - want).abs().amax(dim=(1, 2, 3)) / scale, (bf16.double() - want).abs().amax(dim=(1, 2, 3)) / scale
    print(f"[heads backward |c|<={magnitude} b={b} l={l} n={n}] err16 {float(err16.max()):.2e} err_bf {float(err_bf.max()):.2e}"
          f" worst err16 / (3 err_bf + 2e-7) = {float((err16 / (3 * err_bf + 2e-7)).max()):.2f}")
    assert bool(torch.isfinite(f16).all()) and bool(torch.isfinite(bf16).all()) and bool(torch.isfinite(bound).all())
    assert bool((err16 <= 3 * err_bf + 2e-7).all()), (float(err16.max()), float(err_bf.max()))
    assert float(bound) == float(f16.abs().max())
    # the forget gate's gradient does carry the magnitude
    assert float(want[:, :, 1].abs().max()) > 10 * float(want[:, :, (0, 2, 3)].abs().max())


@pytest.mark.parametrize("b,l,n", HEADS_SHAPES)
@pytest.mark.parametrize("beyond", [5000.0, 1e5])
def test_heads_backward_past_its_limit_fails_loudly(b, l, n, beyond, monkeypatch):
    """|c| of 5000 and 1e5 in a few sequences: the others meet the bar; an affected sequence is at the bar or not
    finite, never finite and wrong; a non-finite dG makes the bound non-finite, and ``hip.lstm_backward`` then returns
    non-finite ``w_hh`` gradients."""
    c0, gates, cs, dout, w, w_hh, hit = _heads_backward_inputs(b, l, n, 1000, beyond=beyond)
    packed = hip.lstm_rows_backward_pack(w_hh)
    f16, bound, bf16 = _both_plane_schemes(c0, gates, cs, dout, w, packed, monkeypatch)
    want = _bptt_fp64(c0, gates, cs, (dout.double() @ w.double()).view(b, l, H), w_hh)
    scale = want.abs().amax(dim=(1, 2, 3), keepdim=True).clamp_min(1e-300)
    err_bf = ((bf16.double() - want).abs() / scale).amax(dim=(1, 2, 3), keepdim=True)
    err16 = (f16.double() - want).abs() / scale
    finite = torch.isfinite(f16)
    lost = sorted(set(torch.nonzero(~finite.all(dim=3).all(dim=2).all(dim=1)).flatten().tolist()))
    print(f"[heads backward past the limit |c|={beyond:g} b={b} l={l} n={n}] sequences not finite: {lost} of {hit};"
          f" bound {float(bound)}")
    assert set(lost) <= set(hit), (lost, hit)
    if beyond == 1e5 and l == 3:   # 25 times the limit with carried gradients: every such sequence overflows a plane
        assert lost == hit, (lost, hit)
    assert bool(torch.isfinite(bf16).all())
    assert bool(((err16 <= 3 * err_bf + 2e-7) | ~finite).all())   # finite means right
    if lost:
        assert not math.isfinite(float(bound))
    else:
        assert float(bound) == float(f16.abs().max())
    g = torch.Generator().manual_seed(b + l)
    x, h0 = torch.randn(b, l, 1, generator=g).to(DEV), (_u(g, b, H) * 0.5).to(DEV)
    hs = _u(g, b, l, H).to(DEV)
    grads = hip.lstm_backward(x, h0, c0, hs, gates, cs, None, None, rows_packed=packed, heads=(dout, w), hs_bound=1.0)
    if lost:
        assert not bool(torch.isfinite(grads["w_hh"]).all())
    else:
        assert bool(torch.isfinite(grads["w_hh"]).all())
