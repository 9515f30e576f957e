"""The input gradient of layer 0 of the narrow LSTMs (``rl8_lstm_narrow_input_grad_f32``: dx = dz x W_ih at hidden
width 64 / 128) against fp64 at the kernel's edges, and through the three autograd nodes that return it
(``fused_lstm.lstm_forward``, ``lstm_heads_forward``, ``lstm_stack_forward``)."""

from __future__ import annotations

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402
from rl8_amd.nn import fused_lstm  # noqa: E402

DEV = "cuda"
CUS, ROWS_PER_TILE = 256, 32  # kCUs (common.hip.h), kStackRows (lstm_narrow_kernels.hip)
WG_PER_CU = {64: 2, 128: 1}  # Geo<H>::kWgPerCU
SHAPES = [(1, 1), (1, 3), (33, 1), (5, 7)]  # one row; partial 32-row tiles; rows past n in the second tile
D_INS = [1, 4, 5, 16]  # both KIN templates (4 / 16) at both ends


def _case(hidden: int, b: int, l: int, d_in: int, seed: int):
    """Random inputs through the public path up to the saved forward: everything the backward takes."""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def randn(*shape, scale=1.0):
        return torch.randn(*shape, device=DEV, generator=g) * scale

    x, h0, c0 = randn(b, l, d_in), randn(b, hidden, scale=0.5), randn(b, hidden, scale=0.5)
    w_ih, w_hh = randn(4 * hidden, d_in, scale=0.3), randn(4 * hidden, hidden, scale=0.1)
    b_ih, b_hh = randn(4 * hidden, scale=0.1), randn(4 * hidden, scale=0.1)
    hs, _, _, gates, cs = hip.lstm_narrow_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh, save=True)
    return dict(x=x, h0=h0, c0=c0, w_ih=w_ih, w_hh=w_hh, hs=hs, gates=gates, cs=cs, dhs=randn(b, l, hidden))


def _backward(c, **kw):
    dhs = None if "heads" in kw else kw.pop("dhs", c["dhs"])
    return hip.lstm_narrow_backward(c["x"], c["h0"], c["c0"], c["w_hh"], c["hs"], c["gates"], c["cs"], dhs, **kw)


def _assert_within_fp32_bound(g, w_ih: torch.Tensor, label) -> None:
    """dx against dz64 @ w_ih64 with dz read back from the workspace: |error| <= 4H 2^-23 (|dz| @ |w_ih|) + 1e-30
    elementwise, the bound of a K = 4H fp32 accumulation in any order (K u sum |terms|, u = 2^-24, with a factor two
    of slack for the products' own roundings)."""
    k = w_ih.shape[0]
    dz = g["dz"].reshape(-1, k).double()
    want = dz @ w_ih.double()
    bound = k * 2.0 ** -23 * (dz.abs() @ w_ih.double().abs()) + 1e-30
    err = (g["dx"].reshape(-1, w_ih.shape[1]).double() - want).abs()
    worst = float((err / bound).max())
    print(f"input grad {label}: max |error| {float(err.max()):.3e}, max error / bound {worst:.3e}")
    assert torch.isfinite(g["dx"]).all() and worst <= 1.0, (label, worst)
    assert float(want.abs().max()) > 0.0, label  # (the comparison is not of zeros)


@pytest.mark.parametrize("d_in", D_INS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"b{s[0]}l{s[1]}")
@pytest.mark.parametrize("hidden", [64, 128])
def test_kernel_matches_fp64_at_the_edges(hidden, shape, d_in):
    b, l = shape
    c = _case(hidden, b, l, d_in, seed=1000 * hidden + 100 * b + 10 * l + d_in)
    g = _backward(c, w_ih=c["w_ih"])
    assert g["dx"].shape == (b, l, d_in) and g["dz"].shape == (b, l, 4, hidden)
    _assert_within_fp32_bound(g, c["w_ih"], (hidden, b, l, d_in))


@pytest.mark.parametrize("d_in", [4, 5])
@pytest.mark.parametrize("hidden", [64, 128])
def test_grid_stride_loop_runs_a_second_pass(hidden, d_in):
    """One tile more than the grid's cap (kCUs * kWgPerCU workgroups of 32 row-steps), the last one partial: some
    workgroup takes two tiles, the second from its prefetched registers. dz is 16.8 MB at either width."""
    cap_rows = CUS * WG_PER_CU[hidden] * ROWS_PER_TILE
    b = cap_rows + 5
    assert b * 4 * hidden * 4 < 100e6
    c = _case(hidden, b, 1, d_in, seed=7 + hidden + d_in)
    g = _backward(c, w_ih=c["w_ih"])
    _assert_within_fp32_bound(g, c["w_ih"], (hidden, b, 1, d_in))
    # the last rows again in a launch of three workgroups: the result does not depend on the grid
    n = 77
    tail = g["dz"][-n:]  # (a row is 4H floats: the slice starts 16-byte aligned)
    dx = torch.empty(n, 1, d_in, device=DEV)
    status = hip.load().rl8_lstm_narrow_input_grad_f32(tail.data_ptr(), n, 1, d_in, c["w_ih"].data_ptr(), hidden,
                                                       dx.data_ptr(), hip._stream())
    assert status == 0
    assert torch.equal(dx.view(torch.int32), g["dx"][-n:].view(torch.int32))


@pytest.mark.parametrize("d_in", D_INS)
@pytest.mark.parametrize("hidden", [64, 128])
def test_exactly_b_l_d_in_floats_are_written_and_two_calls_agree(hidden, d_in):
    b, l = 33, 3
    c = _case(hidden, b, l, d_in, seed=31 * hidden + d_in)
    g = _backward(c, w_ih=c["w_ih"])
    nbytes, off = b * l * d_in * 4, 16
    raw = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    dx = raw[off:off + nbytes].view(torch.float32).view(b, l, d_in)
    # the entry itself, on the gate gradients the backward left at the front of its workspace
    status = hip.load().rl8_lstm_narrow_input_grad_f32(g["dz"].data_ptr(), b, l, d_in, c["w_ih"].data_ptr(), hidden,
                                                       dx.data_ptr(), hip._stream())
    assert status == 0
    torch.cuda.synchronize()
    assert bool((raw[:off] == 0xA5).all()) and bool((raw[off + nbytes:] == 0xA5).all())
    assert torch.equal(dx.view(torch.int32), g["dx"].view(torch.int32))
    again = _backward(c, w_ih=c["w_ih"])
    assert torch.equal(again["dx"].view(torch.int32), g["dx"].view(torch.int32))
    for k in ("w_ih", "w_hh", "b"):
        assert torch.equal(again[k], g[k]), k


@pytest.mark.parametrize("n_heads", [1, 4])
@pytest.mark.parametrize("hidden", [64, 128])
def test_heads_form_leaves_the_same_gate_gradients(hidden, n_heads):
    """dx of the ``heads=`` form is bit-equal to dx of the ``dhs=`` form fed dout @ w. One head output: torch's
    product (one multiplication per element, nothing to reorder). Four: the product as
    ``linear_heads_narrow_backward`` forms it, which include/rl8_amd.h documents as the same bits as the backward
    through time's own (a torch matmul may add the four terms in another order)."""
    b, l, d_in = 33, 4, 4
    c = _case(hidden, b, l, d_in, seed=5 * hidden + n_heads)
    gen = torch.Generator(device=DEV).manual_seed(99)
    dout = torch.randn(b * l, n_heads, device=DEV, generator=gen)
    w = torch.randn(n_heads, hidden, device=DEV, generator=gen) * 0.2
    if n_heads == 1:
        dhs = (dout @ w).view(b, l, hidden)
    else:
        dhs = hip.linear_heads_narrow_backward(c["hs"].view(-1, hidden), dout, w)[0].view(b, l, hidden)
    via_heads = _backward(c, heads=(dout, w), w_ih=c["w_ih"])
    via_dhs = _backward(c, dhs=dhs.contiguous(), w_ih=c["w_ih"])
    assert torch.equal(via_heads["dx"].view(torch.int32), via_dhs["dx"].view(torch.int32))
    assert float(via_heads["dx"].abs().max()) > 0.0


def test_without_w_ih_nothing_is_added():
    c = _case(64, 5, 3, 4, seed=3)
    assert set(_backward(c)) == {"w_ih", "w_hh", "b"}
    with pytest.raises(ValueError, match="w_ih"):
        _backward(c, w_ih=c["w_ih"][:, :3].contiguous())


# --------------------------------------------------------------------------- #
# Autograd.
# --------------------------------------------------------------------------- #
B, L, D_IN = 33, 4, 4


def _module_input_grad(lstm: nn.LSTM, heads, x, h0, c0, weights, dtype, device):
    """dL/dx of L = sum_i sum(head_i(lstm(x)) * weights_i) through torch's own module in ``dtype`` on ``device``
    (h0 / c0 [layers, B, H])."""
    twin = nn.LSTM(lstm.input_size, lstm.hidden_size, num_layers=lstm.num_layers, batch_first=True)
    twin.load_state_dict(lstm.state_dict())
    twin = twin.to(device=device, dtype=dtype)
    xx = x.detach().to(device=device, dtype=dtype).requires_grad_()
    with torch.backends.cudnn.flags(enabled=False):
        hs, _ = twin(xx, (h0.to(device=device, dtype=dtype), c0.to(device=device, dtype=dtype)))
    loss = hs.new_zeros(())
    flat = hs.reshape(-1, hs.shape[2])
    for head, wgt in zip(heads, weights):
        out = flat if head is None else flat @ head.weight.detach().to(flat).T + head.bias.detach().to(flat)
        loss = loss + (out * wgt.to(out)).sum()
    loss.backward()
    return xx.grad.double().cpu()


def _fused_pass(form: str, lstm, heads, x, h0, c0, weights, want_dx: bool):
    """One training pass through the fused node of ``form``; (x.grad or None, the parameter gradients)."""
    for p in (*lstm.parameters(), *(q for h in heads if h is not None for q in h.parameters())):
        p.grad = None
    xx = x.detach().clone().requires_grad_(want_dx)
    if form == "lstm":
        hs, _, _ = fused_lstm.lstm_forward(lstm, xx, h0[0], c0[0])
        outs = [hs.reshape(-1, hs.shape[2])]
    elif form == "heads":
        outs, _, _, _ = fused_lstm.lstm_heads_forward(lstm, list(heads), xx, h0[0], c0[0])
    else:
        hs, _, _ = fused_lstm.lstm_stack_forward(lstm, xx, h0.transpose(0, 1), c0.transpose(0, 1))
        outs = [hs.reshape(-1, hs.shape[2])]
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    grads = {k: p.grad.clone() for k, p in lstm.named_parameters()}
    return xx.grad, grads


@pytest.mark.parametrize("form", ["lstm", "heads", "stack"])
@pytest.mark.parametrize("hidden", [64, 128])
def test_autograd_returns_the_input_gradient(hidden, form):
    """x.grad of the three fused nodes against an fp64 ``nn.LSTM`` (CPU) on the same weights, B = 33, L = 4,
    d_in = 4. Allowed: three times the max-abs error of torch's own fp32 ``nn.LSTM`` input gradient (on the device,
    the cell torch itself fuses) against that fp64 result, plus 1e-7 -- the yardstick is torch's module, measured in
    this very run and printed. Measured on an MI355X (max |dx| 0.01 .. 0.1): torch fp32 2.8e-9 .. 2.5e-8, the fused
    nodes 2.7e-9 .. 2.7e-8, i.e. 0.9 .. 1.4 times torch's at every width and form. The parameter gradients of the same pass are bit-equal to those
    of a pass whose x requires no gradient."""
    torch.manual_seed(hidden + len(form))
    layers = 2 if form == "stack" else 1
    lstm = nn.LSTM(D_IN, hidden, num_layers=layers, batch_first=True).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(B, L, D_IN, device=DEV, generator=gen)
    h0 = torch.randn(layers, B, hidden, device=DEV, generator=gen) * 0.5
    c0 = torch.randn(layers, B, hidden, device=DEV, generator=gen) * 0.5
    if form == "heads":
        heads = [nn.Linear(hidden, 3).to(DEV), nn.Linear(hidden, 1).to(DEV)]
        weights = [torch.randn(B * L, 3, device=DEV, generator=gen), torch.randn(B * L, 1, device=DEV, generator=gen)]
    else:
        heads, weights = [None], [torch.randn(B * L, hidden, device=DEV, generator=gen) * 0.1]
    assert fused_lstm._family(lstm) == ("stack" if form == "stack" else "narrow")

    want = _module_input_grad(lstm, heads, x, h0, c0, weights, torch.float64, "cpu")
    torch32 = _module_input_grad(lstm, heads, x, h0, c0, weights, torch.float32, DEV)
    yardstick = float((torch32 - want).abs().max())
    dx, grads = _fused_pass(form, lstm, heads, x, h0, c0, weights, want_dx=True)
    assert dx is not None and dx.shape == x.shape
    err = float((dx.double().cpu() - want).abs().max())
    print(f"input gradient H={hidden} {form}: max |dx| {float(want.abs().max()):.3e}, torch fp32 error "
          f"{yardstick:.3e}, fused error {err:.3e}, allowed {3 * yardstick + 1e-7:.3e}")
    assert err <= 3 * yardstick + 1e-7, (err, yardstick)

    none, plain = _fused_pass(form, lstm, heads, x, h0, c0, weights, want_dx=False)
    assert none is None
    for k, g in grads.items():
        assert torch.equal(g.view(torch.int32), plain[k].view(torch.int32)), k


@pytest.mark.parametrize("form", ["lstm", "heads"])
def test_launches_without_an_input_gradient_are_those_of_before(form):
    """A training pass whose x requires no gradient launches exactly what it launched before there was an input
    gradient; one whose x requires it adds the one launch."""
    hidden = 64
    torch.manual_seed(0)
    lstm = nn.LSTM(D_IN, hidden, batch_first=True).to(DEV)
    heads = [nn.Linear(hidden, 3).to(DEV), nn.Linear(hidden, 1).to(DEV)] if form == "heads" else [None]
    x = torch.randn(B, L, D_IN, device=DEV)
    h0, c0 = torch.zeros(1, B, hidden, device=DEV), torch.zeros(1, B, hidden, device=DEV)
    weights = [torch.randn(B * L, 3, device=DEV), torch.randn(B * L, 1, device=DEV)] if form == "heads" else \
        [torch.randn(B * L, hidden, device=DEV)]

    def names(want_dx: bool) -> set[str]:
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            _fused_pass(form, lstm, heads, x, h0, c0, weights, want_dx)
            return set(hip.timer.summary())
        finally:
            hip.timer.enabled = False
            hip.timer.reset()

    lstm_names = {"lstm_narrow_forward", "lstm_narrow_backward", "lstm_narrow_reduce"}
    before = names(False)
    assert {n for n in before if n.startswith("lstm_")} == lstm_names, before
    assert names(True) == before | {"lstm_narrow_input_grad"}
