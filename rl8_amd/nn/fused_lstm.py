"""The default recurrent models' LSTM as fused gfx950 kernels.

``torch.nn.LSTM(d_in, 256, num_layers=1, batch_first=True)`` -- what
``DefaultContinuousRecurrentModel`` / ``DefaultDiscreteRecurrentModel`` are built
around (``src/rl8/models/_recurrent.py:201-321`` of the reference) -- runs as one
forward kernel (time loop inside, gates never leave the chip) and, for training,
one backward-through-time kernel plus the weight-gradient kernels, instead of two
GEMMs and a pointwise kernel per timestep. ``nn.LSTM(d_in, 64 | 128)`` with
d_in <= 16 -- the reference's example model is ``nn.LSTM(4, 64)`` -- runs the
narrow kernels (lstm_narrow_kernels.hip: fp32 MFMA forward with the time loop
inside, backward through time, deterministic weight gradient) under the same
rules. Parameters stay the module's own; ``lstm_forward`` returns ``None`` for
any other LSTM (more layers, other widths, projections, bidirectional, non-HIP /
non-fp32 inputs) and the caller runs the module itself. Two or more layers of
width 64 / 128 without dropout have their own entry, ``lstm_stack_forward``:
layer 0 on the narrow kernels, the layers above on the lstm_narrow_stack_*
kernels (input projection over all row-steps, recurrent forward from it, input
gradient for the layer below). The ``Linear(64 | 128, n)`` heads on any of these
run lstm_narrow_heads_kernels.hip, and a training pass through one narrow layer
and heads of at most four outputs is one node (``_NarrowLSTMHeads``), as at 256.

"""

from __future__ import annotations

import dataclasses
import functools
import os

import torch
import torch.nn as nn

from .. import hip

#: Set to False to evaluate LSTMs with PyTorch (A/B comparisons).
ENABLED = True
# ``_plan`` reads these three and RL8_AMD_LSTM_WGRAD_PLANES / _GATES on every call (tests change them at run time).
#: "split": the forward step on the bf16 matrix pipe (fp32-accurate bf16-plane products,
#: lstm_split_kernels.hip) where the input width has a compiled variant; "f32": the
#: fp32-MFMA kernel with the time loop inside (lstm_kernels.hip).
FORWARD_GEMM = os.environ.get("RL8_AMD_LSTM_GEMM", "split")
#: The backward through time on bf16 planes, a wave per 32 sequences (lstm_rows_kernels.hip); 0: the fp32-MFMA kernel.
BACKWARD_ROWS = os.environ.get("RL8_AMD_LSTM_BACKWARD_ROWS", "1") != "0"
#: Training passes through LSTM + heads as one autograd node whose backward forms the heads' data gradient inside the
#: backward-through-time kernel (lstm_heads_forward); 0: two nodes, dL/dh through HBM.
FUSE_HEADS = os.environ.get("RL8_AMD_LSTM_FUSE_HEADS", "1") != "0"


def _rollout_fuse_heads() -> bool:
    """The lean rollout's two-way categorical + value head inside its last kernel (0: two launches); read per rollout."""
    return os.environ.get("RL8_AMD_ROLLOUT_FUSE_HEADS", "1") != "0"


def _eligible(lstm: nn.LSTM, x: torch.Tensor) -> bool:
    return (
        ENABLED
        and x.is_cuda
        and x.dtype == torch.float32
        and x.ndim == 3
        and lstm.num_layers == 1
        and lstm.hidden_size == hip.LSTM_HIDDEN
        and lstm.batch_first
        and lstm.bias
        and not lstm.bidirectional
        and lstm.proj_size == 0
        and x.shape[2] == lstm.input_size
        and hip.lstm_supports(lstm.input_size)
    )


@functools.lru_cache(maxsize=None)
def _narrow_supported(hidden: int, d_in: int) -> bool:
    """The narrow kernels are compiled for this (hidden, d_in): fixed by the build, asked once per pair."""
    return hip.lstm_narrow_supports(hidden, d_in)


def _narrow_eligible(lstm: nn.LSTM, x: torch.Tensor) -> bool:
    """``_eligible`` at hidden width 64 or 128 and d_in <= 16 (lstm_narrow_kernels.hip)."""
    return (
        ENABLED
        and x.is_cuda
        and x.dtype == torch.float32
        and x.ndim == 3
        and lstm.num_layers == 1
        and lstm.hidden_size in hip.LSTM_NARROW_HIDDEN
        and lstm.batch_first
        and lstm.bias
        and not lstm.bidirectional
        and lstm.proj_size == 0
        and x.shape[2] == lstm.input_size
        and _narrow_supported(lstm.hidden_size, lstm.input_size)
    )


def _packs(lstm: nn.LSTM, kind: str):
    """Fragment-ordered copies of the weights for one kernel ("step" / "split": the fp32 / plane forward step,
    "transposed" / "rows": the fp32 / rows backward), cached ON the module and re-made when the optimizer has changed
    a parameter (version counters) or a parameter tensor has been replaced / moved."""
    params = (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
    stamp = tuple((p._version, p.data_ptr()) for p in params)
    cache = lstm.__dict__.setdefault("_rl8_lstm_packs", {})
    hit = cache.get(kind)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    pack = {"step": hip.lstm_pack, "split": hip.lstm_pack_split, "transposed": hip.lstm_pack_transposed,
            "rows": hip.lstm_rows_backward_pack}[kind]
    packed = pack(*params) if kind in ("step", "split") else pack(params[1])
    cache[kind] = (stamp, packed)
    return packed


@functools.lru_cache(maxsize=None)
def _planes_supported(d_in: int) -> bool:
    """The plane kernels are compiled for this input width: fixed by the build, asked once per width."""
    return hip.lstm_split_supports(d_in)


@dataclasses.dataclass(frozen=True)
class _LstmPlan:
    """The kernels one LSTM call runs, forward and backward: made once by ``_plan`` and saved on ``ctx`` so that the
    backward runs what its forward prepared for (its packs: "split" or "step", "rows" or "transposed")."""

    forward_planes: bool  # the step kernel on fp16 planes (training: max |h0| from its state split); else fp32 MFMA
    backward_rows: bool  # the backward through time on planes (rows kernel), which leaves a bound on |dG|; else fp32 MFMA
    wgrad: str  # the weight gradient's route (hip.lstm_backward): "f16-gates", "f16", "bf16" or "f32"
    fuse_heads: bool  # a training pass through LSTM + heads as one node (lstm_heads_forward)


def _plan(d_in: int, b: int) -> _LstmPlan:
    """The one place the LSTM routes are decided, for ``b`` sequences of ``d_in`` floats; reads the switches as they
    are now."""
    forward_planes = FORWARD_GEMM == "split" and _planes_supported(d_in)
    backward_rows = forward_planes and BACKWARD_ROWS
    four_gates = b >= hip.LSTM_WGRAD_GATES_MIN_ROWS and os.environ.get("RL8_AMD_LSTM_WGRAD_GATES", "fused") != "separate"
    wgrad = ("f32" if not forward_planes else
             "bf16" if not backward_rows or os.environ.get("RL8_AMD_LSTM_WGRAD_PLANES", "f16") == "bf16" else
             "f16-gates" if four_gates else "f16")
    return _LstmPlan(forward_planes, backward_rows, wgrad, FUSE_HEADS and backward_rows)


#: The fp16 planes of the last training pass's initial hidden states and max |h0|: the SGD iterations of one step() read
#: the same rows of the buffer (the sequence-major copy of a full-buffer minibatch), whose split is 0.5 GB in, 0.5 GB out.
_h0_cache: dict[str, tuple] = {}
#: Set by ``RecurrentAlgorithm.step()`` while it reads its sequence-major copy of the buffer; off, every pass splits its
#: own h0 (a version counter does not see writes made through raw pointers, e.g. the rollout's into the buffer).
SHARE_H0_PLANES = False


def _h0_planes(h0: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(planes, max |h0|) of ``h0``; with ``SHARE_H0_PLANES`` re-made only unless this very memory, unmodified since,
    was split last time (the entry keeps ``h0`` alive, so the address cannot have been handed to another tensor)."""
    key = (h0.data_ptr(), tuple(h0.shape), tuple(h0.stride()), h0._version, h0.device)
    hit = _h0_cache.get("entry") if SHARE_H0_PLANES else None
    if hit is not None and hit[0] == key:
        return hit[2], hit[3]
    _h0_cache.pop("entry", None)
    bound = torch.empty(1, dtype=torch.float32, device=h0.device)
    planes = hip.lstm_split_state(h0, bound_out=bound)
    if SHARE_H0_PLANES:
        _h0_cache["entry"] = (key, h0, planes, bound)
    return planes, bound


def clear_state_cache() -> None:
    """Drops the cached planes (and the reference to the rows they were made from) and stops sharing."""
    global SHARE_H0_PLANES
    SHARE_H0_PLANES = False
    _h0_cache.clear()


class _FusedLSTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, lstm, grad_mode, plan):  # type: ignore[override]
        need_grad = grad_mode and any(ctx.needs_input_grad[3:7])
        if plan.forward_planes:
            packed, wb = _packs(lstm, "split")
            # max |h0| for the backward's fp16-plane weight gradient comes out of the state split
            planes0, bound = _h0_planes(h0) if need_grad else (None, None)
            hs, _, cn, gates, cs = hip.lstm_forward_split(x, h0, c0, packed, wb, save=need_grad, h0_planes=planes0)
        else:
            bound = None
            hs, _, cn, gates, cs = hip.lstm_forward(x, h0, c0, _packs(lstm, "step"), save=need_grad)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.lstm, ctx.plan, ctx.h0_bound = lstm, plan, bound
            ctx.save_for_backward(x, h0, c0, hs, gates, cs)
        ctx.mark_non_differentiable(cn)
        # (c_n may be the last column of the saved cell states, strided: a training pass, which drops the final
        # states, must not pay for a dense copy of 2^19 rows -- 1.6 ms per iteration of the recurrent bench)
        return hs, cn

    @staticmethod
    def backward(ctx, dhs, dcn):  # type: ignore[override]
        x, h0, c0, hs, gates, cs = ctx.saved_tensors
        dhs = torch.zeros_like(hs) if dhs is None else dhs.contiguous().float()
        packed = _packs(ctx.lstm, "rows" if ctx.plan.backward_rows else "transposed")
        whht, rows = (None, packed) if ctx.plan.backward_rows else (packed, None)
        g = hip.lstm_backward(x, h0, c0, hs, gates, cs, dhs, whht, wgrad=ctx.plan.wgrad, rows_packed=rows,
                              h0_bound=ctx.h0_bound, hs_bound=1.0)  # (hs: this LSTM's own outputs, |o tanh c| < 1)
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], None, None, None


class _NarrowLSTM(torch.autograd.Function):
    """A hidden-64 / 128 LSTM: the weights are read in torch layout (nothing packed, nothing cached); a training
    pass saves the gates and cell states for the backward through time."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, grad_mode):  # type: ignore[override]
        need_grad = grad_mode and any(ctx.needs_input_grad[3:7])
        hs, _, cn, gates, cs = hip.lstm_narrow_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh, save=need_grad)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.save_for_backward(x, h0, c0, w_hh, hs, gates, cs)
        ctx.mark_non_differentiable(cn)
        return hs, cn

    @staticmethod
    def backward(ctx, dhs, dcn):  # type: ignore[override]
        x, h0, c0, w_hh, hs, gates, cs = ctx.saved_tensors
        dhs = torch.zeros_like(hs) if dhs is None else dhs.contiguous().float()
        g = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dhs)
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], None


class _NarrowLSTMHeads(torch.autograd.Function):
    """:class:`_NarrowLSTM` + output heads of a training pass as one node, as :class:`_FusedLSTMHeads` is at 256: the
    heads' data gradient dL/dh_t = dOut x W (n <= 4) is formed inside the backward through time from the 16 bytes
    per row-step it is made of, instead of being written as [B, L, H] by the heads' backward and read back."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, w_heads, b_heads):  # type: ignore[override]
        hs, _, cn, gates, cs = hip.lstm_narrow_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh, save=True)
        out = hip.linear_heads_narrow_forward(hs.view(-1, hs.shape[2]), w_heads, b_heads)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, h0, c0, w_hh, hs, gates, cs, w_heads)
        ctx.mark_non_differentiable(cn)
        return out, hs, cn

    @staticmethod
    def backward(ctx, dout, dhs, dcn):  # type: ignore[override]
        x, h0, c0, w_hh, hs, gates, cs, w_heads = ctx.saved_tensors
        flat = hs.view(-1, hs.shape[2])
        dout = (torch.zeros(flat.shape[0], w_heads.shape[0], dtype=torch.float32, device=flat.device) if dout is None
                else dout.contiguous().float())
        if dhs is None:  # nothing but the heads reads the latents: the usual case
            _, dw, db = hip.linear_heads_narrow_backward(flat, dout, w_heads, need_dh=False)
            g = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, None, heads=(dout, w_heads))
        else:
            dh, dw, db = hip.linear_heads_narrow_backward(flat, dout, w_heads)
            g = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dh.view_as(hs) + dhs.float())
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], dw, db


_STACK_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _stack_eligible(lstm: nn.LSTM, x: torch.Tensor) -> bool:
    """``_narrow_eligible`` with two or more layers and no dropout between them (lstm_narrow_stack_* kernels)."""
    return (
        ENABLED
        and x.is_cuda
        and x.dtype == torch.float32
        and x.ndim == 3
        and lstm.num_layers >= 2
        and lstm.dropout == 0
        and lstm.hidden_size in hip.LSTM_NARROW_HIDDEN
        and lstm.batch_first
        and lstm.bias
        and not lstm.bidirectional
        and lstm.proj_size == 0
        and x.shape[2] == lstm.input_size
        and _narrow_supported(lstm.hidden_size, lstm.input_size)
        and hip.lstm_stack_supports(lstm.hidden_size)
    )


class _StackLSTM(torch.autograd.Function):
    """A stack of hidden-64 / 128 layers as one node: layer 0 on the narrow kernels, every upper layer on the stack
    kernels, each reading the lower layer's ``hs`` where the kernel left it (no torch op between the layers). The
    weights are read in torch layout, nothing packed or cached. ``h0`` / ``c0`` and the returned states are
    [layers, B, H]; a training pass saves every layer's ``hs``, gates and cell states."""

    @staticmethod
    def forward(ctx, x, h0, c0, grad_mode, *weights):  # type: ignore[override]
        layers = len(weights) // 4
        need_grad = grad_mode and any(ctx.needs_input_grad[4:])
        b, l, hidden = x.shape[0], x.shape[1], h0.shape[2]
        hn, cn = torch.empty_like(h0), torch.empty_like(c0)
        zin = torch.empty(b, l, 4, hidden, dtype=torch.float32, device=x.device)  # the projections' scratch
        saved, below = [], x
        for k in range(layers):
            w = weights[4 * k:4 * k + 4]
            run = hip.lstm_narrow_forward if k == 0 else functools.partial(hip.lstm_stack_forward, zin=zin)
            hs, _, _, gates, cs = run(below, h0[k], c0[k], *w, save=need_grad, state_out=(hn[k], cn[k]))
            saved += [w[0], w[1], hs, gates, cs]
            below = hs
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.save_for_backward(x, h0, c0, *saved)
        ctx.mark_non_differentiable(hn, cn)
        return below, hn, cn

    @staticmethod
    def backward(ctx, dhs, dhn, dcn):  # type: ignore[override]
        x, h0, c0, *saved = ctx.saved_tensors
        layers = len(saved) // 5
        top = saved[5 * (layers - 1) + 2]
        dhs = torch.zeros_like(top) if dhs is None else dhs.contiguous().float()
        grads: list = [None] * (4 * layers)
        for k in range(layers - 1, 0, -1):
            w_ih, w_hh, hs, gates, cs = saved[5 * k:5 * k + 5]
            g = hip.lstm_stack_backward(saved[5 * (k - 1) + 2], h0[k], c0[k], w_ih, w_hh, hs, gates, cs, dhs)
            grads[4 * k:4 * k + 4] = g["w_ih"], g["w_hh"], g["b"], g["b"]
            dhs = g["dx"]  # dL/dx of layer k is dL/dhs of layer k - 1: nothing else reads that layer's outputs
        _, w_hh, hs, gates, cs = saved[:5]
        g = hip.lstm_narrow_backward(x, h0[0], c0[0], w_hh, hs, gates, cs, dhs)
        grads[:4] = g["w_ih"], g["w_hh"], g["b"], g["b"]
        return (None, None, None, None, *grads)


def lstm_stack_forward(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``lstm(x, (h0, c0))`` for a stack of two or more layers of width 64 / 128: ``x`` [B, L, d], ``h0`` / ``c0``
    [B, layers, H] (the rollout buffer's layout) -> ``(hs_top [B, L, H], h_n [B, layers, H], c_n [B, layers, H])``,
    or ``None`` when this LSTM / input is not eligible (one layer, other widths, d > 16, no bias, dropout,
    projections, bidirectional, non-HIP / non-fp32 inputs). No gradient flows to ``x``, ``h0``, ``c0`` nor out of
    ``h_n``, ``c_n``."""
    if not _stack_eligible(lstm, x):
        return None
    weights = [getattr(lstm, f"{name}_l{k}") for k in range(lstm.num_layers) for name in _STACK_PARAMS]
    hs, hn, cn = _StackLSTM.apply(
        x.contiguous(), h0.float().transpose(0, 1).contiguous(), c0.float().transpose(0, 1).contiguous(),
        torch.is_grad_enabled(), *weights,
    )
    return hs, hn.transpose(0, 1), cn.transpose(0, 1)


def lstm_forward(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``lstm(x, (h0[None], c0[None]))`` for ``x`` [B, L, d], ``h0`` / ``c0`` [B, H]
    through the fused kernels: ``(hs [B, L, H], h_n [B, H], c_n [B, H])``, or
    ``None`` when this LSTM / input is not eligible (H = 256 with d <= 7, or H = 64 /
    128 with d <= 16). No gradient flows to ``x``, ``h0``, ``c0`` (rollout-buffer
    data) nor out of ``c_n``."""
    if _narrow_eligible(lstm, x):
        hs, cn = _NarrowLSTM.apply(
            x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
            lstm.bias_ih_l0, lstm.bias_hh_l0, torch.is_grad_enabled(),
        )
        return hs, hs[:, -1], cn
    if not _eligible(lstm, x):
        return None
    hs, cn = _FusedLSTM.apply(
        x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
        lstm.bias_ih_l0, lstm.bias_hh_l0, lstm, torch.is_grad_enabled(), _plan(lstm.input_size, x.shape[0]),
    )
    return hs, hs[:, -1], cn  # h_n is h_{L-1}: a view, so a gradient into it reaches dhs by itself


class _FusedHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, b):  # type: ignore[override]
        out = hip.linear_heads_forward(h, w, b)
        ctx.save_for_backward(h, w)
        return out

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        h, w = ctx.saved_tensors
        dh, dw, db = hip.linear_heads_backward(h, dout.contiguous().float(), w)
        return dh, dw, db


class _NarrowHeads(torch.autograd.Function):
    """:class:`_FusedHeads` for latents of width 64 / 128 (lstm_narrow_heads_kernels.hip)."""

    @staticmethod
    def forward(ctx, h, w, b):  # type: ignore[override]
        out = hip.linear_heads_narrow_forward(h, w, b)
        ctx.save_for_backward(h, w)
        return out

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        h, w = ctx.saved_tensors
        dh, dw, db = hip.linear_heads_narrow_backward(h, dout.contiguous().float(), w, need_dh=ctx.needs_input_grad[0])
        return dh, dw, db


class _FusedLSTMHeads(torch.autograd.Function):
    """LSTM + output heads of a training pass as one node: the heads' data gradient dL/dh_t = dOut x W (a rank-n
    product, n <= 4) is formed inside the backward-through-time kernel from the 16 bytes per row-step it is made
    of, instead of being written as [B, L, 256] by the heads' backward and read back (4 KiB of traffic per
    row-step of the recurrent bench less)."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, w_heads, b_heads, lstm, plan):  # type: ignore[override]
        packed, wb = _packs(lstm, "split")
        planes0, bound = _h0_planes(h0)
        hs, _, cn, gates, cs = hip.lstm_forward_split(x, h0, c0, packed, wb, save=True, h0_planes=planes0)
        out = hip.linear_heads_forward(hs.view(-1, hip.LSTM_HIDDEN), w_heads, b_heads)
        ctx.set_materialize_grads(False)
        ctx.lstm, ctx.plan, ctx.h0_bound = lstm, plan, bound
        ctx.save_for_backward(x, h0, c0, hs, gates, cs, w_heads)
        ctx.mark_non_differentiable(cn)
        return out, hs, cn

    @staticmethod
    def backward(ctx, dout, dhs, dcn):  # type: ignore[override]
        x, h0, c0, hs, gates, cs, w_heads = ctx.saved_tensors
        flat = hs.view(-1, hip.LSTM_HIDDEN)
        dout = (torch.zeros(flat.shape[0], w_heads.shape[0], dtype=torch.float32, device=flat.device) if dout is None
                else dout.contiguous().float())
        common = dict(wgrad=ctx.plan.wgrad, rows_packed=_packs(ctx.lstm, "rows"), h0_bound=ctx.h0_bound, hs_bound=1.0)
        if dhs is None:  # nothing but the heads reads the latents: the usual case
            _, dw, db = hip.linear_heads_backward(flat, dout, w_heads, need_dh=False)
            g = hip.lstm_backward(x, h0, c0, hs, gates, cs, None, None, heads=(dout, w_heads), **common)
        else:
            dh, dw, db = hip.linear_heads_backward(flat, dout, w_heads)
            g = hip.lstm_backward(x, h0, c0, hs, gates, cs, dh.view_as(hs) + dhs.float(), None, **common)
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], dw, db, None, None


def _heads_eligible(heads: list[nn.Linear], max_out: int, hidden: int = hip.LSTM_HIDDEN) -> bool:
    if any(h.in_features != hidden or h.bias is None or h.weight.dtype != torch.float32 for h in heads):
        return False
    return sum(h.out_features for h in heads) <= max_out


def _stacked(heads: list[nn.Linear]) -> tuple[torch.Tensor, torch.Tensor, list[int]]:
    """The heads' weights [sum n_i, H] and biases [sum n_i] stacked, and the n_i."""
    w = torch.cat([h.weight for h in heads], 0) if len(heads) > 1 else heads[0].weight
    b = torch.cat([h.bias for h in heads], 0) if len(heads) > 1 else heads[0].bias
    return w, b, [h.out_features for h in heads]


def _narrow_lstm_heads_forward(lstm: nn.LSTM, heads: list[nn.Linear], x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """:func:`lstm_heads_forward` for a one-layer LSTM of width 64 / 128 (``x`` already found ``_narrow_eligible``)."""
    if not (FUSE_HEADS and _heads_eligible(heads, hip.ROWS_BACKWARD_HEADS, lstm.hidden_size)
            and any(p.requires_grad for p in lstm.parameters())):
        return None
    w, b, widths = _stacked(heads)
    out, hs, cn = _NarrowLSTMHeads.apply(
        x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
        lstm.bias_ih_l0, lstm.bias_hh_l0, w, b,
    )
    return list(out.split(widths, dim=1)), hs, hs[:, -1], cn


def lstm_heads_forward(lstm: nn.LSTM, heads: list[nn.Linear], x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """A training pass through ``lstm`` and ``Linear(256, n_i)`` heads on its outputs as one autograd node
    (:class:`_FusedLSTMHeads`): ``([head_i(hs) as [B * L, n_i]], hs [B, L, 256], h_n, c_n)``, or ``None`` when this
    combination is not eligible (no gradient wanted, more than four head outputs, a plan that does not fuse the
    heads): the caller then runs :func:`lstm_forward` and :func:`heads_forward`. A one-layer LSTM of width 64 / 128
    with ``Linear(H, n_i)`` heads has its own node (:class:`_NarrowLSTMHeads`), decided before any width-256 rule."""
    if not torch.is_grad_enabled():
        return None
    if _narrow_eligible(lstm, x):
        return _narrow_lstm_heads_forward(lstm, heads, x, h0, c0)
    if not _eligible(lstm, x):
        return None
    plan = _plan(lstm.input_size, x.shape[0])
    if not (plan.fuse_heads and _heads_eligible(heads, hip.ROWS_BACKWARD_HEADS)
            and any(p.requires_grad for p in lstm.parameters())):
        return None
    widths = [h.out_features for h in heads]
    w = torch.cat([h.weight for h in heads], 0) if len(heads) > 1 else heads[0].weight
    b = torch.cat([h.bias for h in heads], 0) if len(heads) > 1 else heads[0].bias
    out, hs, cn = _FusedLSTMHeads.apply(
        x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
        lstm.bias_ih_l0, lstm.bias_hh_l0, w, b, lstm, plan,
    )
    return list(out.split(widths, dim=1)), hs, hs[:, -1], cn


def heads_forward(heads: list[nn.Linear], latents: torch.Tensor) -> None | list[torch.Tensor]:
    """``[head(latents) for head in heads]`` for ``Linear(H, n_i)`` heads on
    ``latents`` [..., H], H = 256, 64 or 128, in one pass over ``latents`` (and one
    for the backward), or ``None`` when not eligible."""
    hidden = latents.shape[-1]
    narrow = hidden in hip.LSTM_NARROW_HIDDEN
    if not ENABLED or not latents.is_cuda or latents.dtype != torch.float32 or not (narrow or hidden == hip.LSTM_HIDDEN):
        return None
    if any(h.in_features != hidden or h.bias is None for h in heads):
        return None
    w, b, widths = _stacked(heads)
    if sum(widths) > hip.HEADS_MAX_OUT:
        return None
    flat = latents.reshape(-1, hidden)
    out = (_NarrowHeads if narrow else _FusedHeads).apply(flat.contiguous(), w, b)
    return list(out.split(widths, dim=1))
