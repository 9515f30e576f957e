"""``torch.nn.LSTM`` and the ``Linear`` heads on its outputs as fused gfx950 kernels.

The time loop runs inside the kernels and the gates never leave the chip; parameters stay the module's own. Which
kernels a module gets is decided once, by ``_family`` (the module) and ``_input_ok`` (the input); every entry point
returns ``None`` for anything else (other widths, projections, bidirectional, no bias, dropout between layers,
non-HIP / non-fp32 inputs) and the caller runs the module itself.

========  ===================================  =================================  ===========================
family    envelope                             kernels                            entry point
========  ===================================  =================================  ===========================
"256"     one layer, H = 256, d_in <= 7        lstm_kernels.hip, lstm_split_ /    ``lstm_forward``; with
          (``hip.lstm_supports``); the route   lstm_rows_kernels.hip (packs       heads: ``lstm_heads_forward``
          inside it comes from ``_plan``       cached on the module)              (``_FusedLSTMHeads``)
"256-     one layer, H = 256, 8 <= d_in <=     lstm_wide_in_kernels.hip (fp32     the same two entries and
wide-in"  128 (``hip.lstm_wide_in_supports``)  forward, dW_ih / db), the rows     nodes, after ``_family``
          and ``RL8_AMD_WIDE_INPUT_LSTM`` not  backward and W_hh gradients of     has said ``None``
          0: ``_wide_input_family``; routes    "256" (``_wide_input_plan``)
          from ``_wide_input_plan``
"narrow"  one layer, H = 64 / 128, d_in <= 16  lstm_narrow_kernels.hip (weights   ``lstm_forward``; with
          (``hip.lstm_narrow_supports``)       in torch layout: no plan, no       heads: ``lstm_heads_forward``
                                               packs, no planes)                  (``_NarrowLSTMHeads``)
"stack"   two or more layers of the narrow     layer 0 as "narrow", the layers    ``lstm_stack_forward``
          envelope, ``dropout == 0``           above on lstm_narrow_stack_*
          (``hip.lstm_stack_supports``)
"stack-   two or more layers, H = 256, no      layer 0 as "256" / "256-wide-in"   ``lstm_stack256_forward``
256"      dropout, layer 0's input inside one  (``_plan`` / ``_wide_input_plan``),  (the ``_StackLSTM`` node)
          of those two envelopes, and          the layers above on
          ``RL8_AMD_LSTM_STACK_256`` not 0:    lstm_stack256_kernels.hip, the rows
          ``_stack256_family``                 backward and W_hh gradients of "256"
heads     ``Linear(H, n_i)``, sum n_i <= 8,    lstm_kernels.hip (H = 256),        ``heads_forward``
          on latents of any of the widths      lstm_narrow_heads_kernels.hip
========  ===================================  =================================  ===========================

A training pass through one layer and heads of at most four outputs is one autograd node whose backward through time
forms the heads' data gradient itself (``lstm_heads_forward``); the reference's default models are built around
``nn.LSTM(d_in, 256, batch_first=True)`` (``src/rl8/models/_recurrent.py:201-321``), its example around
``nn.LSTM(4, 64)``.

The "narrow" and "stack" families return the gradient of their input ``x`` where it requires one -- a model with
learned parameters in front of the LSTM, such as ``rl8_amd.envs.LSTMTrader``'s embedding -- from one more launch on
the gate gradients the backward through time has left (``rl8_lstm_narrow_input_grad_f32``); an ``x`` that is
rollout-buffer data costs nothing. The "256", "256-wide-in" and "stack256" families form no input gradient and decline an ``x``
that requires one under grad mode; no family forms a gradient for the initial states ``h0`` / ``c0``, and every entry point declines
a call in which one of them requires it (``_declines``). The caller then runs the module, which forms them.

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


@functools.lru_cache(maxsize=None)
def _narrow_supported(hidden: int, d_in: int) -> bool:
    """The narrow kernels are compiled for this (hidden, d_in): fixed by the build, asked once per pair."""
    return hip.lstm_narrow_supports(hidden, d_in)


def _family(lstm: nn.LSTM) -> None | str:
    """The kernels this module's LSTM runs on, the one place that is decided: "256" (one layer of width 256; the
    routes inside that family are ``_plan``'s), "narrow" (one layer of width 64 / 128, d_in <= 16), "stack" (two or
    more such layers without dropout between them) or ``None`` (the module itself). Reads ``ENABLED`` as it is now."""
    if not (ENABLED and lstm.batch_first and lstm.bias and not lstm.bidirectional and lstm.proj_size == 0):
        return None
    hidden, d_in = lstm.hidden_size, lstm.input_size
    if hidden == hip.LSTM_HIDDEN:
        return "256" if lstm.num_layers == 1 and hip.lstm_supports(d_in) else None
    if hidden not in hip.LSTM_NARROW_HIDDEN or not _narrow_supported(hidden, d_in):
        return None
    if lstm.num_layers == 1:
        return "narrow"
    return "stack" if lstm.dropout == 0 and hip.lstm_stack_supports(hidden) else None


def _input_ok(lstm: nn.LSTM, x: torch.Tensor) -> bool:
    """``x`` is what every family's kernels take: float32 [B, L, input_size] on the device."""
    return x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and x.shape[2] == lstm.input_size


def _family_for(lstm: nn.LSTM, x: torch.Tensor) -> None | str:
    """``_family(lstm)`` where ``x`` is an input its kernels take, else ``None``: all an entry point asks."""
    return _family(lstm) if _input_ok(lstm, x) else None


def wide_input_lstm_on() -> bool:
    """``RL8_AMD_WIDE_INPUT_LSTM=0`` (read on every call) keeps width-256 LSTMs behind 8 to 128 input floats on the
    torch module: the tests' and ``tools/lstm_wide_input_ab.py``'s yardstick.  On by default."""
    return os.environ.get("RL8_AMD_WIDE_INPUT_LSTM", "1") != "0"


@functools.lru_cache(maxsize=None)
def _wide_input_supported(d_in: int) -> bool:
    """The wide-input kernels take this input width: fixed by the build, asked once per width."""
    return hip.lstm_wide_in_supports(d_in)


def _wide_input_family(lstm: nn.LSTM) -> None | str:
    """"256-wide-in" for the modules ``_family`` leaves to torch only because ``hip.lstm_supports`` ends at 7 inputs:
    one layer of width 256, batch_first, biased, no projection, one direction, behind 8 to 128 input floats
    (``hip.lstm_wide_in_supports``), with ``ENABLED`` and the switch ``RL8_AMD_WIDE_INPUT_LSTM`` as they are now; else
    ``None``.  Beside ``_family``, not inside it, as ``fused_mlp._wide_input_family`` is: ``_family``'s answers are
    what the lean rollout and the narrow routes are built on."""
    if not (ENABLED and lstm.batch_first and lstm.bias and not lstm.bidirectional and lstm.proj_size == 0):
        return None
    if lstm.hidden_size != hip.LSTM_HIDDEN or lstm.num_layers != 1 or not _wide_input_supported(lstm.input_size):
        return None
    return "256-wide-in" if wide_input_lstm_on() else None


def _wide_input_family_for(lstm: nn.LSTM, x: torch.Tensor) -> None | str:
    """``_wide_input_family(lstm)`` where ``x`` is an input its kernels take, else ``None``."""
    return _wide_input_family(lstm) if _input_ok(lstm, x) else None


def stack256_lstm_on() -> bool:
    """``RL8_AMD_LSTM_STACK_256=0`` (read on every call) keeps width-256 LSTMs of two or more layers on the torch module:
    the tests' and ``tools/lstm_stack256_ab.py``'s yardstick.  On by default."""
    return os.environ.get("RL8_AMD_LSTM_STACK_256", "1") != "0"


def _stack256_family(lstm: nn.LSTM) -> None | str:
    """"stack256" for two or more layers of width 256 without dropout between them -- batch_first, biased, no
    projection, one direction -- whose layer 0 reads an input width of the "256" (``hip.lstm_supports``) or, with its
    switch on, the "256-wide-in" envelope (``hip.lstm_wide_in_supports``), with ``ENABLED`` and the switch
    ``RL8_AMD_LSTM_STACK_256`` as they are now; else ``None``.  Beside ``_family`` and ``_wide_input_family``, which both
    answer ``None`` for such a module: their answers are what the one-layer entries and the lean rollout are built on."""
    if not (ENABLED and lstm.batch_first and lstm.bias and not lstm.bidirectional and lstm.proj_size == 0):
        return None
    if lstm.hidden_size != hip.LSTM_HIDDEN or lstm.num_layers < 2 or lstm.dropout != 0:
        return None
    d_in = lstm.input_size
    if not (hip.lstm_supports(d_in) or (_wide_input_supported(d_in) and wide_input_lstm_on())):
        return None
    return "stack256" if stack256_lstm_on() and hip.lstm_stack256_supports() else None


def _declines(family: None | str, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor) -> bool:
    """A gradient is asked for that ``family``'s node does not form -- of ``h0`` or ``c0`` (any family), of ``x`` at
    "256", "256-wide-in" and "stack256" -- and grad mode is on: the entry returns ``None`` instead of handing autograd a ``None``
    for it.  Three attribute reads for rollout-buffer data; under ``torch.no_grad()`` nothing can follow and nothing is
    declined."""
    return ((h0.requires_grad or c0.requires_grad or (family in ("256", "256-wide-in", "stack256") and x.requires_grad))
            and torch.is_grad_enabled())


def _packs(lstm: nn.LSTM, kind: str):
    """Fragment-ordered copies of the weights for one kernel ("step" / "split": the fp32 / plane forward step, "wide":
    the fp32 forward behind 8 to 128 inputs, "transposed" / "rows": the fp32 / rows backward), cached ON the module and re-made when the optimizer has changed
    a parameter (version counters) or a parameter tensor has been replaced / moved."""
    params = (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
    stamp = tuple((p._version, p.data_ptr()) for p in params)
    cache = lstm.__dict__.setdefault("_rl8_lstm_packs", {})
    hit = cache.get(kind)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    pack = {"step": hip.lstm_pack, "split": hip.lstm_pack_split, "wide": hip.lstm_wide_in_pack,
            "transposed": hip.lstm_pack_transposed, "rows": hip.lstm_rows_backward_pack}[kind]
    packed = pack(*params) if kind in ("step", "split", "wide") else pack(params[1])
    cache[kind] = (stamp, packed)
    return packed


def _layer_packs(params: tuple, kind: str):
    """``_packs`` for layer k of a width-256 stack, whose node is handed the parameters and not the module:
    ``params`` = (weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k}).  Layer 0's kinds are ``_packs``'s; an
    upper layer's are "stack256" (its fp32 forward), "transposed" / "rows" (its backward through time) and
    "transposed-ih" (``weight_ih`` for dL/dhs of the layer below).  Cached ON the layer's ``weight_hh`` parameter under
    the same stamp -- every parameter's ``(_version, data_ptr)`` -- so a pack lives as long as its layer and is re-made
    when the optimizer has changed a parameter or a tensor has been replaced / moved, not per rollout step."""
    stamp = tuple((p._version, p.data_ptr()) for p in params)
    cache = params[1].__dict__.setdefault("_rl8_lstm_packs", {})
    hit = cache.get(kind)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    if kind in ("step", "split", "wide", "stack256"):
        packed = {"step": hip.lstm_pack, "split": hip.lstm_pack_split, "wide": hip.lstm_wide_in_pack,
                  "stack256": hip.lstm_stack256_pack}[kind](*params)
    elif kind == "rows":
        packed = hip.lstm_rows_backward_pack(params[1])
    else:
        packed = hip.lstm_pack_transposed(params[0 if kind == "transposed-ih" else 1])
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
    wide_in: bool = False  # the "256-wide-in" family: the forward of lstm_wide_in_kernels.hip, dW_ih / db from its launch


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


def _wide_input_plan(b: int) -> _LstmPlan:
    """``_plan`` for the "256-wide-in" family and ``b`` sequences: the forward is the fp32 kernel of
    lstm_wide_in_kernels.hip whatever ``RL8_AMD_LSTM_GEMM`` says (there is no plane forward at these widths); the
    backward through time and the ``W_hh`` gradient follow the rules ``_plan`` applies behind the plane forward, since
    neither reads ``x``."""
    backward_rows = BACKWARD_ROWS
    four_gates = b >= hip.LSTM_WGRAD_GATES_MIN_ROWS and os.environ.get("RL8_AMD_LSTM_WGRAD_GATES", "fused") != "separate"
    wgrad = ("f32" if not backward_rows else
             "bf16" if os.environ.get("RL8_AMD_LSTM_WGRAD_PLANES", "f16") == "bf16" else
             "f16-gates" if four_gates else "f16")
    return _LstmPlan(False, backward_rows, wgrad, FUSE_HEADS and backward_rows, wide_in=True)


def _wide_args(plan: _LstmPlan) -> dict[str, bool]:
    """``hip.lstm_backward``'s ``wide_in=`` for a plan of the "256-wide-in" family; nothing for every other plan."""
    return {"wide_in": True} if plan.wide_in else {}


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
        if plan.wide_in:
            bound = None  # (hip.lstm_backward takes max |h0| itself where its planes need it)
            hs, _, cn, gates, cs = hip.lstm_wide_in_forward(x, h0, c0, _packs(lstm, "wide"), save=need_grad)
        elif plan.forward_planes:
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
                              h0_bound=ctx.h0_bound, hs_bound=1.0,  # (hs: this LSTM's own outputs, |o tanh c| < 1)
                              **_wide_args(ctx.plan))
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], None, None, None


def _input_grad_args(ctx, w_ih: torch.Tensor) -> dict[str, torch.Tensor]:
    """``hip.lstm_narrow_backward``'s ``w_ih=`` (layer 0's: it then returns "dx") exactly when the node's ``x``
    requires a gradient; nothing otherwise: the call, its launches and its allocations are those of a pass without."""
    return {"w_ih": w_ih} if ctx.needs_input_grad[0] else {}


class _NarrowLSTM(torch.autograd.Function):
    """A hidden-64 / 128 LSTM: the weights are read in torch layout (nothing packed, nothing cached); a training
    pass saves the gates and cell states for the backward through time. Where ``x`` requires a gradient (learned
    parameters in front of the LSTM) the backward adds one launch, dL/dx = dz x W_ih (``_input_grad_args``)."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, grad_mode):  # type: ignore[override]
        need_grad = grad_mode and (any(ctx.needs_input_grad[3:7]) or ctx.needs_input_grad[0])
        hs, _, cn, gates, cs = hip.lstm_narrow_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh, save=need_grad)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.save_for_backward(x, h0, c0, w_ih, w_hh, hs, gates, cs)
        ctx.mark_non_differentiable(cn)
        return hs, cn

    @staticmethod
    def backward(ctx, dhs, dcn):  # type: ignore[override]
        x, h0, c0, w_ih, w_hh, hs, gates, cs = ctx.saved_tensors
        dhs = torch.zeros_like(hs) if dhs is None else dhs.contiguous().float()
        g = hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dhs, **_input_grad_args(ctx, w_ih))
        return g.get("dx"), None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], None


def _lstm_heads_backward(hs, w_heads, dout, dhs, heads_backward, lstm_backward):
    """The backward of an LSTM + heads node, ``(g, dw, db)``: the heads' parameter gradients (``heads_backward``:
    ``hip.linear_heads_backward`` or its narrow form), then the backward through time as ``lstm_backward(dhs, heads)``.
    Where nothing but the heads reads the latents that kernel forms dL/dh_t from ``heads`` = (dout, w_heads) itself;
    otherwise the heads' backward writes it out and the other readers' ``dhs`` is added."""
    flat = hs.view(-1, hs.shape[2])
    dout = (torch.zeros(flat.shape[0], w_heads.shape[0], dtype=torch.float32, device=flat.device) if dout is None
            else dout.contiguous().float())
    if dhs is None:  # the usual case
        _, dw, db = heads_backward(flat, dout, w_heads, need_dh=False)
        return lstm_backward(None, (dout, w_heads)), dw, db
    dh, dw, db = heads_backward(flat, dout, w_heads)
    return lstm_backward(dh.view_as(hs) + dhs.float(), None), dw, db


class _NarrowLSTMHeads(torch.autograd.Function):
    """:class:`_NarrowLSTM` + output heads of a training pass as one node, as :class:`_FusedLSTMHeads` is at 256: the
    heads' data gradient dL/dh_t = dOut x W (n <= 4) is formed inside the backward through time from the 16 bytes
    per row-step it is made of, instead of being written as [B, L, H] by the heads' backward and read back. dL/dx
    as in :class:`_NarrowLSTM`, where ``x`` requires it."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, w_heads, b_heads):  # type: ignore[override]
        hs, _, cn, gates, cs = hip.lstm_narrow_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh, save=True)
        out = hip.linear_heads_narrow_forward(hs.view(-1, hs.shape[2]), w_heads, b_heads)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, h0, c0, w_ih, w_hh, hs, gates, cs, w_heads)
        ctx.mark_non_differentiable(cn)
        return out, hs, cn

    @staticmethod
    def backward(ctx, dout, dhs, dcn):  # type: ignore[override]
        x, h0, c0, w_ih, w_hh, hs, gates, cs, w_heads = ctx.saved_tensors
        g, dw, db = _lstm_heads_backward(
            hs, w_heads, dout, dhs, hip.linear_heads_narrow_backward,
            lambda dhs, heads: hip.lstm_narrow_backward(x, h0, c0, w_hh, hs, gates, cs, dhs, heads=heads,
                                                        **_input_grad_args(ctx, w_ih)))
        return g.get("dx"), None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], dw, db


_STACK_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


class _StackLSTM(torch.autograd.Function):
    """A stack of hidden-64 / 128 layers as one node: layer 0 on the narrow kernels, every upper layer on the stack
    kernels, each reading the lower layer's ``hs`` where the kernel left it (no torch op between the layers). The
    weights are read in torch layout, nothing packed or cached. ``h0`` / ``c0`` and the returned states are
    [layers, B, H]; a training pass saves every layer's ``hs``, gates and cell states. dL/dx comes from layer 0 as
    in :class:`_NarrowLSTM`, where ``x`` requires it."""

    @staticmethod
    def forward(ctx, x, h0, c0, grad_mode, *weights):  # type: ignore[override]
        if h0.shape[2] == hip.LSTM_HIDDEN:
            return _stack256_node_forward(ctx, x, h0, c0, grad_mode, weights)
        layers = len(weights) // 4
        need_grad = grad_mode and (any(ctx.needs_input_grad[4:]) or ctx.needs_input_grad[0])
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
        if hasattr(ctx, "plans"):
            return _stack256_node_backward(ctx, dhs)
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
        w_ih, w_hh, hs, gates, cs = saved[:5]
        g = hip.lstm_narrow_backward(x, h0[0], c0[0], w_hh, hs, gates, cs, dhs, **_input_grad_args(ctx, w_ih))
        grads[:4] = g["w_ih"], g["w_hh"], g["b"], g["b"]
        return (g.get("dx"), None, None, None, *grads)


def _stack256_node_forward(ctx, x, h0, c0, grad_mode, weights):
    """:class:`_StackLSTM`'s forward at width 256: layer 0 by the calls :class:`_FusedLSTM` makes on its plan, every
    upper layer by ``hip.lstm_stack256_forward`` on the lower layer's ``hs``.  The plans -- layer 0's from ``_plan`` or
    ``_wide_input_plan``, the upper layers' the ``backward_rows`` / ``wgrad`` rules of ``_wide_input_plan`` (their
    forward is fp32 whatever the switches say) -- are made here, from the shapes and the switches as they are now, and
    kept on ``ctx``.  No gradient is formed for ``x``, ``h0`` or ``c0`` (``lstm_stack256_forward`` declines them)."""
    layers = len(weights) // 4
    need_grad = grad_mode and any(ctx.needs_input_grad[4:])
    b, d_in = x.shape[0], x.shape[2]
    plan0 = _plan(d_in, b) if hip.lstm_supports(d_in) else _wide_input_plan(b)
    plans = (plan0, _wide_input_plan(b))
    hn, cn = torch.empty_like(h0), torch.empty_like(c0)
    w0, bound = weights[:4], None
    if plan0.wide_in:
        hs, hn0, cn0, gates, cs = hip.lstm_wide_in_forward(x, h0[0], c0[0], _layer_packs(w0, "wide"), save=need_grad)
    elif plan0.forward_planes:
        packed, wb = _layer_packs(w0, "split")
        planes0, bound = _h0_planes(h0[0]) if need_grad else (None, None)
        hs, hn0, cn0, gates, cs = hip.lstm_forward_split(x, h0[0], c0[0], packed, wb, save=need_grad, h0_planes=planes0)
    else:
        hs, hn0, cn0, gates, cs = hip.lstm_forward(x, h0[0], c0[0], _layer_packs(w0, "step"), save=need_grad)
    hn[0].copy_(hn0)
    cn[0].copy_(cn0)
    saved = [hs, gates, cs]
    for k in range(1, layers):
        hs, _, _, gates, cs = hip.lstm_stack256_forward(hs, h0[k], c0[k], _layer_packs(weights[4 * k:4 * k + 4], "stack256"),
                                                        save=need_grad, state_out=(hn[k], cn[k]))
        saved += [hs, gates, cs]
    ctx.set_materialize_grads(False)
    if need_grad:
        ctx.plans, ctx.weights, ctx.h0_bound = plans, weights, bound
        ctx.save_for_backward(x, h0, c0, *saved)
    ctx.mark_non_differentiable(hn, cn)
    return hs, hn, cn


def _stack256_node_backward(ctx, dhs):
    """The backward of ``_stack256_node_forward``, on the plans it kept: the layers from the top down, each upper
    layer's "dx" the ``dhs`` of the layer below (nothing else reads that layer's outputs), then layer 0 by
    ``hip.lstm_backward`` as :class:`_FusedLSTM` calls it."""
    x, h0, c0, *saved = ctx.saved_tensors
    layers = len(saved) // 3
    plan0, upper = ctx.plans
    dhs = torch.zeros_like(saved[-3]) if dhs is None else dhs.contiguous().float()
    grads: list = [None] * (4 * layers)

    def through_time(params, plan):  # (whht_packed, rows_packed) of a layer, as _FusedLSTM.backward chooses them
        packed = _layer_packs(params, "rows" if plan.backward_rows else "transposed")
        return (None, packed) if plan.backward_rows else (packed, None)

    for k in range(layers - 1, 0, -1):
        params = ctx.weights[4 * k:4 * k + 4]
        hs, gates, cs = saved[3 * k:3 * k + 3]
        whht, rows = through_time(params, upper)
        g = hip.lstm_stack256_backward(saved[3 * (k - 1)], h0[k], c0[k], hs, gates, cs, dhs, whht,
                                       _layer_packs(params, "transposed-ih"), wgrad=upper.wgrad, rows_packed=rows)
        grads[4 * k:4 * k + 4] = g["w_ih"], g["w_hh"], g["b"], g["b"]
        dhs = g["dx"]
    hs, gates, cs = saved[:3]
    whht, rows = through_time(ctx.weights[:4], plan0)
    g = hip.lstm_backward(x, h0[0], c0[0], hs, gates, cs, dhs, whht, wgrad=plan0.wgrad, rows_packed=rows,
                          h0_bound=ctx.h0_bound, hs_bound=1.0, **_wide_args(plan0))
    grads[:4] = g["w_ih"], g["w_hh"], g["b"], g["b"]
    return (None, None, None, None, *grads)


def _stack_apply(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``_StackLSTM`` on ``lstm``'s layers with the states turned from [B, layers, H] to the node's [layers, B, H] and
    back."""
    weights = [getattr(lstm, f"{name}_l{k}") for k in range(lstm.num_layers) for name in _STACK_PARAMS]
    hs, hn, cn = _StackLSTM.apply(
        x.contiguous(), h0.float().transpose(0, 1).contiguous(), c0.float().transpose(0, 1).contiguous(),
        torch.is_grad_enabled(), *weights,
    )
    return hs, hn.transpose(0, 1), cn.transpose(0, 1)


def lstm_stack256_forward(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``lstm(x, (h0, c0))`` for a stack of two or more layers of width 256 (``_stack256_family``): ``x`` [B, L, d],
    ``h0`` / ``c0`` [B, layers, 256] -> ``(hs_top [B, L, 256], h_n [B, layers, 256], c_n [B, layers, 256])``, or ``None``
    when this LSTM / input is not eligible.  The stack forms no gradient for ``x``, ``h0`` or ``c0``: a call in which one
    of them requires it under grad mode is declined (``None``) and the caller runs the module; under
    ``torch.no_grad()`` nothing is declined.  None flows out of ``h_n``, ``c_n``."""
    if not _input_ok(lstm, x) or _stack256_family(lstm) != "stack256" or _declines("stack256", x, h0, c0):
        return None
    return _stack_apply(lstm, x, h0, c0)


def lstm_stack_forward(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``lstm(x, (h0, c0))`` for a stack of two or more layers of width 64 / 128: ``x`` [B, L, d], ``h0`` / ``c0``
    [B, layers, H] (the rollout buffer's layout) -> ``(hs_top [B, L, H], h_n [B, layers, H], c_n [B, layers, H])``,
    or ``None`` when this LSTM / input is not eligible (one layer, other widths, d > 16, no bias, dropout,
    projections, bidirectional, non-HIP / non-fp32 inputs). ``x`` receives its gradient where it requires one (layer
    0's dz x W_ih, one more launch); none flows out of ``h_n``, ``c_n``, and a call whose ``h0`` or ``c0`` requires a
    gradient under grad mode is declined (``None``)."""
    if _family_for(lstm, x) != "stack" or _declines("stack", x, h0, c0):
        return None
    return _stack_apply(lstm, x, h0, c0)


def lstm_forward(lstm: nn.LSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """``lstm(x, (h0[None], c0[None]))`` for ``x`` [B, L, d], ``h0`` / ``c0`` [B, H]
    through the fused kernels: ``(hs [B, L, H], h_n [B, H], c_n [B, H])``, or
    ``None`` when this LSTM / input is not eligible (H = 256 with d <= 7, or H = 64 /
    128 with d <= 16). No gradient flows out of ``c_n``; ``h0`` / ``c0`` are rollout-buffer
    data, and a call in which one of them requires a gradient under grad mode is declined
    (``None``). At H = 64 / 128 ``x`` receives its gradient where it requires one (an
    encoder in front of the LSTM: one more launch, dz x W_ih); at H = 256 the entry
    declines such an ``x`` under grad mode."""
    family = _family_for(lstm, x) or _wide_input_family_for(lstm, x)
    if family not in ("256", "256-wide-in", "narrow"):  # (a stack has its own entry and state layout: lstm_stack_forward)
        return None
    if _declines(family, x, h0, c0):
        return None
    args = (x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
            lstm.bias_ih_l0, lstm.bias_hh_l0)
    if family == "narrow":
        hs, cn = _NarrowLSTM.apply(*args, torch.is_grad_enabled())
    else:
        plan = _wide_input_plan(x.shape[0]) if family == "256-wide-in" else _plan(lstm.input_size, x.shape[0])
        hs, cn = _FusedLSTM.apply(*args, lstm, torch.is_grad_enabled(), plan)
    return hs, hs[:, -1], cn  # h_n is h_{L-1}: a view, so a gradient into it reaches dhs by itself


class _Heads(torch.autograd.Function):
    """``Linear(H, n)`` heads, stacked, on latents ``h`` [M, H]: lstm_kernels.hip at H = 256,
    lstm_narrow_heads_kernels.hip at 64 / 128."""

    @staticmethod
    def forward(ctx, h, w, b):  # type: ignore[override]
        forward = hip.linear_heads_forward if h.shape[1] == hip.LSTM_HIDDEN else hip.linear_heads_narrow_forward
        out = forward(h, w, b)
        ctx.save_for_backward(h, w)
        return out

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        h, w = ctx.saved_tensors
        dout = dout.contiguous().float()
        if h.shape[1] == hip.LSTM_HIDDEN:
            return hip.linear_heads_backward(h, dout, w)
        return hip.linear_heads_narrow_backward(h, dout, w, need_dh=ctx.needs_input_grad[0])


class _FusedLSTMHeads(torch.autograd.Function):
    """LSTM + output heads of a training pass as one node: the heads' data gradient dL/dh_t = dOut x W (a rank-n
    product, n <= 4) is formed inside the backward-through-time kernel from the 16 bytes per row-step it is made
    of, instead of being written as [B, L, 256] by the heads' backward and read back (4 KiB of traffic per
    row-step of the recurrent bench less)."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, w_heads, b_heads, lstm, plan):  # type: ignore[override]
        if plan.wide_in:
            bound = None
            hs, _, cn, gates, cs = hip.lstm_wide_in_forward(x, h0, c0, _packs(lstm, "wide"), save=True)
        else:
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
        common = dict(wgrad=ctx.plan.wgrad, rows_packed=_packs(ctx.lstm, "rows"), h0_bound=ctx.h0_bound, hs_bound=1.0,
                      **_wide_args(ctx.plan))
        g, dw, db = _lstm_heads_backward(
            hs, w_heads, dout, dhs, hip.linear_heads_backward,
            lambda dhs, heads: hip.lstm_backward(x, h0, c0, hs, gates, cs, dhs, None, heads=heads, **common))
        return None, None, None, g["w_ih"], g["w_hh"], g["b"], g["b"], dw, db, None, None


def _heads_eligible(heads: list[nn.Linear], max_out: int, hidden: int) -> bool:
    if any(h.in_features != hidden or h.bias is None or h.weight.dtype != torch.float32 for h in heads):
        return False
    return sum(h.out_features for h in heads) <= max_out


def _stacked(heads: list[nn.Linear]) -> tuple[torch.Tensor, torch.Tensor, list[int]]:
    """The heads' weights [sum n_i, H] and biases [sum n_i] stacked, and the n_i."""
    w = torch.cat([h.weight for h in heads], 0) if len(heads) > 1 else heads[0].weight
    b = torch.cat([h.bias for h in heads], 0) if len(heads) > 1 else heads[0].bias
    return w, b, [h.out_features for h in heads]


def lstm_heads_forward(lstm: nn.LSTM, heads: list[nn.Linear], x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor):
    """A training pass through a one-layer ``lstm`` and ``Linear(H, n_i)`` heads on its outputs as one autograd node
    (:class:`_FusedLSTMHeads` at H = 256, :class:`_NarrowLSTMHeads` at 64 / 128):
    ``([head_i(hs) as [B * L, n_i]], hs [B, L, H], h_n, c_n)``, or ``None`` when this combination is not eligible (no
    gradient wanted, a stack, more than four head outputs, the heads switched off or -- at 256 -- a plan that does not
    fuse them): the caller then runs :func:`lstm_forward` / :func:`lstm_stack_forward` and :func:`heads_forward`.
    The gradient of ``x`` is as in :func:`lstm_forward`: formed at H = 64 / 128 where ``x`` requires it; at 256 the
    entry declines such an ``x``, and at every width an ``h0`` or ``c0`` that requires a gradient."""
    family = (_family_for(lstm, x) or _wide_input_family_for(lstm, x)) if torch.is_grad_enabled() else None
    if family not in ("256", "256-wide-in", "narrow") or _declines(family, x, h0, c0):
        return None
    plan = (_plan(lstm.input_size, x.shape[0]) if family == "256" else
            _wide_input_plan(x.shape[0]) if family == "256-wide-in" else None)  # (the narrow family reads no plan)
    if not ((FUSE_HEADS if plan is None else plan.fuse_heads)
            and _heads_eligible(heads, hip.ROWS_BACKWARD_HEADS, lstm.hidden_size)
            and any(p.requires_grad for p in lstm.parameters())):
        return None
    w, b, widths = _stacked(heads)
    args = (x.contiguous(), h0.contiguous().float(), c0.contiguous().float(), lstm.weight_ih_l0, lstm.weight_hh_l0,
            lstm.bias_ih_l0, lstm.bias_hh_l0, w, b)
    out, hs, cn = _NarrowLSTMHeads.apply(*args) if plan is None else _FusedLSTMHeads.apply(*args, lstm, plan)
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
    out = _Heads.apply(flat.contiguous(), w, b)
    return list(out.split(widths, dim=1))
