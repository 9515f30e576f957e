"""``nn.MultiheadAttention``'s core, ``softmax(Q K^T / sqrt(D) + masks) V``, on the short-sequence attention kernels
(``rl8_amd/csrc/attention_kernels.hip``: ``rl8_attention_f32`` / ``rl8_attention_backward_f32``).

:func:`multihead_attention` is what ``modules/attention.py`` tries first: the module's own in-projection (one
``F.linear`` for self-attention, two for cross-attention), the kernels on the packed projection in place, the module's
own out-projection. The module, its parameters and its ``state_dict`` are untouched; an input the kernels do not take
returns ``None`` and the caller runs the module as before. ``RL8_AMD_ATTENTION_KERNELS=0`` (read on every call) does the
same for every input.

:func:`attention_reference` is the torch expression of what the kernels compute, in any dtype on any device: the
yardstick of the tests.
"""

from __future__ import annotations

import math
import os
from typing import Any

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hip


def attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_padding_mask: None | torch.Tensor,
                        bias: None | torch.Tensor, num_heads: int) -> torch.Tensor:
    """``q [B, Tq, E]`` attending over ``k``, ``v [B, Tk, E]`` in ``num_heads`` heads of ``E / num_heads`` features.
    ``key_padding_mask [B, Tk]`` nonzero = PADDED; ``bias [Tq, Tk]`` is added to the scaled scores and may hold ``-inf``.
    A query without an admissible key attends to nothing: its output and every gradient through it are 0."""
    b, tq, e = q.shape
    tk = k.shape[1]
    d = e // num_heads
    qh = q.reshape(b, tq, num_heads, d).transpose(1, 2)
    kh = k.reshape(b, tk, num_heads, d).transpose(1, 2)
    vh = v.reshape(b, tk, num_heads, d).transpose(1, 2)
    scores = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(d))
    if bias is not None:
        scores = scores + bias.to(scores.dtype)
    if key_padding_mask is not None:
        scores = scores.masked_fill(key_padding_mask.bool()[:, None, None, :], -math.inf)
    dead = (scores == -math.inf).all(dim=-1, keepdim=True)
    p = torch.softmax(scores.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return (p @ vh).transpose(1, 2).reshape(b, tq, e)


class _SelfAttentionCore(torch.autograd.Function):
    """The kernel pair on a packed ``qkv [B, T, 3E]``: saves it, ``out``, ``lse`` and the masks, and returns the
    gradient as one ``[B, T, 3E]`` tensor whose three slices the backward kernels write."""

    @staticmethod
    def forward(ctx: Any, qkv: torch.Tensor, key_padding: None | torch.Tensor, bias: None | torch.Tensor,
                heads: int) -> torch.Tensor:
        e = qkv.shape[-1] // 3
        out, lse = hip.attention(qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:], key_padding, bias, heads)
        ctx.heads, ctx.masks = heads, (key_padding is not None, bias is not None)
        ctx.save_for_backward(qkv, out, lse, *[m for m in (key_padding, bias) if m is not None])
        return out

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor) -> tuple[Any, ...]:
        qkv, out, lse, *masks = ctx.saved_tensors
        key_padding = masks.pop(0) if ctx.masks[0] else None
        bias = masks.pop(0) if ctx.masks[1] else None
        e = qkv.shape[-1] // 3
        dqkv = torch.empty_like(qkv)
        hip.attention_backward(qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:], key_padding, bias, out, lse,
                               dout.contiguous(), ctx.heads, dqkv[..., :e], dqkv[..., e:2 * e], dqkv[..., 2 * e:])
        return dqkv, None, None, None


class _CrossAttentionCore(torch.autograd.Function):
    """The same on ``q [B, Tq, E]`` and a packed ``kv [B, Tk, 2E]``."""

    @staticmethod
    def forward(ctx: Any, q: torch.Tensor, kv: torch.Tensor, key_padding: None | torch.Tensor, bias: None | torch.Tensor,
                heads: int) -> torch.Tensor:
        e = q.shape[-1]
        out, lse = hip.attention(q, kv[..., :e], kv[..., e:], key_padding, bias, heads)
        ctx.heads, ctx.masks = heads, (key_padding is not None, bias is not None)
        ctx.save_for_backward(q, kv, out, lse, *[m for m in (key_padding, bias) if m is not None])
        return out

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor) -> tuple[Any, ...]:
        q, kv, out, lse, *masks = ctx.saved_tensors
        key_padding = masks.pop(0) if ctx.masks[0] else None
        bias = masks.pop(0) if ctx.masks[1] else None
        e = q.shape[-1]
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        hip.attention_backward(q, kv[..., :e], kv[..., e:], key_padding, bias, out, lse, dout.contiguous(), ctx.heads,
                               dq, dkv[..., :e], dkv[..., e:])
        return dq, dkv, None, None, None


def _wants_grad(*tensors: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def self_attention_core(qkv: torch.Tensor, key_padding: None | torch.Tensor, bias: None | torch.Tensor,
                        heads: int) -> torch.Tensor:
    """Attention of a packed, dense ``qkv [B, T, 3E]`` over itself on the kernels: ``[B, T, E]``."""
    if _wants_grad(qkv):
        return _SelfAttentionCore.apply(qkv, key_padding, bias, heads)  # type: ignore[no-any-return]
    e = qkv.shape[-1] // 3
    return hip.attention(qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:], key_padding, bias, heads, want_lse=False)[0]


def cross_attention_core(q: torch.Tensor, kv: torch.Tensor, key_padding: None | torch.Tensor, bias: None | torch.Tensor,
                         heads: int) -> torch.Tensor:
    """Attention of a dense ``q [B, Tq, E]`` over a packed, dense ``kv [B, Tk, 2E]`` on the kernels: ``[B, Tq, E]``."""
    if _wants_grad(q, kv):
        return _CrossAttentionCore.apply(q, kv, key_padding, bias, heads)  # type: ignore[no-any-return]
    e = q.shape[-1]
    return hip.attention(q, kv[..., :e], kv[..., e:], key_padding, bias, heads, want_lse=False)[0]


def attention_kernels_on() -> bool:
    """``RL8_AMD_ATTENTION_KERNELS=0`` (read on every call) keeps every input on ``nn.MultiheadAttention`` itself."""
    return os.environ.get("RL8_AMD_ATTENTION_KERNELS", "1") != "0"


def _on_device(x: torch.Tensor) -> bool:
    return x.is_cuda


def _kernel_input(x: torch.Tensor) -> bool:
    return _on_device(x) and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0


def _kernel_bias(attention_mask: None | torch.Tensor, tq: int, tk: int) -> tuple[bool, None | torch.Tensor]:
    """``(taken, bias)``: a 2-D bool mask as 0 / -inf floats, a 2-D float mask that wants no gradient as it is."""
    if attention_mask is None:
        return True, None
    if not _on_device(attention_mask) or tuple(attention_mask.shape) != (tq, tk):
        return False, None
    if attention_mask.dtype == torch.bool:
        return True, torch.zeros(tq, tk, dtype=torch.float32, device=attention_mask.device).masked_fill_(
            attention_mask, -math.inf)
    if attention_mask.dtype == torch.float32 and not attention_mask.requires_grad:
        return True, attention_mask.contiguous()
    return False, None


def multihead_attention(mha: nn.MultiheadAttention, q: torch.Tensor, kv: torch.Tensor,
                        key_padding_mask: None | torch.Tensor, attention_mask: None | torch.Tensor) -> None | torch.Tensor:
    """``mha(q, kv, kv, key_padding_mask=..., attn_mask=..., need_weights=False)[0]`` with the core on the kernels, or
    ``None`` when this call is not theirs: anything but float32 HIP ``[B, T, E]`` inputs outside autocast, a module
    with separate projection weights, ``batch_first=False``, ``bias_k`` / ``add_zero_attn``, active dropout, masks of other
    types or shapes than ``key_padding_mask [B, Tk]`` bool / uint8 and ``attention_mask [Tq, Tk]`` bool or float without
    a gradient, a shape outside ``hip.attention_supports``, or ``RL8_AMD_ATTENTION_KERNELS=0``."""
    if not (attention_kernels_on() and _kernel_input(q) and _kernel_input(kv)) or torch.is_autocast_enabled():
        return None
    if (not mha._qkv_same_embed_dim or not mha.batch_first or mha.bias_k is not None or mha.bias_v is not None
            or mha.add_zero_attn or (mha.dropout > 0.0 and mha.training)):
        return None
    (b, tq, e), tk, heads = q.shape, kv.shape[1], mha.num_heads
    if kv.shape[0] != b or kv.shape[2] != e or e != mha.embed_dim or mha.in_proj_weight.dtype != torch.float32:
        return None
    if key_padding_mask is not None and not (_on_device(key_padding_mask)
                                             and key_padding_mask.dtype in (torch.bool, torch.uint8)
                                             and tuple(key_padding_mask.shape) == (b, tk)):
        return None
    taken, bias = _kernel_bias(attention_mask, tq, tk)
    if not taken or not hip.attention_supports(tq, tk, heads, e // heads):
        return None
    if key_padding_mask is not None:
        key_padding_mask = key_padding_mask.contiguous()
    w, c = mha.in_proj_weight, mha.in_proj_bias
    if q is kv:
        attended = self_attention_core(F.linear(q, w, c), key_padding_mask, bias, heads)
    else:
        attended = cross_attention_core(F.linear(q, w[:e], None if c is None else c[:e]),
                                        F.linear(kv, w[e:], None if c is None else c[e:]), key_padding_mask, bias, heads)
    return mha.out_proj(attended)  # type: ignore[no-any-return]
