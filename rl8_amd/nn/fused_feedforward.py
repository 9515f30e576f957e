"""The block every ``SelfAttention`` / ``CrossAttention`` ends with, ``skip(y, Linear(act(Linear(LayerNorm(y)))))``, on
the fused feedforward kernels (``rl8_amd/csrc/feedforward_kernels.hip``: ``rl8_feedforward_f32`` /
``rl8_feedforward_backward_f32``).

:func:`skip_feedforward` is what ``modules/skip.py`` tries first for every appended module: one launch per forward with
the hidden vector in registers, nothing but the input saved for the backward. The modules, their parameters and their
``state_dict`` are untouched; a call the kernels do not take returns ``None`` and the caller runs the modules as before.
The route is opt-in: it takes calls only while ``RL8_AMD_FEEDFORWARD_KERNELS=1`` (read on every call); unset, ``0`` or
anything else keeps every input on the modules (DESIGN.md section 8 says why it is not the default).

:func:`feedforward_reference` is the torch expression of what the kernels compute, in any dtype on any device: the
yardstick of the tests.
"""

from __future__ import annotations

import os
from typing import Any

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hip


def feedforward_reference(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, w1: torch.Tensor,
                          b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, residual: bool) -> torch.Tensor:
    """``(x if residual else 0) + W2 relu(W1 LayerNorm(x) + b1) + b2`` over the last dimension of ``x [..., F]``, with
    ``w1 [H, F]`` and ``w2 [F, H]`` as ``nn.Linear`` holds them."""
    n = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    y = F.linear(torch.relu(F.linear(n, w1, b1)), w2, b2)
    return x + y if residual else y


class _FeedforwardBlock(torch.autograd.Function):
    """The kernels on a dense ``x [..., F]``: saves ``x`` (beside the parameters, which exist anyway) and forms the
    normalised row and the pre-activations again in the backward; saves nothing when no gradient is to be formed."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                w2: torch.Tensor, b2: torch.Tensor, eps: float, residual: bool) -> torch.Tensor:
        out = hip.feedforward(x, gamma, beta, eps, w1, b1, w2, b2, residual)
        if any(ctx.needs_input_grad):
            ctx.eps, ctx.residual = eps, residual
            ctx.save_for_backward(x, gamma, beta, w1, b1, w2)
        return out

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor) -> tuple[Any, ...]:
        x, gamma, beta, w1, b1, w2 = ctx.saved_tensors
        grads = hip.feedforward_backward(x, dout.contiguous(), gamma, beta, ctx.eps, w1, b1, w2, ctx.residual,
                                         want_dx=ctx.needs_input_grad[0], want_params=any(ctx.needs_input_grad[1:7]))
        return tuple(g if wanted else None for g, wanted in zip(grads, ctx.needs_input_grad)) + (None, None)


def feedforward_kernels_on() -> bool:
    """``RL8_AMD_FEEDFORWARD_KERNELS=1`` (read on every call) turns the route on; unset or anything else keeps every
    input on the torch modules."""
    return os.environ.get("RL8_AMD_FEEDFORWARD_KERNELS", "0") == "1"


def _on_device(x: torch.Tensor) -> bool:
    return x.is_cuda


def _block(module: nn.Module) -> None | tuple[nn.LayerNorm, nn.Linear, nn.Linear]:
    """The three parameterised layers of exactly ``Sequential(LayerNorm(F), Linear(F, H), ReLU, Dropout, Linear(H, F))``
    with an affine, biased norm over the last dimension, biased Linears and no active dropout."""
    if type(module) is not nn.Sequential or len(module) != 5:
        return None
    norm, up, act, drop, down = module
    if not (type(norm) is nn.LayerNorm and type(up) is nn.Linear and type(act) is nn.ReLU and type(drop) is nn.Dropout
            and type(down) is nn.Linear):
        return None
    if norm.weight is None or norm.bias is None or up.bias is None or down.bias is None:
        return None
    if drop.p > 0.0 and module.training:
        return None
    f, hidden = up.in_features, up.out_features
    if tuple(norm.normalized_shape) != (f,) or (down.in_features, down.out_features) != (hidden, f):
        return None
    return norm, up, down


def skip_feedforward(module: nn.Module, y: torch.Tensor, kind: None | str) -> None | torch.Tensor:
    """``skip_connection(y, module(y), kind)`` with the block on the kernels -- the ``"residual"`` sum inside the
    launch, ``"cat"`` as a ``torch.cat`` behind it -- or ``None`` when this call is not theirs: a module that is not
    exactly the feedforward block of ``modules/attention.py`` with ReLU (an affine, biased LayerNorm, biased Linears,
    dropout off or in eval mode), a shape outside ``hip.feedforward_supports``, parameters or an input that are not
    float32 on a HIP device, autocast, an input that is not dense with last dimension F and at least one element, an
    unknown ``kind``, or ``RL8_AMD_FEEDFORWARD_KERNELS`` not ``1``."""
    if not feedforward_kernels_on() or kind not in ("residual", "cat", None) or torch.is_autocast_enabled():
        return None
    if not (_on_device(y) and y.dtype == torch.float32 and y.dim() >= 1 and y.numel() > 0 and y.is_contiguous()):
        return None
    layers = _block(module)
    if layers is None:
        return None
    norm, up, down = layers
    params = (norm.weight, norm.bias, up.weight, up.bias, down.weight, down.bias)
    if y.shape[-1] != up.in_features or not all(_on_device(p) and p.dtype == torch.float32 for p in params):
        return None
    if not hip.feedforward_supports(up.in_features, up.out_features):
        return None
    out = _FeedforwardBlock.apply(y, *(p.contiguous() for p in params), norm.eps, kind == "residual")
    return torch.cat([y, out], dim=-1) if kind == "cat" else out  # type: ignore[no-any-return]
