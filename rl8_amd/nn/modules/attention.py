"""Attention blocks on ``nn.MultiheadAttention`` (``src/rl8/nn/modules/attention.py``).

The attention module is torch's, as in the reference, with its parameters and ``state_dict``. On float32 HIP tensors with
sequences of at most 64 cells and heads of at most 16 features its core -- softmax(Q K^T / sqrt(D) + masks) V, forward
and backward -- runs on this build's short-sequence attention kernels (``..fused_attention``, ``rl8_attention_f32``),
between the module's own in- and out-projections. Every other call (CPU tensors, attention dropout in training, other
dtypes and mask kinds, longer sequences, ``RL8_AMD_ATTENTION_KERNELS=0``) runs the module itself; on a HIP device its
scaled-dot-product call is then pinned to torch's math backend: these blocks run at head widths of 2 to 16 on sequences
of a few cells, outside what torch's fused backends are written and tested for, and the math backend is the composition
of matmul, softmax and matmul that the reference's CPU run performs.

The feedforward block behind the attention (``_feedforward``) is the reference's ``nn.Sequential`` of torch modules; where
its activation is ReLU and its dropout is off, ``RL8_AMD_FEEDFORWARD_KERNELS=1`` makes ``SequentialSkipConnection`` run
it with its skip connection on this build's fused feedforward kernels (``..fused_feedforward``,
``rl8_feedforward_f32``); without that setting it runs on the modules.

"""

from __future__ import annotations

import contextlib
import copy

import torch
import torch.nn as nn
from torch.nn.attention import SDPBackend, sdpa_kernel

from .. import fused_attention
from .activations import get_activation
from .module import Module
from .skip import SequentialSkipConnection


def _math_attention(x: torch.Tensor):
    return sdpa_kernel(SDPBackend.MATH) if x.is_cuda else contextlib.nullcontext()


def _attend(attention: nn.MultiheadAttention, q: torch.Tensor, kv: torch.Tensor, key_padding_mask: None | torch.Tensor,
            attention_mask: None | torch.Tensor) -> torch.Tensor:
    fused = fused_attention.multihead_attention(attention, q, kv, key_padding_mask, attention_mask)
    if fused is not None:
        return fused
    with _math_attention(q):
        out, _ = attention(q, kv, kv, key_padding_mask=key_padding_mask, attn_mask=attention_mask, need_weights=False)
    return out  # type: ignore[no-any-return]


def _feedforward(skip: SequentialSkipConnection, hidden_dim: int, activation_fn: str, hidden_dropout: float) -> nn.Sequential:
    features = skip.out_features
    return nn.Sequential(
        nn.LayerNorm(features),
        nn.Linear(features, hidden_dim),
        get_activation(activation_fn),
        nn.Dropout(p=hidden_dropout),
        nn.Linear(hidden_dim, features),
    )


class CrossAttention(Module[[torch.Tensor, torch.Tensor, None | torch.Tensor, None | torch.Tensor], torch.Tensor]):
    """Pre-norm multihead attention of a query ``[B, Q, E]`` over keys ``[B, K, E]``, skip-connected to the query and
    followed by a skip-connected feedforward block.

    Args:
        embed_dim: Feature dimension of queries and keys.
        num_heads: Attention heads.
        hidden_dim: Hidden width of the feedforward block.
        activation_fn: Its activation.
        attention_dropout: Dropout inside the attention.
        hidden_dropout: Dropout inside the feedforward block.
        skip_kind: Kind of both skip connections (``"residual"``, ``"cat"`` or ``None``).

    """

    attention: nn.MultiheadAttention
    kv_norm: nn.LayerNorm
    q_norm: nn.LayerNorm
    skip_connection: SequentialSkipConnection

    def __init__(
        self,
        embed_dim: int,
        /,
        num_heads: int = 2,
        hidden_dim: int = 128,
        activation_fn: str = "relu",
        attention_dropout: float = 0.0,
        hidden_dropout: float = 0.0,
        skip_kind: None | str = "cat",
    ) -> None:
        super().__init__()
        self.q_norm = nn.LayerNorm(embed_dim)
        self.kv_norm = nn.LayerNorm(embed_dim)
        self.attention = nn.MultiheadAttention(embed_dim, num_heads, dropout=attention_dropout, batch_first=True)
        self.skip_connection = SequentialSkipConnection(embed_dim, kind=skip_kind)
        self.skip_connection.append(_feedforward(self.skip_connection, hidden_dim, activation_fn, hidden_dropout))

    def forward(
        self,
        q: torch.Tensor,
        kv: torch.Tensor,
        key_padding_mask: None | torch.Tensor = None,
        attention_mask: None | torch.Tensor = None,
    ) -> torch.Tensor:
        """``key_padding_mask [B, K]`` marks PADDED keys, ``attention_mask [Q, K]`` what a query may not attend to
        (torch's conventions). Returns ``[B, Q, E]``."""
        attended = _attend(self.attention, self.q_norm(q), self.kv_norm(kv), key_padding_mask, attention_mask)
        return self.skip_connection(q, attended)


class SelfAttention(Module[[torch.Tensor, None | torch.Tensor, None | torch.Tensor], torch.Tensor]):
    """:class:`CrossAttention` of a sequence ``[B, X, E]`` over itself, with one norm. Same arguments."""

    attention: nn.MultiheadAttention
    skip_connection: SequentialSkipConnection
    x_norm: nn.LayerNorm

    def __init__(
        self,
        embed_dim: int,
        /,
        num_heads: int = 2,
        hidden_dim: int = 128,
        activation_fn: str = "relu",
        attention_dropout: float = 0.0,
        hidden_dropout: float = 0.0,
        skip_kind: None | str = "cat",
    ) -> None:
        super().__init__()
        self.x_norm = nn.LayerNorm(embed_dim)
        self.attention = nn.MultiheadAttention(embed_dim, num_heads, dropout=attention_dropout, batch_first=True)
        self.skip_connection = SequentialSkipConnection(embed_dim, kind=skip_kind)
        self.skip_connection.append(_feedforward(self.skip_connection, hidden_dim, activation_fn, hidden_dropout))

    def forward(
        self,
        x: torch.Tensor,
        key_padding_mask: None | torch.Tensor = None,
        attention_mask: None | torch.Tensor = None,
    ) -> torch.Tensor:
        """``key_padding_mask [B, X]`` marks PADDED cells, ``attention_mask [X, X]`` what a cell may not attend to."""
        normed = self.x_norm(x)
        return self.skip_connection(x, _attend(self.attention, normed, normed, key_padding_mask, attention_mask))


class SelfAttentionStack(Module[[torch.Tensor, None | torch.Tensor, None | torch.Tensor], torch.Tensor]):
    """``num_layers`` applications of a :class:`SelfAttention`: of the one module (``share_parameters``; its
    parameters then appear under every ``layers.{i}`` of the ``state_dict``) or of independent copies."""

    def __init__(self, module: SelfAttention, num_layers: int, /, *, share_parameters: bool = False) -> None:
        super().__init__()
        self.layers = nn.ModuleList(
            [module if share_parameters else copy.deepcopy(module) for _ in range(num_layers)]
        )

    def forward(
        self,
        x: torch.Tensor,
        key_padding_mask: None | torch.Tensor = None,
        attention_mask: None | torch.Tensor = None,
    ) -> torch.Tensor:
        for layer in self.layers:
            x = layer(x, key_padding_mask=key_padding_mask, attention_mask=attention_mask)
        return x
