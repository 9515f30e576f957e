"""Perceiver layers (``src/rl8/nn/modules/perceiver.py``)."""

from __future__ import annotations

from typing import Any

import torch
import torch.nn as nn

from .attention import CrossAttention, SelfAttention, SelfAttentionStack
from .module import Module

_Forward = [torch.Tensor, torch.Tensor, None | torch.Tensor, None | torch.Tensor]


class PerceiverLayer(Module[_Forward, torch.Tensor]):
    """Cross-attention of a latent array ``q [B, Q, E]`` over an input sequence ``kv [B, K, E]``, then a stack of
    self-attention over the latents (arXiv:2103.03206).

    Args:
        embed_dim: Feature dimension of latents and inputs.
        num_heads, hidden_dim, activation_fn, attention_dropout, hidden_dropout, skip_kind: As
            :class:`CrossAttention`, for every block.
        num_layers: Self-attention layers.
        share_parameters: Whether those layers are one module.

    """

    def __init__(
        self,
        embed_dim: int,
        /,
        *,
        num_heads: int = 2,
        hidden_dim: int = 128,
        num_layers: int = 2,
        activation_fn: str = "relu",
        attention_dropout: float = 0.0,
        hidden_dropout: float = 0.0,
        skip_kind: str = "cat",
        share_parameters: bool = False,
    ) -> None:
        super().__init__()
        block: dict[str, Any] = dict(
            num_heads=num_heads, hidden_dim=hidden_dim, activation_fn=activation_fn,
            attention_dropout=attention_dropout, hidden_dropout=hidden_dropout, skip_kind=skip_kind,
        )
        self.cross_attention = CrossAttention(embed_dim, **block)
        self.self_attention = SelfAttentionStack(
            SelfAttention(embed_dim, **block), num_layers, share_parameters=share_parameters
        )

    def forward(
        self,
        q: torch.Tensor,
        kv: torch.Tensor,
        key_padding_mask: None | torch.Tensor = None,
        attention_mask: None | torch.Tensor = None,
    ) -> torch.Tensor:
        """Masks as in :meth:`CrossAttention.forward` (they apply to the cross-attention only). Returns ``[B, Q, E]``."""
        return self.self_attention(self.cross_attention(q, kv, key_padding_mask, attention_mask), None, None)


class PerceiverIOLayer(Module[_Forward, torch.Tensor]):
    """A :class:`PerceiverLayer` whose latents are then read out by a learned query of ``output_seq_dim`` cells
    through one more cross-attention (arXiv:2107.14795). Other arguments as :class:`PerceiverLayer`."""

    def __init__(
        self,
        embed_dim: int,
        output_seq_dim: int,
        /,
        *,
        num_heads: int = 2,
        hidden_dim: int = 128,
        num_layers: int = 2,
        activation_fn: str = "relu",
        attention_dropout: float = 0.0,
        hidden_dropout: float = 0.0,
        skip_kind: str = "cat",
        share_parameters: bool = False,
    ) -> None:
        super().__init__()
        block: dict[str, Any] = dict(
            num_heads=num_heads, hidden_dim=hidden_dim, activation_fn=activation_fn,
            attention_dropout=attention_dropout, hidden_dropout=hidden_dropout, skip_kind=skip_kind,
        )
        self.perceiver_layer = PerceiverLayer(embed_dim, num_layers=num_layers, share_parameters=share_parameters, **block)
        self.output_query = nn.Parameter(torch.zeros([output_seq_dim, embed_dim]))
        with torch.no_grad():
            nn.init.xavier_uniform_(self.output_query)
        self.decoder = CrossAttention(embed_dim, **block)

    def forward(
        self,
        q: torch.Tensor,
        kv: torch.Tensor,
        key_padding_mask: None | torch.Tensor = None,
        attention_mask: None | torch.Tensor = None,
    ) -> torch.Tensor:
        """Returns ``[B, output_seq_dim, E]``."""
        latent = self.perceiver_layer(q, kv, key_padding_mask, attention_mask)
        output_query = self.output_query.unsqueeze(0).expand(q.size(0), *self.output_query.shape)
        return self.decoder(output_query, latent, None, None)
