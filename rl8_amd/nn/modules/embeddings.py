"""Sequence embeddings (``src/rl8/nn/modules/embeddings.py``)."""

from __future__ import annotations

import math

import torch
import torch.nn as nn

from .module import Module


class PositionalEmbedding(Module[[torch.Tensor], torch.Tensor]):
    """Sinusoidal position codes added to ``x [B, T, E]``.

    Args:
        embed_dim: Feature dimension ``E``.
        max_len: Longest sequence.
        dropout: Dropout on the sum.

    """

    dropout: nn.Dropout
    pe: torch.Tensor

    def __init__(self, embed_dim: int, max_len: int, /, *, dropout: float = 0.0) -> None:
        super().__init__()
        position = torch.arange(max_len).unsqueeze(1)
        rate = (-math.log(10_000) / embed_dim * torch.arange(0, embed_dim, 2)).exp()
        pe = torch.zeros(1, max_len, embed_dim)
        pe[0, :, 0::2] = torch.sin(position * rate)
        pe[0, :, 1::2] = torch.cos(position * rate)
        self.dropout = nn.Dropout(p=dropout)
        self.register_buffer("pe", pe)

    def forward(self, x: torch.Tensor, /) -> torch.Tensor:
        return self.dropout(x + self.pe[0, : x.size(1)])  # type: ignore[no-any-return]
