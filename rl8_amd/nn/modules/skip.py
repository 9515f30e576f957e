"""Chained skip connections (``src/rl8/nn/modules/skip.py``)."""

from __future__ import annotations

import torch
import torch.nn as nn

from .. import fused_feedforward
from ..functional import skip_connection
from .module import Module


class SequentialSkipConnection(Module[[torch.Tensor, torch.Tensor], torch.Tensor]):
    """A skip connection between an input and a layer's output, then one around every appended module.

    ``_layers`` alternates: even places hold what follows a skip connection (for ``"cat"`` a ``Linear`` that brings
    the doubled features back to ``embed_dim``, otherwise ``Identity``), odd places the appended modules.

    Args:
        embed_dim: Features of the input.
        kind: ``"residual"`` (sum), ``"cat"`` (concatenate, then project back) or ``None`` (no skip connection: a
            plain sequential module).

    """

    _in_features: list[int]
    _layers: nn.ModuleList
    kind: None | str

    def __init__(self, embed_dim: int, kind: None | str = "cat") -> None:
        super().__init__()
        self.kind = kind
        self._in_features = [embed_dim]
        self._layers = nn.ModuleList([self._fan_in()])

    def _fan_in(self) -> nn.Module:
        """What follows a skip connection over ``_in_features[-1]`` features."""
        if self.kind == "cat":
            return nn.Linear(self._skip_features, self._in_features[0])
        return nn.Identity()

    @property
    def _skip_features(self) -> int:
        """Features that leave a skip connection entered with ``_in_features[-1]``."""
        if self.kind == "cat":
            return 2 * self._in_features[-1]
        if self.kind == "residual" or self.kind is None:
            return self._in_features[-1]
        raise ValueError(f"No skip connection type for {self.kind}.")

    def append(self, module: nn.Module, /) -> int:
        """Put ``module`` behind a skip connection at the end; returns the features that then come out."""
        self._in_features.append(self._skip_features)
        self._layers.append(module)
        if self.kind == "cat":
            self._layers.append(nn.Linear(self._in_features[-1], self._in_features[0]))
            self._in_features.append(self._in_features[0])
        else:
            self._layers.append(nn.Identity())
            self._in_features.append(self._in_features[-1])
        return self.out_features

    def forward(self, x: torch.Tensor, y: torch.Tensor, /) -> torch.Tensor:
        """``x`` and ``y`` ``[B, T, ...]`` of one shape: skip-connect them, then run the layers, each appended module
        inside a skip connection of its own -- the attention modules' feedforward block with its skip connection in one
        kernel launch where ``fused_feedforward.skip_feedforward`` takes the call."""
        y = skip_connection(x, y, kind=self.kind)
        for i, layer in enumerate(self._layers):
            if i % 2:
                fused = fused_feedforward.skip_feedforward(layer, y, self.kind)
                y = fused if fused is not None else skip_connection(y, layer(y), kind=self.kind)
            else:
                y = layer(y)
        return y

    @property
    def in_features(self) -> int:
        return self._in_features[0]

    @property
    def out_features(self) -> int:
        return self._in_features[0] if self.kind == "cat" else self._skip_features
