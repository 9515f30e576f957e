"""Multi-layer perceptron (``src/rl8/nn/modules/mlp.py``)."""

from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .activations import get_activation
from .module import Module


class MLP(nn.Sequential, Module[[torch.Tensor], torch.Tensor]):
    """``Linear -> [norm] -> act -> [dropout] -> ... -> Linear`` (no trailing activation).

    Args:
        input_dim: Input features.
        hiddens: Width of every layer; the last one is the output.
        activation_fn: Hidden activation, after the linear layer or its norm.
        norm_layer: Optional normalisation (``nn.BatchNorm1d``, ``nn.LayerNorm``) after every hidden linear layer.
        bias: Whether the linear layers have one.
        dropout: Dropout after the activation.
        inplace: Whether the activations run in place.

    """

    def __init__(
        self,
        input_dim: int,
        hiddens: Sequence[int],
        /,
        *,
        activation_fn: str = "relu",
        norm_layer: None | type[nn.Module] = None,
        bias: bool = True,
        dropout: float = 0.0,
        inplace: bool = False,
    ) -> None:
        params = {"inplace": inplace} if inplace else {}
        layers: list[nn.Module] = []
        in_dim = input_dim
        for hidden_dim in hiddens[:-1]:
            layers.append(nn.Linear(in_dim, hidden_dim, bias=bias))
            if norm_layer is not None:
                layers.append(norm_layer(hidden_dim))
            layers.append(get_activation(activation_fn, **params))
            if dropout:
                layers.append(nn.Dropout(p=dropout))
            in_dim = hidden_dim
        layers.append(nn.Linear(in_dim, hiddens[-1], bias=bias))
        super().__init__(*layers)
