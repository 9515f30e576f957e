"""Built-in models for :class:`~rl8_amd.envs.AlgoTrading`.

``MLPTrader`` is the feed-forward one: a padded rolling window of the last ``seq_len + 1`` price changes (a tuple-key
view requirement, built by the window kernels), summed over four spans, next to an embedding of ``invested`` and the
change of the price against the position; two BatchNorm towers give masked logits and a value. The towers run as torch
modules by default; with ``RL8_AMD_BATCHNORM_TOWERS=1`` (opt-in, read per call) they run on the narrow tower kernels,
the BatchNorm folded into the first layer from the batch's moments (``nn/fused_mlp.py``, family ``"narrow_bn"``), and
the gradient of the towers' input, which trains ``invested_embedding``, comes from the same backward launch.

``TransformerTrader`` is the attentive feed-forward one: the same window, embedded cell by cell, goes through a
parameter-sharing stack of residual self-attention blocks (``rl8_amd.nn``, on torch's ``nn.MultiheadAttention``) under
the window's padding mask and is averaged over its valid cells by the masked-pool kernel (``nn.functional.masked_avg``).

``LSTMTrader`` is the recurrent one: an embedding of ``invested`` and the two price log-changes go through an LSTM
whose latents feed a logits head and a value head. At hidden width 64 / 128 a training pass is one fused autograd
node (``nn/fused_lstm.py:lstm_heads_forward``) that also returns the gradient of the LSTM's input, which is what
trains the embedding; at any other width the ``nn.LSTM`` module itself runs, so the embedding always has a gradient.

"""

from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from ..data import DataKeys, Device
from ..models import Model
from ..nn import MLP, SelfAttention, SelfAttentionStack, get_activation, masked_avg
from ..models_recurrent import RecurrentModel, _lstm_state_spec, _run_lstm_heads, _small_head
from ..specs import TensorSpec
from ..tensordict import TensorDict
from ..views import ViewRequirement

LOG_CHANGE, LOG_CHANGE_POSITION = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"


def _tower(tower: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """``tower(x)`` for ``Sequential(MLP(..., norm_layer=BatchNorm1d), ReLU, head)``: on the BatchNorm tower kernels
    where ``fused_mlp.tower_forward`` takes the call (``RL8_AMD_BATCHNORM_TOWERS=1``, width 64 / 128, float32 on the
    device), else the modules."""
    from ..nn import fused_mlp

    if not fused_mlp.batchnorm_towers_on():  # (the default route pays for no slicing of the Sequential)
        return tower(x)
    out = fused_mlp.tower_forward(tower[:2], [tower[2]], x)
    return tower(x) if out is None else out


class MLPTrader(Model):
    """The reference's ``MischievousMule`` (``examples/algotrading/models/mlp.py``; its ``state_dict`` loads as is):
    ``("obs", "LOG_CHANGE(price)") -> ViewRequirement(shift=seq_len)`` on top of the default view, the window's sums
    over its first quarter, first half, last half and last quarter, ``Embedding(2, invested_embed_dim)`` on
    ``invested`` and ``LOG_CHANGE(price, position)`` -> two ``MLP(..., norm_layer=BatchNorm1d)`` towers: a
    small-initialised ``Linear(hiddens[-1], 3)`` logits head, masked by ``log(action_mask)``, and a
    ``Linear(hiddens[-1], 1)`` value head."""

    def __init__(
        self,
        observation_spec: TensorSpec,
        action_spec: TensorSpec,
        /,
        *,
        invested_embed_dim: int = 2,
        seq_len: int = 4,
        hiddens: Sequence[int] = (128, 128),
        activation_fn: str = "relu",
    ) -> None:
        super().__init__(observation_spec, action_spec, invested_embed_dim=invested_embed_dim, seq_len=seq_len,
                         hiddens=hiddens, activation_fn=activation_fn)
        assert not seq_len % 4, "`seq_len` must be a factor of 4 for this model."
        self.seq_len = seq_len
        self.view_requirements[(DataKeys.OBS, LOG_CHANGE)] = ViewRequirement(shift=seq_len)
        self.invested_embedding = nn.Embedding(2, invested_embed_dim)

        def tower(head: nn.Linear) -> nn.Sequential:
            return nn.Sequential(
                MLP(invested_embed_dim + 5, hiddens, activation_fn=activation_fn, norm_layer=nn.BatchNorm1d),
                get_activation(activation_fn),
                head,
            )

        self.feature_model = tower(_small_head(hiddens[-1], 3))
        self.vf_model = tower(nn.Linear(hiddens[-1], 1))
        self._value: None | torch.Tensor = None

    def forward(self, batch: TensorDict, /) -> TensorDict:
        obs = batch[DataKeys.OBS]
        x_price = obs[LOG_CHANGE][DataKeys.INPUTS]  # [B, seq_len + 1, 1]
        quarter, half = self.seq_len // 4, self.seq_len // 2
        x = torch.cat(
            [
                self.invested_embedding(obs["invested"].flatten()),
                obs[LOG_CHANGE_POSITION],
                torch.sum(x_price[:, :quarter], dim=1),
                torch.sum(x_price[:, :half], dim=1),
                torch.sum(x_price[:, -half:], dim=1),
                torch.sum(x_price[:, -quarter:], dim=1),
            ],
            dim=-1,
        )
        finfo = torch.finfo(torch.float32)
        mask = torch.clamp(torch.log(obs["action_mask"].to(torch.float32)), min=finfo.min, max=finfo.max)
        logits = _tower(self.feature_model, x).reshape(-1, 1, 3) + mask.reshape(-1, 1, 3)
        self._value = _tower(self.vf_model, x)
        return TensorDict({"logits": logits}, batch_size=batch.batch_size, device=x.device)

    def to(self, device: Device) -> "MLPTrader":  # type: ignore[override]
        self._value = None
        return super().to(device)  # type: ignore[return-value]

    def value_function(self) -> torch.Tensor:
        assert self._value is not None
        return self._value


class TransformerTrader(Model):
    """The reference's ``AttentiveAlpaca`` (``examples/algotrading/models/transformer.py``; its ``state_dict`` loads as
    is): ``("obs", "LOG_CHANGE(price)") -> ViewRequirement(shift=seq_len)`` on top of the default view,
    ``Linear(1, price_embed_dim)`` on every cell of the window, ``num_layers`` passes through ONE residual
    ``SelfAttention(price_embed_dim, num_heads, hidden_dim=hiddens[0])`` with the padded cells masked as keys, the
    average over the valid cells, and next to it ``Embedding(2, invested_embed_dim)`` on ``invested`` and
    ``LOG_CHANGE(price, position)`` -> the two BatchNorm towers and heads of :class:`MLPTrader`."""

    def __init__(
        self,
        observation_spec: TensorSpec,
        action_spec: TensorSpec,
        /,
        invested_embed_dim: int = 2,
        price_embed_dim: int = 8,
        seq_len: int = 4,
        num_heads: int = 4,
        num_layers: int = 2,
        hiddens: Sequence[int] = (64, 64),
        activation_fn: str = "relu",
    ) -> None:
        super().__init__(observation_spec, action_spec, invested_embed_dim=invested_embed_dim,
                         price_embed_dim=price_embed_dim, seq_len=seq_len, num_heads=num_heads, num_layers=num_layers,
                         hiddens=hiddens, activation_fn=activation_fn)
        self.view_requirements[(DataKeys.OBS, LOG_CHANGE)] = ViewRequirement(shift=seq_len)
        self.invested_embedding = nn.Embedding(2, invested_embed_dim)
        self.price_embedding = nn.Linear(1, price_embed_dim)
        self.price_attention = SelfAttentionStack(
            SelfAttention(price_embed_dim, num_heads=num_heads, hidden_dim=hiddens[0], activation_fn=activation_fn,
                          skip_kind="residual"),
            num_layers,
            share_parameters=True,
        )

        def tower() -> list[nn.Module]:
            return [
                MLP(invested_embed_dim + 1 + price_embed_dim, hiddens, activation_fn=activation_fn,
                    norm_layer=nn.BatchNorm1d),
                get_activation(activation_fn),
            ]

        # (modules are created in the reference's order, so one seed initialises both alike)
        self.feature_model = nn.Sequential(*tower())
        self.feature_model.append(_small_head(hiddens[-1], 3))
        self.vf_model = nn.Sequential(*tower(), nn.Linear(hiddens[-1], 1))
        self._value: None | torch.Tensor = None

    def forward(self, batch: TensorDict, /) -> TensorDict:
        obs = batch[DataKeys.OBS]
        window = obs[LOG_CHANGE]
        padding_mask = window[DataKeys.PADDING_MASK]  # [B, seq_len + 1] bool, True = padded; the last cell never is
        x_price = self.price_embedding(window[DataKeys.INPUTS])  # [B, seq_len + 1, price_embed_dim]
        x_price = self.price_attention(x_price, key_padding_mask=padding_mask)
        x = torch.cat(
            [
                self.invested_embedding(obs["invested"].flatten()),
                obs[LOG_CHANGE_POSITION],
                masked_avg(x_price, mask=~padding_mask, dim=1, keepdim=False),
            ],
            dim=-1,
        )
        finfo = torch.finfo(torch.float32)
        mask = torch.clamp(torch.log(obs["action_mask"].to(torch.float32)), min=finfo.min, max=finfo.max)
        logits = _tower(self.feature_model, x).reshape(-1, 1, 3) + mask.reshape(-1, 1, 3)
        self._value = _tower(self.vf_model, x)
        return TensorDict({"logits": logits}, batch_size=batch.batch_size, device=x.device)

    def to(self, device: Device) -> "TransformerTrader":  # type: ignore[override]
        self._value = None
        return super().to(device)  # type: ignore[return-value]

    def value_function(self) -> torch.Tensor:
        assert self._value is not None
        return self._value


class LSTMTrader(RecurrentModel):
    """``Embedding(2, invested_embed_dim)`` on ``invested``, concatenated with ``LOG_CHANGE(price, position)`` and
    ``LOG_CHANGE(price)`` -> ``LSTM(invested_embed_dim + 2, hidden_size)`` -> a small-initialised ``Linear(hidden, 3)``
    logits head, masked by ``log(action_mask)``, and a ``Linear(hidden, 1)`` value head."""

    def __init__(
        self,
        observation_spec: TensorSpec,
        action_spec: TensorSpec,
        /,
        *,
        invested_embed_dim: int = 2,
        hidden_size: int = 64,
    ) -> None:
        super().__init__(observation_spec, action_spec, invested_embed_dim=invested_embed_dim, hidden_size=hidden_size)
        self.state_spec = _lstm_state_spec(1, hidden_size, action_spec.device)
        self.invested_embedding = nn.Embedding(2, invested_embed_dim)
        self.lstm = nn.LSTM(invested_embed_dim + 2, hidden_size, num_layers=1, batch_first=True)
        self.feature_head = _small_head(hidden_size, 3)
        self.vf_head = nn.Linear(hidden_size, 1)
        self._value: None | torch.Tensor = None

    def forward(self, batch: TensorDict, states: TensorDict, /) -> tuple[TensorDict, TensorDict]:
        from ..nn import fused_lstm

        obs = batch[DataKeys.OBS]
        invested = obs["invested"]  # [B, T, 1] int64
        b, t = invested.shape[:2]
        x = torch.cat(
            [
                self.invested_embedding(invested.reshape(b, t)),
                obs["LOG_CHANGE(price, position)"],
                obs["LOG_CHANGE(price)"],
            ],
            dim=-1,
        )
        heads = [self.feature_head, self.vf_head]
        if fused_lstm._family(self.lstm) in ("narrow", "stack"):
            # the fused families that return dL/dx: the embedding is trained through the kernels
            outs, new_states = _run_lstm_heads(self.lstm, heads, x, states)
        else:
            # (no fused family forms a gradient for x at this width: the module, as models_recurrent._run_lstm runs it)
            h_0 = states[DataKeys.HIDDEN_STATES][:, 0, ...].permute(1, 0, 2).contiguous()
            c_0 = states[DataKeys.CELL_STATES][:, 0, ...].permute(1, 0, 2).contiguous()
            with torch.backends.cudnn.flags(enabled=False):
                latents, (h_n, c_n) = self.lstm(x, (h_0, c_0))
            outs = [head(latents) for head in heads]
            new_states = TensorDict(
                {DataKeys.HIDDEN_STATES: h_n.permute(1, 0, 2), DataKeys.CELL_STATES: c_n.permute(1, 0, 2)}, batch_size=b
            )
        mask = torch.clamp(torch.log(obs["action_mask"].float()), min=torch.finfo(torch.float32).min)
        logits = outs[0].reshape(-1, 1, 3) + mask.reshape(-1, 1, 3)
        self._value = outs[1].reshape(-1, 1)
        return TensorDict({"logits": logits}, batch_size=logits.size(0), device=x.device), new_states

    def to(self, device: Device) -> "LSTMTrader":  # type: ignore[override]
        self._value = None
        return super().to(device)  # type: ignore[return-value]

    def value_function(self) -> torch.Tensor:
        assert self._value is not None
        return self._value


__all__ = ["LSTMTrader", "MLPTrader", "TransformerTrader"]
