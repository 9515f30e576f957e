"""View requirements: how a ``[B, T, ...]`` buffer leaf becomes model input.

Mirrors the reference's ``src/rl8/views.py`` (``pad_last_sequence`` :54-90,
``pad_whole_sequence`` :93-123, ``rolling_window`` :126-152, ``RollingWindow``
:155-237, ``PaddedRollingWindow`` :240-321, ``ViewRequirement`` :324-453).

``shift = 0`` is the PPO hot path: a flatten for training, the last timestep for
sampling (no copy on the time-major buffer). ``shift > 0`` gives sequence models
the last ``shift + 1`` observations of every sample, either as a plain rolling
window (a strided view; the first ``shift`` samples of each row are dropped) or
padded with zeros in front plus a mask (no samples dropped).

Windows are built with ``Tensor.unfold`` -- a stride trick, no data movement
until a consumer asks for a dense tensor -- on any device.

``window_plan`` decides, once per model, whether the observation views can be
built by the gather kernels instead (``rl8_window_last`` during the rollout,
``rl8_gather_windows`` per minibatch): padded windows on ``"obs"`` /
``("obs", leaf)`` only. Everything else keeps the torch route above.

"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Literal, Sequence

import torch

from .data import DataKeys
from .tensordict import TensorDict

ViewKind = Literal["last", "all"]
ViewMethod = Literal["rolling_window", "padded_rolling_window"]


def _padded(x: torch.Tensor, pad: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``pad`` zero steps in front of ``x`` along time, and the mask marking them."""
    b, t = x.shape[:2]
    front = x.new_zeros(b, pad, *x.shape[2:])
    mask = torch.zeros(b, t + pad, dtype=torch.bool, device=x.device)
    mask[:, :pad] = True
    return torch.cat([front, x], dim=1), mask


def _inputs_and_mask(inputs: torch.Tensor, mask: torch.Tensor) -> TensorDict:
    out = TensorDict({}, batch_size=list(mask.shape), device=inputs.device)
    out[DataKeys.INPUTS] = inputs
    out[DataKeys.PADDING_MASK] = mask
    return out


def pad_last_sequence(x: torch.Tensor, size: int, /) -> TensorDict:
    """The last ``size`` steps of ``x`` ``[B, T, ...]``, zero-padded in front when
    ``T < size``: ``{"inputs": [B, size, ...], "padding_mask": [B, size]}``."""
    t = x.shape[1]
    if t < size:
        return _inputs_and_mask(*_padded(x, size - t))
    mask = torch.zeros(x.shape[0], size, dtype=torch.bool, device=x.device)
    return _inputs_and_mask(x[:, -size:, ...], mask)


def pad_whole_sequence(x: torch.Tensor, size: int, /) -> TensorDict:
    """``size - 1`` zero steps in front of ``x`` ``[B, T, ...]`` so that a rolling
    window of ``size`` over the result has ``T`` positions."""
    return _inputs_and_mask(*_padded(x, size - 1))


def rolling_window(x: torch.Tensor, size: int, /, *, step: int = 1) -> torch.Tensor:
    """``[B, T, ...] -> [B, (T - size) / step + 1, size, ...]``: every run of
    ``size`` consecutive steps, as a strided view."""
    windows = x.unfold(1, size, step)  # the window lands in the LAST dimension
    return windows.movedim(-1, 2)


def _map(x: torch.Tensor | TensorDict, fn: Callable[[torch.Tensor], torch.Tensor | TensorDict],
         batch_size: list[int]) -> torch.Tensor | TensorDict:
    """``fn`` on a tensor, or on every leaf of a (nested) tensordict."""
    if isinstance(x, torch.Tensor):
        return fn(x)
    return x.apply(fn, batch_size=batch_size)


class RollingWindow:
    """Plain rolling window: no padding, no mask; the first ``size - 1`` steps of
    each row cannot start a window and are dropped."""

    @staticmethod
    def apply_all(x: torch.Tensor | TensorDict, size: int, /) -> torch.Tensor | TensorDict:
        """``[B, T, ...] -> [B * (T - size + 1), size, ...]``."""
        if isinstance(x, torch.Tensor):
            return rolling_window(x, size).reshape(-1, size, *x.shape[2:])
        b, t = x.shape[:2]
        return x.apply(lambda leaf: rolling_window(leaf, size), batch_size=[b, t - size + 1]).reshape(-1)

    @staticmethod
    def apply_last(x: torch.Tensor | TensorDict, size: int, /) -> torch.Tensor | TensorDict:
        """``[B, T, ...] -> [B, min(T, size), ...]``: the most recent steps."""
        b, t = x.shape[:2]
        return _map(x, lambda leaf: leaf[:, -size:, ...], [b, min(t, size)])

    @staticmethod
    def drop_size(size: int, /) -> int:
        return size - 1


class PaddedRollingWindow:
    """Rolling window over a front-padded sequence: every step keeps a window;
    the padding is flagged in ``"padding_mask"``."""

    @staticmethod
    def apply_all(x: torch.Tensor | TensorDict, size: int, /) -> TensorDict:
        """``[B, T, ...] -> [B * T]`` batch of ``{"inputs": [size, ...],
        "padding_mask": [size]}`` (per leaf for a tensordict)."""
        b, t = x.shape[:2]
        padded = _map(x, lambda leaf: pad_whole_sequence(leaf, size), [b, t + size - 1])
        return RollingWindow.apply_all(padded, size)  # type: ignore[return-value]

    @staticmethod
    def apply_last(x: torch.Tensor | TensorDict, size: int, /) -> TensorDict:
        """``[B, T, ...] -> [B, size]`` batch, zero-padded in front while ``T < size``."""
        return _map(x, lambda leaf: pad_last_sequence(leaf, size), [x.shape[0], size])  # type: ignore[return-value]

    @staticmethod
    def drop_size(size: int, /) -> int:
        return 0


_METHODS = {"rolling_window": RollingWindow, "padded_rolling_window": PaddedRollingWindow}


class ViewRequirement:
    """Preprocessing of one buffer key before it reaches the model.

    Args:
        shift: Number of additional previous timesteps each sample sees.
        method: ``"rolling_window"`` (cheap, drops the first ``shift`` samples
            of each row) or ``"padded_rolling_window"`` (keeps every sample,
            adds a padding mask).

    """

    #: :class:`RollingWindow` or :class:`PaddedRollingWindow`.
    method: type[RollingWindow] | type[PaddedRollingWindow]

    shift: int

    def __init__(self, *, shift: int = 0, method: ViewMethod = "padded_rolling_window") -> None:
        if shift < 0:
            raise ValueError(f"{self.__class__.__name__} `shift` must be non-negative.")
        if method not in _METHODS:
            raise ValueError(f"Unknown view method {method!r}; expected one of {sorted(_METHODS)}.")
        self.shift = shift
        self.method = _METHODS[method]

    @property
    def is_identity(self) -> bool:
        """No windowing: training flattens, sampling takes the last step."""
        return self.shift == 0

    def apply_all(self, key: str | tuple[str, ...], batch: TensorDict, /) -> torch.Tensor | TensorDict:
        """``[B, T, ...] -> [B*T, ...]`` for ``shift = 0``, else ``[B_NEW, shift + 1, ...]``
        with ``B_NEW <= B * T`` depending on the method."""
        item = batch[key]
        with torch.no_grad():
            if not self.shift:
                if isinstance(item, torch.Tensor):
                    return item.flatten(end_dim=1)
                return item.reshape(-1)
            return self.method.apply_all(item, self.shift + 1)

    def apply_last(self, key: str | tuple[str, ...], batch: TensorDict, /) -> torch.Tensor | TensorDict:
        """``[B, T, ...] -> [B, ...]`` (most recent timestep) for ``shift = 0``,
        else ``[B, shift + 1, ...]``."""
        item = batch[key]
        with torch.no_grad():
            if not self.shift:
                return item[:, -1, ...]
            return self.method.apply_last(item, self.shift + 1)

    @property
    def drop_size(self) -> int:
        """Samples lost at the start of every row by the method."""
        return self.method.drop_size(self.shift + 1)


# --------------------------------------------------------------------------- #
# The kernel route for observation views.
# --------------------------------------------------------------------------- #
#: What one gather launch takes (``RL8_MAX_GATHER_FIELDS`` of include/rl8_amd.h).
MAX_WINDOW_FIELDS = 8

#: Leaf dtypes the window kernels move (4-, 8- and 1-byte elements).
WINDOW_DTYPES = (torch.float32, torch.int64, torch.bool)


@dataclass(frozen=True)
class WindowLeaf:
    """One field of a window launch: the observation leaf (``None``: the tensor observation itself) and its window
    length ``shift + 1``. ``size > 1`` becomes ``{"inputs", "padding_mask"}`` in the views, ``size == 1`` stays a
    tensor."""

    name: None | str
    size: int


@dataclass(frozen=True)
class WindowPlan:
    """Which observation leaves a model reads and with which window, in launch order; the views tensordict built
    from a launch's outputs has the keys ``Model.apply_view_requirements`` gives."""

    leaves: tuple[WindowLeaf, ...]

    @property
    def sizes(self) -> list[int]:
        return [leaf.size for leaf in self.leaves]

    def sources(self, obs: torch.Tensor | TensorDict) -> list[torch.Tensor]:
        """The buffer leaves of the fields, in launch order, out of ``buffer["obs"]``."""
        return [obs if leaf.name is None else obs[leaf.name] for leaf in self.leaves]

    def layout(self) -> dict[str, Any]:
        """Key structure of the views: ``None`` for a tensor, ``{"inputs": None, "padding_mask": None}`` for a
        window, nested by leaf name for dict observations."""
        def entry(leaf: WindowLeaf) -> Any:
            return None if leaf.size == 1 else {DataKeys.INPUTS: None, DataKeys.PADDING_MASK: None}

        if len(self.leaves) == 1 and self.leaves[0].name is None:
            return {DataKeys.OBS: entry(self.leaves[0])}
        return {DataKeys.OBS: {leaf.name: entry(leaf) for leaf in self.leaves}}

    def views(self, outs: Sequence[tuple[torch.Tensor, None | torch.Tensor]]) -> TensorDict:
        """The views tensordict from one launch's ``(inputs, padding_mask | None)`` per field."""
        rows = outs[0][0].shape[0]

        def entry(out: tuple[torch.Tensor, None | torch.Tensor]) -> torch.Tensor | TensorDict:
            inputs, mask = out
            if mask is None:
                return inputs
            window = TensorDict({}, batch_size=[rows], device=inputs.device)
            window[DataKeys.INPUTS] = inputs
            window[DataKeys.PADDING_MASK] = mask
            return window

        if len(self.leaves) == 1 and self.leaves[0].name is None:
            obs: Any = entry(outs[0])
        else:
            obs = TensorDict({leaf.name: entry(out) for leaf, out in zip(self.leaves, outs)}, batch_size=[rows],
                             device=outs[0][0].device)
        return TensorDict({DataKeys.OBS: obs}, batch_size=[rows], device=outs[0][0].device)


def window_kernels_enabled() -> bool:
    """``RL8_AMD_WINDOW_KERNELS=0`` keeps every view on the torch route (read per call)."""
    return os.environ.get("RL8_AMD_WINDOW_KERNELS", "1") != "0"


def window_plan(model: Any, observation_spec: Any, /) -> None | WindowPlan:
    """The kernel route for ``model``'s observation views, or ``None`` for the torch route.

    The kernels take over when every view key is ``"obs"`` or ``("obs", leaf)``, every leaf read is a float32, int64
    or bool tensor leaf (one level of nesting at most), every ``shift > 0`` uses ``padded_rolling_window`` and at
    most ``MAX_WINDOW_FIELDS`` fields result. Keys apply in the order of ``model.view_requirements``, as
    ``Model.apply_view_requirements`` assigns them: ``"obs"`` sets every leaf, a later ``("obs", leaf)`` overwrites
    that leaf.

    """
    from .specs import Composite

    if not window_kernels_enabled():
        return None
    requirements = getattr(model, "view_requirements", None)
    if not requirements:  # (recurrent models take observations as they are)
        return None
    composite = isinstance(observation_spec, Composite)
    if composite:
        names = list(observation_spec.keys())
        specs = [observation_spec[name] for name in names]
    else:
        names, specs = [None], [observation_spec]
    if any(isinstance(spec, Composite) or getattr(spec, "dtype", None) not in WINDOW_DTYPES for spec in specs):
        return None
    sizes: dict[None | str, int] = {}
    for key, requirement in requirements.items():
        if requirement.shift > 0 and requirement.method is not PaddedRollingWindow:
            return None
        if key == DataKeys.OBS:
            sizes = {name: requirement.shift + 1 for name in names}
        elif (composite and isinstance(key, tuple) and len(key) == 2 and key[0] == DataKeys.OBS
              and key[1] in names):
            sizes[key[1]] = requirement.shift + 1
        else:
            return None
    if not 1 <= len(sizes) <= MAX_WINDOW_FIELDS:
        return None
    return WindowPlan(tuple(WindowLeaf(name, size) for name, size in sizes.items()))
