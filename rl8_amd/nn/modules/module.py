"""``Module[[argument types], return type]``: an ``nn.Module`` whose call signature type checkers can see
(``src/rl8/nn/modules/module.py``)."""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Generic, ParamSpec, TypeVar

import torch.nn as nn

_Args = ParamSpec("_Args")
_Out = TypeVar("_Out")


class Module(ABC, Generic[_Args, _Out], nn.Module):
    """``nn.Module`` parametrised by the arguments and the result of ``forward``."""

    def __call__(self, *args: _Args.args, **kwargs: _Args.kwargs) -> _Out:
        return nn.Module.__call__(self, *args, **kwargs)  # type: ignore[no-any-return]

    @abstractmethod
    def forward(self, *args: _Args.args, **kwargs: _Args.kwargs) -> _Out:
        """What the module computes."""
