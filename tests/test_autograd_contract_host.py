"""The autograd contract of every ``torch.autograd.Function`` under ``rl8_amd``, as one table that must stay complete.

A fused route does one of three things for a tensor it is handed that requires a gradient: it forms that gradient
("formed"), it declines at its public entry so that the caller runs the torch modules ("declined"), or it raises
before any launch and names the argument ("refused").  It never hands autograd ``None`` for such a tensor and carries
on: torch then leaves ``.grad`` of everything in front of the node at ``None`` without a word.

``CONTRACT`` names, for every node, every parameter of its ``forward`` and what becomes of it; this file (no GPU) fails
when a node is missing from the table, when the table names a node that no longer exists, or when a ``forward`` has a
parameter the table does not name.  ``tests/test_autograd_contract_gpu.py`` holds every row to fp64 on the device.

Kinds of an input:

``"formed"``         the node's backward returns its gradient
``"declined"``       the public entry returns ``None`` / takes the torch route when it requires a gradient under grad mode
``"refused"``        the public entry raises ``ValueError`` / ``TypeError`` naming it, before any launch
``"no-grad dtype"``  an integer or bool tensor
``"kernel output"``  a float tensor the entry itself made from kernel outputs a moment ago (a recorded activation, a
                     precomputed gradient): never a caller's tensor, so it cannot require a gradient
``"not a tensor"``   a module, a plan, a number, a flag

An output is ``"differentiable"`` or ``"non-differentiable"`` (it went through ``mark_non_differentiable``: a loss on it
alone fails loudly in torch).
"""

from __future__ import annotations

import importlib
import inspect

import pytest
import torch

MODULES = ("rl8_amd.models", "rl8_amd.models_recurrent", "rl8_amd.nn.functional", "rl8_amd.nn.fused_mlp",
           "rl8_amd.nn.fused_lstm", "rl8_amd.nn.fused_attention", "rl8_amd.nn.fused_feedforward",
           "rl8_amd.nn.piecewise_mlp")

INPUT_KINDS = ("formed", "declined", "refused", "no-grad dtype", "kernel output", "not a tensor")
OUTPUT_KINDS = ("differentiable", "non-differentiable")

_F, _D, _R, _I, _K, _N = INPUT_KINDS
_TOWER_PARAMS = {k: _F for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
_LSTM_PARAMS = {k: _F for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
_DIFF, _NONDIFF = OUTPUT_KINDS

#: node -> {"entry": its public entry, "inputs": {forward parameter: kind}, "outputs": {returned tensor: kind}};
#: ``"entry_inputs"``: float tensors the public entry takes that never reach the node.  A ``*args`` parameter maps to a
#: dict of its parts.
CONTRACT: dict[str, dict] = {
    "rl8_amd.models._MeanAndLogStd": {
        "entry": "DefaultContinuousModel.forward",
        "inputs": {"out": _F, "a": _N},
        "outputs": {"mean": _DIFF, "log_std": _DIFF},
    },
    "rl8_amd.nn.fused_mlp._FusedTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _D, **_TOWER_PARAMS, "layer2": _N, "grad_mode": _N, "plan": _N, "w3_key": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_mlp._ReplayedTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _D, **_TOWER_PARAMS, "layer2": _N, "plan": _N, "w3_key": _N, "out": _K, "gate": _I, "h2": _K},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_mlp._NarrowTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _F, **_TOWER_PARAMS},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_mlp._NarrowBatchNormTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _F, "w1": _F, "b1": _F, "gamma": _F, "beta": _F, "w2": _F, "b2": _F, "w3": _F, "b3": _F,
                   "norm": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_mlp._WideInputTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _D, **_TOWER_PARAMS, "layer1": _N, "layer2": _N, "grad_mode": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.piecewise_mlp._PiecewiseTower": {
        "entry": "fused_mlp.tower_forward",
        "inputs": {"x": _D, **_TOWER_PARAMS, "table": _N, "grad_mode": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_lstm._FusedLSTM": {
        "entry": "fused_lstm.lstm_forward",
        "inputs": {"x": _D, "h0": _D, "c0": _D, **_LSTM_PARAMS, "lstm": _N, "grad_mode": _N, "plan": _N},
        "outputs": {"hs": _DIFF, "c_n": _NONDIFF},
    },
    "rl8_amd.nn.fused_lstm._NarrowLSTM": {
        "entry": "fused_lstm.lstm_forward",
        "inputs": {"x": _F, "h0": _D, "c0": _D, **_LSTM_PARAMS, "grad_mode": _N},
        "outputs": {"hs": _DIFF, "c_n": _NONDIFF},
    },
    "rl8_amd.nn.fused_lstm._NarrowLSTMHeads": {
        "entry": "fused_lstm.lstm_heads_forward",
        "inputs": {"x": _F, "h0": _D, "c0": _D, **_LSTM_PARAMS, "w_heads": _F, "b_heads": _F},
        "outputs": {"out": _DIFF, "hs": _DIFF, "c_n": _NONDIFF},
    },
    "rl8_amd.nn.fused_lstm._StackLSTM": {
        "entry": "fused_lstm.lstm_stack_forward",
        "inputs": {"x": _F, "h0": _D, "c0": _D, "grad_mode": _N, "weights": {"every layer's four parameters": _F}},
        "outputs": {"hs": _DIFF, "h_n": _NONDIFF, "c_n": _NONDIFF},
    },
    "rl8_amd.nn.fused_lstm._Heads": {
        "entry": "fused_lstm.heads_forward",
        "inputs": {"h": _F, "w": _F, "b": _F},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_lstm._FusedLSTMHeads": {
        "entry": "fused_lstm.lstm_heads_forward",
        "inputs": {"x": _D, "h0": _D, "c0": _D, **_LSTM_PARAMS, "w_heads": _F, "b_heads": _F, "lstm": _N, "plan": _N},
        "outputs": {"out": _DIFF, "hs": _DIFF, "c_n": _NONDIFF},
    },
    "rl8_amd.nn.fused_attention._SelfAttentionCore": {
        "entry": "fused_attention.multihead_attention",
        "inputs": {"qkv": _F, "key_padding": _I, "bias": _D, "heads": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_attention._CrossAttentionCore": {
        "entry": "fused_attention.multihead_attention",
        "inputs": {"q": _F, "kv": _F, "key_padding": _I, "bias": _D, "heads": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.fused_feedforward._FeedforwardBlock": {
        "entry": "fused_feedforward.skip_feedforward",
        "inputs": {"x": _F, "gamma": _F, "beta": _F, "w1": _F, "b1": _F, "w2": _F, "b2": _F, "eps": _N, "residual": _N},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.functional._AttachPrecomputedGrads": {
        "entry": "nn.functional.ppo_losses",
        "inputs": {"total": _K, "n_inputs": _N,
                   "tensors": {"the features and the values": _F, "their gradients from the loss kernel": _K}},
        "entry_inputs": {"actions": _R, "logp": _R, "advantages": _R, "returns": _R},
        "outputs": {"total": _DIFF},
    },
    "rl8_amd.nn.functional._MaskedAvg": {
        "entry": "nn.functional.masked_avg",
        "inputs": {"x": _F, "mask": _I},
        "outputs": {"avg": _DIFF},
    },
    "rl8_amd.nn.functional._MaskedMax": {
        "entry": "nn.functional.masked_max",
        "inputs": {"x": _F, "mask": _I},
        "outputs": {"max": _DIFF, "index": _NONDIFF},
    },
    "rl8_amd.nn.functional._MaskedLogSoftmax": {
        "entry": "nn.functional.masked_log_softmax",
        "inputs": {"x": _F, "mask": _I},
        "outputs": {"out": _DIFF},
    },
    "rl8_amd.nn.functional._MaskedSample": {
        "entry": "nn.functional.masked_categorical_sample",
        "inputs": {"x": _F, "mask": _I, "noise": _D, "seed": _N, "step": _N, "row_offset": _N},
        "outputs": {"value": _DIFF, "index": _NONDIFF},
    },
}


def _subclasses(cls: type) -> list[type]:
    found = []
    for sub in cls.__subclasses__():
        found.append(sub)
        found.extend(_subclasses(sub))
    return found


def nodes() -> dict[str, type]:
    """Qualified name -> class, for every ``torch.autograd.Function`` subclass defined under ``rl8_amd``."""
    for name in MODULES:
        importlib.import_module(name)
    return {f"{c.__module__}.{c.__qualname__}": c for c in _subclasses(torch.autograd.Function)
            if c.__module__ == "rl8_amd" or c.__module__.startswith("rl8_amd.")}


def _leaves(kind) -> list:
    return [leaf for v in kind.values() for leaf in _leaves(v)] if isinstance(kind, dict) else [kind]


def problems(found: dict[str, type], contract: dict[str, dict]) -> list[str]:
    """Everything that keeps ``contract`` from being the complete declaration of ``found``; empty when it is."""
    out = [f"{name}: an autograd node without a row in CONTRACT" for name in sorted(set(found) - set(contract))]
    out += [f"{name}: a row in CONTRACT for a node that does not exist" for name in sorted(set(contract) - set(found))]
    for name in sorted(set(found) & set(contract)):
        row = contract[name]
        if not row.get("entry"):
            out.append(f"{name}: no public entry named")
        parameters = list(inspect.signature(found[name].forward).parameters.values())[1:]  # (without ctx)
        declared = row.get("inputs", {})
        for p in parameters:
            if p.name not in declared:
                typed = "tensor-typed " if "Tensor" in str(p.annotation) else ""
                out.append(f"{name}: forward's {typed}parameter {p.name!r} is not in its row")
            elif "Tensor" in str(p.annotation) and _N in _leaves(declared[p.name]):
                out.append(f"{name}: {p.name!r} is annotated as a tensor and declared {_N!r}")
            elif p.kind is inspect.Parameter.VAR_POSITIONAL and not isinstance(declared[p.name], dict):
                out.append(f"{name}: *{p.name} wants a dict of its parts")
        out += [f"{name}: the row names {k!r}, which forward does not take"
                for k in declared if k not in {p.name for p in parameters}]
        for k, kind in {**declared, **row.get("entry_inputs", {})}.items():
            out += [f"{name}: {k!r} has the unknown kind {leaf!r}" for leaf in _leaves(kind) if leaf not in INPUT_KINDS]
        if not row.get("outputs"):
            out.append(f"{name}: no outputs declared")
        out += [f"{name}: output {k!r} has the unknown kind {kind!r}" for k, kind in row.get("outputs", {}).items()
                if kind not in OUTPUT_KINDS]
    return out


def undifferentiated(kinds: tuple[str, ...] = (_D, _R)) -> list[tuple[str, str]]:
    """Every ``(node, input)`` whose gradient the kernels do not form: where someone who wants one of them starts."""
    pairs = []
    for name, row in CONTRACT.items():
        for k, kind in {**row["inputs"], **row.get("entry_inputs", {})}.items():
            if any(leaf in kinds for leaf in _leaves(kind)):
                pairs.append((name.rsplit(".", 1)[1], k))
    return pairs


def test_every_node_under_rl8_amd_has_a_complete_row():
    found = nodes()
    assert len(found) >= 21, sorted(found)
    assert problems(found, CONTRACT) == []


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_a_deleted_row_is_noticed(name):
    without = {k: v for k, v in CONTRACT.items() if k != name}
    assert any(p.startswith(name + ":") and "without a row" in p for p in problems(nodes(), without))


def test_a_new_node_is_noticed_until_it_declares_its_contract():
    class _Dummy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x: torch.Tensor, scale: float):  # type: ignore[override]
            return x * scale

        @staticmethod
        def backward(ctx, dout):  # type: ignore[override]
            return None, None  # (the very bug: a silent drop)

    found = {**nodes(), "rl8_amd.nn.scratch._Dummy": _Dummy}
    assert problems(found, CONTRACT) == ["rl8_amd.nn.scratch._Dummy: an autograd node without a row in CONTRACT"]
    row = {"entry": "scratch.dummy", "inputs": {"scale": _N}, "outputs": {"out": _DIFF}}
    assert problems(found, {**CONTRACT, "rl8_amd.nn.scratch._Dummy": row}) == [
        "rl8_amd.nn.scratch._Dummy: forward's tensor-typed parameter 'x' is not in its row"]
    row["inputs"]["x"] = _N
    assert problems(found, {**CONTRACT, "rl8_amd.nn.scratch._Dummy": row}) == [
        "rl8_amd.nn.scratch._Dummy: 'x' is annotated as a tensor and declared 'not a tensor'"]
    row["inputs"]["x"] = _R
    assert problems(found, {**CONTRACT, "rl8_amd.nn.scratch._Dummy": row}) == []
    # the subclass walk itself sees a class whose module lies under rl8_amd
    _Dummy.__module__, _Dummy.__qualname__ = "rl8_amd.nn.scratch", "_Dummy"
    try:
        assert "rl8_amd.nn.scratch._Dummy" in "".join(problems(nodes(), CONTRACT))
    finally:
        _Dummy.__module__ = __name__


def test_a_stale_row_and_an_unknown_kind_are_noticed():
    stale = {**CONTRACT, "rl8_amd.nn.fused_mlp._Gone": CONTRACT["rl8_amd.nn.fused_mlp._NarrowTower"]}
    assert problems(nodes(), stale) == ["rl8_amd.nn.fused_mlp._Gone: a row in CONTRACT for a node that does not exist"]
    name = "rl8_amd.nn.fused_mlp._NarrowTower"
    odd = {**CONTRACT, name: {**CONTRACT[name], "inputs": {**CONTRACT[name]["inputs"], "x": "dropped"}}}
    assert problems(nodes(), odd) == [f"{name}: 'x' has the unknown kind 'dropped'"]
    more = {**CONTRACT, name: {**CONTRACT[name], "inputs": {**CONTRACT[name]["inputs"], "y": _F}}}
    assert problems(nodes(), more) == [f"{name}: the row names 'y', which forward does not take"]


def test_what_the_kernels_do_not_differentiate_is_listed():
    """The list that goes into the notes of a change to this table: 19 inputs declined, 4 refused."""
    assert len(undifferentiated((_D,))) == 19 and len(undifferentiated((_R,))) == 4, undifferentiated()
    assert ("_FusedTower", "x") in undifferentiated() and ("_NarrowLSTM", "h0") in undifferentiated()
