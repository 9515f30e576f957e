"""Golden vectors for the ``rl8_amd.nn`` surface: the reference's own ``rl8.nn`` (``src/rl8/nn/functional.py``,
``src/rl8/nn/modules``) evaluated on the CPU on small seeded inputs.

Like the other generators this runs only where the reference is checked out next to the repository and imports it
unmodified (through ``generate_fixtures``, which also supplies ``save``). ``nn_reference.npz`` holds arrays and name
lists only:

* ``function_cases`` / ``module_cases``: the case names;
* per function case ``f_<case>_spec`` (a JSON line: the function's name and its non-tensor keyword arguments, and the
  torch seed where the function draws), ``f_<case>_arg_<name>`` (tensor arguments; ``x``, ``y`` and ``lengths`` are
  positional) and ``f_<case>_out<i>``;
* per module case ``m_<case>_spec`` (a JSON line: class, constructor arguments, what is appended or wrapped),
  ``m_<case>_sd_names`` and ``m_<case>_sd_<i>`` (the reference's ``state_dict``), ``m_<case>_in<i>`` (positional
  inputs of ``forward``) and ``m_<case>_out``.

``tests/test_nn_surface_host.py`` rebuilds every case from its spec with ``rl8_amd.nn`` (``build_module`` below is
restated there), loads the state dict strictly and compares. Float and bool masks, padded and fully padded rows are
included; modules run in training mode with gradients enabled, so ``nn.MultiheadAttention`` takes its ordinary path.

Usage::

    python tests/golden/generate_nn_fixtures.py

"""

from __future__ import annotations

import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))

ATTENTION = dict(num_heads=4, hidden_dim=64)
MODULE_SPECS: dict[str, dict] = {
    "self_attention_residual": {"cls": "SelfAttention", "args": [8], "kwargs": {**ATTENTION, "skip_kind": "residual"},
                                "inputs": ["seq", "padding"]},
    "self_attention_cat": {"cls": "SelfAttention", "args": [8], "kwargs": {**ATTENTION, "skip_kind": "cat"},
                           "inputs": ["seq", "padding"]},
    "self_attention_none": {"cls": "SelfAttention", "args": [8], "kwargs": {**ATTENTION, "skip_kind": None},
                            "inputs": ["seq", "padding"]},
    "cross_attention": {"cls": "CrossAttention", "args": [8], "kwargs": {"num_heads": 2, "hidden_dim": 16},
                        "inputs": ["query", "seq", "padding"]},
    "stack_shared": {"cls": "SelfAttentionStack", "args": [3], "kwargs": {"share_parameters": True},
                     "wraps": {"args": [8], "kwargs": {**ATTENTION, "skip_kind": "residual"}}, "inputs": ["seq", "padding"]},
    "stack_unshared": {"cls": "SelfAttentionStack", "args": [2], "kwargs": {"share_parameters": False},
                       "wraps": {"args": [8], "kwargs": {"num_heads": 2, "hidden_dim": 16}}, "inputs": ["seq", "padding"]},
    "perceiver": {"cls": "PerceiverLayer", "args": [8], "kwargs": {"num_heads": 2, "hidden_dim": 16, "num_layers": 2},
                  "inputs": ["query", "seq", "padding"]},
    "perceiver_io": {"cls": "PerceiverIOLayer", "args": [8, 2],
                     "kwargs": {"num_heads": 2, "hidden_dim": 16, "num_layers": 1, "skip_kind": "residual",
                                "share_parameters": True},
                     "inputs": ["query", "seq", "padding"]},
    "positional_embedding": {"cls": "PositionalEmbedding", "args": [8, 16], "kwargs": {}, "inputs": ["seq"]},
    "skip_cat_appended": {"cls": "SequentialSkipConnection", "args": [8], "kwargs": {"kind": "cat"}, "append": [8, 8],
                          "inputs": ["seq", "seq2"]},
    "skip_residual_appended": {"cls": "SequentialSkipConnection", "args": [8], "kwargs": {"kind": "residual"},
                               "append": [8, 8], "inputs": ["seq", "seq2"]},
    "mlp_plain": {"cls": "MLP", "args": [8, [16, 16, 3]], "kwargs": {"activation_fn": "tanh"}, "inputs": ["rows"]},
    "mlp_batchnorm": {"cls": "MLP", "args": [8, [16, 3]], "kwargs": {"norm_layer": "BatchNorm1d"}, "inputs": ["rows"]},
    "mlp_layernorm_squared_relu": {"cls": "MLP", "args": [8, [16, 3]],
                                   "kwargs": {"norm_layer": "LayerNorm", "activation_fn": "squared_relu", "bias": False},
                                   "inputs": ["rows"]},
}


def build_module(namespace, spec: dict) -> nn.Module:
    """The module a spec describes, from ``namespace`` (the reference's ``rl8.nn`` here)."""
    kwargs = dict(spec["kwargs"])
    if "norm_layer" in kwargs:
        kwargs["norm_layer"] = getattr(nn, kwargs["norm_layer"])
    args = list(spec["args"])
    if "wraps" in spec:
        args.insert(0, namespace.SelfAttention(*spec["wraps"]["args"], **spec["wraps"]["kwargs"]))
    module = getattr(namespace, spec["cls"])(*args, **kwargs)
    if "append" in spec:
        module.append(nn.Linear(*spec["append"]))
    return module


def module_inputs() -> dict[str, torch.Tensor]:
    gen = torch.Generator().manual_seed(7)
    padding = torch.tensor([[True, True, False, False, False], [False] * 5, [True, False, False, False, False]])
    return {
        "seq": torch.randn(3, 5, 8, generator=gen),
        "seq2": torch.randn(3, 5, 8, generator=gen),
        "query": torch.randn(3, 2, 8, generator=gen),
        "rows": torch.randn(6, 8, generator=gen),
        "padding": padding,  # True = PADDED (torch's key_padding_mask); no sequence is padded throughout
    }


def function_cases() -> dict[str, dict]:
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 5, 3, generator=gen)
    valid = torch.tensor([[False, False, True, True, True], [True] * 5, [False] * 5, [True, False, True, False, True]])
    logits = torch.randn(4, 6, generator=gen)
    classes = torch.tensor([[True, False, True, True, False, True], [True] * 6, [False] * 6,
                            [False, False, False, False, True, False]])
    cube = torch.randn(2, 3, 4, generator=gen)
    rows = torch.tensor([[True, False, True], [True, True, False]])
    binary = valid.long()
    return {
        "binary_to_float": {"fn": "binary_mask_to_float_mask", "args": {"x": binary}},
        "float_to_binary": {"fn": "float_mask_to_binary_mask",
                            "args": {"x": torch.where(valid, 0.0, float("-inf"))}},
        "mask_from_lengths": {"fn": "mask_from_lengths", "args": {"x": x, "lengths": torch.tensor([0, 5, 2, 3])}},
        "avg_bool": {"fn": "masked_avg", "args": {"x": x, "mask": valid}, "kwargs": {"dim": 1, "keepdim": False}},
        "avg_float_keepdim": {"fn": "masked_avg", "args": {"x": x, "mask": valid.float()},
                              "kwargs": {"dim": 1, "keepdim": True}},
        "avg_none": {"fn": "masked_avg", "args": {"x": x}, "kwargs": {}},
        "max_bool": {"fn": "masked_max", "args": {"x": x, "mask": valid}, "kwargs": {"dim": 1}},
        "max_float": {"fn": "masked_max", "args": {"x": x, "mask": valid.float()}, "kwargs": {}},
        "max_none": {"fn": "masked_max", "args": {"x": x}, "kwargs": {}},
        "log_softmax_bool": {"fn": "masked_log_softmax", "args": {"x": logits, "mask": classes}, "kwargs": {"dim": -1}},
        "log_softmax_float": {"fn": "masked_log_softmax", "args": {"x": logits, "mask": classes.float()}, "kwargs": {}},
        "log_softmax_none": {"fn": "masked_log_softmax", "args": {"x": logits}, "kwargs": {}},
        "log_softmax_rows_of_a_cube": {"fn": "masked_log_softmax", "args": {"x": cube, "mask": rows}, "kwargs": {"dim": 1}},
        "sample_bool": {"fn": "masked_categorical_sample", "args": {"x": logits, "mask": classes}, "kwargs": {"dim": 1},
                        "seed": 5},
        "sample_none": {"fn": "masked_categorical_sample", "args": {"x": logits}, "kwargs": {}, "seed": 6},
        "skip_residual": {"fn": "skip_connection", "args": {"x": x, "y": x.flip(0)}, "kwargs": {"kind": "residual"}},
        "skip_cat": {"fn": "skip_connection", "args": {"x": x, "y": x.flip(0)}, "kwargs": {"kind": "cat", "dim": -1}},
        "skip_none": {"fn": "skip_connection", "args": {"x": x, "y": x.flip(0)}, "kwargs": {"kind": None}},
    }


POSITIONAL = ("x", "y", "lengths")


def call_function(namespace, case: dict):
    """``case`` evaluated with the functions of ``namespace``: a tuple of tensors."""
    args = case["args"]
    if "seed" in case:
        torch.manual_seed(case["seed"])
    out = getattr(namespace, case["fn"])(*(args[k] for k in POSITIONAL if k in args),
                                         **{k: v for k, v in args.items() if k not in POSITIONAL}, **case.get("kwargs", {}))
    return out if isinstance(out, tuple) else (out,)


def main() -> None:
    sys.path.insert(0, HERE)
    import generate_fixtures as gf  # imports the reference (and the stubs it needs)
    import rl8.nn as ref_nn
    import rl8.nn.functional as ref_f

    arrays: dict = {}
    cases = function_cases()
    arrays["function_cases"] = list(cases)
    for name, case in cases.items():
        spec = {k: case[k] for k in ("fn", "kwargs", "seed") if k in case}
        arrays[f"f_{name}_spec"] = json.dumps(spec)
        for key, value in case["args"].items():
            arrays[f"f_{name}_arg_{key}"] = value
        for i, out in enumerate(call_function(ref_f, case)):
            arrays[f"f_{name}_out{i}"] = out

    inputs = module_inputs()
    arrays["module_cases"] = list(MODULE_SPECS)
    for name, spec in MODULE_SPECS.items():
        torch.manual_seed(100 + len(name))
        module = build_module(ref_nn, spec)
        state = {k: v.clone() for k, v in module.state_dict().items()}  # (before forward: BatchNorm updates its buffers)
        arrays[f"m_{name}_spec"] = json.dumps(spec)
        arrays[f"m_{name}_sd_names"] = list(state)
        for i, value in enumerate(state.values()):
            arrays[f"m_{name}_sd_{i}"] = value
        for i, key in enumerate(spec["inputs"]):
            arrays[f"m_{name}_in{i}"] = inputs[key]
        out = module(*(inputs[key] for key in spec["inputs"]))
        assert torch.isfinite(out).all(), name
        arrays[f"m_{name}_out"] = out
        print(f"{name}: {len(state)} tensors, out {tuple(out.shape)}")
    gf.save("nn_reference.npz", **arrays)


if __name__ == "__main__":
    main()
