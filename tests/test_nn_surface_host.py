"""The ``rl8_amd.nn`` surface without a GPU: the reference's 21 names; the eight mask / masked / skip functions and
the eleven modules on CPU tensors against the reference's own outputs (``tests/golden/nn_reference.npz``; generator:
``tests/golden/generate_nn_fixtures.py``); ``TransformerTrader`` built on specs alone and loading the reference's
``AttentiveAlpaca`` state dict; the ``rl8_masked_*`` entries exported, bound and refusing bad arguments before any
launch; their kernels compiled for gfx950 without scratch, stack or LDS.

The functions and modules run the same torch ops on the same library as the generator did, so the bar is
``rtol=1e-6, atol=1e-7``: the margin is for GEMM threading only."""

import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import rl8_amd.nn
from rl8_amd import hip, models
from rl8_amd.data import DataKeys
from rl8_amd.envs import AlgoTrading, TransformerTrader
from rl8_amd.nn import functional as F
from rl8_amd.views import ViewRequirement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIXTURE = "nn_reference.npz"
REFERENCE_NAMES = [
    "MLP", "CrossAttention", "Module", "PerceiverIOLayer", "PerceiverLayer", "PositionalEmbedding", "SelfAttention",
    "SelfAttentionStack", "SequentialSkipConnection", "SquaredReLU", "binary_mask_to_float_mask",
    "float_mask_to_binary_mask", "generalized_advantage_estimate", "get_activation", "mask_from_lengths", "masked_avg",
    "masked_categorical_sample", "masked_log_softmax", "masked_max", "ppo_losses", "skip_connection",
]
FUNCTION_CASES = [
    "binary_to_float", "float_to_binary", "mask_from_lengths", "avg_bool", "avg_float_keepdim", "avg_none", "max_bool",
    "max_float", "max_none", "log_softmax_bool", "log_softmax_float", "log_softmax_none", "log_softmax_rows_of_a_cube",
    "sample_bool", "sample_none", "skip_residual", "skip_cat", "skip_none",
]
MODULE_CASES = [
    "self_attention_residual", "self_attention_cat", "self_attention_none", "cross_attention", "stack_shared",
    "stack_unshared", "perceiver", "perceiver_io", "positional_embedding", "skip_cat_appended", "skip_residual_appended",
    "mlp_plain", "mlp_batchnorm", "mlp_layernorm_squared_relu",
]
ENTRIES = ("rl8_masked_rows_route", "rl8_masked_pool_f32", "rl8_masked_pool_backward_f32", "rl8_masked_log_softmax_f32",
           "rl8_masked_log_softmax_backward_f32", "rl8_masked_categorical_sample_f32")
POSITIONAL = ("x", "y", "lengths")


def close(got, want, what):
    torch.testing.assert_close(got, torch.from_numpy(want), rtol=1e-6, atol=1e-7, equal_nan=True, msg=lambda m: f"{what}: {m}")


# --- the surface --------------------------------------------------------------------------------------------------
def test_nn_exports_the_reference_s_names():
    assert len(REFERENCE_NAMES) == 21 and set(rl8_amd.nn.__all__) == set(REFERENCE_NAMES)
    for name in REFERENCE_NAMES:
        assert hasattr(rl8_amd.nn, name), name
    assert models.MLP is rl8_amd.nn.MLP and models.get_activation is rl8_amd.nn.get_activation


def test_fixture_holds_the_cases_listed_here(golden):
    g = golden(FIXTURE)
    assert list(g["function_cases"]) == FUNCTION_CASES and list(g["module_cases"]) == MODULE_CASES
    assert {json.loads(str(g[f"f_{c}_spec"]))["fn"] for c in FUNCTION_CASES} == {
        "binary_mask_to_float_mask", "float_mask_to_binary_mask", "mask_from_lengths", "masked_avg",
        "masked_categorical_sample", "masked_log_softmax", "masked_max", "skip_connection"}


@pytest.mark.parametrize("case", FUNCTION_CASES)
def test_function_matches_the_reference_on_cpu(golden, case):
    g = golden(FIXTURE)
    spec = json.loads(str(g[f"f_{case}_spec"]))
    prefix = f"f_{case}_arg_"
    args = {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}
    if "seed" in spec:  # (the draw is torch's own on the CPU, as in the reference)
        torch.manual_seed(spec["seed"])
    out = getattr(F, spec["fn"])(*(args[k] for k in POSITIONAL if k in args),
                                 **{k: v for k, v in args.items() if k not in POSITIONAL}, **spec.get("kwargs", {}))
    out = out if isinstance(out, tuple) else (out,)
    want = [g[f"f_{case}_out{i}"] for i in range(len(out))]
    assert f"f_{case}_out{len(out)}" not in g
    for i, (o, w) in enumerate(zip(out, want)):
        assert o.dtype == torch.from_numpy(w).dtype and o.shape == w.shape, (case, i, o.dtype, o.shape)
        close(o, w, f"{case} output {i}")


def test_fully_padded_rows_are_in_the_fixture(golden):
    g = golden(FIXTURE)
    assert np.isnan(g["f_avg_bool_out0"][2]).all() and np.isfinite(g["f_avg_bool_out0"][[0, 1, 3]]).all()
    np.testing.assert_allclose(g["f_log_softmax_bool_out0"][2], -np.log(6.0), rtol=1e-6)  # (uniform, not NaN)


def build_module(spec):
    """``generate_nn_fixtures.build_module`` with ``rl8_amd.nn`` as the namespace."""
    kwargs = dict(spec["kwargs"])
    if "norm_layer" in kwargs:
        kwargs["norm_layer"] = getattr(nn, kwargs["norm_layer"])
    args = list(spec["args"])
    if "wraps" in spec:
        args.insert(0, rl8_amd.nn.SelfAttention(*spec["wraps"]["args"], **spec["wraps"]["kwargs"]))
    module = getattr(rl8_amd.nn, spec["cls"])(*args, **kwargs)
    if "append" in spec:
        module.append(nn.Linear(*spec["append"]))
    return module


@pytest.mark.parametrize("case", MODULE_CASES)
def test_module_loads_the_reference_s_state_dict_and_reproduces_its_output(golden, case):
    g = golden(FIXTURE)
    spec = json.loads(str(g[f"m_{case}_spec"]))
    module = build_module(spec)
    assert isinstance(module, rl8_amd.nn.Module) and isinstance(module, nn.Module)
    names = [str(n) for n in g[f"m_{case}_sd_names"]]
    assert list(module.state_dict()) == names  # (the reference's names, in its order)
    module.load_state_dict({n: torch.from_numpy(g[f"m_{case}_sd_{i}"]) for i, n in enumerate(names)}, strict=True)
    inputs = [torch.from_numpy(g[f"m_{case}_in{i}"]) for i in range(len(spec["inputs"]))]
    close(module(*inputs), g[f"m_{case}_out"], case)


def test_shared_stack_is_one_module_and_unshared_are_copies():
    shared = rl8_amd.nn.SelfAttentionStack(rl8_amd.nn.SelfAttention(8), 3, share_parameters=True)
    assert all(layer is shared.layers[0] for layer in shared.layers) and len(list(shared.parameters())) == 16
    copies = rl8_amd.nn.SelfAttentionStack(rl8_amd.nn.SelfAttention(8), 2)
    assert copies.layers[0] is not copies.layers[1] and len(list(copies.parameters())) == 32


def test_skip_connection_refuses_an_unknown_kind():
    x = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="No skip connection type"):
        F.skip_connection(x, x, kind="sum")
    with pytest.raises(ValueError, match="No skip connection type"):
        rl8_amd.nn.SequentialSkipConnection(8, kind="sum").out_features


def test_squared_relu_and_the_activation_registry():
    x = torch.tensor([-2.0, 0.0, 3.0])
    assert torch.equal(rl8_amd.nn.SquaredReLU()(x), torch.tensor([0.0, 0.0, 9.0]))
    assert isinstance(rl8_amd.nn.get_activation("squared_relu"), rl8_amd.nn.SquaredReLU)
    assert isinstance(rl8_amd.nn.get_activation("leaky_relu", negative_slope=0.2), nn.LeakyReLU)


def test_masked_functions_keep_the_torch_route_off_the_gpu():
    """CPU tensors never reach a kernel wrapper (those refuse them): the functions are differentiable there."""
    x = torch.randn(3, 4, 2, requires_grad=True)
    mask = torch.tensor([[False, True, True, True]] * 3)
    F.masked_avg(x, mask=mask).sum().backward()
    assert torch.equal(x.grad[:, 0], torch.zeros(3, 2)) and torch.allclose(x.grad[:, 1:], torch.full((3, 3, 2), 1 / 3))
    values, index = F.masked_categorical_sample(torch.randn(5, 4), mask=mask[0].expand(5, 4),
                                                noise=torch.rand(5, 4) + 0.1)
    assert values.shape == index.shape == (5, 1) and (index > 0).all()


# --- TransformerTrader --------------------------------------------------------------------------------------------
def test_transformer_trader_builds_on_specs_and_loads_the_reference_s_state_dict(golden):
    env = AlgoTrading(4, device="cpu")
    model = TransformerTrader(env.observation_spec, env.action_spec)
    key = (DataKeys.OBS, "LOG_CHANGE(price)")
    assert set(model.view_requirements) == {DataKeys.OBS, key}
    assert isinstance(model.view_requirements[key], ViewRequirement) and model.view_requirements[key].shift == 4
    assert model.config == dict(invested_embed_dim=2, price_embed_dim=8, seq_len=4, num_heads=4, num_layers=2,
                                hiddens=(64, 64), activation_fn="relu")
    g = golden("first_update_ff_algotrading_transformer.npz")
    init = {k[len("init_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init_")}
    assert list(model.state_dict()) == list(init) and sum(v.numel() for v in init.values()) == 13482
    assert "price_attention.layers.1.skip_connection._layers.1.4.weight" in init
    model.load_state_dict(init, strict=True)
    assert model.price_attention.layers[0] is model.price_attention.layers[1]


# --- the C entries ------------------------------------------------------------------------------------------------
def test_masked_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert hip.ABI_VERSION == 107  # (new entries only: no bump)


def test_masked_rows_route():
    lib = hip.load()
    assert lib.rl8_masked_rows_route(1) == hip.MASKED_ROWS_LANE == 0
    assert lib.rl8_masked_rows_route(64) == hip.MASKED_ROWS_LANE
    assert lib.rl8_masked_rows_route(65) == hip.MASKED_ROWS_WAVE == 1
    assert lib.rl8_masked_rows_route(0) == -2 and lib.rl8_masked_rows_route(-5) == -2
    assert hip.masked_rows_route(1000) == hip.MASKED_ROWS_WAVE
    with pytest.raises(ValueError):
        hip.masked_rows_route(0)


def test_masked_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p, q, r = 4096, 8192, 12288  # (never dereferenced: every call fails its checks first)
    avg, mx = hip.POOL_AVG, hip.POOL_MAX
    pool, pool_b = lib.rl8_masked_pool_f32, lib.rl8_masked_pool_backward_f32
    lsm, lsm_b, draw = (lib.rl8_masked_log_softmax_f32, lib.rl8_masked_log_softmax_backward_f32,
                        lib.rl8_masked_categorical_sample_f32)
    # RL8_ENULL: a required pointer; the indices in MAX mode only; the mask and the noise are optional
    assert pool(None, None, 8, 5, 3, avg, q, None, None) == -1
    assert pool(p, None, 8, 5, 3, avg, None, None, None) == -1
    assert pool(p, None, 8, 5, 3, mx, q, None, None) == -1
    assert pool_b(None, None, None, 8, 5, 3, avg, q, None) == -1
    assert pool_b(p, None, None, 8, 5, 3, avg, None, None) == -1
    assert pool_b(p, None, None, 8, 5, 3, mx, q, None) == -1
    assert lsm(None, None, 8, 3, q, None) == -1 and lsm(p, None, 8, 3, None, None) == -1
    assert lsm_b(None, q, 8, 3, r, None) == -1 and lsm_b(p, None, 8, 3, r, None) == -1
    assert lsm_b(p, q, 8, 3, None, None) == -1
    assert draw(None, None, None, 8, 3, 0, 0, 0, q, r, None) == -1
    assert draw(p, None, None, 8, 3, 0, 0, 0, None, r, None) == -1
    assert draw(p, None, None, 8, 3, 0, 0, 0, q, None, None) == -1
    # RL8_ESIZE: rows, t, e, k < 1
    for rows, t, e in ((0, 5, 3), (-1, 5, 3), (8, 0, 3), (8, 5, 0), (8, -2, 3)):
        for mode in (avg, mx):
            assert pool(p, None, rows, t, e, mode, q, r, None) == -2, (rows, t, e)
            assert pool_b(p, None, r, rows, t, e, mode, q, None) == -2, (rows, t, e)
    for rows, k in ((0, 3), (8, 0), (-1, 3), (8, -1)):
        assert lsm(p, None, rows, k, q, None) == -2
        assert lsm_b(p, q, rows, k, r, None) == -2
        assert draw(p, None, None, rows, k, 0, 0, 0, q, r, None) == -2
    # RL8_ECONFIG: an unknown mode
    for mode in (-1, 2, 7):
        assert pool(p, None, 8, 5, 3, mode, q, r, None) == -4
        assert pool_b(p, None, r, 8, 5, 3, mode, q, None) == -4
    # RL8_EALIGN: floats off 4 bytes, indices off 8
    assert pool(p + 2, None, 8, 5, 3, avg, q, None, None) == -3 and pool(p, None, 8, 5, 3, avg, q + 1, None, None) == -3
    assert pool(p, None, 8, 5, 3, mx, q, r + 4, None) == -3
    assert pool_b(p + 2, None, None, 8, 5, 3, avg, q, None) == -3 and pool_b(p, None, None, 8, 5, 3, avg, q + 3, None) == -3
    assert pool_b(p, None, r + 4, 8, 5, 3, mx, q, None) == -3
    assert lsm(p + 1, None, 8, 3, q, None) == -3 and lsm(p, None, 8, 3, q + 2, None) == -3
    assert lsm_b(p + 2, q, 8, 3, r, None) == -3 and lsm_b(p, q + 2, 8, 3, r, None) == -3
    assert lsm_b(p, q, 8, 3, r + 2, None) == -3
    assert draw(p + 2, None, None, 8, 3, 0, 0, 0, q, r, None) == -3
    assert draw(p, None, p + 2, 8, 3, 0, 0, 0, q, r, None) == -3
    assert draw(p, None, None, 8, 3, 0, 0, 0, q + 2, r, None) == -3
    assert draw(p, None, None, 8, 3, 0, 0, 0, q, r + 4, None) == -3


def test_wrappers_refuse_host_tensors():
    with pytest.raises(hip.HipExtensionError):
        hip.masked_pool(torch.zeros(2, 3, 4), None, hip.POOL_AVG)
    with pytest.raises(hip.HipExtensionError):
        hip.masked_log_softmax(torch.zeros(2, 3), None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_masked_kernels_compile_without_scratch_stack_or_lds(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "masked.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "masked_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    wanted = ("masked_avg_kernel", "masked_avg_backward_kernel", "masked_max_kernel", "masked_max_backward_kernel",
              "masked_log_softmax_lane_kernel", "masked_log_softmax_wave_kernel", "masked_log_softmax_backward_lane_kernel",
              "masked_log_softmax_backward_wave_kernel", "masked_sample_lane_kernel", "masked_sample_wave_kernel")
    assert len(kernels) == len(wanted) and all(any(w in name for name in kernels) for w in wanted), sorted(kernels)
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name
