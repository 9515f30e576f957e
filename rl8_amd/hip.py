"""ctypes binding of ``librl8_amd.so`` (the gfx950 kernels behind
``include/rl8_amd.h``) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the stream. Every wrapper
passes ``tensor.data_ptr()`` and the current HIP stream to the C ABI, checks the
integer status, and returns. Nothing synchronises.

There is NO CPU fallback: if the shared library is missing, or a tensor is not
on a HIP device, the call raises.

"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Any, NamedTuple, Sequence

import torch

_LIB_NAME = "librl8_amd.so"
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)
# Kernel-tuning runs point this at an experimental build of the SAME ABI
# (tools/diag_mlp.sh); there is still no fallback if the file is missing.
_LIB_PATH = os.environ.get("RL8_AMD_LIBRARY", _LIB_PATH)
_lib: None | C.CDLL = None

_ERRORS = {
    -1: "required pointer is NULL",
    -2: "size / shape argument out of range",
    -3: "pointer not aligned as required",
    -4: "unsupported combination of options",
}

MAX_CLASSES = 64
MAX_WIDE_CLASSES = 65536  # RL8_MAX_WIDE_CLASSES: the wave-per-row categorical kernels
MAX_GATHER_FIELDS = 8
LAYOUT_ENV_MAJOR = 0
LAYOUT_TIME_MAJOR = 1
POOL_AVG, POOL_MAX = 0, 1  # RL8_POOL_*
MASKED_ROWS_LANE, MASKED_ROWS_WAVE = 0, 1  # RL8_MASKED_ROWS_*


class HipExtensionError(RuntimeError):
    """The HIP extension is missing or a kernel launch failed."""


class CartPoleCfg(C.Structure):
    _fields_ = [
        ("force_mag", C.c_float),
        ("gravity", C.c_float),
        ("length", C.c_float),
        ("pole_mass", C.c_float),
        ("pole_mass_length", C.c_float),
        ("total_mass", C.c_float),
        ("tau", C.c_float),
        ("semi_implicit", C.c_int32),
    ]


class MountainCarCfg(C.Structure):
    """``rl8_mountain_car_cfg`` (include/rl8_amd.h)."""

    _fields_ = [(name, C.c_float) for name in ("force_mag", "goal_position", "goal_velocity", "gravity",
                                               "max_position", "max_speed", "min_position")]


class PendulumCfg(C.Structure):
    """``rl8_pendulum_cfg`` (include/rl8_amd.h)."""

    _fields_ = [(name, C.c_float) for name in ("dt", "gravity_coeff", "torque_coeff", "max_speed", "max_torque")]



class PPOHparams(C.Structure):
    _fields_ = [
        ("clip_param", C.c_float),
        ("dual_clip_param", C.c_float),
        ("entropy_coeff", C.c_float),
        ("vf_clip_param", C.c_float),
        ("vf_coeff", C.c_float),
        ("grad_scale", C.c_float),
    ]


class GatherField(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("env_stride", C.c_int64),
        ("time_stride", C.c_int64),
        ("row_elems", C.c_int32),
        ("elem_bytes", C.c_int32),
    ]


class WindowField(C.Structure):
    """``rl8_window_field`` (include/rl8_amd.h)."""

    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("mask", C.c_void_p),
        ("env_stride", C.c_int64),
        ("time_stride", C.c_int64),
        ("row_elems", C.c_int32),
        ("elem_bytes", C.c_int32),
        ("size", C.c_int32),
    ]


class ScatterLeaf(C.Structure):
    """``rl8_scatter_leaf`` (include/rl8_amd.h)."""

    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64)]


class GaePlanStruct(C.Structure):
    """``rl8_gae_plan_t`` (include/rl8_amd.h)."""

    _fields_ = [("route", C.c_int), ("envs_per_block", C.c_int), ("chunk", C.c_int), ("lds_stride", C.c_int),
                ("lds_bytes", C.c_int64), ("grid", C.c_int)]


class StatsPlanStruct(C.Structure):
    """``rl8_stats_plan_t`` (include/rl8_amd.h)."""

    _fields_ = [("route", C.c_int), ("grid", C.c_int), ("trips", C.c_int64)]


class PackPlanStruct(C.Structure):
    """``rl8_pack_plan_t`` (include/rl8_amd.h)."""

    _fields_ = [("tile_steps", C.c_int), ("lds_bytes", C.c_int), ("tiles", C.c_int64), ("grid", C.c_int)]


_vp, _i64, _u64, _i32, _f32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_float

# name -> argtypes, mirroring include/rl8_amd.h one to one.
SIGNATURES: dict[str, list[Any]] = {
    "rl8_abi_version": [C.c_char_p, _i32],
    "rl8_pw_max_breaks": [],
    "rl8_pw_workspace_bytes": [_i32, _i32],
    "rl8_pw_tower_forward_f32": [_vp, _i64, _vp, _i32, _i32, _vp, _vp],
    "rl8_pw_segment_sums_f32": [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp],
    "rl8_scratch_bytes": [],
    "rl8_dummy_env_step_f32": [_vp, _vp, _i32, _vp, _i64, _vp],
    "rl8_dummy_env_reset_f32": [_vp, _i64, _f32, _u64, _u64, _i64, _vp],
    "rl8_cartpole_step_f32": [_vp, _vp, C.POINTER(CartPoleCfg), _vp, _i64, _vp, _i64, _vp],
    "rl8_cartpole_reset_f32": [_vp, _i64, _f32, _u64, _u64, _i64, _vp, _i64, _vp],
    "rl8_categorical_sample_logp_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _u64, _u64, _i64, _i32, _vp],
    "rl8_categorical_wide_sample_logp_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _u64, _u64, _i64, _i32, _vp],
    "rl8_normal_sample_logp_f32": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _u64, _u64, _i64, _i32, _vp],
    "rl8_rollout_scatter_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _vp],
    "rl8_rollout_scatter_leaves_f32": [_vp, _i64, _vp, _vp, _vp, C.POINTER(ScatterLeaf), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _f32,
                                       _i64, _vp],
    "rl8_algotrading_reset_f32": [_vp, _i64, _f32, _f32, _f32, _u64, _u64, _i64, _vp, _vp, _vp, _vp, _vp],
    "rl8_algotrading_step_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "rl8_rollout_step_algotrading_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64,
                                         _u64, _i64, _i32, _vp],
    "rl8_rollout_step_dummy_f32": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64, _u64, _i64, _i32, _vp],
    "rl8_rollout_step_dummy_heads_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64,
                                         _u64, _i64, _i32, _vp],
    "rl8_rollout_step_dummy_heads_narrow_f32": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32,
                                                _i64, _u64, _u64, _i64, _i32, _vp],
    "rl8_mountain_car_step_f32": [_vp, _vp, C.POINTER(MountainCarCfg), _vp, _i64, _vp, _i64, _vp],
    "rl8_mountain_car_reset_f32": [_vp, _i64, _u64, _u64, _i64, _vp, _i64, _vp],
    "rl8_rollout_step_mountain_car_f32": [_vp, _vp, _vp, _vp, C.POINTER(MountainCarCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64, _u64, _i64, _i32, _vp],
    "rl8_pendulum_step_f32": [_vp, _vp, C.POINTER(PendulumCfg), _vp, _i64, _vp, _i64, _vp],
    "rl8_pendulum_reset_f32": [_vp, _i64, _u64, _u64, _i64, _vp, _i64, _vp],
    "rl8_rollout_step_pendulum_f32": [_i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(PendulumCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64, _u64, _i64, _i32, _vp],
    "rl8_rollout_step_cartpole_f32": [_vp, _vp, _vp, _vp, C.POINTER(CartPoleCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _u64, _u64, _i64, _i32, _vp],
    "rl8_rollout_stats_f32": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "rl8_rollout_stats_plan": [_i64, _i64, _i64, _i64, _i32, C.POINTER(StatsPlanStruct)],
    "rl8_gae_scan_f32": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _f32, _f32, _f32, _i32, _vp, _vp, _vp],
    "rl8_advantage_normalise_f32": [_vp, _i64, _i64, _i32, _vp, _vp],
    "rl8_gae_plan": [_i64, _i64, _i32, _i32, C.POINTER(GaePlanStruct)],
    "rl8_advantage_normalise_route": [_i64, _i64, _i32, _i32],
    "rl8_ppo_loss_categorical_fwd_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, C.POINTER(PPOHparams), _vp, _vp, _vp, _vp, _vp],
    "rl8_ppo_loss_categorical_wide_fwd_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, C.POINTER(PPOHparams), _vp, _vp, _vp,
                                                  _vp, _vp],
    "rl8_ppo_loss_normal_fwd_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, C.POINTER(PPOHparams), _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_gather_minibatch": [_vp, _i64, _i64, C.POINTER(GatherField), _i32, _vp],
    "rl8_gather_minibatch_plan": [_i32, _i64, _i64, C.POINTER(GatherField), _i32, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)],
    "rl8_gather_sequences": [_vp, _i64, _i32, _i64, C.POINTER(GatherField), _i32, _vp],
    "rl8_gather_windows": [_vp, _i64, _i64, C.POINTER(WindowField), _i32, _vp],
    "rl8_window_last": [_i64, _i64, C.POINTER(WindowField), _i32, _vp],
    "rl8_masked_rows_route": [_i32],
    "rl8_masked_pool_f32": [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp],
    "rl8_masked_pool_backward_f32": [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "rl8_masked_log_softmax_f32": [_vp, _vp, _i64, _i32, _vp, _vp],
    "rl8_masked_log_softmax_backward_f32": [_vp, _vp, _i64, _i32, _vp, _vp],
    "rl8_masked_categorical_sample_f32": [_vp, _vp, _vp, _i64, _i32, _u64, _u64, _i64, _vp, _vp, _vp],
    "rl8_attention_supports": [_i32, _i32, _i32, _i32],
    "rl8_attention_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "rl8_attention_backward_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp,
                                   _i64, _vp, _vp, _i64, _vp, _vp],
    "rl8_feedforward_supports": [_i32, _i32],
    "rl8_feedforward_limits": [C.POINTER(C.c_int)],
    "rl8_feedforward_workspace_floats": [_i64, _i32, _i32],
    "rl8_feedforward_f32": [_vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "rl8_feedforward_backward_f32": [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp],
    "rl8_pack_samples": [_vp, _i32, _i64, _i64, _vp, _i32, _vp],
    "rl8_gather_packed": [_vp, _i64, _vp, _i32, _vp, _i32, _vp],
    "rl8_pack_plan": [_i64, _i64, _i32, C.POINTER(PackPlanStruct)],
    "rl8_lstm_supports": [_i32],
    "rl8_lstm_pack_floats": [],
    "rl8_lstm_pack_f32": [_vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "rl8_lstm_forward_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_split_supports": [_i32],
    "rl8_lstm_split_packed_bytes": [],
    "rl8_lstm_split_wb_floats": [],
    "rl8_lstm_split_state_bytes": [_i64],
    "rl8_lstm_pack_split": [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "rl8_lstm_split_state": [_vp, _i64, _i64, _vp, _vp],
    "rl8_lstm_split_state_bound": [_vp, _i64, _i64, _vp, _vp, _vp],
    "rl8_lstm_step_split_f32": [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    "rl8_lstm_rows_backward_pack_bytes": [],
    "rl8_lstm_rows_backward_pack": [_vp, _vp, _vp],
    "rl8_lstm_rows_backward_f32": [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_rows_backward_heads_f32": [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_mlp_wgrad_f16_strided_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, C.POINTER(C.c_int), _vp],
    "rl8_lstm_wgrad_f16_f32": [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, C.POINTER(C.c_int), _vp],
    "rl8_lstm_backward_partial_floats": [_i32],
    "rl8_lstm_backward_max_rows": [],
    "rl8_lstm_backward_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int), _vp],
    "rl8_lstm_backward_dgates_f32": [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_wide_in_supports": [_i32],
    "rl8_lstm_wide_in_lds_bytes": [_i32, _i32],
    "rl8_lstm_wide_in_pack_floats": [_i32],
    "rl8_lstm_wide_in_pack_f32": [_vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "rl8_lstm_wide_in_forward_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_wide_in_workspace_bytes": [_i32],
    "rl8_lstm_wide_in_wgrad_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack256_supports": [],
    "rl8_lstm_stack256_lds_bytes": [_i32],
    "rl8_lstm_stack256_pack_floats": [],
    "rl8_lstm_stack256_pack_f32": [_vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack256_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack256_workspace_bytes": [_i64],
    "rl8_lstm_stack256_dx_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "rl8_linear_heads_max_rows": [],
    "rl8_linear_heads_forward_f32": [_vp, _i64, _vp, _vp, _i32, _vp, _vp],
    "rl8_linear_heads_forward_pair_f32": [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
    "rl8_linear_heads_backward_f32": [_vp, _vp, _i64, _vp, _i32, _vp, _vp, C.POINTER(C.c_int), _vp],
    "rl8_mlp_wgrad_strided_f32": [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp],
    "rl8_mlp_wgrad_split_strided_f32": [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _i32, _vp, C.POINTER(C.c_int), _vp],
    "rl8_mlp_pack_w2_f32": [_vp, _vp, _i32, _vp],
    "rl8_mlp_tower_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_backward_partial_floats": [_i32, _i32],
    "rl8_mlp_backward_max_rows": [],
    "rl8_mlp_tower_backward_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, C.POINTER(C.c_int), _vp],
    "rl8_mlp_backward_f16_supports": [_i32, _i32],
    "rl8_mlp_tower_backward_f16_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, C.POINTER(C.c_int), _vp, _vp],
    "rl8_mlp_dout_pair_check": [_vp, _i64, _vp, _vp],
    "rl8_mlp_wgrad_fused_pair_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_pack_w2_f16_gate": [_vp, _vp, _i32, _vp, _vp],
    "rl8_mlp_tower_backward_gate_f16_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, C.POINTER(C.c_int), _vp, _vp],
    "rl8_mlp_wgrad_gate_bits_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_f16_packed_bytes": [],
    "rl8_mlp_forward_f16_supports": [_i32, _i32],
    "rl8_mlp_pack_w2_f16": [_vp, _i32, _vp, _vp],
    "rl8_mlp_tower_forward_f16_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    "rl8_mlp_wgrad_split_f32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "rl8_mlp_wgrad_fused_split_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_wgrad_workspace_bytes": [],
    "rl8_mlp_wgrad_f32": [_vp, _vp, _i64, _vp, _vp, _i32, _vp],
    "rl8_mlp_narrow_supports": [_i32, _i32, _i32],
    "rl8_mlp_narrow_workspace_bytes": [_i64, _i32, _i32, _i32],
    "rl8_mlp_narrow_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "rl8_mlp_narrow_backward_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "rl8_mlp_narrow_reduce_f32": [_vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "rl8_mlp_narrow_backward_dx_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "rl8_mlp_wide_in_supports": [_i32, _i32],
    "rl8_mlp_wide_in_lds_bytes": [_i32, _i32],
    "rl8_mlp_wide_in_pack_floats": [_i32],
    "rl8_mlp_wide_in_pack_w1_f32": [_vp, _i32, _vp, _vp],
    "rl8_mlp_wide_in_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_wide_in_partial_floats": [_i32],
    "rl8_mlp_wide_in_max_rows": [],
    "rl8_mlp_wide_in_backward_f32": [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, C.POINTER(C.c_int), _vp],
    "rl8_mlp_wide_in_workspace_bytes": [_i32],
    "rl8_mlp_wide_in_wgrad_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "rl8_mlp_wide_out_supports": [_i32, _i32],
    "rl8_mlp_wide_out_lds_bytes": [_i32, _i32],
    "rl8_mlp_wide_out_pack_floats": [_i32, _i32],
    "rl8_mlp_wide_out_pack_f32": [_vp, _i32, _i32, _vp, _vp],
    "rl8_mlp_wide_out_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "rl8_mlp_wide_out_partial_floats": [_i32],
    "rl8_mlp_wide_out_max_rows": [],
    "rl8_mlp_wide_out_backward_f32": [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, C.POINTER(C.c_int), _vp],
    "rl8_mlp_wide_out_workspace_bytes": [_i32],
    "rl8_mlp_wide_out_wgrad_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp],
    "rl8_tower_limits": [C.POINTER(C.c_int)],
    "rl8_tower_moments_workspace_bytes": [_i64, _i32],
    "rl8_tower_moments_f64": [_vp, _i64, _i32, _vp, _vp, _vp, _vp],
    "rl8_batchnorm_fold_f32": [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, C.c_double, _vp,
                               _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_narrow_supports": [_i32, _i32],
    "rl8_lstm_narrow_workspace_bytes": [_i64, _i32, _i32, _i32],
    "rl8_lstm_narrow_forward_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                    _vp],
    "rl8_lstm_narrow_backward_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_narrow_reduce_f32": [_vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "rl8_lstm_narrow_backward_heads_f32": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_narrow_input_grad_f32": [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp],
    "rl8_linear_heads_narrow_workspace_bytes": [_i64, _i32, _i32],
    "rl8_linear_heads_narrow_forward_f32": [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp],
    "rl8_linear_heads_narrow_forward_pair_f32": [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
    "rl8_linear_heads_narrow_backward_f32": [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack_supports": [_i32],
    "rl8_lstm_stack_workspace_bytes": [_i64, _i32, _i32],
    "rl8_lstm_stack_forward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack_backward_f32": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rl8_lstm_stack_reduce_f32": [_vp, _i64, _i32, _i32, _vp, _vp],
}


#: RL8_ABI_VERSION of include/rl8_amd.h this binding is written against (checked against the library in ``load``).
ABI_VERSION = 107


def library_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the extension (after torch, so that the HIP runtime torch already
    mapped -- soname ``libamdhip64.so.7`` -- is the one the kernels launch on)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise HipExtensionError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import"
                " __graft_entry__ as g; g.build()'` (or `make -C rl8_amd/csrc`)."
                " rl8_amd has no CPU fallback."
            )
        lib = C.CDLL(_LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = (
                C.c_int64
                if name in ("rl8_scratch_bytes", "rl8_mlp_backward_partial_floats", "rl8_mlp_wgrad_workspace_bytes",
                            "rl8_lstm_pack_floats", "rl8_lstm_backward_partial_floats",
                            "rl8_lstm_split_packed_bytes", "rl8_lstm_split_wb_floats", "rl8_lstm_split_state_bytes",
                            "rl8_mlp_f16_packed_bytes", "rl8_lstm_rows_backward_pack_bytes", "rl8_pw_workspace_bytes",
                            "rl8_mlp_narrow_workspace_bytes", "rl8_lstm_narrow_workspace_bytes",
                            "rl8_lstm_stack_workspace_bytes", "rl8_linear_heads_narrow_workspace_bytes",
                            "rl8_feedforward_workspace_floats", "rl8_tower_moments_workspace_bytes",
                            "rl8_mlp_wide_in_pack_floats", "rl8_mlp_wide_in_partial_floats", "rl8_mlp_wide_in_lds_bytes",
                            "rl8_mlp_wide_in_workspace_bytes", "rl8_lstm_wide_in_pack_floats",
                            "rl8_mlp_wide_out_pack_floats", "rl8_mlp_wide_out_partial_floats",
                            "rl8_mlp_wide_out_lds_bytes", "rl8_mlp_wide_out_workspace_bytes",
                            "rl8_lstm_wide_in_lds_bytes", "rl8_lstm_wide_in_workspace_bytes",
                            "rl8_lstm_stack256_lds_bytes", "rl8_lstm_stack256_pack_floats",
                            "rl8_lstm_stack256_workspace_bytes")
                else C.c_int
            )
        built = int(lib.rl8_abi_version(None, 0))
        if built != ABI_VERSION:
            raise HipExtensionError(
                f"{_LIB_PATH} was built with ABI version {built}, this binding is written against {ABI_VERSION}"
                " (include/rl8_amd.h: RL8_ABI_VERSION): rebuild with `make -C rl8_amd/csrc`."
            )
        _lib = lib
    return _lib


def _check(status: int, name: str) -> None:
    if status == 0:
        return
    if status < 0:
        raise ValueError(f"{name}: {_ERRORS.get(status, 'argument check failed')} ({status})")
    raise HipExtensionError(f"{name}: HIP launch failed with hipError_t {status}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of launches, per ABI entry point. Events are
    recorded on the stream the kernel is launched on (torch's current stream);
    nothing synchronises until :meth:`summary` is called. Used by ``bench.py``
    for the roofline figures; off by default."""

    def __init__(self) -> None:
        self.enabled = False
        self.records: dict[str, list[tuple[torch.cuda.Event, torch.cuda.Event, float]]] = {}

    def reset(self) -> None:
        self.records = {}

    def summary(self) -> dict[str, dict[str, float]]:
        torch.cuda.synchronize()
        out = {}
        for name, events in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in events]
            units = [u for _, _, u in events]
            out[name] = {
                "launches": len(ms),
                "total_ms": sum(ms),
                "avg_ms": sum(ms) / len(ms),
                "units_per_launch": sum(units) / len(units),
            }
        return out


timer = KernelTimer()


class _timed:
    __slots__ = ("name", "units", "start")

    def __init__(self, name: str, units: float) -> None:
        self.name, self.units = name, units

    def __enter__(self) -> None:
        if timer.enabled:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record()

    def __exit__(self, *exc: Any) -> None:
        if timer.enabled:
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            timer.records.setdefault(self.name, []).append((self.start, end, self.units))


_UNTIMED = contextlib.nullcontext()


def _ptr(t: None | torch.Tensor) -> None | int:
    if t is None:
        return None
    if not t.is_cuda:
        raise HipExtensionError(
            "rl8_amd kernels take HIP device tensors only (got a"
            f" {t.device} tensor); there is no CPU fallback."
        )
    return t.data_ptr()


def _dense(t: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t


def _shaped(t: torch.Tensor, shape: tuple, what: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``t`` when it is a dense ``dtype`` tensor of exactly ``shape``, else an error naming it."""
    _dense(t, dtype, what)
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t


_scratch: dict[tuple[int, int], torch.Tensor] = {}


def scratch(device: torch.device) -> torch.Tensor:
    """Per (device, stream) reduction scratch, allocated once."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    buf = _scratch.get(key)
    if buf is None:
        nbytes = int(load().rl8_scratch_bytes())
        buf = torch.zeros(nbytes // 8, dtype=torch.float64, device=device)
        _scratch[key] = buf
    return buf


def abi_version() -> tuple[int, str]:
    buf = C.create_string_buffer(16)
    v = load().rl8_abi_version(buf, 16)
    return int(v), buf.value.decode()


# --------------------------------------------------------------------------- #
# Environments.
# --------------------------------------------------------------------------- #
def dummy_env_step(state: torch.Tensor, action: torch.Tensor, reward_out: torch.Tensor) -> None:
    n = state.numel()
    discrete = action.dtype == torch.int64
    if not discrete and action.dtype != torch.float32:
        raise TypeError(f"dummy env actions must be int64 or float32, got {action.dtype}")
    _dense(state, torch.float32, "state")
    _dense(reward_out, torch.float32, "reward_out")
    if action.numel() != n or reward_out.numel() != n or not action.is_contiguous():
        raise ValueError("state, action and reward_out must be dense with one element per env")
    _check(
        load().rl8_dummy_env_step_f32(_ptr(state), _ptr(action), int(discrete), _ptr(reward_out), n, _stream()),
        "rl8_dummy_env_step_f32",
    )


def dummy_env_reset(state: torch.Tensor, bounds: float, seed: int, reset_count: int, env_offset: int = 0) -> None:
    _dense(state, torch.float32, "state")
    _check(
        load().rl8_dummy_env_reset_f32(_ptr(state), state.numel(), bounds, seed, reset_count, env_offset, _stream()),
        "rl8_dummy_env_reset_f32",
    )


def cartpole_step(state: torch.Tensor, action: torch.Tensor, cfg: CartPoleCfg, obs_out: torch.Tensor, reward_out: torch.Tensor) -> None:
    _dense(state, torch.float32, "state")
    _dense(action, torch.int64, "action")
    _dense(obs_out, torch.float32, "obs_out")
    _dense(reward_out, torch.float32, "reward_out")
    n = state.shape[1]
    if state.shape[0] != 4 or action.numel() != n or obs_out.numel() != 5 * n or reward_out.numel() != n:
        raise ValueError("cartpole_step: state [4,N], action [N,1], obs_out [N,5], reward_out [N,1]")
    _check(
        load().rl8_cartpole_step_f32(_ptr(state), _ptr(action), C.byref(cfg), _ptr(obs_out), 5, _ptr(reward_out), n, _stream()),
        "rl8_cartpole_step_f32",
    )


def cartpole_reset(state: torch.Tensor, std: float, seed: int, reset_count: int, env_offset: int, obs_out: None | torch.Tensor) -> None:
    _dense(state, torch.float32, "state")
    n = state.shape[1]
    if obs_out is not None:
        _dense(obs_out, torch.float32, "obs_out")
        if obs_out.numel() != 5 * n:
            raise ValueError("obs_out must be [N,5]")
    _check(
        load().rl8_cartpole_reset_f32(_ptr(state), n, std, seed, reset_count, env_offset, _ptr(obs_out), 5, _stream()),
        "rl8_cartpole_reset_f32",
    )


def _classic_step(symbol: str, obs_dim: int, action_dtype: torch.dtype, state: torch.Tensor, action: torch.Tensor,
                  cfg: C.Structure, obs_out: torch.Tensor, reward_out: torch.Tensor) -> None:
    _dense(state, torch.float32, "state")
    _dense(action, action_dtype, "action")
    _dense(obs_out, torch.float32, "obs_out")
    _dense(reward_out, torch.float32, "reward_out")
    n = state.shape[1]
    if state.shape[0] != 2 or action.numel() != n or obs_out.numel() != obs_dim * n or reward_out.numel() != n:
        raise ValueError(f"{symbol}: state [2,N], action [N,1], obs_out [N,{obs_dim}], reward_out [N,1]")
    _check(
        getattr(load(), symbol)(_ptr(state), _ptr(action), C.byref(cfg), _ptr(obs_out), obs_dim, _ptr(reward_out), n, _stream()),
        symbol,
    )


def _classic_reset(symbol: str, obs_dim: int, state: torch.Tensor, seed: int, reset_count: int, env_offset: int,
                   obs_out: None | torch.Tensor) -> None:
    _dense(state, torch.float32, "state")
    n = state.shape[1]
    if state.shape[0] != 2:
        raise ValueError(f"{symbol}: state must be [2,N]")
    if obs_out is not None:
        _dense(obs_out, torch.float32, "obs_out")
        if obs_out.numel() != obs_dim * n:
            raise ValueError(f"obs_out must be [N,{obs_dim}]")
    _check(getattr(load(), symbol)(_ptr(state), n, seed, reset_count, env_offset, _ptr(obs_out), obs_dim, _stream()), symbol)


def mountain_car_step(state: torch.Tensor, action: torch.Tensor, cfg: MountainCarCfg, obs_out: torch.Tensor,
                      reward_out: torch.Tensor) -> None:
    """examples/mountain_car/env.py:12-38: state [2,N] in place, obs_out [N,2], reward_out [N,1]."""
    _classic_step("rl8_mountain_car_step_f32", 2, torch.int64, state, action, cfg, obs_out, reward_out)


def mountain_car_reset(state: torch.Tensor, seed: int, reset_count: int, env_offset: int, obs_out: None | torch.Tensor) -> None:
    _classic_reset("rl8_mountain_car_reset_f32", 2, state, seed, reset_count, env_offset, obs_out)


def pendulum_step(state: torch.Tensor, action: torch.Tensor, cfg: PendulumCfg, obs_out: torch.Tensor,
                  reward_out: torch.Tensor) -> None:
    """examples/pendulum/env.py:12-39: state [2,N] in place, obs_out [N,3], reward_out [N,1]."""
    _classic_step("rl8_pendulum_step_f32", 3, torch.float32, state, action, cfg, obs_out, reward_out)


def pendulum_reset(state: torch.Tensor, seed: int, reset_count: int, env_offset: int, obs_out: None | torch.Tensor) -> None:
    _classic_reset("rl8_pendulum_reset_f32", 3, state, seed, reset_count, env_offset, obs_out)


#: Rows of AlgoTrading's ``[9, N]`` state (``AlgoTradingState`` in csrc/device_math.hip.h).
ALGOTRADING_STATE_ROWS = ("invested", "position", "f", "k_cyclic", "k_market", "t", "price", "LOG_CHANGE(price)",
                          "LOG_CHANGE(price, position)")
#: Its observation leaves, in the order the kernels take them, with dtype and row width.
ALGOTRADING_LEAVES = (("action_mask", torch.bool, 3), ("invested", torch.int64, 1), ("LOG_CHANGE(price)", torch.float32, 1),
                      ("LOG_CHANGE(price, position)", torch.float32, 1))


def _algotrading_leaves(name: str, n: int, obs: Any) -> list[torch.Tensor]:
    """The four leaf tensors of ``obs`` (a mapping by leaf name), checked: dense ``[N, d]`` of the leaf's dtype."""
    out = []
    for key, dtype, d in ALGOTRADING_LEAVES:
        t = obs[key]
        if t.dtype != dtype or t.numel() != n * d or not t.is_contiguous():
            raise ValueError(f"{name}: leaf {key!r} must be a dense [N, {d}] {dtype} tensor")
        out.append(t)
    return out


def algotrading_reset(state: torch.Tensor, f_bounds: float, k_cyclic_bounds: float, k_market_bounds: float, seed: int,
                      reset_count: int, env_offset: int, obs_out: Any) -> None:
    """examples/algotrading/env.py:80-129: state ``[9, N]`` drawn in place; ``obs_out`` maps the four leaf names to
    ``[N, d]`` outputs."""
    _dense(state, torch.float32, "state")
    if state.ndim != 2 or state.shape[0] != len(ALGOTRADING_STATE_ROWS):
        raise ValueError("rl8_algotrading_reset_f32: state must be [9,N]")
    n = state.shape[1]
    leaves = _algotrading_leaves("rl8_algotrading_reset_f32", n, obs_out)
    with _timed("algotrading_reset", n):
        _check(load().rl8_algotrading_reset_f32(_ptr(state), n, f_bounds, k_cyclic_bounds, k_market_bounds, seed,
                                                reset_count, env_offset, *(_ptr(t) for t in leaves), _stream()),
               "rl8_algotrading_reset_f32")


def algotrading_step(state: torch.Tensor, action: torch.Tensor, obs_out: Any, reward_out: torch.Tensor) -> None:
    """examples/algotrading/env.py:131-183: state ``[9, N]`` in place, action ``[N, 1]`` int64, the four leaves of
    ``obs_out`` and reward_out ``[N, 1]`` written."""
    _dense(state, torch.float32, "state")
    _dense(action, torch.int64, "action")
    _dense(reward_out, torch.float32, "reward_out")
    if state.ndim != 2 or state.shape[0] != len(ALGOTRADING_STATE_ROWS):
        raise ValueError("rl8_algotrading_step_f32: state must be [9,N]")
    n = state.shape[1]
    if action.numel() != n or reward_out.numel() != n:
        raise ValueError("rl8_algotrading_step_f32: action [N,1], reward_out [N,1]")
    leaves = _algotrading_leaves("rl8_algotrading_step_f32", n, obs_out)
    with _timed("algotrading_step", n):
        _check(load().rl8_algotrading_step_f32(_ptr(state), _ptr(action), *(_ptr(t) for t in leaves), _ptr(reward_out), n,
                                               _stream()), "rl8_algotrading_step_f32")


# --------------------------------------------------------------------------- #
# Samplers.
# --------------------------------------------------------------------------- #
def categorical_sample_logp(
    logits: torch.Tensor,
    noise: None | torch.Tensor,
    *,
    seed: int = 0,
    step: int = 0,
    row_offset: int = 0,
    deterministic: bool = False,
) -> tuple[torch.Tensor, torch.Tensor]:
    """logits [M, A, K] -> (actions [M, A] int64, logp [M, 1])."""
    logits = _dense(logits.detach(), torch.float32, "logits")
    m, a, k = logits.shape
    if noise is not None:
        noise = _dense(noise, torch.float32, "noise")
        if noise.shape != logits.shape:
            raise ValueError("noise must have the shape of logits")
    actions = torch.empty(m, a, dtype=torch.int64, device=logits.device)
    logp = torch.empty(m, 1, dtype=torch.float32, device=logits.device)
    _check(
        load().rl8_categorical_sample_logp_f32(
            _ptr(logits), _ptr(noise), _ptr(actions), _ptr(logp), m, a, k, seed, step, row_offset,
            int(deterministic), _stream(),
        ),
        "rl8_categorical_sample_logp_f32",
    )
    return actions, logp


def _check_wide_classes(a: int, k: int) -> None:
    if k > MAX_WIDE_CLASSES:
        raise ValueError(f"a categorical of {k} classes is above the limit of {MAX_WIDE_CLASSES} (MAX_WIDE_CLASSES)")
    if a * k >= 1 << 31:
        raise ValueError(f"{a} action dimensions of {k} classes: a * k must stay below 2^31")


def categorical_sample_logp_wide(
    logits: torch.Tensor,
    noise: None | torch.Tensor,
    *,
    seed: int = 0,
    step: int = 0,
    row_offset: int = 0,
    deterministic: bool = False,
) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`categorical_sample_logp` for 2 <= K <= ``MAX_WIDE_CLASSES``: one wave per row."""
    logits = _dense(logits.detach(), torch.float32, "logits")
    m, a, k = logits.shape
    _check_wide_classes(a, k)
    if noise is not None:
        noise = _dense(noise, torch.float32, "noise")
        if noise.shape != logits.shape:
            raise ValueError("noise must have the shape of logits")
    actions = torch.empty(m, a, dtype=torch.int64, device=logits.device)
    logp = torch.empty(m, 1, dtype=torch.float32, device=logits.device)
    with _timed("categorical_sample_logp_wide", m):
        _check(
            load().rl8_categorical_wide_sample_logp_f32(
                _ptr(logits), _ptr(noise), _ptr(actions), _ptr(logp), m, a, k, seed, step, row_offset,
                int(deterministic), _stream(),
            ),
            "rl8_categorical_wide_sample_logp_f32",
        )
    return actions, logp


def normal_sample_logp(
    mean: torch.Tensor,
    log_std: torch.Tensor,
    noise: None | torch.Tensor,
    *,
    squashed: bool,
    seed: int = 0,
    step: int = 0,
    row_offset: int = 0,
    deterministic: bool = False,
) -> tuple[torch.Tensor, torch.Tensor]:
    mean = _dense(mean.detach(), torch.float32, "mean")
    log_std = _dense(log_std.detach(), torch.float32, "log_std")
    m, a = mean.shape
    if log_std.shape != mean.shape:
        raise ValueError("mean and log_std must have the same shape")
    if noise is not None:
        noise = _dense(noise, torch.float32, "noise")
        if noise.shape != mean.shape:
            raise ValueError("noise must have the shape of mean")
    actions = torch.empty(m, a, dtype=torch.float32, device=mean.device)
    logp = torch.empty(m, 1, dtype=torch.float32, device=mean.device)
    _check(
        load().rl8_normal_sample_logp_f32(
            _ptr(mean), _ptr(log_std), _ptr(noise), _ptr(actions), _ptr(logp), m, a, int(squashed),
            seed, step, row_offset, int(deterministic), _stream(),
        ),
        "rl8_normal_sample_logp_f32",
    )
    return actions, logp


# --------------------------------------------------------------------------- #
# Rollout bookkeeping: one timestep's column writes, alone (``rollout_scatter*``, for a generic Env) or fused with
# the action draw and ``env.step`` (``rollout_step_*``).  One validator and one launcher serve them all.
# --------------------------------------------------------------------------- #
_F32 = torch.float32


def _check_step_tensors(name: str, specs: Any) -> None:
    """``specs``: (what, tensor or None, dtype, elements) -- each tensor present must be dense, of that dtype and
    size.  Nothing here touches the library or a pointer, so a bad call fails before either."""
    for what, t, dtype, count in specs:
        if t is None:
            continue
        if t.dtype != dtype:
            raise TypeError(f"{name}: {what} must be {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
        if t.numel() != count:
            raise ValueError(f"{name}: {what} must hold {count} elements, got {t.numel()}")


def _step_columns(n: int, action_dtype: torch.dtype, action_col: torch.Tensor, logp_col: torch.Tensor,
                  value_col: torch.Tensor, reward_col: torch.Tensor) -> list:
    return [("action_col", action_col, action_dtype, n), ("logp_col", logp_col, _F32, n),
            ("value_col", value_col, _F32, n), ("reward_col", reward_col, _F32, n)]


def _rdr_pair(n: int, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor) -> list:
    return [("rdr_t", rdr_t, _F32, n), ("rdr_t1", rdr_t1, _F32, n)]


def _rollout_step(entry: str, n: int, head: Sequence, action_dtype: torch.dtype, obs: Sequence, columns: tuple,
                  tail: tuple, timed: None | str = None) -> None:
    """Check and launch one fused timestep.  ``head`` is the entry's leading arguments in ABI order and ``obs`` its
    ``obs[t+1]`` column(s): a (what, tensor or None, dtype, elements) tuple is checked and passed as its pointer, any
    other value is passed as it is.  ``columns``: (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1), one
    element per env each; ``tail``: (gamma, seed, step, env_offset, deterministic).  Every entry takes them in this order."""
    gamma, seed, step, env_offset, deterministic = tail
    args = (*head, *_step_columns(n, action_dtype, *columns[:4]), *obs, *_rdr_pair(n, *columns[4:]))
    _check_step_tensors(entry, [a for a in args if type(a) is tuple])
    args = [_ptr(a[1]) if type(a) is tuple else a for a in args]
    with _timed(timed, n) if timed else _UNTIMED:
        _check(getattr(load(), entry)(*args, gamma, n, seed, step, env_offset, int(deterministic), _stream()), entry)


def _scatter_columns(name: str, n: int, action: torch.Tensor, logp: torch.Tensor, value: torch.Tensor,
                     reward: torch.Tensor, columns: tuple) -> None:
    """The checks the two scatter wrappers share: the sampled tensors against the columns they go to."""
    action_col = columns[0]
    if action.dtype != action_col.dtype or action.numel() != action_col.numel():
        raise ValueError(f"{name}: action and action_col must match")
    _check_step_tensors(name, [("action", action, action.dtype, action.numel()), ("logp", logp, _F32, n),
                               ("value", value, _F32, n), ("reward", reward, _F32, n),
                               ("action_col", action_col, action.dtype, action.numel()),
                               *_step_columns(n, action.dtype, *columns[:4])[1:], *_rdr_pair(n, *columns[4:])])


def rollout_scatter(
    action: torch.Tensor, logp: torch.Tensor, value: torch.Tensor, reward: torch.Tensor, obs: torch.Tensor,
    action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor, reward_col: torch.Tensor,
    obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor, gamma: float,
) -> None:
    name = "rl8_rollout_scatter_f32"
    n = logp.shape[0]
    _scatter_columns(name, n, action, logp, value, reward, (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1))
    _check_step_tensors(name, [("obs", obs, _F32, obs.numel()), ("obs_col_next", obs_col_next, _F32, obs.numel())])
    _check(
        load().rl8_rollout_scatter_f32(
            _ptr(action), action.element_size() * (action.numel() // n), _ptr(logp), _ptr(value), _ptr(reward),
            _ptr(obs), obs.numel() // n, _ptr(action_col), _ptr(logp_col), _ptr(value_col), _ptr(reward_col),
            _ptr(obs_col_next), _ptr(rdr_t), _ptr(rdr_t1), gamma, n, _stream(),
        ),
        name,
    )


def rollout_scatter_leaves(
    action: torch.Tensor, logp: torch.Tensor, value: torch.Tensor, reward: torch.Tensor,
    obs: Sequence[torch.Tensor], action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor,
    reward_col: torch.Tensor, obs_cols_next: Sequence[torch.Tensor], rdr_t: None | torch.Tensor,
    rdr_t1: None | torch.Tensor, gamma: float,
) -> None:
    """``rollout_scatter`` for dict observations: ``obs[i]`` ``[N, ...]`` (any dtype) goes to ``obs_cols_next[i]`` in
    the same launch as the five other columns."""
    name = "rl8_rollout_scatter_leaves_f32"
    n = logp.shape[0]
    _scatter_columns(name, n, action, logp, value, reward, (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1))
    if not obs or len(obs) != len(obs_cols_next) or len(obs) > MAX_GATHER_FIELDS:
        raise ValueError(f"between 1 and {MAX_GATHER_FIELDS} observation leaves, as many columns")
    for i, (src, dst) in enumerate(zip(obs, obs_cols_next)):
        if src.dtype != dst.dtype or src.numel() != dst.numel() or src.shape[0] != n or src.numel() == 0:
            raise ValueError(f"obs[{i}] and obs_cols_next[{i}] must match ([N, ...], one dtype)")
        _check_step_tensors(name, [(f"obs[{i}]", src, src.dtype, src.numel()),
                                   (f"obs_cols_next[{i}]", dst, src.dtype, src.numel())])
    leaves = (ScatterLeaf * len(obs))(*(ScatterLeaf(_ptr(src), _ptr(dst), src.element_size() * (src.numel() // n))
                                        for src, dst in zip(obs, obs_cols_next)))
    with _timed("rollout_scatter_leaves", n):
        _check(
            load().rl8_rollout_scatter_leaves_f32(
                _ptr(action), action.element_size() * (action.numel() // n), _ptr(logp), _ptr(value), _ptr(reward),
                leaves, len(obs), _ptr(action_col), _ptr(logp_col), _ptr(value_col), _ptr(reward_col), _ptr(rdr_t),
                _ptr(rdr_t1), gamma, n, _stream(),
            ),
            name,
        )


def rollout_step_dummy(
    *, discrete: bool, squashed: bool, features: torch.Tensor, features2: None | torch.Tensor, value: torch.Tensor,
    noise: None | torch.Tensor, state: torch.Tensor, action_col: torch.Tensor, logp_col: torch.Tensor,
    value_col: torch.Tensor, reward_col: torch.Tensor, obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor,
    rdr_t1: None | torch.Tensor, gamma: float, seed: int, step: int, env_offset: int, deterministic: bool,
) -> None:
    n = state.numel()
    k = 2 if discrete else 1  # two logits per env, or a mean (features) and a log-std (features2)
    head = (int(discrete), int(squashed), ("features", features, _F32, k * n), ("features2", features2, _F32, n),
            ("value", value, _F32, n), ("noise", noise, _F32, k * n), ("state", state, _F32, n))
    _rollout_step("rl8_rollout_step_dummy_f32", n, head, torch.int64 if discrete else _F32,
                  [("obs_col_next", obs_col_next, _F32, n)],
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (gamma, seed, step, env_offset, deterministic), timed="rollout_step_dummy")


def _logits_head(n: int, logits: torch.Tensor, value: torch.Tensor, noise: None | torch.Tensor, state: torch.Tensor,
                 state_rows: int, cfg: Any) -> tuple:
    """The leading arguments of a three-way categorical env with struct-of-arrays state and a config struct."""
    return (("logits", logits, _F32, 3 * n), ("value", value, _F32, n), ("noise", noise, _F32, 3 * n),
            ("state", state, _F32, state_rows * n), C.byref(cfg))


def rollout_step_cartpole(
    *, logits: torch.Tensor, value: torch.Tensor, noise: None | torch.Tensor, state: torch.Tensor, cfg: CartPoleCfg,
    action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor, reward_col: torch.Tensor,
    obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor, gamma: float, seed: int,
    step: int, env_offset: int, deterministic: bool,
) -> None:
    n = state.shape[1]
    _rollout_step("rl8_rollout_step_cartpole_f32", n, _logits_head(n, logits, value, noise, state, 4, cfg), torch.int64,
                  [("obs_col_next", obs_col_next, _F32, 5 * n)],
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (gamma, seed, step, env_offset, deterministic))


def rollout_step_mountain_car(
    *, logits: torch.Tensor, value: torch.Tensor, noise: None | torch.Tensor, state: torch.Tensor, cfg: MountainCarCfg,
    action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor, reward_col: torch.Tensor,
    obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor, gamma: float, seed: int,
    step: int, env_offset: int, deterministic: bool,
) -> None:
    n = state.shape[1]
    _rollout_step("rl8_rollout_step_mountain_car_f32", n, _logits_head(n, logits, value, noise, state, 2, cfg),
                  torch.int64, [("obs_col_next", obs_col_next, _F32, 2 * n)],
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (gamma, seed, step, env_offset, deterministic))


def rollout_step_pendulum(
    *, squashed: bool, mean: torch.Tensor, log_std: torch.Tensor, value: torch.Tensor, noise: None | torch.Tensor,
    state: torch.Tensor, cfg: PendulumCfg, action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor,
    reward_col: torch.Tensor, obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor,
    gamma: float, seed: int, step: int, env_offset: int, deterministic: bool,
) -> None:
    n = state.shape[1]
    head = (int(squashed), ("mean", mean, _F32, n), ("log_std", log_std, _F32, n), ("value", value, _F32, n),
            ("noise", noise, _F32, n), ("state", state, _F32, 2 * n), C.byref(cfg))
    _rollout_step("rl8_rollout_step_pendulum_f32", n, head, _F32, [("obs_col_next", obs_col_next, _F32, 3 * n)],
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (gamma, seed, step, env_offset, deterministic))


def rollout_step_algotrading(
    *, logits: torch.Tensor, value: torch.Tensor, noise: None | torch.Tensor, state: torch.Tensor,
    action_col: torch.Tensor, logp_col: torch.Tensor, value_col: torch.Tensor, reward_col: torch.Tensor,
    obs_col_next: Any, rdr_t: None | torch.Tensor, rdr_t1: None | torch.Tensor, gamma: float, seed: int, step: int,
    env_offset: int, deterministic: bool,
) -> None:
    """``obs_col_next`` maps the four leaf names to their ``t+1`` columns."""
    n = state.shape[1]
    head = (("logits", logits, _F32, 3 * n), ("value", value, _F32, n), ("noise", noise, _F32, 3 * n),
            ("state", state, _F32, len(ALGOTRADING_STATE_ROWS) * n))
    obs = [(f"leaf {key!r}", obs_col_next[key], dtype, d * n) for key, dtype, d in ALGOTRADING_LEAVES]
    _rollout_step("rl8_rollout_step_algotrading_f32", n, head, torch.int64, obs,
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (gamma, seed, step, env_offset, deterministic), timed="rollout_step_algotrading")


def buffer_layout(leaf: torch.Tensor) -> tuple[int, int, int]:
    """(layout, env_stride, time_stride) of a [N, T, 1] (or [N, T]) buffer leaf."""
    n, t = leaf.shape[0], leaf.shape[1]
    es, ts = leaf.stride(0), leaf.stride(1)
    if leaf.ndim == 3 and leaf.shape[2] != 1:
        raise ValueError("expected a [N, T, 1] leaf")
    if (ts == 1 or t == 1) and (es == t or n == 1):
        return LAYOUT_ENV_MAJOR, es, ts
    if (es == 1 or n == 1) and (ts == n or t == 1):
        return LAYOUT_TIME_MAJOR, es, ts
    return -1, es, ts


def rollout_stats(rewards: torch.Tensor, rdr: None | torch.Tensor) -> torch.Tensor:
    """rewards / rdr [N, H+1, 1] in either layout -> 12 raw moments (fp64, device)."""
    n, h1 = rewards.shape[0], rewards.shape[1]
    _, es, ts = buffer_layout(rewards)
    if rewards.dtype != torch.float32:
        raise TypeError("rewards must be float32")
    if rdr is not None and (rdr.stride() != rewards.stride() or rdr.shape != rewards.shape):
        raise ValueError("rdr must share the layout of rewards")
    out = torch.empty(12, dtype=torch.float64, device=rewards.device)
    with _timed("rollout_stats", n * (h1 - 1)):
        _check(
            load().rl8_rollout_stats_f32(_ptr(rewards), _ptr(rdr), n, h1 - 1, es, ts, _ptr(out),
                                         _ptr(scratch(rewards.device)), _stream()),
            "rl8_rollout_stats_f32",
        )
    return out


#: route names of ``rl8_rollout_stats_plan`` / ``rl8_gather_minibatch_plan``, indexed by their RL8_STATS_* / RL8_GATHER_* codes
STATS_ROUTES = ("STATS_VEC4", "STATS_VEC1")
GATHER_ROUTES = ("GATHER_GENERAL", "GATHER_WIDE_ROWS", "GATHER_TILED")


class StatsPlan(NamedTuple):
    """What ``rl8_rollout_stats_f32`` launches (``rl8_stats_plan_t``)."""

    route: str
    grid: int
    trips: int


def rollout_stats_plan(n: int, h: int, env_stride: int, time_stride: int, aligned16_all: bool = True) -> StatsPlan:
    """The statistics' launch plan; host arithmetic in the library, no device needed."""
    p = StatsPlanStruct()
    _check(load().rl8_rollout_stats_plan(n, h, env_stride, time_stride, int(aligned16_all), C.byref(p)),
           "rl8_rollout_stats_plan")
    return StatsPlan(STATS_ROUTES[p.route], p.grid, p.trips)


class GatherPlan(NamedTuple):
    """What ``rl8_gather_minibatch`` launches: per field its route and tiled group (-1: none), and the launch count."""

    routes: tuple[str, ...]
    groups: tuple[int, ...]
    launches: int


def gather_minibatch_plan(indexed: bool, m: int, h: int, fields: Any, n_fields: int) -> GatherPlan:
    """``fields``: a ``GatherField`` array as ``rl8_gather_minibatch`` takes it; its pointers are judged for alignment
    only. Host arithmetic in the library, no device needed."""
    routes, groups, launches = (C.c_int * MAX_GATHER_FIELDS)(), (C.c_int * MAX_GATHER_FIELDS)(), C.c_int(0)
    _check(load().rl8_gather_minibatch_plan(int(indexed), m, h, fields, n_fields, routes, groups, C.byref(launches)),
           "rl8_gather_minibatch_plan")
    return GatherPlan(tuple(GATHER_ROUTES[routes[f]] for f in range(n_fields)), tuple(groups[f] for f in range(n_fields)),
                      launches.value)


class PackPlan(NamedTuple):
    """The launch of the tiled transposition (``rl8_pack_plan_t``)."""

    tile_steps: int
    lds_bytes: int
    tiles: int
    grid: int


def pack_plan(n: int, h: int, row_words: int) -> PackPlan:
    """Tile shape and grid of ``rl8_pack_samples`` / ``rl8_gather_minibatch(index=NULL)``; no device needed."""
    p = PackPlanStruct()
    _check(load().rl8_pack_plan(n, h, row_words, C.byref(p)), "rl8_pack_plan")
    return PackPlan(p.tile_steps, p.lds_bytes, p.tiles, p.grid)


# --------------------------------------------------------------------------- #
# GAE.
# --------------------------------------------------------------------------- #
#: route names of ``rl8_gae_plan`` / ``rl8_advantage_normalise_route``, indexed by their RL8_GAE_* / RL8_NORM_* codes
GAE_ROUTES = ("TIME_VEC4", "TIME_VEC1", "ENV_PIPELINED", "ENV_FLAT", "ENV_CHUNKED")
NORMALISE_ROUTES = ("FLAT_VEC4", "FLAT_VEC1", "ENV_MAJOR")


class GaePlan(NamedTuple):
    """What ``rl8_gae_scan_f32`` launches for a shape, a layout and an alignment (``rl8_gae_plan_t``)."""

    route: str
    envs_per_block: int
    chunk: int
    lds_stride: int
    lds_bytes: int
    grid: int


def gae_plan(n: int, h: int, layout: int, aligned16_all: bool = True) -> GaePlan:
    """The scan's launch plan; host arithmetic in the library, no device needed."""
    p = GaePlanStruct()
    _check(load().rl8_gae_plan(n, h, layout, int(aligned16_all), C.byref(p)), "rl8_gae_plan")
    return GaePlan(GAE_ROUTES[p.route], p.envs_per_block, p.chunk, p.lds_stride, p.lds_bytes, p.grid)


def advantage_normalise_route(n: int, h: int, layout: int, aligned16: bool = True) -> str:
    """The kernel ``advantage_normalise`` launches; host arithmetic in the library, no device needed."""
    route = load().rl8_advantage_normalise_route(n, h, layout, int(aligned16))
    if route < 0:
        _check(route, "rl8_advantage_normalise_route")
    return NORMALISE_ROUTES[route]


def gae_scan(
    rewards: torch.Tensor, values: torch.Tensor, adv: torch.Tensor, ret: torch.Tensor, *, layout: int,
    n: int, h: int, gamma: float, gamma_lambda: float, reward_denominator: float, write_scaled_rewards: bool,
) -> torch.Tensor:
    """Launches the scan; returns the device moments tensor (count, sum, sumsq)."""
    moments = torch.empty(3, dtype=torch.float64, device=rewards.device)
    with _timed("gae_scan", n * h):
        _check(
            load().rl8_gae_scan_f32(
                _ptr(rewards), _ptr(values), _ptr(adv), _ptr(ret), n, h, layout, gamma, gamma_lambda,
                reward_denominator, int(write_scaled_rewards), _ptr(moments), _ptr(scratch(rewards.device)),
                _stream(),
            ),
            "rl8_gae_scan_f32",
        )
    return moments


def advantage_normalise(adv: torch.Tensor, *, layout: int, n: int, h: int, moments: torch.Tensor) -> None:
    if moments.dtype != torch.float64 or moments.numel() < 3:
        raise TypeError("moments must be 3 float64 values")
    with _timed("advantage_normalise", n * h):
        _check(
            load().rl8_advantage_normalise_f32(_ptr(adv), n, h, layout, _ptr(moments), _stream()),
            "rl8_advantage_normalise_f32",
        )


# --------------------------------------------------------------------------- #
# PPO loss.
# --------------------------------------------------------------------------- #
def ppo_hparams(
    *, clip_param: float, dual_clip_param: None | float, entropy_coeff: float, vf_clip_param: float,
    vf_coeff: float, grad_scale: float,
) -> PPOHparams:
    return PPOHparams(clip_param, dual_clip_param if dual_clip_param else 0.0, entropy_coeff, vf_clip_param,
                      vf_coeff, grad_scale)


def _loss_inputs(m: int, *named: tuple[str, torch.Tensor, torch.dtype, int]) -> None:
    for name, t, dtype, numel in named:
        _dense(t, dtype, name)
        if t.numel() != numel:
            raise ValueError(f"{name} has {t.numel()} elements, expected {numel} for M={m}")


def ppo_loss_categorical(
    logits: torch.Tensor, value: torch.Tensor, action: torch.Tensor, logp_old: torch.Tensor, adv: torch.Tensor,
    ret: torch.Tensor, hp: PPOHparams, *, with_grad: bool = True,
) -> tuple[torch.Tensor, None | torch.Tensor, None | torch.Tensor]:
    """Returns (loss_sums[5] fp64 device, grad_logits, grad_value)."""
    m, a, k = logits.shape
    _loss_inputs(m, ("logits", logits, torch.float32, m * a * k), ("value", value, torch.float32, m),
                 ("action", action, torch.int64, m * a), ("logp_old", logp_old, torch.float32, m),
                 ("adv", adv, torch.float32, m), ("ret", ret, torch.float32, m))
    sums = torch.empty(5, dtype=torch.float64, device=logits.device)
    g_logits = torch.empty_like(logits) if with_grad else None
    g_value = torch.empty_like(value) if with_grad else None
    with _timed("ppo_loss_categorical", m):
        _check(
            load().rl8_ppo_loss_categorical_fwd_bwd_f32(
                _ptr(logits), _ptr(value), _ptr(action), _ptr(logp_old), _ptr(adv), _ptr(ret), m, a, k,
                C.byref(hp), _ptr(g_logits), _ptr(g_value), _ptr(sums), _ptr(scratch(logits.device)), _stream(),
            ),
            "rl8_ppo_loss_categorical_fwd_bwd_f32",
        )
    return sums, g_logits, g_value


def ppo_loss_categorical_wide(
    logits: torch.Tensor, value: torch.Tensor, action: torch.Tensor, logp_old: torch.Tensor, adv: torch.Tensor,
    ret: torch.Tensor, hp: PPOHparams, *, with_grad: bool = True,
) -> tuple[torch.Tensor, None | torch.Tensor, None | torch.Tensor]:
    """:func:`ppo_loss_categorical` for 2 <= K <= ``MAX_WIDE_CLASSES``: one wave per sample."""
    m, a, k = logits.shape
    _check_wide_classes(a, k)
    _loss_inputs(m, ("logits", logits, torch.float32, m * a * k), ("value", value, torch.float32, m),
                 ("action", action, torch.int64, m * a), ("logp_old", logp_old, torch.float32, m),
                 ("adv", adv, torch.float32, m), ("ret", ret, torch.float32, m))
    sums = torch.empty(5, dtype=torch.float64, device=logits.device)
    g_logits = torch.empty_like(logits) if with_grad else None
    g_value = torch.empty_like(value) if with_grad else None
    with _timed("ppo_loss_categorical_wide", m):
        _check(
            load().rl8_ppo_loss_categorical_wide_fwd_bwd_f32(
                _ptr(logits), _ptr(value), _ptr(action), _ptr(logp_old), _ptr(adv), _ptr(ret), m, a, k,
                C.byref(hp), _ptr(g_logits), _ptr(g_value), _ptr(sums), _ptr(scratch(logits.device)), _stream(),
            ),
            "rl8_ppo_loss_categorical_wide_fwd_bwd_f32",
        )
    return sums, g_logits, g_value


def ppo_loss_normal(
    mean: torch.Tensor, log_std: torch.Tensor, value: torch.Tensor, action: torch.Tensor, logp_old: torch.Tensor,
    adv: torch.Tensor, ret: torch.Tensor, hp: PPOHparams, *, squashed: bool, with_grad: bool = True,
):
    m, a = mean.shape
    _loss_inputs(m, ("mean", mean, torch.float32, m * a), ("log_std", log_std, torch.float32, m * a),
                 ("value", value, torch.float32, m), ("action", action, torch.float32, m * a),
                 ("logp_old", logp_old, torch.float32, m), ("adv", adv, torch.float32, m),
                 ("ret", ret, torch.float32, m))
    sums = torch.empty(5, dtype=torch.float64, device=mean.device)
    g_mean = torch.empty_like(mean) if with_grad else None
    g_ls = torch.empty_like(log_std) if with_grad else None
    g_value = torch.empty_like(value) if with_grad else None
    with _timed("ppo_loss_normal", m):
        _check(
            load().rl8_ppo_loss_normal_fwd_bwd_f32(
                _ptr(mean), _ptr(log_std), _ptr(value), _ptr(action), _ptr(logp_old), _ptr(adv), _ptr(ret), m, a,
                int(squashed), C.byref(hp), _ptr(g_mean), _ptr(g_ls), _ptr(g_value), _ptr(sums),
                _ptr(scratch(mean.device)), _stream(),
            ),
            "rl8_ppo_loss_normal_fwd_bwd_f32",
        )
    return sums, g_mean, g_ls, g_value


# --------------------------------------------------------------------------- #
# Minibatch gather.
# --------------------------------------------------------------------------- #
def gather_minibatch(index: None | torch.Tensor, h: int, leaves: Sequence[torch.Tensor]) -> list[torch.Tensor]:
    """index [M] int64 of reference sample ids (env*H + t); leaves are [N, T, d]
    buffer leaves (any stride over env/time, dense over d). Returns dense [M, d]
    tensors. ``index=None``: every sample in order (``M = N * h``): a tiled
    transposition for leaves of up to 128 bytes per sample (in groups that fit a
    tile row), the general kernels with the implicit index for wider ones."""
    if index is None:
        m = leaves[0].shape[0] * h
    else:
        _dense(index, torch.int64, "index")
        m = index.numel()
    if len(leaves) > MAX_GATHER_FIELDS:
        raise ValueError(f"at most {MAX_GATHER_FIELDS} leaves per gather")
    fields = (GatherField * len(leaves))()
    outs = []
    for i, leaf in enumerate(leaves):
        if leaf.ndim < 2:
            raise ValueError("leaves must be [N, T, ...]")
        trailing = leaf.shape[2:]
        row = 1
        for d in trailing:
            row *= d
        # trailing dims must be dense
        expect = 1
        for d, st in zip(reversed(trailing), reversed(leaf.stride()[2:])):
            if d != 1 and st != expect:
                raise ValueError("leaf trailing dims must be dense")
            expect *= d
        if leaf.element_size() not in (4, 8):
            raise TypeError("leaf elements must be 4 or 8 bytes wide")
        dst = torch.empty((m, *trailing), dtype=leaf.dtype, device=leaf.device)
        fields[i] = GatherField(_ptr(leaf), _ptr(dst), leaf.stride(0), leaf.stride(1), row, leaf.element_size())
        outs.append(dst)
    with _timed("gather_minibatch", m):
        _check(load().rl8_gather_minibatch(_ptr(index) if index is not None else None, m, h, fields, len(leaves), _stream()),
               "rl8_gather_minibatch")
    return outs


def gather_sequences(seq_index: None | torch.Tensor, seq_len: int, h: int,
                     leaves: Sequence[torch.Tensor]) -> list[torch.Tensor]:
    """Whole sequences of ``seq_len`` samples out of [N, T, ...] buffer leaves (any stride over env / time, dense over
    the rest; elements of 1, 4 or 8 bytes: bool masks beside int64 and float32 leaves): sequence
    ``q = env * (h // seq_len) + s`` is samples ``q * seq_len + j`` (the reference's numbering). ``seq_index`` [S]
    int64, or None for every sequence in order (``S = N * h // seq_len``). Returns dense ``[S * seq_len, ...]``
    tensors of the leaves' dtypes, row ``i * seq_len + j`` holding ``leaf[env, s * seq_len + j]``."""
    if seq_len < 1 or h < 1 or h % seq_len:
        raise ValueError(f"gather_sequences: h={h} must be a positive multiple of seq_len={seq_len}")
    if seq_index is None:
        num_seqs = leaves[0].shape[0] * (h // seq_len)
    else:
        _dense(seq_index, torch.int64, "seq_index")
        num_seqs = seq_index.numel()
    if len(leaves) > MAX_GATHER_FIELDS:
        raise ValueError(f"at most {MAX_GATHER_FIELDS} leaves per gather")
    rows = num_seqs * seq_len
    fields = (GatherField * len(leaves))()
    outs = []
    for i, leaf in enumerate(leaves):
        if leaf.ndim < 2 or leaf.shape[1] < h:
            raise ValueError(f"leaves must be [N, T >= {h}, ...]")
        trailing = leaf.shape[2:]
        row, expect = 1, 1
        for d, st in zip(reversed(trailing), reversed(leaf.stride()[2:])):
            if d != 1 and st != expect:
                raise ValueError("leaf trailing dims must be dense")
            expect *= d
            row *= d
        dst = torch.empty((rows, *trailing), dtype=leaf.dtype, device=leaf.device)
        fields[i] = GatherField(_ptr(leaf), _ptr(dst), leaf.stride(0), leaf.stride(1), row, leaf.element_size())
        outs.append(dst)
    with _timed("gather_sequences", rows):
        _check(load().rl8_gather_sequences(_ptr(seq_index) if seq_index is not None else None, num_seqs, seq_len, h,
                                           fields, len(leaves), _stream()), "rl8_gather_sequences")
    return outs


def _window_fields(rows: int, leaves: Sequence[torch.Tensor], sizes: Sequence[int]):
    """The ``rl8_window_field`` array of ``[N, T, ...]`` leaves with window lengths ``sizes``, and the fresh outputs
    it points at: per leaf ``(inputs [rows, size, ...], padding_mask [rows, size] bool)``, or ``(dst [rows, ...],
    None)`` for ``size == 1``."""
    if not leaves or len(leaves) != len(sizes) or len(leaves) > MAX_GATHER_FIELDS:
        raise ValueError(f"between 1 and {MAX_GATHER_FIELDS} leaves per launch, one window length each")
    fields = (WindowField * len(leaves))()
    outs: list[tuple[torch.Tensor, None | torch.Tensor]] = []
    for i, (leaf, size) in enumerate(zip(leaves, sizes)):
        if leaf.ndim < 2:
            raise ValueError("leaves must be [N, T, ...]")
        if size < 1:
            raise ValueError(f"window length {size} must be at least 1")
        trailing = leaf.shape[2:]
        row, expect = 1, 1
        for d, st in zip(reversed(trailing), reversed(leaf.stride()[2:])):
            if d != 1 and st != expect:
                raise ValueError("leaf trailing dims must be dense")
            expect *= d
            row *= d
        if leaf.element_size() not in (1, 4, 8):
            raise TypeError("leaf elements must be 1, 4 or 8 bytes wide")
        if size == 1:
            dst, mask = torch.empty((rows, *trailing), dtype=leaf.dtype, device=leaf.device), None
        else:
            dst = torch.empty((rows, size, *trailing), dtype=leaf.dtype, device=leaf.device)
            mask = torch.empty((rows, size), dtype=torch.bool, device=leaf.device)
        fields[i] = WindowField(_ptr(leaf), _ptr(dst), _ptr(mask), leaf.stride(0), leaf.stride(1), row,
                                leaf.element_size(), size)
        outs.append((dst, mask))
    return fields, outs


def gather_windows(index: None | torch.Tensor, h: int, leaves: Sequence[torch.Tensor],
                   sizes: Sequence[int]) -> list[tuple[torch.Tensor, None | torch.Tensor]]:
    """Padded rolling windows of a minibatch: ``index`` [M] int64 of reference sample ids (``env * h + t``; ``None``:
    every sample in order, ``M = N * h``), ``leaves`` [N, T, ...] buffer leaves (any stride over env / time, dense
    over the rest; float32, int64 or bool) and one window length ``shift + 1`` per leaf. Per leaf ``(inputs [M, size,
    ...], padding_mask [M, size])`` -- what ``PaddedRollingWindow.apply_all(leaf[:, :h], size)[index]`` holds -- or
    ``(leaf's rows [M, ...], None)`` for ``size == 1``. One launch."""
    if h < 1:
        raise ValueError(f"gather_windows: h={h} must be positive")
    if index is None:
        m = leaves[0].shape[0] * h
    else:
        _dense(index, torch.int64, "index")
        m = index.numel()
    fields, outs = _window_fields(m, leaves, sizes)
    with _timed("gather_windows", m):
        _check(load().rl8_gather_windows(_ptr(index) if index is not None else None, m, h, fields, len(outs), _stream()),
               "rl8_gather_windows")
    return outs


def window_last(t: int, leaves: Sequence[torch.Tensor],
                sizes: Sequence[int]) -> list[tuple[torch.Tensor, None | torch.Tensor]]:
    """The windows that end at step ``t`` of every env: per leaf what ``pad_last_sequence(leaf[:, :t + 1], size)``
    holds (``(inputs [N, size, ...], padding_mask [N, size])``), or ``(leaf[:, t] as a dense copy, None)`` for
    ``size == 1``. One launch."""
    if not leaves or any(not 0 <= t < leaf.shape[1] for leaf in leaves):
        raise ValueError(f"window_last: step {t} outside the leaves")
    n = leaves[0].shape[0]
    fields, outs = _window_fields(n, leaves, sizes)
    with _timed("window_last", n):
        _check(load().rl8_window_last(t, n, fields, len(outs), _stream()), "rl8_window_last")
    return outs


# --------------------------------------------------------------------------- #
# Masked sequence ops (rl8_amd/csrc/masked_kernels.hip).
# --------------------------------------------------------------------------- #
def _byte_mask(mask: None | torch.Tensor, shape: tuple, what: str) -> None | torch.Tensor:
    """``mask`` (bool or uint8, nonzero = VALID) as the dense byte array the kernels read; ``None`` stays ``None``."""
    if mask is None:
        return None
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what} must be bool or uint8, got {mask.dtype}")
    if tuple(mask.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(mask.shape)}")
    if not mask.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return mask


def masked_rows_route(k: int) -> int:
    """``MASKED_ROWS_LANE`` or ``MASKED_ROWS_WAVE`` for rows of ``k`` classes (host only)."""
    route = int(load().rl8_masked_rows_route(k))
    _check(min(route, 0), "rl8_masked_rows_route")
    return route


def masked_pool(x: torch.Tensor, mask: None | torch.Tensor, mode: int) -> tuple[torch.Tensor, None | torch.Tensor]:
    """``x [rows, T, E]`` pooled over T under ``mask [rows, T]`` (nonzero = valid, ``None`` = no mask):
    ``(out [rows, E], index [rows, E] int64 in MAX mode or None)``."""
    x = _dense(x.detach(), torch.float32, "x")
    rows, t, e = x.shape
    mask = _byte_mask(mask, (rows, t), "mask")
    out = torch.empty(rows, e, dtype=torch.float32, device=x.device)
    index = torch.empty(rows, e, dtype=torch.int64, device=x.device) if mode == POOL_MAX else None
    with _timed("masked_pool", rows):
        _check(load().rl8_masked_pool_f32(_ptr(x), _ptr(mask), rows, t, e, mode, _ptr(out), _ptr(index), _stream()),
               "rl8_masked_pool_f32")
    return out, index


def masked_pool_backward(dout: torch.Tensor, mask: None | torch.Tensor, index: None | torch.Tensor, t: int,
                         mode: int) -> torch.Tensor:
    """Gradient ``[rows, T, E]`` of :func:`masked_pool`'s input from ``dout [rows, E]``; every element is written."""
    dout = _dense(dout.detach(), torch.float32, "dout")
    rows, e = dout.shape
    mask = _byte_mask(mask, (rows, t), "mask")
    if index is not None:
        _shaped(index, (rows, e), "index", torch.int64)
    dx = torch.empty(rows, t, e, dtype=torch.float32, device=dout.device)
    with _timed("masked_pool_backward", rows):
        _check(load().rl8_masked_pool_backward_f32(_ptr(dout), _ptr(mask), _ptr(index), rows, t, e, mode, _ptr(dx),
                                                   _stream()), "rl8_masked_pool_backward_f32")
    return dx


def masked_log_softmax(x: torch.Tensor, mask: None | torch.Tensor) -> torch.Tensor:
    """Log-softmax of ``x [rows, K]`` along K under ``mask [rows, K]`` (nonzero = valid, ``None`` = no mask)."""
    x = _dense(x.detach(), torch.float32, "x")
    rows, k = x.shape
    mask = _byte_mask(mask, (rows, k), "mask")
    out = torch.empty_like(x)
    with _timed("masked_log_softmax", rows):
        _check(load().rl8_masked_log_softmax_f32(_ptr(x), _ptr(mask), rows, k, _ptr(out), _stream()),
               "rl8_masked_log_softmax_f32")
    return out


def masked_log_softmax_backward(dout: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    dout = _dense(dout.detach(), torch.float32, "dout")
    rows, k = dout.shape
    _shaped(out, (rows, k), "out")
    dx = torch.empty_like(dout)
    with _timed("masked_log_softmax_backward", rows):
        _check(load().rl8_masked_log_softmax_backward_f32(_ptr(dout), _ptr(out), rows, k, _ptr(dx), _stream()),
               "rl8_masked_log_softmax_backward_f32")
    return dx


def masked_categorical_sample(x: torch.Tensor, mask: None | torch.Tensor, noise: None | torch.Tensor, *, seed: int = 0,
                              step: int = 0, row_offset: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """One draw per row of ``x [rows, K]`` under ``mask``: ``(masked logit of the class [rows], class [rows] int64)``.
    ``noise`` [rows, K] are injected Exp(1) draws; ``None`` takes the Philox stream at ``(seed, row_offset + row, step)``."""
    x = _dense(x.detach(), torch.float32, "x")
    rows, k = x.shape
    mask = _byte_mask(mask, (rows, k), "mask")
    if noise is not None:
        _shaped(noise, (rows, k), "noise")
    value = torch.empty(rows, dtype=torch.float32, device=x.device)
    index = torch.empty(rows, dtype=torch.int64, device=x.device)
    with _timed("masked_categorical_sample", rows):
        _check(load().rl8_masked_categorical_sample_f32(_ptr(x), _ptr(mask), _ptr(noise), rows, k, seed, step, row_offset,
                                                        _ptr(value), _ptr(index), _stream()),
               "rl8_masked_categorical_sample_f32")
    return value, index


# --------------------------------------------------------------------------- #
# Short-sequence attention (rl8_amd/csrc/attention_kernels.hip).
# --------------------------------------------------------------------------- #
def attention_supports(tq: int, tk: int, heads: int, d: int) -> bool:
    """Whether the attention kernels take ``tq`` queries over ``tk`` keys with ``heads`` heads of ``d`` floats (host
    only)."""
    status = int(load().rl8_attention_supports(tq, tk, heads, d))
    _check(min(status, 0), "rl8_attention_supports")
    return status == 1


def _rows(t: torch.Tensor, shape: tuple, what: str) -> int:
    """Row stride in floats of ``t [B, T, E]`` float32, which may be a slice along the last dimension of a dense
    ``[B, T, n E]`` tensor: unit stride inside a row, rows evenly spaced over both leading dimensions."""
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be {torch.float32}, got {t.dtype}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    batch_stride, row_stride, unit = t.stride()
    if shape[1] == 1:  # (the stride of a dimension of one element says nothing)
        row_stride = batch_stride if shape[0] > 1 else shape[2]
    if shape[0] == 1:
        batch_stride = shape[1] * row_stride
    if (unit != 1 and shape[2] > 1) or row_stride < shape[2] or batch_stride != shape[1] * row_stride:
        raise ValueError(f"{what} must be dense or a last-dimension slice of a dense tensor, got strides {t.stride()}")
    return int(row_stride)


def _padding_mask(mask: None | torch.Tensor, shape: tuple) -> None | torch.Tensor:
    """``key_padding`` (bool or uint8, nonzero = PADDED -- the opposite of :func:`_byte_mask`'s masks) as dense bytes."""
    return _byte_mask(mask, shape, "key_padding")


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_padding: None | torch.Tensor,
              bias: None | torch.Tensor, heads: int, *, want_lse: bool = True) -> tuple[torch.Tensor, None | torch.Tensor]:
    """``softmax(q k^T / sqrt(D) + bias, padded keys at -inf) v`` per head: ``(out [B, Tq, E], lse [B, heads, Tq])``.
    ``q [B, Tq, E]`` and ``k``, ``v [B, Tk, E]`` may be slices of a packed projection (:func:`_rows`; ``k`` and ``v``
    with one row stride); ``key_padding [B, Tk]`` nonzero = PADDED, ``bias [Tq, Tk]`` float32, both optional. A query
    without an admissible key gives 0 and ``lse = +inf``."""
    q, k, v = q.detach(), k.detach(), v.detach()
    b, tq, e = q.shape
    tk = k.shape[1]
    q_stride, kv_stride = _rows(q, (b, tq, e), "q"), _rows(k, (b, tk, e), "k")
    if _rows(v, (b, tk, e), "v") != kv_stride:
        raise ValueError("k and v must have the same row stride")
    if heads < 1 or e % heads:
        raise ValueError(f"{heads} heads do not divide rows of {e} floats")
    key_padding = _padding_mask(key_padding, (b, tk))
    if bias is not None:
        _shaped(bias, (tq, tk), "bias")
    out = torch.empty(b, tq, e, dtype=torch.float32, device=q.device)
    lse = torch.empty(b, heads, tq, dtype=torch.float32, device=q.device) if want_lse else None
    with _timed("attention", b):
        _check(load().rl8_attention_f32(_ptr(q), q_stride, _ptr(k), _ptr(v), kv_stride, _ptr(key_padding), _ptr(bias), b,
                                        tq, tk, heads, e // heads, _ptr(out), _ptr(lse), _stream()), "rl8_attention_f32")
    return out, lse


def attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_padding: None | torch.Tensor,
                       bias: None | torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, heads: int,
                       dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor) -> None:
    """Gradients of :func:`attention`'s ``q``, ``k``, ``v`` written into ``dq [B, Tq, E]``, ``dk``, ``dv [B, Tk, E]``,
    which may be slices of one packed gradient buffer like the operands; every element of the three is written."""
    q, k, v = q.detach(), k.detach(), v.detach()
    b, tq, e = q.shape
    tk = k.shape[1]
    q_stride, kv_stride = _rows(q, (b, tq, e), "q"), _rows(k, (b, tk, e), "k")
    dq_stride, dkv_stride = _rows(dq, (b, tq, e), "dq"), _rows(dk, (b, tk, e), "dk")
    if _rows(v, (b, tk, e), "v") != kv_stride or _rows(dv, (b, tk, e), "dv") != dkv_stride:
        raise ValueError("k and v, and dk and dv, must have the same row stride")
    if heads < 1 or e % heads:
        raise ValueError(f"{heads} heads do not divide rows of {e} floats")
    key_padding = _padding_mask(key_padding, (b, tk))
    if bias is not None:
        _shaped(bias, (tq, tk), "bias")
    _shaped(out, (b, tq, e), "out")
    _shaped(lse, (b, heads, tq), "lse")
    _shaped(dout, (b, tq, e), "dout")
    delta = torch.empty(b, heads, tq, dtype=torch.float32, device=q.device)
    with _timed("attention_backward", b):
        _check(load().rl8_attention_backward_f32(_ptr(q), q_stride, _ptr(k), _ptr(v), kv_stride, _ptr(key_padding),
                                                 _ptr(bias), _ptr(out), _ptr(lse), _ptr(dout), b, tq, tk, heads,
                                                 e // heads, _ptr(dq), dq_stride, _ptr(dk), _ptr(dv), dkv_stride,
                                                 _ptr(delta), _stream()), "rl8_attention_backward_f32")


# --------------------------------------------------------------------------- #
# The fused LayerNorm feedforward block (rl8_amd/csrc/feedforward_kernels.hip).
# --------------------------------------------------------------------------- #
def feedforward_supports(f: int, hidden: int) -> bool:
    """Whether the feedforward kernels take rows of ``f`` features through ``hidden`` hidden units (host only)."""
    status = int(load().rl8_feedforward_supports(f, hidden))
    _check(min(status, 0), "rl8_feedforward_supports")
    return status == 1


class FeedforwardLimits(NamedTuple):
    """``rl8_feedforward_limits``: the row-per-lane kernels' grid cap and lanes per workgroup, the weight-gradient
    kernel's grid cap and rows staged per workgroup. Beyond ``cap x rows`` a workgroup strides."""

    grid_cap: int
    block: int
    wgrad_grid_cap: int
    wgrad_rows: int


def feedforward_limits() -> FeedforwardLimits:
    limits = (C.c_int * 4)()
    _check(load().rl8_feedforward_limits(limits), "rl8_feedforward_limits")
    return FeedforwardLimits(*(int(v) for v in limits))


def feedforward_workspace_floats(rows: int, f: int, hidden: int) -> int:
    """Floats of workspace ``rl8_feedforward_backward_f32`` needs for its parameter gradients (host only)."""
    floats = int(load().rl8_feedforward_workspace_floats(rows, f, hidden))
    _check(min(floats, 0), "rl8_feedforward_workspace_floats")
    return floats


def _feedforward_operands(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                          w2: torch.Tensor, b2: None | torch.Tensor, dout: None | torch.Tensor) -> tuple[int, int, int]:
    """``(rows, f, hidden)`` of a dense float32 ``x [..., f]``, the block's parameters and ``dout`` like ``x``: every
    layout checked, then every device."""
    _dense(x, torch.float32, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x must be [..., f] with at least one element, got {tuple(x.shape)}")
    f = int(x.shape[-1])
    if w1.dim() != 2:
        raise ValueError(f"w1 must be [hidden, {f}], got {tuple(w1.shape)}")
    hidden = int(w1.shape[0])
    for t, shape, what in ((gamma, (f,), "gamma"), (beta, (f,), "beta"), (w1, (hidden, f), "w1"), (b1, (hidden,), "b1"),
                           (w2, (f, hidden), "w2"), (b2, (f,), "b2"), (dout, tuple(x.shape), "dout")):
        if t is not None:
            _shaped(t, shape, what)
    for t in (x, gamma, beta, w1, b1, w2, b2, dout):
        _ptr(t)
    return x.numel() // f, f, hidden


def feedforward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, w1: torch.Tensor, b1: torch.Tensor,
                w2: torch.Tensor, b2: torch.Tensor, residual: bool) -> torch.Tensor:
    """``(x if residual else 0) + linear(relu(linear(layer_norm(x), w1, b1)), w2, b2)`` per row of a dense
    ``x [..., f]``: ``w1 [hidden, f]``, ``w2 [f, hidden]``, ``gamma``, ``beta``, ``b2 [f]``, ``b1 [hidden]``."""
    x, gamma, beta, w1, b1, w2, b2 = (t.detach() for t in (x, gamma, beta, w1, b1, w2, b2))
    rows, f, hidden = _feedforward_operands(x, gamma, beta, w1, b1, w2, b2, None)
    out = torch.empty_like(x)
    with _timed("feedforward", rows):
        _check(load().rl8_feedforward_f32(_ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                          rows, f, hidden, int(residual), _ptr(out), _stream()), "rl8_feedforward_f32")
    return out


class FeedforwardGrads(NamedTuple):
    """What :func:`feedforward_backward` returns; a piece that was not asked for is ``None``."""

    dx: None | torch.Tensor
    dgamma: None | torch.Tensor
    dbeta: None | torch.Tensor
    dw1: None | torch.Tensor
    db1: None | torch.Tensor
    dw2: None | torch.Tensor
    db2: None | torch.Tensor


def feedforward_backward(x: torch.Tensor, dout: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                         w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, residual: bool, *, want_dx: bool = True,
                         want_params: bool = True) -> FeedforwardGrads:
    """Gradients of :func:`feedforward` from ``x`` and ``dout`` alone: ``dx`` like ``x`` and / or the six parameter
    gradients (the same bits on every run)."""
    x, dout, gamma, beta, w1, b1, w2 = (t.detach() for t in (x, dout, gamma, beta, w1, b1, w2))
    rows, f, hidden = _feedforward_operands(x, gamma, beta, w1, b1, w2, None, dout)

    def new(*shape: int) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=x.device)

    dx = torch.empty_like(x) if want_dx else None
    params = (new(f), new(f), new(hidden, f), new(hidden), new(f, hidden), new(f)) if want_params else (None,) * 6
    workspace = new(feedforward_workspace_floats(rows, f, hidden)) if want_params else None
    with _timed("feedforward_backward", rows):
        _check(load().rl8_feedforward_backward_f32(_ptr(x), _ptr(dout), _ptr(gamma), _ptr(beta), eps, _ptr(w1), _ptr(b1),
                                                   _ptr(w2), rows, f, hidden, int(residual), _ptr(dx),
                                                   *(_ptr(p) for p in params), _ptr(workspace), _stream()),
               "rl8_feedforward_backward_f32")
    return FeedforwardGrads(dx, *params)


class PackedSamples:
    """The training fields of every sample of a rollout buffer, side by side in
    the reference's sample order (``rl8_pack_samples``); ``gather(index)`` returns
    the dense minibatch tensors, one per field."""

    def __init__(self, h: int, leaves: Sequence[torch.Tensor]) -> None:
        if not leaves or len(leaves) > MAX_GATHER_FIELDS:
            raise ValueError(f"between 1 and {MAX_GATHER_FIELDS} leaves per pack")
        n = leaves[0].shape[0]
        self.fields = (GatherField * len(leaves))()
        self.meta: list[tuple[tuple[int, ...], torch.dtype]] = []
        words = 0
        for i, leaf in enumerate(leaves):
            if leaf.ndim < 2 or leaf.shape[0] != n or leaf.shape[1] < h:
                raise ValueError("leaves must be [N, >= H, ...] views of one buffer")
            if leaf.element_size() not in (4, 8):
                raise TypeError("leaf elements must be 4 or 8 bytes wide")
            trailing = tuple(leaf.shape[2:])
            row = 1
            for d in trailing:
                row *= d
            if leaf[0, 0].numel() and not leaf[0, 0].is_contiguous():
                raise ValueError("leaf trailing dims must be dense")
            self.fields[i] = GatherField(_ptr(leaf), None, leaf.stride(0), leaf.stride(1), row, leaf.element_size())
            self.meta.append((trailing, leaf.dtype))
            words += row * (leaf.element_size() // 4)
        self.row_words = (words + 3) // 4 * 4
        self.samples = n * h
        self.device = leaves[0].device
        self.packed = torch.empty(self.samples * self.row_words, dtype=torch.int32, device=self.device)
        with _timed("pack_samples", self.samples):
            _check(load().rl8_pack_samples(self.fields, len(leaves), n, h, _ptr(self.packed), self.row_words, _stream()),
                   "rl8_pack_samples")

    def gather(self, index: torch.Tensor) -> list[torch.Tensor]:
        _dense(index, torch.int64, "index")
        m = index.numel()
        outs = []
        for i, (trailing, dtype) in enumerate(self.meta):
            dst = torch.empty((m, *trailing), dtype=dtype, device=self.device)
            self.fields[i].dst = _ptr(dst)
            outs.append(dst)
        with _timed("gather_packed", m):
            _check(load().rl8_gather_packed(_ptr(index), m, _ptr(self.packed), self.row_words, self.fields,
                                            len(self.meta), _stream()), "rl8_gather_packed")
        return outs


# --------------------------------------------------------------------------- #
# Fused MLP tower (N1).
# --------------------------------------------------------------------------- #
MLP_HIDDEN = 256
MLP_MAX_IN = 16
MLP_MAX_OUT = 8


def mlp_pack_w2(w2: torch.Tensor, *, transposed: bool = False) -> torch.Tensor:
    """[256, 256] nn.Linear weight -> MFMA fragment order (65536 floats)."""
    w2 = _dense(w2.detach(), torch.float32, "w2")
    if tuple(w2.shape) != (MLP_HIDDEN, MLP_HIDDEN):
        raise ValueError("w2 must be [256, 256]")
    packed = torch.empty(MLP_HIDDEN * MLP_HIDDEN, dtype=torch.float32, device=w2.device)
    _check(load().rl8_mlp_pack_w2_f32(_ptr(w2), _ptr(packed), int(transposed), _stream()), "rl8_mlp_pack_w2_f32")
    return packed


def _tower_shapes(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor,
                  b3: torch.Tensor) -> tuple[torch.Tensor, int, int, int]:
    """(dense x, M, d_in, n_out) of a width-256 tower call whose parameters have the shapes that go with them."""
    x = _dense(x.detach(), torch.float32, "x")
    m, d_in = x.shape
    n_out = w3.shape[0]
    for name, t, shape in (("w1", w1, (MLP_HIDDEN, d_in)), ("b1", b1, (MLP_HIDDEN,)), ("b2", b2, (MLP_HIDDEN,)),
                           ("w3", w3, (n_out, MLP_HIDDEN)), ("b3", b3, (n_out,))):
        _shaped(t, shape, name)
    return x, m, d_in, n_out


def mlp_tower_forward(
    x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor, b2: torch.Tensor,
    w3: torch.Tensor, b3: torch.Tensor, *, save: bool = False,
) -> tuple[torch.Tensor, None | torch.Tensor, None | torch.Tensor]:
    """x [M, d_in] -> out [M, n_out]; with ``save`` also the post-ReLU activations
    h1, h2 ([M, 256]) for the backward pass."""
    x, m, d_in, n_out = _tower_shapes(x, w1, b1, b2, w3, b3)
    if w2_packed.numel() != MLP_HIDDEN * MLP_HIDDEN:
        raise ValueError("w2_packed must come from mlp_pack_w2")
    out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    h1 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    h2 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    with _timed("mlp_tower_forward_save" if save else "mlp_tower_forward", m):
        _check(
            load().rl8_mlp_tower_forward_f32(
                _ptr(x), m, d_in, _ptr(w1.detach()), _ptr(b1.detach()), _ptr(w2_packed), _ptr(b2.detach()),
                _ptr(w3.detach()), _ptr(b3.detach()), n_out, _ptr(out), _ptr(h1), _ptr(h2), _stream(),
            ),
            "rl8_mlp_tower_forward_f32",
        )
    return out, h1, h2


def mlp_forward_f16_supports(d_in: int, n_out: int) -> bool:
    return bool(load().rl8_mlp_forward_f16_supports(int(d_in), int(n_out)))


def mlp_backward_f16_supports(d_in: int, n_out: int) -> bool:
    return bool(load().rl8_mlp_backward_f16_supports(int(d_in), int(n_out)))


def mlp_gates_on() -> bool:
    """Whether the towers' rank-one gate kernels may run: ``RL8_WGRAD_GATE_OFF=1`` turns them off (A/B runs).
    Read on every call."""
    return not int(os.environ.get("RL8_WGRAD_GATE_OFF", "0") or 0)


def mlp_pack_w2_f16(w2: torch.Tensor, *, transposed: bool = False) -> torch.Tensor:
    """[256, 256] nn.Linear weight -> two fp16 planes of 2^e * w (hi = fp16(v),
    lo = fp16(v - hi)) in fragment order, followed by {2^e, 2^-e} (uint8)."""
    w2 = _dense(w2.detach(), torch.float32, "w2")
    if tuple(w2.shape) != (MLP_HIDDEN, MLP_HIDDEN):
        raise ValueError("w2 must be [256, 256]")
    lib = load()
    packed = torch.empty(int(lib.rl8_mlp_f16_packed_bytes()), dtype=torch.uint8, device=w2.device)
    _check(lib.rl8_mlp_pack_w2_f16(_ptr(w2), int(transposed), _ptr(packed), _stream()), "rl8_mlp_pack_w2_f16")
    return packed


def mlp_pack_w2_f16_gate(w2: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """B operand of the data-gradient kernel's gate mode: fp16 planes of ``w2[k][i] * w3e[k]`` with
    ``w3e = w3[0]`` (one output) or ``w3[0] - w3[1]`` (two outputs with opposite gradients)."""
    w2 = _dense(w2.detach(), torch.float32, "w2")
    w3 = _dense(w3.detach(), torch.float32, "w3")
    if tuple(w2.shape) != (MLP_HIDDEN, MLP_HIDDEN) or w3.ndim != 2 or w3.shape[1] != MLP_HIDDEN or w3.shape[0] not in (1, 2):
        raise ValueError("w2 must be [256, 256] and w3 [1 or 2, 256]")
    lib = load()
    packed = torch.empty(int(lib.rl8_mlp_f16_packed_bytes()), dtype=torch.uint8, device=w2.device)
    _check(lib.rl8_mlp_pack_w2_f16_gate(_ptr(w2), _ptr(w3), int(w3.shape[0]), _ptr(packed), _stream()),
           "rl8_mlp_pack_w2_f16_gate")
    return packed


def mlp_tower_forward_split(
    x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2_split: torch.Tensor, b2: torch.Tensor,
    w3: torch.Tensor, b3: torch.Tensor, *, save: bool = False, save_h1: bool = True, save_gate: bool = False,
    save_h2: bool = True, out: None | torch.Tensor = None, h2_out: None | torch.Tensor = None,
    gate_out: None | torch.Tensor = None, timer_name: None | str = None,
) -> tuple[torch.Tensor, ...]:
    """``mlp_tower_forward`` with the 256x256 product as three fp16-plane MFMAs per
    16 k (fp32 accuracy, fp32 in / out / accumulate; ``w2_split`` from
    ``mlp_pack_w2_f16``). ``save_h1=False`` keeps only h2 (the plane backward kernels
    recompute h1). ``save_gate=True`` (with
    ``save``) appends a fourth result, the ReLU gate of h2 as bits ([M, 8] int32:
    bit j of row s = h2[s, j] > 0), which the data-gradient kernel reads instead of h2.
    ``save_h2=False`` (fp16-plane pack, with ``save_gate``): the gate bits ALONE are kept -- all the
    backward pass of a rank-one head needs (``mlp_tower_backward(..., h2=None, w2=..., b2=...)``).
    ``out`` / ``h2_out`` / ``gate_out``: caller-owned dense destinations ([M, n_out] fp32, [M, 256] fp32,
    [M, 8] int32) instead of fresh tensors -- the rollout writes each timestep's rows straight into the slabs the
    first SGD pass reads back (``fused_mlp.RolloutRecord``)."""
    x, m, d_in, n_out = _tower_shapes(x, w1, b1, b2, w3, b3)
    lib = load()
    if w2_split.dtype != torch.uint8 or w2_split.numel() != int(lib.rl8_mlp_f16_packed_bytes()):  # fp16 two-plane pack
        raise ValueError("w2_split must come from mlp_pack_w2_f16")
    for name, t, dtype, shape in (("out", out, torch.float32, (m, n_out)), ("h2_out", h2_out, torch.float32, (m, MLP_HIDDEN)),
                                  ("gate_out", gate_out, torch.int32, (m, 8))):
        if t is not None:
            _shaped(t, shape, name, dtype)
    if out is None:
        out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    if save and not save_h2:
        if not save_gate:
            raise ValueError("save_h2=False needs save_gate=True")
        save_h1 = False
    h1 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save and save_h1 else None
    h2 = (h2_out if h2_out is not None else torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device)) \
        if save and save_h2 else None
    gate = (gate_out if gate_out is not None else torch.empty(m, 8, dtype=torch.int32, device=x.device)) \
        if save and save_gate else None
    with _timed(timer_name or ("mlp_tower_forward_save" if save else "mlp_tower_forward"), m):
        _check(
            lib.rl8_mlp_tower_forward_f16_f32(
                _ptr(x), m, d_in, _ptr(w1.detach()), _ptr(b1.detach()), _ptr(w2_split), _ptr(b2.detach()),
                _ptr(w3.detach()), _ptr(b3.detach()), n_out, _ptr(out), _ptr(h1), _ptr(h2), _ptr(gate), _stream(),
            ),
            "rl8_mlp_tower_forward_f16_f32",
        )
    return (out, h1, h2, gate) if save_gate else (out, h1, h2)


def _column_sums(t: torch.Tensor) -> torch.Tensor:
    """``t.sum(0)`` of a tall ``[m, n]`` matrix with a few columns.  torch's reduction over
    the long dimension of a [2^23, 3] tensor runs at 24 GB/s (4.1 ms per call, 14 % of the
    CartPole bench's kernel time); folded to [m / 1024, 1024 n] the same sum is a column
    reduction with a contiguous inner dimension."""
    m, n = t.shape
    fold = 1024
    if n == 1 or m < 64 * fold or not t.is_contiguous():
        return t.sum(0)
    groups = m // fold
    out = t[: groups * fold].view(groups, fold * n).sum(0).view(fold, n).sum(0)
    if groups * fold < m:
        out = out + t[groups * fold :].sum(0)
    return out


def mlp_tower_backward(
    x: torch.Tensor, h1: None | torch.Tensor, h2: None | torch.Tensor, dout: torch.Tensor,
    w2t_packed: torch.Tensor, w3: torch.Tensor,
    w1: None | torch.Tensor = None, b1: None | torch.Tensor = None, *, wgrad_split: bool = False,
    gate2: None | torch.Tensor = None, gate_pack=None, w2: None | torch.Tensor = None, b2: None | torch.Tensor = None,
    h2_fn=None, info: None | dict = None, assume_general: bool = False, assume_pair: bool = False,
    gates_on: None | bool = None,
) -> dict[str, torch.Tensor]:
    """Gradients of one tower's parameters given ``dout`` [M, n_out] and the
    activations saved by the forward pass. Returns ``w1, b1, w2, b2, w3, b3``.

    ``w2t_packed`` from ``mlp_pack_w2(..., transposed=True)`` selects the fp32 MFMA
    kernel; from ``mlp_pack_w2_f16(..., transposed=True)`` (uint8) the fp16-plane
    kernels (fused mode), which also need layer 1 (``w1``, ``b1``) -- they recompute
    the ReLU gate of h1 instead of reading h1 back -- and ``gate2`` (``save_gate`` of
    the forward): the gate bits of h2. ``wgrad_split`` forms dW2 with the plane
    weight-gradient kernel (any width; needs ``w1``, ``b1``) even when the
    data-gradient half runs on the fp32 kernel. ``gate_pack``: a
    callable returning ``mlp_pack_w2_f16_gate(w2, w3)`` -- with it, single-output heads and two-output
    heads whose gradients are exact negatives (checked on ``dout``) run the data gradient in gate mode.
    ``h2=None`` (a forward with ``save_h2=False``: gate bits only) with the layer's own ``w2`` [256, 256] and
    ``b2``: such rank-one heads then take dW3 from the weight-gradient sums (``rl8_mlp_wgrad_gate_bits_f32``) and
    h2 is never touched; if the head turns out not to be rank-one, ``h2_fn()`` must supply h2 (a forward re-run).
    ``info`` (a dict) receives ``rank_one``: whether the gate kernels ran.  ``assume_general`` (with ``h2``): a
    two-output head already known not to be a pair skips the check of ``dout`` (a pass over it and a host read per
    call) and runs the general kernels, which are right for any ``dout``.  ``assume_pair``: ``dout`` [M, 2] is an exact
    pair by construction (the caller vouches: the two-class loss kernel's own output) -- no check either.
    ``gates_on``: whether the gate kernels may run at all (default ``mlp_gates_on()``)."""
    m, d_in = x.shape
    n_out = w3.shape[0]
    planes = w2t_packed.dtype == torch.uint8
    if planes and w2t_packed.numel() != int(load().rl8_mlp_f16_packed_bytes()):
        raise ValueError("w2t_packed: a uint8 pack must come from mlp_pack_w2_f16(..., transposed=True)")
    if planes and gate2 is None:
        raise ValueError("the fp16-plane backward needs gate2 (mlp_tower_forward_split(save_gate=True))")
    if h1 is None and not planes:
        raise ValueError("h1 may be omitted only on the fp16-plane path")
    for name, t, numel in (("x", x, m * d_in), ("h1", h1, m * MLP_HIDDEN), ("h2", h2, m * MLP_HIDDEN),
                           ("dout", dout, m * n_out)):
        if t is None:
            continue
        _dense(t, torch.float32, name)
        if t.numel() != numel:
            raise ValueError(f"{name} has the wrong number of elements")
    if gate2 is not None and (gate2.dtype != torch.int32 or tuple(gate2.shape) != (m, 8) or not gate2.is_contiguous()):
        raise ValueError("gate2 must be the [M, 8] int32 gate of mlp_tower_forward_split(save_gate=True)")
    lib = load()
    width = int(lib.rl8_mlp_backward_partial_floats(d_in, n_out))
    max_rows = int(lib.rl8_mlp_backward_max_rows())
    partials = torch.empty(max_rows, width, dtype=torch.float32, device=x.device)
    rows = C.c_int(0)
    dw2 = None
    if planes:
        # fused: the data-gradient kernel stores no dZ2; the weight-gradient kernel
        # re-forms it (and h1) and accumulates the head gradients
        if w1 is None or b1 is None:
            raise ValueError("the fp16-plane backward needs w1 and b1")
        w1p, b1p = _ptr(_dense(w1.detach(), torch.float32, "w1")), _ptr(_dense(b1.detach(), torch.float32, "b1"))
        w3p = _ptr(w3.detach())
        if gates_on is None:
            gates_on = mlp_gates_on()
        # two outputs with exactly opposite gradients (a two-way categorical head) are rank-one too: checked on the
        # data, the answer read back behind the data-gradient launch so that the GPU has work while the host waits
        pair = n_out == 2 and gates_on and assume_pair
        pair_flag = None
        if n_out == 2 and gates_on and not pair and not (assume_general and h2 is not None):
            pair_flag = _pair_flag(x.device)
            _check(lib.rl8_mlp_dout_pair_check(_ptr(dout), m, _ptr(pair_flag), _stream()), "rl8_mlp_dout_pair_check")
            if gate_pack is not None or h2 is None:  # needed before the data gradient: read it now (a short bubble)
                pair, pair_flag = int(pair_flag[0].item()) == 0, None
        rank_one = gates_on and (n_out == 1 or pair)
        if h2 is None and not (rank_one and w2 is not None and b2 is not None):
            if h2_fn is None:
                raise ValueError("h2=None needs a rank-one head on the fp16-plane path (with w2, b2) or h2_fn")
            h2 = h2_fn()  # not a rank-one head after all: the forward is re-run for h2
        # data gradient: gate mode (B operand w2 * w3e) for rank-one heads, general mode (w2^T and w3) otherwise
        gate_dgrad = gate_pack is not None and rank_one
        with _timed("mlp_tower_backward_gate" if gate_dgrad else "mlp_tower_backward", m):
            name, b_args = (("rl8_mlp_tower_backward_gate_f16_f32", (_ptr(gate_pack()),)) if gate_dgrad
                            else ("rl8_mlp_tower_backward_f16_f32", (_ptr(w2t_packed), w3p)))
            _check(getattr(lib, name)(_ptr(x), w1p, b1p, _ptr(dout), m, d_in, *b_args, n_out, _ptr(partials),
                                      C.byref(rows), _ptr(gate2), _stream()), name)
        dw2 = torch.empty(MLP_HIDDEN, MLP_HIDDEN, dtype=torch.float32, device=x.device)
        pair = pair or (pair_flag is not None and int(pair_flag[0].item()) == 0)
        rank_one = gates_on and (n_out == 1 or pair)
        if info is not None:
            info["rank_one"] = rank_one
        # weight gradient: a rank-one head with gate bits only takes dW3 from the weight-gradient sums, a pair the pair
        # kernel, anything else the general entry (which runs the gate-plane kernel itself for one output)
        with _timed("mlp_wgrad_gate" if rank_one else "mlp_wgrad", m):
            name, args = (
                ("rl8_mlp_wgrad_gate_bits_f32", (_ptr(gate2), _ptr(dout), _ptr(x), w1p, b1p,
                                                 _ptr(_dense(w2.detach(), torch.float32, "w2")),
                                                 _ptr(_dense(b2.detach(), torch.float32, "b2")), w3p, m, d_in, n_out))
                if h2 is None else
                ("rl8_mlp_wgrad_fused_pair_f32", (_ptr(h2), _ptr(dout), _ptr(x), w1p, b1p, w3p, m, d_in)) if pair else
                ("rl8_mlp_wgrad_fused_split_f32", (_ptr(h2), _ptr(dout), _ptr(x), w1p, b1p, w3p, m, d_in, n_out)))
            _check(getattr(lib, name)(*args, _ptr(_wgrad_workspace(x.device)), _ptr(dw2), _ptr(partials), _stream()),
                   name)
    else:
        dz2 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device)
        with _timed("mlp_tower_backward", m):
            _check(
                lib.rl8_mlp_tower_backward_f32(
                    _ptr(x), _ptr(h1), _ptr(h2), _ptr(dout), m, d_in, _ptr(w2t_packed), _ptr(w3.detach()), n_out,
                    _ptr(dz2), _ptr(partials), C.byref(rows), _stream()),
                "rl8_mlp_tower_backward_f32",
            )
    small = partials[: rows.value].sum(0)
    o1 = MLP_HIDDEN * d_in
    grads = {
        "w1": small[:o1].view(MLP_HIDDEN, d_in),
        "b1": small[o1 : o1 + MLP_HIDDEN],
        "b2": small[o1 + MLP_HIDDEN : o1 + 2 * MLP_HIDDEN],
        "w3": small[o1 + 2 * MLP_HIDDEN : o1 + 2 * MLP_HIDDEN + n_out * MLP_HIDDEN].view(n_out, MLP_HIDDEN),
        # (the fused plane backward leaves db3 -- a column sum of dout -- to the caller)
        "b3": _column_sums(dout) if planes else small[o1 + 2 * MLP_HIDDEN + n_out * MLP_HIDDEN :],
        "w2": dw2 if planes else (mlp_wgrad_split(dz2, x, w1, b1) if wgrad_split else mlp_wgrad(dz2, h1)),
    }
    return grads


def _per_stream(cache: dict[tuple[int, int], torch.Tensor], device: torch.device, make) -> torch.Tensor:
    """``cache``'s tensor for (``device``, the current stream): ``make()`` on first use."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    if key not in cache:
        cache[key] = make()
    return cache[key]


_pair_flags: dict[tuple[int, int], torch.Tensor] = {}
_wgrad_ws: dict[tuple[int, int], torch.Tensor] = {}


def _pair_flag(device: torch.device) -> torch.Tensor:
    return _per_stream(_pair_flags, device, lambda: torch.zeros(4, dtype=torch.int32, device=device))


def _wgrad_workspace(device: torch.device) -> torch.Tensor:
    def make() -> torch.Tensor:
        ws = torch.empty(int(load().rl8_mlp_wgrad_workspace_bytes()) // 4, dtype=torch.float32, device=device)
        ws[-64:].zero_()  # (the guard's lifetime counters live there: include/rl8_amd.h, rl8_mlp_wgrad_workspace_bytes)
        return ws
    return _per_stream(_wgrad_ws, device, make)


def wgrad_guard_counts() -> tuple[int, int]:
    """(weight-gradient calls that consulted the guard of the fp16 planes, calls it sent to the exact bf16 planes)
    over the lifetime of this process's workspaces; one host sync."""
    calls = fires = 0
    for ws in _wgrad_ws.values():
        words = ws[-64:].view(torch.int32)[32:34].tolist()
        calls, fires = calls + words[0], fires + words[1]
    return calls, fires


def mlp_wgrad_split(dz2: torch.Tensor, x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """dW2 [256, 256] = dz2^T @ relu(x @ w1^T + b1) over the rows: bf16-plane MFMAs at
    fp32 accuracy, h1 recomputed from the observations (deterministic)."""
    _dense(dz2, torch.float32, "dz2")
    _dense(x, torch.float32, "x")
    m, d_in = x.shape
    if tuple(dz2.shape) != (m, MLP_HIDDEN):
        raise ValueError("dz2 must be [M, 256] with M = x.shape[0]")
    out = torch.empty(MLP_HIDDEN, MLP_HIDDEN, dtype=torch.float32, device=dz2.device)
    with _timed("mlp_wgrad", m):
        _check(load().rl8_mlp_wgrad_split_f32(_ptr(dz2), _ptr(x), _ptr(_dense(w1.detach(), torch.float32, "w1")),
                                              _ptr(_dense(b1.detach(), torch.float32, "b1")), m, d_in,
                                              _ptr(_wgrad_workspace(dz2.device)), _ptr(out), 0, _stream()),
               "rl8_mlp_wgrad_split_f32")
    return out


def mlp_wgrad(dz2: torch.Tensor, h1: torch.Tensor, *, out: None | torch.Tensor = None,
              accumulate: bool = False, planes: bool = False) -> torch.Tensor:
    """dW2 [256, 256] = dz2^T @ h1 over the rows (fp32 MFMA, deterministic).  ``out`` with ``accumulate``: added to
    what ``out`` holds (the segments of a long batch, in order).  ``planes``: the same product, both operands from
    memory, on three exact bf16 planes per operand (``rl8_mlp_wgrad_split_strided_f32``: fp32 accuracy, deterministic)."""
    _dense(dz2, torch.float32, "dz2")
    _dense(h1, torch.float32, "h1")
    if dz2.shape != h1.shape or dz2.shape[1] != MLP_HIDDEN:
        raise ValueError("dz2 and h1 must both be [M, 256]")
    lib = load()
    ws = _wgrad_workspace(dz2.device)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(MLP_HIDDEN, MLP_HIDDEN, dtype=torch.float32, device=dz2.device)
    _shaped(out, (MLP_HIDDEN, MLP_HIDDEN), "out")
    with _timed("mlp_wgrad", dz2.shape[0]):
        if planes:
            _check(lib.rl8_mlp_wgrad_split_strided_f32(_ptr(dz2), MLP_HIDDEN, _ptr(h1), MLP_HIDDEN, dz2.shape[0], _ptr(ws),
                                                       _ptr(out), int(accumulate), None, 0, None, None, _stream()),
                   "rl8_mlp_wgrad_split_strided_f32")
        else:
            _check(lib.rl8_mlp_wgrad_f32(_ptr(dz2), _ptr(h1), dz2.shape[0], _ptr(ws), _ptr(out), int(accumulate), _stream()),
                   "rl8_mlp_wgrad_f32")
    return out


# --------------------------------------------------------------------------- #
# Narrow towers: hidden width 64 or 128 (mlp_narrow_kernels.hip).
# --------------------------------------------------------------------------- #
MLP_NARROW_HIDDEN = (64, 128)


def mlp_narrow_supports(hidden: int, d_in: int, n_out: int) -> bool:
    return bool(load().rl8_mlp_narrow_supports(hidden, d_in, n_out))


def _narrow_params(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                   w3: torch.Tensor, b3: None | torch.Tensor) -> tuple[int, int, int, int]:
    """(m, d_in, hidden, n_out) after the dtype / contiguity / shape checks of the narrow entries."""
    _dense(x, torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    hidden, n_out = w1.shape[0], w3.shape[0]
    shapes = (("w1", w1, (hidden, d_in)), ("b1", b1, (hidden,)), ("w2", w2, (hidden, hidden)), ("b2", b2, (hidden,)),
              ("w3", w3, (n_out, hidden)), ("b3", b3, (n_out,)))
    for name, t, shape in shapes:
        if t is not None:
            _shaped(t, shape, name)
    if m < 1 or not mlp_narrow_supports(hidden, d_in, n_out):
        raise ValueError(f"no narrow tower kernel for m={m}, hidden={hidden}, d_in={d_in}, n_out={n_out}")
    return m, d_in, hidden, n_out


def mlp_narrow_forward(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                       w3: torch.Tensor, b3: torch.Tensor) -> torch.Tensor:
    """out [M, n_out] = relu(relu(x w1^T + b1) w2^T + b2) w3^T + b3 for hidden width 64 or 128 (nothing saved)."""
    x, w1, b1, w2, b2, w3, b3 = (t.detach() for t in (x, w1, b1, w2, b2, w3, b3))
    m, d_in, hidden, n_out = _narrow_params(x, w1, b1, w2, b2, w3, b3)
    out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    with _timed("mlp_narrow_forward", m):
        _check(load().rl8_mlp_narrow_forward_f32(_ptr(x), m, d_in, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3),
                                                 _ptr(b3), n_out, hidden, _ptr(out), _stream()),
               "rl8_mlp_narrow_forward_f32")
    return out


def mlp_narrow_backward(x: torch.Tensor, dout: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                        b2: torch.Tensor, w3: torch.Tensor, *, want_dx: bool = False) -> dict[str, torch.Tensor]:
    """Gradients of the six tower parameters ("w1", "b1", "w2", "b2", "w3", "b3") for the output gradient ``dout``
    [M, n_out]: the forward recomputed from x, partial slabs per workgroup summed in a fixed order (deterministic).
    ``want_dx``: the gradient of x too ("x", [M, d_in]) from the same launch (``rl8_mlp_narrow_backward_dx_f32``, timed
    as "mlp_narrow_backward_dx"); the parameter gradients hold the same bits either way."""
    x, dout, w1, b1, w2, b2, w3 = (t.detach() for t in (x, dout, w1, b1, w2, b2, w3))
    m, d_in, hidden, n_out = _narrow_params(x, w1, b1, w2, b2, w3, None)
    _shaped(dout, (m, n_out), "dout")
    lib = load()
    ws = torch.empty(int(lib.rl8_mlp_narrow_workspace_bytes(m, hidden, d_in, n_out)) // 4, dtype=torch.float32,
                     device=x.device)
    sizes = (hidden * d_in, hidden, hidden * hidden, hidden, n_out * hidden, n_out)
    grads = torch.empty(sum(sizes), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_dx else None
    if want_dx:
        with _timed("mlp_narrow_backward_dx", m):
            _check(lib.rl8_mlp_narrow_backward_dx_f32(_ptr(x), _ptr(dout), m, d_in, _ptr(w1), _ptr(b1), _ptr(w2),
                                                      _ptr(b2), _ptr(w3), n_out, hidden, _ptr(ws), _ptr(dx), _stream()),
                   "rl8_mlp_narrow_backward_dx_f32")
    else:
        with _timed("mlp_narrow_backward", m):
            _check(lib.rl8_mlp_narrow_backward_f32(_ptr(x), _ptr(dout), m, d_in, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                                   _ptr(w3), n_out, hidden, _ptr(ws), _stream()),
                   "rl8_mlp_narrow_backward_f32")
    with _timed("mlp_narrow_reduce", m):
        _check(lib.rl8_mlp_narrow_reduce_f32(_ptr(ws), m, hidden, d_in, n_out, _ptr(grads), _stream()),
               "rl8_mlp_narrow_reduce_f32")
    parts = torch.split(grads, sizes)
    shapes = ((hidden, d_in), (hidden,), (hidden, hidden), (hidden,), (n_out, hidden), (n_out,))
    got = {k: p.view(s) for k, p, s in zip(("w1", "b1", "w2", "b2", "w3", "b3"), parts, shapes)}
    if dx is not None:
        got["x"] = dx
    return got


# --------------------------------------------------------------------------- #
# Wide-input towers: hidden width 256, 17 to 128 inputs (mlp_wide_in_kernels.hip).
# --------------------------------------------------------------------------- #
def mlp_wide_in_supports(d_in: int, n_out: int) -> bool:
    return bool(load().rl8_mlp_wide_in_supports(int(d_in), int(n_out)))


def mlp_wide_in_pack_w1(w1: torch.Tensor) -> torch.Tensor:
    """[256, d_in] nn.Linear weight -> MFMA fragment order, zero-padded to whole k-groups of 8."""
    w1 = _dense(w1.detach(), torch.float32, "w1")
    if w1.ndim != 2 or w1.shape[0] != MLP_HIDDEN:
        raise ValueError("w1 must be [256, d_in]")
    lib = load()
    floats = int(lib.rl8_mlp_wide_in_pack_floats(w1.shape[1]))
    if floats < 0:
        raise ValueError(f"no wide-input tower kernel for d_in={w1.shape[1]}")
    packed = torch.empty(floats, dtype=torch.float32, device=w1.device)
    _check(lib.rl8_mlp_wide_in_pack_w1_f32(_ptr(w1), w1.shape[1], _ptr(packed), _stream()), "rl8_mlp_wide_in_pack_w1_f32")
    return packed


def mlp_wide_in_forward(
    x: torch.Tensor, w1_packed: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor, b2: torch.Tensor,
    w3: torch.Tensor, b3: torch.Tensor, *, save: bool = False,
) -> tuple[torch.Tensor, None | torch.Tensor, None | torch.Tensor]:
    """x [M, d_in], 17 <= d_in <= 128 -> out [M, n_out]; with ``save`` also the post-ReLU activations h1, h2 ([M, 256])
    for the backward pass.  ``w1_packed`` from ``mlp_wide_in_pack_w1``, ``w2_packed`` from ``mlp_pack_w2``."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    n_out = w3.shape[0]
    for name, t, shape in (("b1", b1, (MLP_HIDDEN,)), ("b2", b2, (MLP_HIDDEN,)), ("w3", w3, (n_out, MLP_HIDDEN)),
                           ("b3", b3, (n_out,))):
        _shaped(t, shape, name)
    lib = load()
    if m < 1 or not mlp_wide_in_supports(d_in, n_out):
        raise ValueError(f"no wide-input tower kernel for m={m}, d_in={d_in}, n_out={n_out}")
    if w1_packed.numel() != int(lib.rl8_mlp_wide_in_pack_floats(d_in)) or w1_packed.dtype != torch.float32:
        raise ValueError("w1_packed must come from mlp_wide_in_pack_w1 for this d_in")
    if w2_packed.numel() != MLP_HIDDEN * MLP_HIDDEN or w2_packed.dtype != torch.float32:
        raise ValueError("w2_packed must come from mlp_pack_w2")
    out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    h1 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    h2 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    with _timed("mlp_wide_in_forward_save" if save else "mlp_wide_in_forward", m):
        _check(lib.rl8_mlp_wide_in_forward_f32(_ptr(x), m, d_in, _ptr(w1_packed), _ptr(b1.detach()), _ptr(w2_packed),
                                               _ptr(b2.detach()), _ptr(w3.detach()), _ptr(b3.detach()), n_out, _ptr(out),
                                               _ptr(h1), _ptr(h2), _stream()),
               "rl8_mlp_wide_in_forward_f32")
    return out, h1, h2


def mlp_wide_in_backward(h1: torch.Tensor, h2: torch.Tensor, dout: torch.Tensor, w2t_packed: torch.Tensor,
                         w3: torch.Tensor, dz1: torch.Tensor, dz2: torch.Tensor, partials: torch.Tensor) -> int:
    """The data gradient of the ``rows`` = ``h1.shape[0]`` rows: fills ``dz1`` / ``dz2`` ([rows, 256]) and the first
    rows of ``partials`` ([rl8_mlp_wide_in_max_rows, 512 + 257 n_out]: db1 | db2 | dW3 | db3 per workgroup); returns how
    many partial rows were written."""
    rows, n_out = h1.shape[0], w3.shape[0]
    if rows < 1 or not 1 <= n_out <= MLP_MAX_OUT:
        raise ValueError(f"no wide-input tower kernel for m={rows}, n_out={n_out}")
    lib = load()
    width = int(lib.rl8_mlp_wide_in_partial_floats(n_out))
    for name, t, shape in (("h1", h1, (rows, MLP_HIDDEN)), ("h2", h2, (rows, MLP_HIDDEN)), ("dout", dout, (rows, n_out)),
                           ("w3", w3, (n_out, MLP_HIDDEN)), ("dz1", dz1, (rows, MLP_HIDDEN)), ("dz2", dz2, (rows, MLP_HIDDEN)),
                           ("partials", partials, (int(lib.rl8_mlp_wide_in_max_rows()), width))):
        _shaped(t, shape, name)
    if w2t_packed.numel() != MLP_HIDDEN * MLP_HIDDEN or w2t_packed.dtype != torch.float32:
        raise ValueError("w2t_packed must come from mlp_pack_w2(..., transposed=True)")
    written = C.c_int(0)
    with _timed("mlp_wide_in_backward", rows):
        _check(lib.rl8_mlp_wide_in_backward_f32(_ptr(h1), _ptr(h2), _ptr(dout), rows, _ptr(w2t_packed), _ptr(w3.detach()),
                                                n_out, _ptr(dz1), _ptr(dz2), _ptr(partials), C.byref(written), _stream()),
               "rl8_mlp_wide_in_backward_f32")
    return written.value


_wide_in_ws: dict[tuple[int, int], torch.Tensor] = {}


def mlp_wide_in_wgrad(dz1: torch.Tensor, x: torch.Tensor, out: None | torch.Tensor = None, *,
                      accumulate: bool = False) -> torch.Tensor:
    """dW1 [256, d_in] = dz1^T @ x over the M rows (fp32 MFMA, deterministic).  ``out`` with ``accumulate``: added to
    what ``out`` holds (the segments of a long batch, in order)."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    _shaped(dz1, (m, MLP_HIDDEN), "dz1")
    if m < 1 or not mlp_wide_in_supports(d_in, 1):
        raise ValueError(f"no wide-input tower kernel for m={m}, d_in={d_in}")
    lib = load()
    nbytes = int(lib.rl8_mlp_wide_in_workspace_bytes(128))
    ws = _per_stream(_wide_in_ws, x.device, lambda: torch.empty(nbytes // 4, dtype=torch.float32, device=x.device))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(MLP_HIDDEN, d_in, dtype=torch.float32, device=x.device)
    _shaped(out, (MLP_HIDDEN, d_in), "out")
    with _timed("mlp_wide_in_wgrad", m):
        _check(lib.rl8_mlp_wide_in_wgrad_f32(_ptr(dz1), _ptr(x), m, d_in, _ptr(ws), _ptr(out), int(accumulate), _stream()),
               "rl8_mlp_wide_in_wgrad_f32")
    return out


# --------------------------------------------------------------------------- #
# Wide-head towers: hidden width 256, 1 to 128 inputs, heads of 9 to 128 outputs in all (mlp_wide_out_kernels.hip).
# --------------------------------------------------------------------------- #
MLP_WIDE_OUT_W1, MLP_WIDE_OUT_W3, MLP_WIDE_OUT_W3T = 0, 1, 2  # the `matrix` of rl8_mlp_wide_out_pack_f32


def mlp_wide_out_supports(d_in: int, n_out: int) -> bool:
    return bool(load().rl8_mlp_wide_out_supports(int(d_in), int(n_out)))


def _mlp_wide_out_pack(w: torch.Tensor, matrix: int, n: int, name: str) -> torch.Tensor:
    lib = load()
    floats = int(lib.rl8_mlp_wide_out_pack_floats(matrix, n))
    if floats < 0:
        raise ValueError(f"no wide-head tower kernel for a {name} of {tuple(w.shape)}")
    packed = torch.empty(floats, dtype=torch.float32, device=w.device)
    _check(lib.rl8_mlp_wide_out_pack_f32(_ptr(w), matrix, n, _ptr(packed), _stream()), "rl8_mlp_wide_out_pack_f32")
    return packed


def mlp_wide_out_pack_w1(w1: torch.Tensor) -> torch.Tensor:
    """[256, d_in] nn.Linear weight, 1 <= d_in <= 128 -> MFMA fragment order, zero-padded to whole k-groups of 8."""
    w1 = _dense(w1.detach(), torch.float32, "w1")
    if w1.ndim != 2 or w1.shape[0] != MLP_HIDDEN:
        raise ValueError("w1 must be [256, d_in]")
    return _mlp_wide_out_pack(w1, MLP_WIDE_OUT_W1, w1.shape[1], "w1")


def mlp_wide_out_pack_w3(w3: torch.Tensor, *, transposed: bool = False) -> torch.Tensor:
    """[n_out, 256] head weight (the heads of a tower concatenated), 9 <= n_out <= 128 -> MFMA fragment order: the B
    operand of the forward's ``h2 @ w3.T`` (n_out zero-padded to 32-column tiles), or, ``transposed``, of the data
    gradient's ``dout @ w3`` (n_out zero-padded to k-groups of 8)."""
    w3 = _dense(w3.detach(), torch.float32, "w3")
    if w3.ndim != 2 or w3.shape[1] != MLP_HIDDEN:
        raise ValueError("w3 must be [n_out, 256]")
    return _mlp_wide_out_pack(w3, MLP_WIDE_OUT_W3T if transposed else MLP_WIDE_OUT_W3, w3.shape[0], "w3")


def mlp_wide_out_forward(
    x: torch.Tensor, w1_packed: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor, b2: torch.Tensor,
    w3_packed: torch.Tensor, b3: torch.Tensor, *, save: bool = False,
) -> tuple[torch.Tensor, None | torch.Tensor, None | torch.Tensor]:
    """x [M, d_in], 1 <= d_in <= 128 -> out [M, n_out], n_out = ``b3.shape[0]`` in 9..128; with ``save`` also the
    post-ReLU activations h1, h2 ([M, 256]) for the backward pass (``out`` is the same bits either way).  ``w1_packed``
    from ``mlp_wide_out_pack_w1``, ``w2_packed`` from ``mlp_pack_w2``, ``w3_packed`` from ``mlp_wide_out_pack_w3``."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    n_out = b3.shape[0]
    for name, t, shape in (("b1", b1, (MLP_HIDDEN,)), ("b2", b2, (MLP_HIDDEN,)), ("b3", b3, (n_out,))):
        _shaped(t, shape, name)
    lib = load()
    if m < 1 or not mlp_wide_out_supports(d_in, n_out):
        raise ValueError(f"no wide-head tower kernel for m={m}, d_in={d_in}, n_out={n_out}")
    if w1_packed.numel() != int(lib.rl8_mlp_wide_out_pack_floats(MLP_WIDE_OUT_W1, d_in)) or w1_packed.dtype != torch.float32:
        raise ValueError("w1_packed must come from mlp_wide_out_pack_w1 for this d_in")
    if w2_packed.numel() != MLP_HIDDEN * MLP_HIDDEN or w2_packed.dtype != torch.float32:
        raise ValueError("w2_packed must come from mlp_pack_w2")
    if w3_packed.numel() != int(lib.rl8_mlp_wide_out_pack_floats(MLP_WIDE_OUT_W3, n_out)) or w3_packed.dtype != torch.float32:
        raise ValueError("w3_packed must come from mlp_wide_out_pack_w3 for this n_out")
    out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    h1 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    h2 = torch.empty(m, MLP_HIDDEN, dtype=torch.float32, device=x.device) if save else None
    with _timed("mlp_wide_out_forward_save" if save else "mlp_wide_out_forward", m):
        _check(lib.rl8_mlp_wide_out_forward_f32(_ptr(x), m, d_in, _ptr(w1_packed), _ptr(b1.detach()), _ptr(w2_packed),
                                                _ptr(b2.detach()), _ptr(w3_packed), _ptr(b3.detach()), n_out, _ptr(out),
                                                _ptr(h1), _ptr(h2), _stream()),
               "rl8_mlp_wide_out_forward_f32")
    return out, h1, h2


def mlp_wide_out_backward(h1: torch.Tensor, h2: torch.Tensor, dout: torch.Tensor, w2t_packed: torch.Tensor,
                          w3t_packed: torch.Tensor, dz1: torch.Tensor, dz2: torch.Tensor, partials: torch.Tensor) -> int:
    """The data gradient of the ``rows`` = ``h1.shape[0]`` rows: fills ``dz1`` / ``dz2`` ([rows, 256]) and the first
    rows of ``partials`` ([rl8_mlp_wide_out_max_rows, 512 + n_out]: db1 | db2 | db3 per workgroup); returns how many
    partial rows were written.  ``w3t_packed`` from ``mlp_wide_out_pack_w3(w3, transposed=True)``."""
    rows, n_out = h1.shape[0], dout.shape[-1]
    lib = load()
    width = int(lib.rl8_mlp_wide_out_partial_floats(n_out))
    if rows < 1 or width < 0:
        raise ValueError(f"no wide-head tower kernel for m={rows}, n_out={n_out}")
    for name, t, shape in (("h1", h1, (rows, MLP_HIDDEN)), ("h2", h2, (rows, MLP_HIDDEN)), ("dout", dout, (rows, n_out)),
                           ("dz1", dz1, (rows, MLP_HIDDEN)), ("dz2", dz2, (rows, MLP_HIDDEN)),
                           ("partials", partials, (int(lib.rl8_mlp_wide_out_max_rows()), width))):
        _shaped(t, shape, name)
    if w2t_packed.numel() != MLP_HIDDEN * MLP_HIDDEN or w2t_packed.dtype != torch.float32:
        raise ValueError("w2t_packed must come from mlp_pack_w2(..., transposed=True)")
    if w3t_packed.numel() != int(lib.rl8_mlp_wide_out_pack_floats(MLP_WIDE_OUT_W3T, n_out)) or w3t_packed.dtype != torch.float32:
        raise ValueError("w3t_packed must come from mlp_wide_out_pack_w3(..., transposed=True) for this n_out")
    written = C.c_int(0)
    with _timed("mlp_wide_out_backward", rows):
        _check(lib.rl8_mlp_wide_out_backward_f32(_ptr(h1), _ptr(h2), _ptr(dout), rows, _ptr(w2t_packed), _ptr(w3t_packed),
                                                 n_out, _ptr(dz1), _ptr(dz2), _ptr(partials), C.byref(written), _stream()),
               "rl8_mlp_wide_out_backward_f32")
    return written.value


def mlp_wide_out_wgrad(a: torch.Tensor, b: torch.Tensor, out: None | torch.Tensor = None, *, accumulate: bool = False,
                       transpose: bool = False) -> torch.Tensor:
    """[256, c] = a^T @ b over the M rows, a [M, 256], b [M, c], 1 <= c <= 128 (fp32 MFMA, deterministic); with
    ``transpose`` the result is written [c, 256].  ``out`` with ``accumulate``: added to what ``out`` holds (the
    segments of a long batch, in order).  dW1 = ``(dz1, x)``; dW3 = ``(h2, dout, transpose=True)``."""
    b = _dense(b.detach(), torch.float32, "b")
    if b.ndim != 2:
        raise ValueError("b must be [M, c]")
    m, c = b.shape
    _shaped(a, (m, MLP_HIDDEN), "a")
    lib = load()
    nbytes = int(lib.rl8_mlp_wide_out_workspace_bytes(c))
    if m < 1 or nbytes < 0:
        raise ValueError(f"no wide-head tower kernel for m={m}, c={c}")
    # (the slabs of the wide-input towers' dW1: the same size at 128 columns, the same stream order)
    ws = _per_stream(_wide_in_ws, b.device, lambda: torch.empty(int(lib.rl8_mlp_wide_out_workspace_bytes(128)) // 4,
                                                                 dtype=torch.float32, device=b.device))
    shape = (c, MLP_HIDDEN) if transpose else (MLP_HIDDEN, c)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(shape, dtype=torch.float32, device=b.device)
    _shaped(out, shape, "out")
    with _timed("mlp_wide_out_wgrad", m):
        _check(lib.rl8_mlp_wide_out_wgrad_f32(_ptr(a), _ptr(b), m, c, _ptr(ws), _ptr(out), int(accumulate), int(transpose),
                                              _stream()),
               "rl8_mlp_wide_out_wgrad_f32")
    return out


# --------------------------------------------------------------------------- #
# A BatchNorm1d behind the first layer of a narrow tower, folded into that layer (batchnorm_tower_kernels.hip).
# --------------------------------------------------------------------------- #
class TowerLimits(NamedTuple):
    """``rl8_tower_limits``: the moments kernel's workgroup cap and rows per step, the narrow tower kernels' workgroup
    caps at width 64 and 128 and their rows per step. Beyond ``cap x rows`` a workgroup strides."""

    moments_grid_cap: int
    moments_rows: int
    narrow_grid_cap_64: int
    narrow_grid_cap_128: int
    narrow_rows: int


def tower_limits() -> TowerLimits:
    limits = (C.c_int * 5)()
    _check(load().rl8_tower_limits(limits), "rl8_tower_limits")
    return TowerLimits(*(int(v) for v in limits))


def tower_moments(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mu [d_in], C [d_in, d_in])`` of ``x`` [M, d_in <= 16] in float64: the batch mean and the biased covariance, one
    pass over x, bitwise reproducible."""
    x = x.detach()
    _dense(x, torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    lib = load()
    nbytes = int(lib.rl8_tower_moments_workspace_bytes(m, d_in))
    _check(min(nbytes, 0), "rl8_tower_moments_workspace_bytes")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    stats = torch.empty(d_in + d_in * d_in, dtype=torch.float64, device=x.device)
    mu, cov = stats[:d_in], stats[d_in:].view(d_in, d_in)
    with _timed("tower_moments", m):
        _check(lib.rl8_tower_moments_f64(_ptr(x), m, d_in, _ptr(mu), _ptr(cov), _ptr(ws), _stream()),
               "rl8_tower_moments_f64")
    return mu, cov


def batchnorm_fold(w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, *,
                   moments: None | tuple[torch.Tensor, torch.Tensor, int] = None,
                   running_mean: None | torch.Tensor = None, running_var: None | torch.Tensor = None,
                   factor: float = 0.0, tracked: None | torch.Tensor = None) -> tuple[torch.Tensor, ...]:
    """The layer ``BatchNorm1d(Linear(x))`` is on this batch. ``moments`` = ``(mu, C, m)`` (training): returns ``(A, c,
    r, m_z, v)`` -- ``A`` [H, d_in] and ``c`` [H] float32, the statistics float64 -- and moves ``running_mean`` /
    ``running_var`` in place by ``factor`` (by ``1 / tracked`` with the device counter ``tracked`` given). ``moments``
    ``None`` (eval): ``(A, c)`` from the running statistics."""
    w1, b1, gamma, beta = (t.detach() for t in (w1, b1, gamma, beta))
    _dense(w1, torch.float32, "w1")
    if w1.ndim != 2:
        raise ValueError("w1 must be [H, d_in]")
    hidden, d_in = w1.shape
    for name, t in (("b1", b1), ("gamma", gamma), ("beta", beta), ("running_mean", running_mean),
                    ("running_var", running_var)):
        if t is not None:
            _shaped(t, (hidden,), name)
    if tracked is not None:
        _shaped(tracked, (), "tracked", torch.int64)
    a = torch.empty(hidden, d_in, dtype=torch.float32, device=w1.device)
    c = torch.empty(hidden, dtype=torch.float32, device=w1.device)
    if moments is None:
        mu = cov = r = m_z = v = None
        m = 0
    else:
        mu, cov, m = moments
        _shaped(mu, (d_in,), "mu", torch.float64)
        _shaped(cov, (d_in, d_in), "C", torch.float64)
        r, m_z, v = torch.empty(3, hidden, dtype=torch.float64, device=w1.device).unbind(0)
    with _timed("batchnorm_fold", hidden):
        _check(load().rl8_batchnorm_fold_f32(_ptr(mu), _ptr(cov), m, d_in, hidden, _ptr(w1), _ptr(b1), _ptr(gamma),
                                             _ptr(beta), float(eps), _ptr(running_mean), _ptr(running_var),
                                             float(factor), _ptr(tracked), int(moments is not None), _ptr(a), _ptr(c),
                                             _ptr(r), _ptr(m_z), _ptr(v), _stream()), "rl8_batchnorm_fold_f32")
    return (a, c) if moments is None else (a, c, r, m_z, v)


# --------------------------------------------------------------------------- #
# OPT-IN: towers of a scalar observation as piecewise-linear tables (nn/piecewise_mlp.py).
# --------------------------------------------------------------------------- #
def pw_max_breaks() -> int:
    return int(load().rl8_pw_max_breaks())


def pw_tower_forward(x: torch.Tensor, table: torch.Tensor, p: int, n_out: int) -> torch.Tensor:
    """x [M, 1] -> out [M, n_out] from ``table`` = [breaks p | anchor p + 1 | value (p + 1) n | slope (p + 1) n] (fp32)."""
    x = _dense(x.detach(), torch.float32, "x")
    _dense(table, torch.float32, "table")
    m = x.shape[0]
    if x.numel() != m or table.numel() != p + (p + 1) * (1 + 2 * n_out):
        raise ValueError("pw_tower_forward: x must be [M, 1] and the table p + (p + 1) (1 + 2 n_out) floats")
    out = torch.empty(m, n_out, dtype=torch.float32, device=x.device)
    with _timed("pw_tower_forward", m):
        _check(load().rl8_pw_tower_forward_f32(_ptr(x), m, _ptr(table), p, n_out, _ptr(out), _stream()),
               "rl8_pw_tower_forward_f32")
    return out


_pw_ws: dict[tuple, torch.Tensor] = {}


def pw_segment_sums(x: torch.Tensor, dout: torch.Tensor, breaks: torch.Tensor, p: int) -> torch.Tensor:
    """[(p + 1), 2, n_out] fp64: per interval the sums of dout and of dout * x over its rows (exact, order-independent)."""
    x = _dense(x.detach(), torch.float32, "x")
    dout = _dense(dout.detach(), torch.float32, "dout")
    m, n_out = dout.shape
    if x.numel() != m:
        raise ValueError("pw_segment_sums: x must be [M, 1] with M = dout.shape[0]")
    lib = load()
    key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), _stream(), p, n_out)
    ws = _pw_ws.get(key)
    if ws is None:
        _pw_ws.clear()  # (one table shape at a time per process is the common case)
        ws = _pw_ws[key] = torch.empty(int(lib.rl8_pw_workspace_bytes(p, n_out)) // 8 + 2, dtype=torch.int64, device=x.device)
    sums = torch.empty(p + 1, 2, n_out, dtype=torch.float64, device=x.device)
    with _timed("pw_segment_sums", m):
        for lo in range(0, m, 1 << 25):  # (2^25 rows per call: the integer accumulators' headroom)
            hi = min(m, lo + (1 << 25))
            part = sums if lo == 0 else torch.empty_like(sums)
            _check(lib.rl8_pw_segment_sums_f32(_ptr(x[lo:hi]), _ptr(dout[lo:hi]), hi - lo, n_out, _ptr(breaks), p, _ptr(ws),
                                               _ptr(part), _stream()), "rl8_pw_segment_sums_f32")
            if lo:
                sums += part
    return sums


# --------------------------------------------------------------------------- #
# Fused LSTM (a-9): one layer, hidden 256, batch_first.
# --------------------------------------------------------------------------- #
LSTM_HIDDEN = 256


def lstm_supports(d_in: int) -> bool:
    return bool(load().rl8_lstm_supports(int(d_in)))


def _lstm_pack_params(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> int:
    """d_in after the dtype / contiguity / shape checks of a width-256 ``torch.nn.LSTM`` layer's parameters."""
    d_in = w_ih.shape[1]
    for name, t, shape in (("w_ih", w_ih, (4 * LSTM_HIDDEN, d_in)), ("w_hh", w_hh, (4 * LSTM_HIDDEN, LSTM_HIDDEN)),
                           ("b_ih", b_ih, (4 * LSTM_HIDDEN,)), ("b_hh", b_hh, (4 * LSTM_HIDDEN,))):
        _shaped(t, shape, name)
    return d_in


def _lstm_states_256(h0: torch.Tensor, c0: torch.Tensor, b: int) -> None:
    """The dtype / contiguity / shape checks of the width-256 forwards' initial states."""
    for name, t in (("h0", h0), ("c0", c0)):
        _dense(t, torch.float32, name)
        if tuple(t.shape) != (b, LSTM_HIDDEN):
            raise ValueError(f"{name} must be [{b}, {LSTM_HIDDEN}], got {tuple(t.shape)}")


def _lstm_outputs(b: int, l: int, hidden: int, device: torch.device, save: bool,
                  state_out: None | tuple[torch.Tensor, torch.Tensor] = None):
    """(hs [B, L, H], hn, cn [B, H], gates [B, L, 4, H], cs [B, L, H]) for a forward to write: ``gates`` and ``cs``
    only with ``save``; ``hn`` / ``cn`` are the caller's ``state_out`` (checked) where given."""
    def new(*shape: int) -> torch.Tensor:
        return torch.empty(*shape, dtype=torch.float32, device=device)

    hs = new(b, l, hidden)
    if state_out is None:
        hn, cn = new(b, hidden), new(b, hidden)
    else:
        hn, cn = (_shaped(t, (b, hidden), name) for name, t in zip(("hn", "cn"), state_out))
    return hs, hn, cn, new(b, l, 4, hidden) if save else None, new(b, l, hidden) if save else None


def _heads_padded(dout: torch.Tensor, w: torch.Tensor, n: int, rows: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(dout4 [rows, 4], w4 [4, H]) for a backward through time with the heads inside: four floats per row-step and
    four weight rows (one 16-byte piece per sequence and head-row segment), zero-padded from ``n``."""
    dout4 = torch.zeros(rows, ROWS_BACKWARD_HEADS, dtype=torch.float32, device=w.device)
    dout4[:, :n] = dout.detach().reshape(rows, n)
    w4 = torch.zeros(ROWS_BACKWARD_HEADS, w.shape[1], dtype=torch.float32, device=w.device)
    w4[:n] = w.detach()
    return dout4, w4


def lstm_pack(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """torch.nn.LSTM parameters (``weight_ih_l0`` [1024, d], ``weight_hh_l0``
    [1024, 256], ``bias_ih_l0``, ``bias_hh_l0`` [1024]) -> forward weights in MFMA
    fragment order with the input projection and biases folded in."""
    d_in = _lstm_pack_params(w_ih, w_hh, b_ih, b_hh)
    lib = load()
    packed = torch.empty(int(lib.rl8_lstm_pack_floats()), dtype=torch.float32, device=w_hh.device)
    _check(lib.rl8_lstm_pack_f32(_ptr(w_ih.detach()), _ptr(w_hh.detach()), _ptr(b_ih.detach()), _ptr(b_hh.detach()),
                                 d_in, _ptr(packed), _stream()), "rl8_lstm_pack_f32")
    return packed


def lstm_forward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_packed: torch.Tensor, *, save: bool = False):
    """x [B, L, d], h0 / c0 [B, 256] -> (hs [B, L, 256], hn, cn [B, 256], gates, cs);
    ``gates`` [B, L, 4, 256] and ``cs`` [B, L, 256] only with ``save``."""
    x = _dense(x.detach(), torch.float32, "x")
    b, l, d_in = x.shape
    _lstm_states_256(h0, c0, b)
    hs, hn, cn, gates, cs = _lstm_outputs(b, l, LSTM_HIDDEN, x.device, save)
    with _timed("lstm_forward_save" if save else "lstm_forward", b * l):
        _check(load().rl8_lstm_forward_f32(_ptr(x), b, l, d_in, _ptr(h0), _ptr(c0), _ptr(w_packed), _ptr(hs), _ptr(hn),
                                           _ptr(cn), _ptr(gates), _ptr(cs), _stream()), "rl8_lstm_forward_f32")
    return hs, hn, cn, gates, cs


# --------------------------------------------------------------------------- #
# The same LSTM behind 8 to 128 input floats (lstm_wide_in_kernels.hip).
# --------------------------------------------------------------------------- #
def lstm_wide_in_supports(d_in: int) -> bool:
    return bool(load().rl8_lstm_wide_in_supports(int(d_in)))


def lstm_wide_in_pack(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """torch.nn.LSTM parameters (``weight_ih_l0`` [1024, d], 8 <= d <= 128, ``weight_hh_l0`` [1024, 256], the two
    biases [1024]) -> per gate ``[w_hh | w_ih | b_ih + b_hh | 0..]`` in MFMA fragment order, K = 256 + 8 ceil((d + 1) / 8)."""
    d_in = _lstm_pack_params(w_ih, w_hh, b_ih, b_hh)
    lib = load()
    floats = int(lib.rl8_lstm_wide_in_pack_floats(d_in))
    if floats < 0:
        raise ValueError(f"no wide-input LSTM kernel for d_in={d_in}")
    packed = torch.empty(floats, dtype=torch.float32, device=w_hh.device)
    _check(lib.rl8_lstm_wide_in_pack_f32(_ptr(w_ih.detach()), _ptr(w_hh.detach()), _ptr(b_ih.detach()), _ptr(b_hh.detach()),
                                         d_in, _ptr(packed), _stream()), "rl8_lstm_wide_in_pack_f32")
    return packed


def lstm_wide_in_forward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_packed: torch.Tensor, *,
                         save: bool = False):
    """x [B, L, d], 8 <= d <= 128, h0 / c0 [B, 256] -> (hs [B, L, 256], hn, cn [B, 256], gates, cs) as
    :func:`lstm_forward` returns them; ``w_packed`` from :func:`lstm_wide_in_pack` for this ``d``."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 3:
        raise ValueError("x must be [B, L, d_in]")
    b, l, d_in = x.shape
    lib = load()
    if b < 1 or l < 1 or not lstm_wide_in_supports(d_in):
        raise ValueError(f"no wide-input LSTM kernel for b={b}, l={l}, d_in={d_in}")
    _lstm_states_256(h0, c0, b)
    if w_packed.numel() != int(lib.rl8_lstm_wide_in_pack_floats(d_in)) or w_packed.dtype != torch.float32:
        raise ValueError("w_packed must come from lstm_wide_in_pack for this d_in")
    hs, hn, cn, gates, cs = _lstm_outputs(b, l, LSTM_HIDDEN, x.device, save)
    with _timed("lstm_wide_in_forward_save" if save else "lstm_wide_in_forward", b * l):
        _check(lib.rl8_lstm_wide_in_forward_f32(_ptr(x), b, l, d_in, _ptr(h0), _ptr(c0), _ptr(w_packed), _ptr(hs),
                                                _ptr(hn), _ptr(cn), _ptr(gates), _ptr(cs), _stream()),
               "rl8_lstm_wide_in_forward_f32")
    return hs, hn, cn, gates, cs


_lstm_wide_in_ws: dict[tuple[int, int], torch.Tensor] = {}


def lstm_wide_in_wgrad(dgates: torch.Tensor, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(dW_ih [1024, d] = dgates^T @ x, db [1024] = the column sums of dgates) over the M rows of ``dgates`` [M, 1024]
    and ``x`` [M, d], 8 <= d <= 128: one launch and its slab reduction, fp32 MFMA, deterministic."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 2:
        raise ValueError("x must be [M, d_in]")
    m, d_in = x.shape
    _shaped(dgates, (m, 4 * LSTM_HIDDEN), "dgates")
    if m < 1 or not lstm_wide_in_supports(d_in):
        raise ValueError(f"no wide-input LSTM kernel for m={m}, d_in={d_in}")
    lib = load()
    nbytes = int(lib.rl8_lstm_wide_in_workspace_bytes(128))
    ws = _per_stream(_lstm_wide_in_ws, x.device, lambda: torch.empty(nbytes // 4, dtype=torch.float32, device=x.device))
    dw_ih = torch.empty(4 * LSTM_HIDDEN, d_in, dtype=torch.float32, device=x.device)
    db = torch.empty(4 * LSTM_HIDDEN, dtype=torch.float32, device=x.device)
    with _timed("lstm_wide_in_wgrad", m):
        _check(lib.rl8_lstm_wide_in_wgrad_f32(_ptr(dgates), _ptr(x), m, d_in, _ptr(ws), _ptr(dw_ih), _ptr(db), _stream()),
               "rl8_lstm_wide_in_wgrad_f32")
    return dw_ih, db


# --------------------------------------------------------------------------- #
# The layers above the first of a width-256 stack: their input is the layer below's hs (lstm_stack256_kernels.hip).
# --------------------------------------------------------------------------- #
def lstm_stack256_supports() -> bool:
    return bool(load().rl8_lstm_stack256_supports())


def lstm_stack256_pack(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """An upper layer's torch.nn.LSTM parameters (``weight_ih_lk``, ``weight_hh_lk`` [1024, 256], the two biases
    [1024]) -> per gate ``[w_hh | w_ih | b_ih + b_hh | 0 x 7]`` in MFMA fragment order, K = 520."""
    if _lstm_pack_params(w_ih, w_hh, b_ih, b_hh) != LSTM_HIDDEN:
        raise ValueError(f"w_ih must be [1024, {LSTM_HIDDEN}]")
    lib = load()
    packed = torch.empty(int(lib.rl8_lstm_stack256_pack_floats()), dtype=torch.float32, device=w_hh.device)
    _check(lib.rl8_lstm_stack256_pack_f32(_ptr(w_ih.detach()), _ptr(w_hh.detach()), _ptr(b_ih.detach()), _ptr(b_hh.detach()),
                                          _ptr(packed), _stream()), "rl8_lstm_stack256_pack_f32")
    return packed


def lstm_stack256_forward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_packed: torch.Tensor, *,
                          save: bool = False, state_out: None | tuple[torch.Tensor, torch.Tensor] = None):
    """x [B, L, 256] (the layer below's ``hs``), h0 / c0 [B, 256] -> (hs [B, L, 256], hn, cn [B, 256], gates, cs) as
    :func:`lstm_forward` returns them; ``w_packed`` from :func:`lstm_stack256_pack`. ``state_out``: the caller's
    ``(hn, cn)`` to write."""
    x = _dense(x.detach(), torch.float32, "x")
    if x.ndim != 3 or x.shape[2] != LSTM_HIDDEN or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x must be [B, L, {LSTM_HIDDEN}]")
    b, l = x.shape[0], x.shape[1]
    lib = load()
    _lstm_states_256(h0, c0, b)
    if w_packed.numel() != int(lib.rl8_lstm_stack256_pack_floats()) or w_packed.dtype != torch.float32:
        raise ValueError("w_packed must come from lstm_stack256_pack")
    hs, hn, cn, gates, cs = _lstm_outputs(b, l, LSTM_HIDDEN, x.device, save, state_out)
    with _timed("lstm_stack256_forward_save" if save else "lstm_stack256_forward", b * l):
        _check(lib.rl8_lstm_stack256_forward_f32(_ptr(x), b, l, _ptr(h0), _ptr(c0), _ptr(w_packed), _ptr(hs), _ptr(hn),
                                                 _ptr(cn), _ptr(gates), _ptr(cs), _stream()),
               "rl8_lstm_stack256_forward_f32")
    return hs, hn, cn, gates, cs


_lstm_stack256_ws: dict[tuple[int, int], torch.Tensor] = {}


def lstm_stack256_dx(dgates: torch.Tensor, wiht_packed: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(dx [M, 256] = dgates @ w_ih, db [1024] = the column sums of dgates) from one read of ``dgates`` [M, 1024];
    ``wiht_packed`` = :func:`lstm_pack_transposed` of the layer's ``weight_ih_lk`` [1024, 256]. fp32 MFMA; the column
    sums in fp32 per workgroup, then over the workgroups in order in fp64: deterministic."""
    dgates = _dense(dgates, torch.float32, "dgates")
    if dgates.ndim != 2 or dgates.shape[1] != 4 * LSTM_HIDDEN or dgates.shape[0] < 1:
        raise ValueError("dgates must be [M, 1024]")
    if wiht_packed.numel() != 4 * LSTM_HIDDEN * LSTM_HIDDEN or wiht_packed.dtype != torch.float32:
        raise ValueError("wiht_packed must come from lstm_pack_transposed(weight_ih)")
    m, lib, dev = dgates.shape[0], load(), dgates.device
    nbytes = int(lib.rl8_lstm_stack256_workspace_bytes(1 << 40))  # (the widest grid: one workspace per stream)
    ws = _per_stream(_lstm_stack256_ws, dev, lambda: torch.empty(nbytes // 4, dtype=torch.float32, device=dev))
    dx = torch.empty(m, LSTM_HIDDEN, dtype=torch.float32, device=dev)
    db = torch.empty(4 * LSTM_HIDDEN, dtype=torch.float32, device=dev)
    with _timed("lstm_stack256_dx", m):
        _check(lib.rl8_lstm_stack256_dx_f32(_ptr(dgates), m, _ptr(wiht_packed), _ptr(ws), _ptr(dx), _ptr(db), _stream()),
               "rl8_lstm_stack256_dx_f32")
    return dx, db


def lstm_stack256_backward(below: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, hs: torch.Tensor, gates: torch.Tensor,
                           cs: torch.Tensor, dhs: torch.Tensor, whht_packed: None | torch.Tensor,
                           wiht_packed: torch.Tensor, *, wgrad: str, rows_packed: None | torch.Tensor = None,
                           h0_bound: None | torch.Tensor = None) -> dict[str, torch.Tensor]:
    """The backward of a layer above the first of a width-256 stack: ``below`` [B, L, 256] is the layer below's ``hs``,
    the rest what :func:`lstm_stack256_forward` saved. :func:`lstm_backward`'s backward through time and ``W_hh``
    loop on its ``wgrad`` route; ``w_ih`` = dgates^T @ below from one more accumulation of that route's entry over all
    B * L rows; ``b`` and ``dx`` [B, L, 256] -- dL/dhs of the layer below -- from :func:`lstm_stack256_dx`."""
    return lstm_backward(below, h0, c0, hs, gates, cs, dhs, whht_packed, wgrad=wgrad, rows_packed=rows_packed,
                         h0_bound=h0_bound, hs_bound=1.0, wide_in=True, upper=wiht_packed)


# --------------------------------------------------------------------------- #
# Narrow LSTMs: one layer (or layer 0 of a stack), hidden width 64 or 128, d_in <= 16 (lstm_narrow_kernels.hip).
# --------------------------------------------------------------------------- #
LSTM_NARROW_HIDDEN = (64, 128)


def lstm_narrow_supports(hidden: int, d_in: int) -> bool:
    return bool(load().rl8_lstm_narrow_supports(int(hidden), int(d_in)))


def _lstm_layer_params(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_ih: None | torch.Tensor, w_hh: torch.Tensor,
                       b_ih: None | torch.Tensor, b_hh: None | torch.Tensor, *,
                       upper: bool = False) -> tuple[int, int, int, int]:
    """(b, l, d_in, hidden) after the dtype / contiguity / shape checks of the narrow LSTM entries (``x`` [B, L, d_in],
    H from ``w_hh``) or, with ``upper``, of the stacked ones (``x`` [B, L, H], the lower layer's hs: d_in = H). A
    parameter the entry does not read is None."""
    _dense(x, torch.float32, "x")
    if x.ndim != 3:
        raise ValueError("x must be [B, L, H]" if upper else "x must be [B, L, d_in]")
    b, l, d_in = x.shape
    hidden = d_in if upper else w_hh.shape[1] if w_hh.ndim == 2 else -1
    shapes = (("h0", h0, (b, hidden)), ("c0", c0, (b, hidden)), ("w_ih", w_ih, (4 * hidden, d_in)),
              ("w_hh", w_hh, (4 * hidden, hidden)), ("b_ih", b_ih, (4 * hidden,)), ("b_hh", b_hh, (4 * hidden,)))
    for name, t, shape in shapes:
        if t is not None:
            _shaped(t, shape, name)
    if b < 1 or l < 1 or not (lstm_stack_supports(hidden) if upper else lstm_narrow_supports(hidden, d_in)):
        raise ValueError(f"no stacked LSTM kernel for b={b}, l={l}, hidden={hidden}" if upper else
                         f"no narrow LSTM kernel for b={b}, l={l}, hidden={hidden}, d_in={d_in}")
    return b, l, d_in, hidden


def lstm_narrow_forward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
                        b_ih: torch.Tensor, b_hh: torch.Tensor, *, save: bool = False,
                        state_out: None | tuple[torch.Tensor, torch.Tensor] = None):
    """x [B, L, d], h0 / c0 [B, H] (H = 64 or 128) -> (hs [B, L, H], hn, cn [B, H], gates, cs); ``gates``
    [B, L, 4, H] (post-activation, order i, f, g, o) and ``cs`` [B, L, H] only with ``save``. ``state_out``: the
    (hn, cn) tensors to write (layer 0 of a stack writes its rows of the stack's states)."""
    x, h0, c0, w_ih, w_hh, b_ih, b_hh = (t.detach() for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh))
    b, l, d_in, hidden = _lstm_layer_params(x, h0, c0, w_ih, w_hh, b_ih, b_hh)
    hs, hn, cn, gates, cs = _lstm_outputs(b, l, hidden, x.device, save, state_out)
    with _timed("lstm_narrow_forward", b * l):
        _check(load().rl8_lstm_narrow_forward_f32(_ptr(x), b, l, d_in, _ptr(h0), _ptr(c0), _ptr(w_ih), _ptr(w_hh),
                                                  _ptr(b_ih), _ptr(b_hh), hidden, _ptr(hs), _ptr(hn), _ptr(cn),
                                                  _ptr(gates), _ptr(cs), _stream()), "rl8_lstm_narrow_forward_f32")
    return hs, hn, cn, gates, cs


def lstm_narrow_backward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_hh: torch.Tensor, hs: torch.Tensor,
                         gates: torch.Tensor, cs: torch.Tensor, dhs: None | torch.Tensor, *,
                         heads: None | tuple[torch.Tensor, torch.Tensor] = None,
                         w_ih: None | torch.Tensor = None) -> dict[str, torch.Tensor]:
    """Gradients ("w_ih", "w_hh", "b": of b_ih and b_hh alike) for dL/dhs ``dhs`` [B, L, H], from what
    :func:`lstm_narrow_forward` saved: backward through time, partial slabs per sequence chunk summed in a fixed
    order (deterministic). No gradient for h0, c0. ``heads`` = (dout [B * L, n], w [n, H]), n <= 4, instead of
    ``dhs`` (None): dL/dh_t = dout x w is formed inside the backward through time (rl8_lstm_narrow_backward_heads_f32).
    ``w_ih`` [4H, d_in] given: one more launch (rl8_lstm_narrow_input_grad_f32, timed as "lstm_narrow_input_grad")
    forms "dx" [B, L, d_in] = dz x w_ih, the gradient of x, from the gate gradients in the workspace, which are then
    returned as well ("dz" [B, L, 4, H], a view of the workspace). Without it: no gradient for x, nothing more launched
    or allocated."""
    if (heads is None) == (dhs is None):
        raise ValueError("lstm_narrow_backward: either dhs or heads")
    x, h0, c0, w_hh, hs, gates, cs = (t.detach() for t in (x, h0, c0, w_hh, hs, gates, cs))
    b, l, d_in, hidden = _lstm_layer_params(x, h0, c0, None, w_hh, None, None)
    for name, t, shape in (("hs", hs, (b, l, hidden)), ("gates", gates, (b, l, 4, hidden)), ("cs", cs, (b, l, hidden)),
                           *([("dhs", dhs.detach(), (b, l, hidden))] if heads is None else [])):
        _shaped(t, shape, name)
    lib = load()
    ws = torch.empty(int(lib.rl8_lstm_narrow_workspace_bytes(b, l, hidden, d_in)) // 4, dtype=torch.float32,
                     device=x.device)
    sizes = (4 * hidden * d_in, 4 * hidden * hidden, 4 * hidden)
    grads = torch.empty(sum(sizes), dtype=torch.float32, device=x.device)
    if heads is not None:
        dout, w = heads
        n = w.shape[0] if w.ndim == 2 else -1
        if not 1 <= n <= ROWS_BACKWARD_HEADS or tuple(w.shape) != (n, hidden) or dout.numel() != b * l * n \
                or dout.dtype != torch.float32 or w.dtype != torch.float32:
            raise ValueError(f"heads: float32 dout [B * L, n], w [n, {hidden}], n <= {ROWS_BACKWARD_HEADS}")
        dout4, w4 = _heads_padded(dout, w, n, b * l)
        with _timed("lstm_narrow_backward", b * l):  # (one name for both forms, as "lstm_rows_backward" is at 256)
            _check(lib.rl8_lstm_narrow_backward_heads_f32(_ptr(x), b, l, d_in, _ptr(h0), _ptr(c0), _ptr(w_hh), hidden,
                                                          _ptr(hs), _ptr(gates), _ptr(cs), _ptr(dout4), _ptr(w4),
                                                          _ptr(ws), _stream()), "rl8_lstm_narrow_backward_heads_f32")
    else:
        with _timed("lstm_narrow_backward", b * l):
            _check(lib.rl8_lstm_narrow_backward_f32(_ptr(x), b, l, d_in, _ptr(h0), _ptr(c0), _ptr(w_hh), hidden,
                                                    _ptr(hs), _ptr(gates), _ptr(cs), _ptr(dhs.detach()), _ptr(ws),
                                                    _stream()), "rl8_lstm_narrow_backward_f32")
    with _timed("lstm_narrow_reduce", b * l):
        _check(lib.rl8_lstm_narrow_reduce_f32(_ptr(ws), b, l, hidden, d_in, _ptr(grads), _stream()),
               "rl8_lstm_narrow_reduce_f32")
    w_ih_grad, w_hh_grad, db = torch.split(grads, sizes)
    out = {"w_ih": w_ih_grad.view(4 * hidden, d_in), "w_hh": w_hh_grad.view(4 * hidden, hidden), "b": db}
    if w_ih is not None:
        w_ih = _shaped(w_ih.detach(), (4 * hidden, d_in), "w_ih")
        dx = torch.empty(b, l, d_in, dtype=torch.float32, device=x.device)
        with _timed("lstm_narrow_input_grad", b * l):
            _check(lib.rl8_lstm_narrow_input_grad_f32(_ptr(ws), b, l, d_in, _ptr(w_ih), hidden, _ptr(dx), _stream()),
                   "rl8_lstm_narrow_input_grad_f32")
        out["dx"] = dx
        out["dz"] = ws[:b * l * 4 * hidden].view(b, l, 4, hidden)
    return out


# --------------------------------------------------------------------------- #
# Stacked LSTMs: layers 1.. of a hidden-64 / 128 LSTM, whose input is the lower layer's hs (lstm_narrow_stack_*
# kernels of lstm_narrow_kernels.hip). One upper layer per call; layer 0 runs the narrow entries above.
# --------------------------------------------------------------------------- #
def lstm_stack_supports(hidden: int) -> bool:
    return bool(load().rl8_lstm_stack_supports(int(hidden)))


def lstm_stack_forward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
                       b_ih: torch.Tensor, b_hh: torch.Tensor, *, save: bool = False,
                       zin: None | torch.Tensor = None,
                       state_out: None | tuple[torch.Tensor, torch.Tensor] = None):
    """One upper layer: x [B, L, H] (the lower layer's hs), h0 / c0 [B, H] -> (hs [B, L, H], hn, cn [B, H], gates,
    cs) as :func:`lstm_narrow_forward`. ``zin``: [B, L, 4, H] floats of scratch for the input projection (made here
    when None; a stack hands the same one to every layer)."""
    x, h0, c0, w_ih, w_hh, b_ih, b_hh = (t.detach() for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh))
    b, l, _, hidden = _lstm_layer_params(x, h0, c0, w_ih, w_hh, b_ih, b_hh, upper=True)
    if zin is None:
        zin = torch.empty(b, l, 4, hidden, dtype=torch.float32, device=x.device)
    _shaped(zin, (b, l, 4, hidden), "zin")
    hs, hn, cn, gates, cs = _lstm_outputs(b, l, hidden, x.device, save, state_out)
    with _timed("lstm_stack_forward", b * l):
        _check(load().rl8_lstm_stack_forward_f32(_ptr(x), b, l, _ptr(h0), _ptr(c0), _ptr(w_ih), _ptr(w_hh), _ptr(b_ih),
                                                 _ptr(b_hh), hidden, _ptr(zin), _ptr(hs), _ptr(hn), _ptr(cn),
                                                 _ptr(gates), _ptr(cs), _stream()), "rl8_lstm_stack_forward_f32")
    return hs, hn, cn, gates, cs


def lstm_stack_backward(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
                        hs: torch.Tensor, gates: torch.Tensor, cs: torch.Tensor,
                        dhs: torch.Tensor) -> dict[str, torch.Tensor]:
    """Gradients ("w_ih", "w_hh", "b": of b_ih and b_hh alike) of one upper layer and "dx" [B, L, H] = dL/dx (the
    lower layer's dL/dhs) for ``dhs`` [B, L, H], from what :func:`lstm_stack_forward` saved (deterministic). No
    gradient for h0, c0."""
    x, h0, c0, w_ih, w_hh, hs, gates, cs, dhs = (t.detach() for t in (x, h0, c0, w_ih, w_hh, hs, gates, cs, dhs))
    b, l, _, hidden = _lstm_layer_params(x, h0, c0, w_ih, w_hh, None, None, upper=True)
    for name, t, shape in (("hs", hs, (b, l, hidden)), ("gates", gates, (b, l, 4, hidden)), ("cs", cs, (b, l, hidden)),
                           ("dhs", dhs, (b, l, hidden))):
        _shaped(t, shape, name)
    lib = load()
    ws = torch.empty(int(lib.rl8_lstm_stack_workspace_bytes(b, l, hidden)) // 4, dtype=torch.float32, device=x.device)
    sizes = (4 * hidden * hidden, 4 * hidden * hidden, 4 * hidden)
    grads = torch.empty(sum(sizes), dtype=torch.float32, device=x.device)
    dx = torch.empty(b, l, hidden, dtype=torch.float32, device=x.device)
    with _timed("lstm_stack_backward", b * l):
        _check(lib.rl8_lstm_stack_backward_f32(_ptr(x), b, l, _ptr(h0), _ptr(c0), _ptr(w_ih), _ptr(w_hh), hidden,
                                               _ptr(hs), _ptr(gates), _ptr(cs), _ptr(dhs), _ptr(ws), _ptr(dx),
                                               _stream()), "rl8_lstm_stack_backward_f32")
    with _timed("lstm_stack_reduce", b * l):
        _check(lib.rl8_lstm_stack_reduce_f32(_ptr(ws), b, l, hidden, _ptr(grads), _stream()),
               "rl8_lstm_stack_reduce_f32")
    w_ih_grad, w_hh_grad, db = torch.split(grads, sizes)
    return {"w_ih": w_ih_grad.view(4 * hidden, hidden), "w_hh": w_hh_grad.view(4 * hidden, hidden), "b": db,
            "dx": dx}


def lstm_split_supports(d_in: int) -> bool:
    return bool(load().rl8_lstm_split_supports(int(d_in)))


def lstm_pack_split(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor):
    """torch.nn.LSTM parameters -> (W_hh as bf16 planes in the step kernel's fragment order,
    ``wb`` [1024, 8] = [w_ih | 0.. | b_ih + b_hh])."""
    d_in = _lstm_pack_params(w_ih, w_hh, b_ih, b_hh)
    lib = load()
    packed = torch.empty(int(lib.rl8_lstm_split_packed_bytes()), dtype=torch.uint8, device=w_hh.device)
    wb = torch.empty(int(lib.rl8_lstm_split_wb_floats()), dtype=torch.float32, device=w_hh.device)
    _check(lib.rl8_lstm_pack_split(_ptr(w_ih.detach()), _ptr(w_hh.detach()), _ptr(b_ih.detach()), _ptr(b_hh.detach()),
                                   d_in, _ptr(packed), _ptr(wb), _stream()), "rl8_lstm_pack_split")
    return packed, wb


def lstm_state_planes(rows: int, device: torch.device | str, copies: int = 1) -> torch.Tensor:
    """``copies`` buffers (whole 128-row tiles each) for the bf16 planes of ``rows`` rows of
    hidden state; a multi-step forward ping-pongs between two."""
    return torch.empty(copies * int(load().rl8_lstm_split_state_bytes(int(rows))), dtype=torch.uint8, device=device)


def lstm_split_state(h: torch.Tensor, *, out: None | torch.Tensor = None,
                     bound_out: None | torch.Tensor = None) -> torch.Tensor:
    """``h`` [B, 256] -> its fp16 planes in the step kernel's operand order (``out`` or a fresh buffer);
    ``bound_out`` (one float32 element) receives max |h|. ``h`` may be of any finite size (a caller's ``h0``): from
    max |h| = 2 up the planes carry a power of two of their own, kept in the buffer's last sixteen bytes, where the
    step kernel reads it (include/rl8_amd.h has the envelope)."""
    h = _dense(h, torch.float32, "h")
    b, dev, lib = h.shape[0], h.device, load()
    if h.ndim != 2 or h.shape[1] != LSTM_HIDDEN:
        raise ValueError("lstm_split_state: h must be [B, 256]")
    if out is None:
        out = lstm_state_planes(b, dev)
    elif out.dtype != torch.uint8 or out.device != dev or out.numel() < int(lib.rl8_lstm_split_state_bytes(b)):
        raise ValueError("lstm_split_state: `out` must hold the planes of b rows")
    if bound_out is not None:
        if bound_out.dtype != torch.float32 or bound_out.numel() != 1 or bound_out.device != dev:
            raise ValueError("bound_out must be one float32 element on h's device")
        _check(lib.rl8_lstm_split_state_bound(_ptr(h), LSTM_HIDDEN, b, _ptr(out), _ptr(bound_out), _stream()),
               "rl8_lstm_split_state_bound")
    else:
        _check(lib.rl8_lstm_split_state(_ptr(h), LSTM_HIDDEN, b, _ptr(out), _stream()), "rl8_lstm_split_state")
    return out


def lstm_forward_split(x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, packed: torch.Tensor, wb: torch.Tensor,
                       *, save: bool = False, planes: None | torch.Tensor = None,
                       h0_bound_out: None | torch.Tensor = None, h0_planes: None | torch.Tensor = None):
    """As :func:`lstm_forward` on the fp16-plane step kernel: one state split + one step
    launch per timestep. Same outputs and saved layouts (``gates`` [B, L, 4, 256], ``cs``).
    ``h0_bound_out`` (one float32 element): receives max |h0|, which the state split sees
    anyway (:func:`lstm_backward`'s ``h0_bound``). ``h0_planes``: the planes of ``h0`` from an
    earlier :func:`lstm_split_state` (read only; no split is made here)."""
    x = _dense(x.detach(), torch.float32, "x")
    b, l, d_in = x.shape
    _lstm_states_256(h0, c0, b)
    dev, lib = x.device, load()
    hs = torch.empty(b, l, LSTM_HIDDEN, dtype=torch.float32, device=dev)
    cs = torch.empty(b, l, LSTM_HIDDEN, dtype=torch.float32, device=dev)
    gates = torch.empty(b, l, 4, LSTM_HIDDEN, dtype=torch.float32, device=dev) if save else None
    if planes is None:
        planes = lstm_state_planes(b, dev, copies=2 if l > 1 else 1)
    # two plane buffers: a step reads h_{t-1}'s planes from one and leaves h_t's in the other
    half = planes.numel() // 2 if l > 1 else 0
    if l > 1 and half < int(lib.rl8_lstm_split_state_bytes(b)):
        raise ValueError("lstm_forward_split: `planes` must hold two state-plane buffers for L > 1")
    H, stream = LSTM_HIDDEN, _stream()
    xp, hsp, csp, gp, pp = _ptr(x), _ptr(hs), _ptr(cs), _ptr(gates), _ptr(planes)
    if h0_planes is not None:
        if h0_bound_out is not None:
            raise ValueError("lstm_forward_split: h0_bound_out comes from the split that made h0_planes")
        if h0_planes.dtype != torch.uint8 or h0_planes.device != dev or h0_planes.numel() < int(lib.rl8_lstm_split_state_bytes(b)):
            raise ValueError("lstm_forward_split: h0_planes must hold the planes of b rows")
    else:
        lstm_split_state(h0, out=planes, bound_out=h0_bound_out)
    for t in range(l):
        c_prev, c_pitch = (_ptr(c0), H) if t == 0 else (csp + (t - 1) * H * 4, l * H)
        p_in, p_out = pp + (t & 1) * half, (pp + ((t + 1) & 1) * half) if t + 1 < l else None
        if t == 0 and h0_planes is not None:
            p_in = _ptr(h0_planes)
        with _timed("lstm_step_save" if save else "lstm_step", b):
            _check(lib.rl8_lstm_step_split_f32(
                xp + t * d_in * 4, l * d_in, d_in, p_in, c_prev, c_pitch, _ptr(packed), _ptr(wb), b,
                hsp + t * H * 4, l * H, csp + t * H * 4, l * H, (gp + t * 4 * H * 4) if save else None, l * 4 * H,
                p_out, stream), "rl8_lstm_step_split_f32")
    hn, cn = hs[:, l - 1], cs[:, l - 1]
    return hs, hn, cn, gates, (cs if save else None)


def lstm_pack_transposed(w_hh: torch.Tensor) -> torch.Tensor:
    """``weight_hh_l0`` [1024, 256] -> the four gate blocks packed for the backward
    data-gradient product (``rl8_mlp_pack_w2_f32(..., transposed=1)`` per gate)."""
    w_hh = _dense(w_hh.detach(), torch.float32, "w_hh")
    if tuple(w_hh.shape) != (4 * LSTM_HIDDEN, LSTM_HIDDEN):
        raise ValueError("w_hh must be [1024, 256]")
    return torch.cat([mlp_pack_w2(w_hh[LSTM_HIDDEN * q : LSTM_HIDDEN * (q + 1)], transposed=True) for q in range(4)])


def lstm_rows_backward_pack(w_hh: torch.Tensor) -> torch.Tensor:
    """``w_hh`` [1024, 256] -> the bf16 planes of ``W_hh^T`` in the order
    ``rl8_lstm_rows_backward_f32`` streams them."""
    w_hh = _dense(w_hh.detach(), torch.float32, "w_hh")
    if tuple(w_hh.shape) != (4 * LSTM_HIDDEN, LSTM_HIDDEN):
        raise ValueError("w_hh must be [1024, 256]")
    lib = load()
    packed = torch.empty(int(lib.rl8_lstm_rows_backward_pack_bytes()), dtype=torch.uint8, device=w_hh.device)
    _check(lib.rl8_lstm_rows_backward_pack(_ptr(w_hh), _ptr(packed), _stream()), "rl8_lstm_rows_backward_pack")
    return packed


ROWS_BACKWARD_HEADS = 4  # head outputs rl8_lstm_rows_backward_heads_f32 takes


def lstm_rows_backward(c0: torch.Tensor, gates: torch.Tensor, cs: torch.Tensor, dhs: None | torch.Tensor,
                       packed: torch.Tensor, *, with_bound: bool = False,
                       heads: None | tuple[torch.Tensor, torch.Tensor] = None):
    """dgates [B, L, 4, 256] from what the forward saved and dhs [B, L, 256]: the
    backward through time with the recurrent product on bf16 planes. ``with_bound``:
    also a one-element device tensor holding max |dgates| (what the fp16-plane weight
    gradient scales its first operand by). ``heads`` = (dout [B * L, n], w [n, 256]),
    n <= 4, instead of ``dhs`` (None): dL/dh_t = dout x w is formed inside the kernel."""
    b, l = gates.shape[0], gates.shape[1]
    checks = [("c0", c0, (b, LSTM_HIDDEN)), ("gates", gates, (b, l, 4, LSTM_HIDDEN)), ("cs", cs, (b, l, LSTM_HIDDEN))]
    if heads is None:
        checks.append(("dhs", dhs, (b, l, LSTM_HIDDEN)))
    elif dhs is not None:
        raise ValueError("lstm_rows_backward: either dhs or heads")
    for name, t, shape in checks:
        _shaped(t, shape, name)
    dev = gates.device
    dgates = torch.empty(b, l, 4, LSTM_HIDDEN, dtype=torch.float32, device=dev)
    dc = torch.empty(b, LSTM_HIDDEN, dtype=torch.float32, device=dev)
    bound = torch.empty(1, dtype=torch.float32, device=dev) if with_bound else None
    if heads is not None:
        dout, w = heads
        n = w.shape[0]
        if n > ROWS_BACKWARD_HEADS or tuple(w.shape) != (n, LSTM_HIDDEN) or dout.numel() != b * l * n:
            raise ValueError(f"heads: dout [B * L, n], w [n, 256], n <= {ROWS_BACKWARD_HEADS}")
        dout4, w4 = _heads_padded(dout, w, n, b * l)
        with _timed("lstm_rows_backward", b * l):
            _check(load().rl8_lstm_rows_backward_heads_f32(b, l, _ptr(c0), _ptr(gates), _ptr(cs), _ptr(dout4), _ptr(w4),
                                                           _ptr(packed), _ptr(dgates), _ptr(dc), _ptr(bound), _stream()),
                   "rl8_lstm_rows_backward_heads_f32")
        return (dgates, bound) if with_bound else dgates
    with _timed("lstm_rows_backward", b * l):
        _check(load().rl8_lstm_rows_backward_f32(b, l, _ptr(c0), _ptr(gates), _ptr(cs), _ptr(dhs), _ptr(packed),
                                                 _ptr(dgates), _ptr(dc), _ptr(bound), _stream()), "rl8_lstm_rows_backward_f32")
    return (dgates, bound) if with_bound else dgates


#: column-sum partial rows of the plane LSTM weight gradients, per (device, stream, L, d_in[, "gates"])
_lstm_colsum_ws: dict[tuple, torch.Tensor] = {}
#: fewest sequences the four-gate weight-gradient launch takes (rl8_lstm_wgrad_f16_f32)
LSTM_WGRAD_GATES_MIN_ROWS = 128
#: rows one launch of a weight-gradient kernel sums (tower_launch.hip.h: kWgradSegmentRows)
WGRAD_SEGMENT_ROWS = 1 << 23


def lstm_backward(
    x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, hs: torch.Tensor, gates: torch.Tensor, cs: torch.Tensor,
    dhs: None | torch.Tensor, whht_packed: None | torch.Tensor, *, wgrad: None | str = None, split: bool = True,
    rows_packed: None | torch.Tensor = None, h0_bound: None | torch.Tensor = None,
    heads: None | tuple[torch.Tensor, torch.Tensor] = None, hs_bound: None | float = None, wide_in: bool = False,
    upper: None | torch.Tensor = None,
) -> dict[str, torch.Tensor]:
    """Parameter gradients of the LSTM given ``dhs`` [B, L, 256] (gradient of every
    ``h_t``) and what ``lstm_forward(..., save=True)`` returned. Returns ``w_ih``,
    ``w_hh``, ``b`` (the gradient of each of the two bias vectors). ``wgrad``: the weight
    gradient's route (``fused_lstm._plan``) -- "f16-gates" (four gates per launch, from
    ``LSTM_WGRAD_GATES_MIN_ROWS`` sequences) or "f16" (one) on fp16 planes scaled by the bound on
    |dG| the ``rows_packed`` kernel leaves, "bf16" on exact planes (these three sum dW_ih and the
    bias too, at the widths of :func:`lstm_split_supports`), "f32" on the fp32 MFMA. None: "f32"
    with ``split=False``, else the fp16 routes behind ``rows_packed``, "bf16" behind ``whht_packed``.
    ``rows_packed`` (:func:`lstm_rows_backward_pack`): the backward through time runs
    on bf16 planes too (``rl8_lstm_rows_backward_f32``) instead of the fp32-MFMA kernel
    that reads ``whht_packed``. ``h0_bound``: one float32 element >= max |h0| when the caller
    has it (:func:`lstm_forward_split`'s ``h0_bound_out``); computed here otherwise.
    ``heads`` (with ``rows_packed``, ``dhs`` None): see :func:`lstm_rows_backward`.
    ``hs_bound``: a number >= max |hs| the caller vouches for -- 1.0 when ``hs`` is this LSTM's own output
    (|o * tanh(c)| < 1), which is what ``nn.fused_lstm`` passes; None: taken from ``hs`` here (one reduction over it).
    The fp16 planes of the weight gradient are scaled by it: a value above the bound would overflow them.
    ``wide_in``: ``x`` is 8 to 128 floats wide (what :func:`lstm_wide_in_forward` saved): without ``rows_packed`` the
    backward through time is ``rl8_lstm_backward_dgates_f32``, every ``W_hh`` launch runs without column sums (no
    per-step copies of ``x``), and ``w_ih`` / ``b`` come from one :func:`lstm_wide_in_wgrad` launch over all rows.
    ``upper`` (with ``wide_in``; :func:`lstm_stack256_backward`): this is a layer above the first of a stack, ``x`` the 256-wide
    ``hs`` of the layer below and ``upper`` its ``weight_ih`` from :func:`lstm_pack_transposed`: ``w_ih`` comes from one
    more accumulation of the route's entry over all B * L rows, ``b`` and "dx" [B, L, 256] from :func:`lstm_stack256_dx`."""
    x = _dense(x.detach(), torch.float32, "x")
    b, l, d_in = x.shape
    if upper is not None and not (wide_in and d_in == LSTM_HIDDEN):
        raise ValueError(f"lstm_backward: upper needs wide_in and x [B, L, {LSTM_HIDDEN}]")
    if wide_in and upper is None and not lstm_wide_in_supports(d_in):
        raise ValueError(f"lstm_backward: wide_in with d_in={d_in}")
    if heads is not None and (rows_packed is None or dhs is not None):
        raise ValueError("lstm_backward: heads needs rows_packed and no dhs")
    for name, t, shape in (("h0", h0, (b, LSTM_HIDDEN)), ("c0", c0, (b, LSTM_HIDDEN)), ("hs", hs, (b, l, LSTM_HIDDEN)),
                           ("gates", gates, (b, l, 4, LSTM_HIDDEN)), ("cs", cs, (b, l, LSTM_HIDDEN)),
                           *([("dhs", dhs, (b, l, LSTM_HIDDEN))] if heads is None else [])):
        _shaped(t, shape, name)
    if wgrad is None:
        wgrad = ("f32" if not split else "bf16" if rows_packed is None else
                 "f16-gates" if b >= LSTM_WGRAD_GATES_MIN_ROWS else "f16")
    name = {"f16-gates": "rl8_lstm_wgrad_f16_f32", "f16": "rl8_mlp_wgrad_f16_strided_f32",  # the route's entry point
            "bf16": "rl8_mlp_wgrad_split_strided_f32", "f32": "rl8_mlp_wgrad_strided_f32"}.get(wgrad)
    if name is None:
        raise ValueError(f"lstm_backward: wgrad must be 'f16-gates', 'f16', 'bf16' or 'f32', got {wgrad!r}")
    planes, f16, four_gates = wgrad != "f32", wgrad in ("f16", "f16-gates"), wgrad == "f16-gates"
    if rows_packed is not None and not planes:
        raise ValueError("rows_packed needs a plane weight gradient (wgrad 'bf16', 'f16' or 'f16-gates')")
    if f16 and rows_packed is None:
        raise ValueError(f"wgrad {wgrad!r} needs rows_packed: its planes are scaled by the rows kernel's bound on |dG|")
    lib, dev, H = load(), x.device, LSTM_HIDDEN
    rows, partials = C.c_int(0), None
    if rows_packed is not None:
        dgates, dg_bound = lstm_rows_backward(c0, gates, cs, dhs, rows_packed, with_bound=True, heads=heads)
    elif wide_in:  # the data-gradient kernel alone: it reads no x
        dgates = torch.empty(b, l, 4, H, dtype=torch.float32, device=dev)
        with _timed("lstm_backward", b * l):
            _check(lib.rl8_lstm_backward_dgates_f32(b, l, _ptr(c0), _ptr(gates), _ptr(cs), _ptr(dhs), _ptr(whht_packed),
                                                    _ptr(dgates), _stream()), "rl8_lstm_backward_dgates_f32")
    else:
        dgates = torch.empty(b, l, 4, H, dtype=torch.float32, device=dev)
        if not planes:  # dW_ih and the bias come out of this kernel's partials
            partials = torch.empty(int(lib.rl8_lstm_backward_max_rows()), int(lib.rl8_lstm_backward_partial_floats(d_in)),
                                   dtype=torch.float32, device=dev)
        with _timed("lstm_backward", b * l):
            _check(lib.rl8_lstm_backward_f32(_ptr(x), b, l, d_in, _ptr(c0), _ptr(gates), _ptr(cs), _ptr(dhs),
                                             _ptr(whht_packed), _ptr(dgates), _ptr(partials), C.byref(rows), _stream()),
                   "rl8_lstm_backward_f32")
    ws, dw_hh = _wgrad_workspace(dev), torch.empty(4 * H, H, dtype=torch.float32, device=dev)
    dgp, hsp, h0p, wsp, dwp, stream = _ptr(dgates), _ptr(hs), _ptr(h0), _ptr(ws), _ptr(dw_hh), _stream()
    if wide_in:  # no per-step copies of x, no column sums: dW_ih and the bias come from one launch over dG below
        small = None
    elif planes:
        xt = [x[:, t].contiguous() for t in range(l)]            # dense [B][d] per step (the kernel's scalar loads)
        width = H * (d_in + 1)                                    # a column-sum row: dW_ih^T, then the bias
        # kept between calls: [gate][step][workgroup][...]; four gates per launch: [step][gate][workgroup of gate][...]
        key = (dev.index or 0, _stream() or 0, l, d_in, *(("gates",) if four_gates else ()))
        cols = _lstm_colsum_ws.get(key)
        if cols is None:
            cols = _lstm_colsum_ws[key] = torch.empty(*((l, 4, 64) if four_gates else (4, l, 256)), width,
                                                      dtype=torch.float32, device=dev)
        crow = C.c_int(0)
    else:
        small = partials[: rows.value].sum(0)
    if f16:
        # three products instead of six: dG scaled by one power of two for the tensor, h_{t-1} by one from max |h0|
        # (t = 0) or 1 (an LSTM's own outputs)
        if h0_bound is None:
            h0_bound = torch.linalg.vector_norm(h0, ord=float("inf")).reshape(1)
        elif h0_bound.dtype != torch.float32 or h0_bound.numel() != 1 or h0_bound.device != dev:
            raise ValueError("h0_bound must be one float32 element on x's device")
        if hs_bound is None:  # (one pass over hs: callers that know their hs say so)
            one = torch.linalg.vector_norm(hs, ord=float("inf")).reshape(1) if l > 1 else torch.ones(1, dtype=torch.float32, device=dev)
        else:
            one = torch.full((1,), float(hs_bound), dtype=torch.float32, device=dev)
    # per gate (or the four at once) and timestep dW_hh[q] += dG_q^T h_{t-1} over the B rows of that step: h_{t-1} is
    # h0 for t = 0 and hs[:, t-1] (row pitch L*256) after, so no shifted copy of hs is made
    dg_scale = (_ptr(dg_bound),) if f16 else ()
    with _timed("lstm_wgrad", b * l):
        for q in range(1 if four_gates else 4):
            for t in range(l):
                h_prev, h_pitch = (h0p, H) if t == 0 else (hsp + (t - 1) * H * 4, l * H)
                h_scale = (_ptr(h0_bound if t == 0 else one),) if f16 else ()
                col_sums = (() if not planes else (None, 0, None, None) if wide_in else
                            (_ptr(xt[t]), d_in, _ptr(cols[t] if four_gates else cols[q, t]), C.byref(crow)))
                _check(getattr(lib, name)(dgp + (t * 4 * H + q * H) * 4, l * 4 * H, *dg_scale, h_prev, h_pitch, *h_scale, b,
                                          wsp, dwp + 4 * H * H * q, int(t > 0), *col_sums, stream), name)
    if upper is not None:
        # dW_ih = dG^T hs_below over all m rows: the W_hh product without the shift, so one accumulation per gate (or one
        # for the four); |hs_below| < 1.  The plane entries walk their own segments; the fp32 one is handed them here,
        # and the four-gate entry's last segment must hold its 128 rows.
        m, dw_ih = b * l, torch.empty(4 * H, H, dtype=torch.float32, device=dev)
        entry, gates_at_once = name, four_gates
        if four_gates and (m - 1) % WGRAD_SEGMENT_ROWS + 1 < LSTM_WGRAD_GATES_MIN_ROWS:
            entry, gates_at_once = "rl8_mlp_wgrad_f16_strided_f32", False
        segment = m if planes else WGRAD_SEGMENT_ROWS
        h_scale = (_ptr(torch.ones(1, dtype=torch.float32, device=dev)),) if f16 else ()
        col_sums = (None, 0, None, None) if planes else ()
        xp, dwip = _ptr(x), _ptr(dw_ih)
        with _timed("lstm_wgrad", m):
            for q in range(1 if gates_at_once else 4):
                for at in range(0, m, segment):
                    _check(getattr(lib, entry)(dgp + (at * 4 * H + q * H) * 4, 4 * H, *dg_scale, xp + at * H * 4, H, *h_scale,
                                               min(segment, m - at), wsp, dwip + 4 * H * H * q, int(at > 0), *col_sums,
                                               stream), entry)
        dx, db = lstm_stack256_dx(dgates.view(m, 4 * H), upper)
        return {"w_ih": dw_ih, "w_hh": dw_hh, "b": db, "dx": dx.view(b, l, H)}
    if wide_in:
        dw_ih, db = lstm_wide_in_wgrad(dgates.view(b * l, 4 * H), x.view(b * l, d_in))
        return {"w_ih": dw_ih, "w_hh": dw_hh, "b": db}
    if not planes:
        return {"w_ih": small[: 4 * H * d_in].view(4 * H, d_in), "w_hh": dw_hh, "b": small[4 * H * d_in :]}
    if four_gates:  # (a step's rows sit gate-major, crow.value per gate -- 64 at the sizes that fill the chip)
        sums = cols.view(l, -1)[:, : 4 * crow.value * width].reshape(l, 4, crow.value, width).sum(dim=(0, 2))
    else:
        sums = cols[:, :, : crow.value].sum(dim=(1, 2))          # [4][256*(d+1)], steps then workgroups in order
    return {"w_ih": sums[:, : H * d_in].reshape(4 * H, d_in), "w_hh": dw_hh, "b": sums[:, H * d_in :].reshape(4 * H)}


HEADS_MAX_OUT = 8  # outputs of one linear-heads launch


def linear_heads_forward_pair(h: torch.Tensor, w_a: torch.Tensor, b_a: torch.Tensor, w_b: torch.Tensor,
                              b_b: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Two layers on the same rows in one pass: (h x w_a^T + b_a [M, n_a], h x w_b^T + b_b [M, n_b])."""
    h = _dense(h.detach(), torch.float32, "h")
    w_a, b_a, w_b, b_b = (_dense(t.detach(), torch.float32, n) for t, n in ((w_a, "w_a"), (b_a, "b_a"), (w_b, "w_b"), (b_b, "b_b")))
    m, n_a, n_b = h.shape[0], w_a.shape[0], w_b.shape[0]
    if h.shape[1] != LSTM_HIDDEN or w_a.shape[1] != LSTM_HIDDEN or w_b.shape[1] != LSTM_HIDDEN or b_a.numel() != n_a \
            or b_b.numel() != n_b:
        raise ValueError("linear_heads_forward_pair: h [M, 256], w [n, 256], b [n]")
    out_a = torch.empty(m, n_a, dtype=torch.float32, device=h.device)
    out_b = torch.empty(m, n_b, dtype=torch.float32, device=h.device)
    with _timed("linear_heads_forward", m):
        _check(load().rl8_linear_heads_forward_pair_f32(_ptr(h), m, _ptr(w_a), _ptr(b_a), n_a, _ptr(out_a), _ptr(w_b),
                                                        _ptr(b_b), n_b, _ptr(out_b), _stream()),
               "rl8_linear_heads_forward_pair_f32")
    return out_a, out_b


def linear_heads_forward(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """h [M, 256] x w [n, 256]^T + b [n] -> [M, n] (n <= 8)."""
    h = _dense(h.detach(), torch.float32, "h")
    w = _dense(w.detach(), torch.float32, "w")
    b = _dense(b.detach(), torch.float32, "b")
    m, n = h.shape[0], w.shape[0]
    if h.shape[1] != LSTM_HIDDEN or w.shape[1] != LSTM_HIDDEN or b.numel() != n:
        raise ValueError("linear_heads_forward: h [M, 256], w [n, 256], b [n]")
    out = torch.empty(m, n, dtype=torch.float32, device=h.device)
    with _timed("linear_heads_forward", m):
        _check(load().rl8_linear_heads_forward_f32(_ptr(h), m, _ptr(w), _ptr(b), n, _ptr(out), _stream()),
               "rl8_linear_heads_forward_f32")
    return out


def linear_heads_backward(h: torch.Tensor, dout: torch.Tensor, w: torch.Tensor, *,
                          need_dh: bool = True) -> tuple[None | torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dh [M, 256], dw [n, 256], db [n]); ``need_dh=False``: dh is None and never written."""
    h = _dense(h.detach(), torch.float32, "h")
    dout = _dense(dout, torch.float32, "dout")
    w = _dense(w.detach(), torch.float32, "w")
    m, n = h.shape[0], w.shape[0]
    if tuple(dout.shape) != (m, n):
        raise ValueError("linear_heads_backward: dout must be [M, n]")
    lib = load()
    dh = torch.empty(m, LSTM_HIDDEN, dtype=torch.float32, device=h.device) if need_dh else None
    partials = torch.empty(int(lib.rl8_linear_heads_max_rows()), n * LSTM_HIDDEN + n, dtype=torch.float32, device=h.device)
    rows = C.c_int(0)
    with _timed("linear_heads_backward", m):
        _check(lib.rl8_linear_heads_backward_f32(_ptr(h), _ptr(dout), m, _ptr(w), n, _ptr(dh), _ptr(partials),
                                                 C.byref(rows), _stream()), "rl8_linear_heads_backward_f32")
    small = partials[: rows.value].sum(0)
    return dh, small[: n * LSTM_HIDDEN].view(n, LSTM_HIDDEN), small[n * LSTM_HIDDEN :]


# --------------------------------------------------------------------------- #
# Output heads of the narrow recurrent models: Linear(H, n) layers on h [M, H], H = 64 or 128
# (lstm_narrow_heads_kernels.hip).
# --------------------------------------------------------------------------- #
def _heads_narrow_params(name: str, h: torch.Tensor, *layers: tuple[torch.Tensor, None | torch.Tensor]) -> tuple[int, int]:
    """(m, hidden) after the dtype / contiguity / shape checks of the narrow heads entries; ``layers``: (w, b) pairs."""
    _dense(h, torch.float32, "h")
    hidden = h.shape[1] if h.ndim == 2 else -1
    if hidden not in LSTM_NARROW_HIDDEN or h.shape[0] < 1:
        raise ValueError(f"{name}: h [M, H], M >= 1, H in {LSTM_NARROW_HIDDEN}, got {tuple(h.shape)}")
    for w, b in layers:
        _dense(w, torch.float32, "w")
        if w.ndim != 2 or w.shape[1] != hidden or (b is not None and (_dense(b, torch.float32, "b").numel() != w.shape[0])):
            raise ValueError(f"{name}: w [n, {hidden}], b [n]")
    if not 1 <= sum(w.shape[0] for w, _ in layers) <= HEADS_MAX_OUT:
        raise ValueError(f"{name}: 1 to {HEADS_MAX_OUT} outputs")
    return h.shape[0], hidden


def linear_heads_narrow_forward(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """h [M, H] x w [n, H]^T + b [n] -> [M, n] (H = 64 or 128, n <= 8)."""
    h, w, b = h.detach(), w.detach(), b.detach()
    m, hidden = _heads_narrow_params("linear_heads_narrow_forward", h, (w, b))
    n = w.shape[0]
    out = torch.empty(m, n, dtype=torch.float32, device=h.device)
    with _timed("linear_heads_narrow_forward", m):
        _check(load().rl8_linear_heads_narrow_forward_f32(_ptr(h), m, hidden, _ptr(w), _ptr(b), n, _ptr(out), _stream()),
               "rl8_linear_heads_narrow_forward_f32")
    return out


def linear_heads_narrow_forward_pair(h: torch.Tensor, w_a: torch.Tensor, b_a: torch.Tensor, w_b: torch.Tensor,
                                     b_b: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Two layers on the same rows in one pass: (h x w_a^T + b_a [M, n_a], h x w_b^T + b_b [M, n_b])."""
    h, w_a, b_a, w_b, b_b = (t.detach() for t in (h, w_a, b_a, w_b, b_b))
    m, hidden = _heads_narrow_params("linear_heads_narrow_forward_pair", h, (w_a, b_a), (w_b, b_b))
    n_a, n_b = w_a.shape[0], w_b.shape[0]
    out_a = torch.empty(m, n_a, dtype=torch.float32, device=h.device)
    out_b = torch.empty(m, n_b, dtype=torch.float32, device=h.device)
    with _timed("linear_heads_narrow_forward", m):
        _check(load().rl8_linear_heads_narrow_forward_pair_f32(_ptr(h), m, hidden, _ptr(w_a), _ptr(b_a), n_a, _ptr(out_a),
                                                               _ptr(w_b), _ptr(b_b), n_b, _ptr(out_b), _stream()),
               "rl8_linear_heads_narrow_forward_pair_f32")
    return out_a, out_b


def linear_heads_narrow_backward(h: torch.Tensor, dout: torch.Tensor, w: torch.Tensor, *,
                                 need_dh: bool = True) -> tuple[None | torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dh [M, H], dw [n, H], db [n]); ``need_dh=False``: dh is None and never written. Deterministic."""
    h, dout, w = h.detach(), _dense(dout.detach(), torch.float32, "dout"), w.detach()
    m, hidden = _heads_narrow_params("linear_heads_narrow_backward", h, (w, None))
    n = w.shape[0]
    if tuple(dout.shape) != (m, n):
        raise ValueError("linear_heads_narrow_backward: dout must be [M, n]")
    lib = load()
    dh = torch.empty(m, hidden, dtype=torch.float32, device=h.device) if need_dh else None
    ws = torch.empty(int(lib.rl8_linear_heads_narrow_workspace_bytes(m, hidden, n)) // 4, dtype=torch.float32,
                     device=h.device)
    grads = torch.empty(n * hidden + n, dtype=torch.float32, device=h.device)
    with _timed("linear_heads_narrow_backward", m):
        _check(lib.rl8_linear_heads_narrow_backward_f32(_ptr(h), _ptr(dout), m, hidden, _ptr(w), n, _ptr(dh), _ptr(ws),
                                                        _ptr(grads), _stream()), "rl8_linear_heads_narrow_backward_f32")
    return dh, grads[: n * hidden].view(n, hidden), grads[n * hidden:]


def rollout_step_dummy_heads_narrow(
    h: torch.Tensor, w_pol: torch.Tensor, b_pol: torch.Tensor, w_vf: torch.Tensor, b_vf: torch.Tensor,
    noise: None | torch.Tensor, state: torch.Tensor, action_col: torch.Tensor, logp_col: torch.Tensor,
    value_col: torch.Tensor, reward_col: torch.Tensor, obs_col_next: torch.Tensor, rdr_t: None | torch.Tensor,
    rdr_t1: None | torch.Tensor, gamma: float, seed: int, step: int, env_offset: int = 0, deterministic: bool = False,
) -> None:
    """One rollout timestep of the discrete dummy env behind a narrow LSTM: two-way logits head and value head on
    ``h`` [N, H] (as :func:`linear_heads_narrow_forward` forms them), then sampler + ``env.step`` + bookkeeping as
    :func:`rollout_step_dummy` does them, in one launch."""
    h, w_pol, b_pol, w_vf, b_vf = (t.detach() for t in (h, w_pol, b_pol, w_vf, b_vf))
    n, hidden = _heads_narrow_params("rollout_step_dummy_heads_narrow", h, (w_pol, b_pol), (w_vf, b_vf))
    if w_pol.shape[0] != 2 or w_vf.shape[0] != 1:
        raise ValueError("rollout_step_dummy_heads_narrow: w_pol [2, H], w_vf [1, H]")
    head = (("h", h, _F32, n * hidden), hidden, ("w_pol", w_pol, _F32, 2 * hidden), ("b_pol", b_pol, _F32, 2),
            ("w_vf", w_vf, _F32, hidden), ("b_vf", b_vf, _F32, 1), ("noise", noise, _F32, 2 * n), ("state", state, _F32, n))
    _rollout_step("rl8_rollout_step_dummy_heads_narrow_f32", n, head, torch.int64, [("obs_col_next", obs_col_next, _F32, n)],
                  (action_col, logp_col, value_col, reward_col, rdr_t, rdr_t1),
                  (float(gamma), int(seed), int(step), int(env_offset), deterministic),
                  timed="rollout_step_dummy_heads_narrow")
