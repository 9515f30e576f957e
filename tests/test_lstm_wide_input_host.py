"""The width-256 LSTM behind 8 to 128 input floats (rl8_amd/csrc/lstm_wide_in_kernels.hip) without a GPU: the entries
exported, bound, declared and refusing bad arguments before any launch; the kernels compiled for gfx950 without scratch
and inside the CU's LDS; and the host route -- ``fused_lstm._wide_input_family`` / ``_wide_input_plan`` and the two
autograd nodes -- on stubbed envelope queries and kernels."""

from __future__ import annotations

import itertools
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from rl8_amd import hip
from rl8_amd.data import DataKeys
from rl8_amd.nn import fused_lstm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_lstm_wide_in_supports", "rl8_lstm_wide_in_lds_bytes", "rl8_lstm_wide_in_pack_floats",
           "rl8_lstm_wide_in_pack_f32", "rl8_lstm_wide_in_forward_f32", "rl8_lstm_wide_in_workspace_bytes",
           "rl8_lstm_wide_in_wgrad_f32", "rl8_lstm_backward_dgates_f32")
CU_LDS_BYTES = 160 * 1024  # MI355X: LDS per CU
WIDTHS = (8, 9, 15, 16, 17, 24, 31, 32, 40, 63, 64, 65, 127, 128)


def test_entries_are_exported_bound_and_declared():
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "rl8_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        assert re.search(rf"\b{name}\(", header), name
    assert hip.ABI_VERSION == 107 and "#define RL8_ABI_VERSION 107" in header
    for name in ("lstm_wide_in_supports", "lstm_wide_in_pack", "lstm_wide_in_forward", "lstm_wide_in_wgrad"):
        assert callable(getattr(hip, name)), name


def test_envelope_answers():
    lib = hip.load()
    assert [lib.rl8_lstm_wide_in_supports(d) for d in (0, 7, 8, 128, 129)] == [0, 0, 1, 1, 0]
    assert [hip.lstm_wide_in_supports(d) for d in (0, 7, 8, 128, 129)] == [False, False, True, True, False]
    assert lib.rl8_lstm_supports(8) == 0 and lib.rl8_lstm_supports(7) == 1  # the narrow-input entries keep theirs


def test_sizes_equal_their_formulas():
    lib = hip.load()
    for d in WIDTHS:
        k = 256 + 8 * -(-(d + 1) // 8)
        assert lib.rl8_lstm_wide_in_pack_floats(d) == 4 * 256 * k, d
        # one [256][d + 1] slab per gate and workgroup, a workgroup per CU: 256 CUs / 4 gates
        assert lib.rl8_lstm_wide_in_workspace_bytes(d) == 4 * 64 * 256 * (d + 1) * 4, d
        xg = -(-(d + 1) // 8)
        cls = next(c for c in (2, 4, 8, 17) if c >= xg)
        assert lib.rl8_lstm_wide_in_lds_bytes(0, d) == 4 * 32 * (256 + 8 * cls + 1), d
        ct = -(-(d + 1) // 32)
        assert lib.rl8_lstm_wide_in_lds_bytes(1, d) == 4 * 2 * (32 * 320 + 32 * (32 * ct + 32)), d
        # the LDS row pitch stays odd; two forward workgroups and one weight-gradient workgroup fit a CU
        assert (lib.rl8_lstm_wide_in_lds_bytes(0, d) // (4 * 32)) % 2 == 1, d
        assert 2 * lib.rl8_lstm_wide_in_lds_bytes(0, d) <= CU_LDS_BYTES, d
        assert lib.rl8_lstm_wide_in_lds_bytes(1, d) <= CU_LDS_BYTES, d
    for d in (0, 7, 129, -1):
        assert lib.rl8_lstm_wide_in_pack_floats(d) == -2, d
        assert lib.rl8_lstm_wide_in_workspace_bytes(d) == -2, d
        assert lib.rl8_lstm_wide_in_lds_bytes(0, d) == -2 and lib.rl8_lstm_wide_in_lds_bytes(1, d) == -2, d
    assert lib.rl8_lstm_wide_in_lds_bytes(2, 24) == -2 and lib.rl8_lstm_wide_in_lds_bytes(-1, 24) == -2


def test_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    pack, fwd = lib.rl8_lstm_wide_in_pack_f32, lib.rl8_lstm_wide_in_forward_f32
    wgrad, dgates = lib.rl8_lstm_wide_in_wgrad_f32, lib.rl8_lstm_backward_dgates_f32

    def args(defaults, **kw):
        a = dict(defaults)
        a.update(kw)
        return list(a.values())

    pack_a = dict(w_ih=fake, w_hh=fake, b_ih=fake, b_hh=fake, d_in=24, packed=fake, stream=None)
    fwd_a = dict(x=fake, b=10, l=2, d_in=24, h0=fake, c0=fake, w_packed=fake, hs=fake, hn=fake, cn=fake, save_gates=None,
                 save_c=None, stream=None)
    wgrad_a = dict(dgates=fake, x=fake, m=10, d_in=24, workspace=fake, dw_ih_out=fake, db_out=fake, stream=None)
    dgates_a = dict(b=10, l=2, c0=fake, gates=fake, cs=fake, dhs=fake, whht_packed=fake, dgates=fake, stream=None)
    # NULL pointers (save_gates / save_c: both or neither)
    for name in ("w_ih", "w_hh", "b_ih", "b_hh", "packed"):
        assert pack(*args(pack_a, **{name: None})) == -1, name
    for name in ("x", "h0", "c0", "w_packed", "hs", "hn", "cn"):
        assert fwd(*args(fwd_a, **{name: None})) == -1, name
    assert fwd(*args(fwd_a, save_gates=fake)) == -1 and fwd(*args(fwd_a, save_c=fake)) == -1
    for name in ("dgates", "x", "workspace", "dw_ih_out", "db_out"):
        assert wgrad(*args(wgrad_a, **{name: None})) == -1, name
    for name in ("c0", "gates", "cs", "dhs", "whht_packed", "dgates"):
        assert dgates(*args(dgates_a, **{name: None})) == -1, name
    # sizes: the envelope's two ends, empty batches, and the 32-bit addressing bound 32 * l * 4096 < 2^31
    for d in (0, 7, 129):
        assert pack(*args(pack_a, d_in=d)) == -2 and fwd(*args(fwd_a, d_in=d)) == -2 and wgrad(*args(wgrad_a, d_in=d)) == -2
    for kw in ({"b": 0}, {"l": 0}, {"b": -1}, {"l": 1 << 14}):
        assert fwd(*args(fwd_a, **kw)) == -2, kw
        assert dgates(*args(dgates_a, **kw)) == -2, kw
    assert wgrad(*args(wgrad_a, m=0)) == -2
    # alignment
    assert pack(*args(pack_a, packed=fake + 4)) == -3 and pack(*args(pack_a, w_ih=fake + 2)) == -3
    assert fwd(*args(fwd_a, w_packed=fake + 4)) == -3 and fwd(*args(fwd_a, h0=fake + 8)) == -3
    assert fwd(*args(fwd_a, x=fake + 2)) == -3 and fwd(*args(fwd_a, hs=fake + 1)) == -3
    assert fwd(*args(fwd_a, save_gates=fake + 2, save_c=fake)) == -3
    assert wgrad(*args(wgrad_a, dgates=fake + 4)) == -3 and wgrad(*args(wgrad_a, x=fake + 2)) == -3
    assert wgrad(*args(wgrad_a, db_out=fake + 1)) == -3
    assert dgates(*args(dgates_a, whht_packed=fake + 4)) == -3


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_compile_without_scratch_and_inside_the_lds(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "lstm_wide_in.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "lstm_wide_in_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    want = {f"lstm_wide_in_forward_kernelILi{xg}ELb{save}EE" for xg in (2, 4, 8, 17) for save in (0, 1)}
    want |= {f"lstm_wide_in_wgrad_kernelILi{ct}EE" for ct in (1, 2, 3, 4, 5)}
    want |= {"lstm_wide_in_pack_kernel", "lstm_wide_in_wgrad_reduce_kernel"}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    assert len(kernels) == len(want), sorted(kernels)
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        # all LDS is dynamic: what rl8_lstm_wide_in_lds_bytes reports is all a workgroup takes
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name


# --- the host route, on stubbed envelope queries ---------------------------------------------------------------------------
@pytest.fixture
def envelopes(monkeypatch):
    """The build's envelope queries stubbed with what ``include/rl8_amd.h`` documents; the calls of the new one."""
    calls = []

    def wide(d_in):
        calls.append(d_in)
        return 8 <= d_in <= 128

    monkeypatch.setattr(hip, "lstm_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_split_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: hidden in (64, 128) and 1 <= d_in <= 16)
    monkeypatch.setattr(hip, "lstm_stack_supports", lambda hidden: hidden in (64, 128))
    monkeypatch.setattr(hip, "lstm_wide_in_supports", wide)
    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM", raising=False)
    caches = (fused_lstm._narrow_supported, fused_lstm._planes_supported, fused_lstm._wide_input_supported)
    for c in caches:
        c.cache_clear()
    yield calls
    for c in caches:  # (before the stubs go: nothing may keep their answers)
        c.cache_clear()


def _model():
    from rl8_amd import models_recurrent
    from rl8_amd.specs import Categorical as CategoricalSpec, Unbounded

    return models_recurrent.DefaultDiscreteRecurrentModel(
        Unbounded(shape=torch.Size([1]), device="cpu"), CategoricalSpec(2, shape=torch.Size([1]), device="cpu"), hidden_size=8)


def test_wide_input_family_truth_table(envelopes, monkeypatch):
    """Every clause ``_wide_input_family`` names flipped, on one module whose attributes are set row by row; ``_family``
    answers ``None`` wherever the new family says yes, and the lean rollout stays unavailable there."""
    from rl8_amd.algorithms._recurrent import _LeanRollout
    from rl8_amd.distributions import Categorical
    from rl8_amd.env import DiscreteDummyEnv

    ns = types.SimpleNamespace
    model = _model()
    lstm = model.lstm
    algo = ns(policy=ns(model=model, distribution_cls=Categorical), _tm={DataKeys.OBS: torch.zeros(2, 1, 1)},
              env=object.__new__(DiscreteDummyEnv))
    inputs = list(itertools.product((True, False), (torch.float32, torch.float16), (3, 2), (0, 1)))
    yes = 0
    for enabled, switch, hidden, layers, d_in, bias, batch_first, bidirectional, proj in itertools.product(
            (True, False), (None, "1", "0"), (128, 256), (1, 2), (1, 7, 8, 24, 128, 129), (True, False), (True, False),
            (False, True), (0, 16)):
        monkeypatch.setattr(fused_lstm, "ENABLED", enabled)
        if switch is None:
            monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM", raising=False)
        else:
            monkeypatch.setenv("RL8_AMD_WIDE_INPUT_LSTM", switch)
        lstm.hidden_size, lstm.num_layers, lstm.input_size, lstm.bias = hidden, layers, d_in, bias
        lstm.batch_first, lstm.bidirectional, lstm.proj_size = batch_first, bidirectional, proj
        want = bool(enabled and switch != "0" and hidden == 256 and layers == 1 and 8 <= d_in <= 128 and bias
                    and batch_first and not bidirectional and proj == 0)
        got = fused_lstm._wide_input_family(lstm)
        assert got == ("256-wide-in" if want else None), (enabled, switch, vars(lstm))
        if want:
            yes += 1
            assert fused_lstm._family(lstm) is None and _LeanRollout.available(algo) is False
        for is_cuda, dtype, ndim, wider in inputs:
            x = ns(is_cuda=is_cuda, dtype=dtype, ndim=ndim, shape=(4, 3, d_in + wider)[:ndim] + (0,) * (3 - ndim))
            ok = is_cuda and dtype == torch.float32 and ndim == 3 and wider == 0
            assert fused_lstm._wide_input_family_for(lstm, x) == (got if ok else None)
            if got is not None:
                assert fused_lstm._family_for(lstm, x) is None
    assert yes == 2 * 3  # (switch unset / "1") x (d_in 8, 24, 128)


def test_switch_is_read_per_call_and_the_build_once(envelopes, monkeypatch):
    lstm = torch.nn.LSTM(24, 256, batch_first=True)
    assert fused_lstm._wide_input_family(lstm) == "256-wide-in"
    monkeypatch.setenv("RL8_AMD_WIDE_INPUT_LSTM", "0")
    assert fused_lstm._wide_input_family(lstm) is None
    monkeypatch.setenv("RL8_AMD_WIDE_INPUT_LSTM", "off")  # anything but "0" means the kernels
    assert fused_lstm._wide_input_family(lstm) == "256-wide-in"
    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_LSTM")
    assert fused_lstm._wide_input_family(lstm) == "256-wide-in"
    assert envelopes == [24]  # one query per width, then the memo


def _switches(monkeypatch, gemm="split", rows=True, fuse=True, planes=None, gates=None):
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", gemm)
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", rows)
    monkeypatch.setattr(fused_lstm, "FUSE_HEADS", fuse)
    for name, value in zip(("RL8_AMD_LSTM_WGRAD_PLANES", "RL8_AMD_LSTM_WGRAD_GATES"), (planes, gates)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def test_wide_input_plan_under_every_switch(envelopes, monkeypatch):
    for gemm, rows, fuse, planes, gates in itertools.product(("split", "f32"), (True, False), (True, False),
                                                             (None, "f16", "bf16"), (None, "fused", "separate")):
        _switches(monkeypatch, gemm, rows, fuse, planes, gates)
        for b in (1, 127, 128, 4096):
            plan = fused_lstm._wide_input_plan(b)
            want_wgrad = ("f32" if not rows else "bf16" if planes == "bf16" else
                          "f16-gates" if b >= 128 and gates != "separate" else "f16")
            assert plan.wide_in is True and plan.forward_planes is False  # the new forward, whatever RL8_AMD_LSTM_GEMM says
            assert (plan.backward_rows, plan.wgrad, plan.fuse_heads) == (rows, want_wgrad, fuse and rows), (gemm, rows, fuse, planes, gates, b)
    # _plan's own answers at eight inputs are what they were, and no plan of its making is a wide one
    _switches(monkeypatch)
    for b in (1, 128, 4096):
        plan = fused_lstm._plan(8, b)
        assert (plan.forward_planes, plan.backward_rows, plan.wgrad, plan.fuse_heads, plan.wide_in) == (False, False, "f32", False, False)
    assert fused_lstm._plan(3, 4096).wide_in is False and fused_lstm._plan(3, 4096).wgrad == "f16-gates"


class _Ctx:
    """What the two nodes' ``forward`` / ``backward`` ask of an autograd context."""

    def __init__(self, n_inputs):
        self.needs_input_grad = (False, False, False, True, True, True, True) + (True,) * (n_inputs - 7)
        self.saved_tensors = ()

    def set_materialize_grads(self, value):
        pass

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


@pytest.mark.parametrize("made_under", [{}, {"planes": "bf16"}, {"gates": "separate"}, {"rows": False}, {"gemm": "f32"}])
def test_both_nodes_backwards_run_the_plan_their_forward_saved(envelopes, monkeypatch, made_under):
    """The forward of either node calls ``hip.lstm_wide_in_forward`` on the "wide" pack and nothing of the plane
    forward; switches flipped between forward and backward do not reach the backward, which follows ``ctx.plan``."""
    _switches(monkeypatch, **made_under)
    b, l, d = 256, 2, 24
    plan = fused_lstm._wide_input_plan(b)
    packs, forwards, seen = [], [], []
    z = torch.zeros
    monkeypatch.setattr(fused_lstm, "_packs", lambda lstm, kind: packs.append(kind) or kind)

    def wide_forward(x, h0, c0, w_packed, *, save=False):
        forwards.append((w_packed, save))
        return z(b, l, 256), z(b, 256), z(b, 256), z(b, l, 4, 256) if save else None, z(b, l, 256) if save else None

    def backward(x, h0, c0, hs, gates, cs, dhs, whht_packed, *, wgrad, rows_packed=None, wide_in=False, h0_bound=None, **kw):
        seen.append((wgrad, whht_packed, rows_packed, wide_in, h0_bound))
        return {"w_ih": None, "w_hh": None, "b": None}

    def refuse(*a, **kw):
        raise AssertionError("a wide-input plan ran a kernel of the narrow-input family")

    monkeypatch.setattr(hip, "lstm_wide_in_forward", wide_forward)
    monkeypatch.setattr(hip, "lstm_backward", backward)
    for name in ("lstm_forward", "lstm_forward_split", "lstm_split_state", "lstm_pack", "lstm_pack_split"):
        monkeypatch.setattr(hip, name, refuse)
    monkeypatch.setattr(hip, "linear_heads_forward", lambda h, w, bias: z(h.shape[0], w.shape[0]))
    monkeypatch.setattr(hip, "linear_heads_backward",
                        lambda h, dout, w, need_dh=True: (torch.zeros_like(h) if need_dh else None, None, None))
    lstm = torch.nn.LSTM(d, 256, batch_first=True)
    params = (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
    want = (plan.wgrad, None, "rows", True, None) if plan.backward_rows else (plan.wgrad, "transposed", None, True, None)

    ctx = _Ctx(10)
    fused_lstm._FusedLSTM.forward(ctx, z(b, l, d), z(b, 256), z(b, 256), *params, lstm, True, plan)
    assert packs == ["wide"] and forwards == [("wide", True)] and ctx.plan is plan and ctx.h0_bound is None
    # every switch the other way before the backward
    _switches(monkeypatch, gemm="f32", rows=not plan.backward_rows, fuse=False,
              planes="f16" if plan.wgrad == "bf16" else "bf16", gates="separate")
    packs.clear()
    fused_lstm._FusedLSTM.backward(ctx, z(b, l, 256), None)
    assert packs == (["rows"] if plan.backward_rows else ["transposed"]) and seen == [want]
    # a pass that wants no gradient saves nothing
    packs.clear(), forwards.clear()
    fused_lstm._FusedLSTM.forward(_Ctx(10), z(b, l, d), z(b, 256), z(b, 256), *params, lstm, False, plan)
    assert packs == ["wide"] and forwards == [("wide", False)]

    if plan.fuse_heads:  # the heads node exists only where its plan runs the rows kernel
        _switches(monkeypatch, **made_under)
        for dhs in (None, z(b, l, 256)):
            packs.clear(), forwards.clear(), seen.clear()
            ctx = _Ctx(11)
            fused_lstm._FusedLSTMHeads.forward(ctx, z(b, l, d), z(b, 256), z(b, 256), *params, z(3, 256), z(3), lstm, plan)
            assert packs == ["wide"] and forwards == [("wide", True)] and ctx.plan is plan and ctx.h0_bound is None
            _switches(monkeypatch, gemm="f32", rows=False, fuse=False, planes="bf16", gates="separate")
            packs.clear()
            fused_lstm._FusedLSTMHeads.backward(ctx, z(b * l, 3), dhs, None)
            assert packs == ["rows"] and seen == [(plan.wgrad, None, "rows", True, None)]
