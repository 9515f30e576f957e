"""Stacked LSTMs of width 256 (rl8_amd/csrc/lstm_stack256_kernels.hip) without a GPU: the entries exported, bound,
declared and refusing bad arguments before any launch; the kernels compiled for gfx950 without scratch and with all LDS
dynamic; and the host route -- ``fused_lstm._stack256_family`` on stubbed envelope queries, its switch, and the
``_StackLSTM`` node it goes through."""

from __future__ import annotations

import inspect
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
ENTRIES = ("rl8_lstm_stack256_supports", "rl8_lstm_stack256_lds_bytes", "rl8_lstm_stack256_pack_floats",
           "rl8_lstm_stack256_pack_f32", "rl8_lstm_stack256_forward_f32", "rl8_lstm_stack256_workspace_bytes",
           "rl8_lstm_stack256_dx_f32")
CU_LDS_BYTES = 160 * 1024  # MI355X: LDS per CU


def test_entries_are_exported_bound_and_declared():
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "rl8_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        assert re.search(rf"\b{name}\(", header), name
    assert hip.ABI_VERSION == 107 and "#define RL8_ABI_VERSION 107" in header  # new entries only: no bump
    for name in ("lstm_stack256_supports", "lstm_stack256_pack", "lstm_stack256_forward", "lstm_stack256_dx",
                 "lstm_stack256_backward"):
        assert callable(getattr(hip, name)), name


def test_envelope_answers_and_sizes():
    lib = hip.load()
    assert lib.rl8_lstm_stack256_supports() == 1 and hip.lstm_stack256_supports() is True
    # the siblings keep their answers
    assert lib.rl8_lstm_stack_supports(256) == 0 and lib.rl8_lstm_wide_in_supports(129) == 0 and lib.rl8_lstm_supports(8) == 0
    # [h (256) | x (256) | 1 | 0 x 7]: K = 520, 65 k-groups
    assert lib.rl8_lstm_stack256_pack_floats() == 1024 * 520
    fwd, dx = lib.rl8_lstm_stack256_lds_bytes(0), lib.rl8_lstm_stack256_lds_bytes(1)
    assert fwd == 4 * 32 * (256 + 8 * 33 + 1) == 66688 and dx == 4 * 2 * 32 * 257
    assert (fwd // (4 * 32)) % 2 == 1  # the LDS row pitch stays odd
    assert 2 * fwd <= CU_LDS_BYTES and 2 * dx <= CU_LDS_BYTES  # two workgroups of either kernel fit a CU
    assert lib.rl8_lstm_stack256_lds_bytes(2) == -2 and lib.rl8_lstm_stack256_lds_bytes(-1) == -2
    # one [1024] slab per workgroup, a workgroup per 32-row tile up to two per CU: a function of m alone
    for m, grid in ((1, 1), (32, 1), (33, 2), (32 * 511 + 1, 512), (1 << 30, 512)):
        assert lib.rl8_lstm_stack256_workspace_bytes(m) == grid * 1024 * 4, m
    assert lib.rl8_lstm_stack256_workspace_bytes(0) == -2 and lib.rl8_lstm_stack256_workspace_bytes(-5) == -2


def test_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    pack, fwd, dx = lib.rl8_lstm_stack256_pack_f32, lib.rl8_lstm_stack256_forward_f32, lib.rl8_lstm_stack256_dx_f32

    def args(defaults, **kw):
        a = dict(defaults)
        a.update(kw)
        return list(a.values())

    pack_a = dict(w_ih=fake, w_hh=fake, b_ih=fake, b_hh=fake, packed=fake, stream=None)
    fwd_a = dict(x=fake, b=10, l=2, h0=fake, c0=fake, w_packed=fake, hs=fake, hn=fake, cn=fake, save_gates=None, save_c=None,
                 stream=None)
    dx_a = dict(dgates=fake, m=10, wiht_packed=fake, workspace=fake, dx_out=fake, db_out=fake, stream=None)
    # NULL pointers (save_gates / save_c: both or neither)
    for name in ("w_ih", "w_hh", "b_ih", "b_hh", "packed"):
        assert pack(*args(pack_a, **{name: None})) == -1, name
    for name in ("x", "h0", "c0", "w_packed", "hs", "hn", "cn"):
        assert fwd(*args(fwd_a, **{name: None})) == -1, name
    assert fwd(*args(fwd_a, save_gates=fake)) == -1 and fwd(*args(fwd_a, save_c=fake)) == -1
    for name in ("dgates", "wiht_packed", "workspace", "dx_out", "db_out"):
        assert dx(*args(dx_a, **{name: None})) == -1, name
    # sizes: empty batches and the 32-bit addressing bound 32 * l * 4096 < 2^31
    for kw in ({"b": 0}, {"l": 0}, {"b": -1}, {"l": 1 << 14}):
        assert fwd(*args(fwd_a, **kw)) == -2, kw
    assert dx(*args(dx_a, m=0)) == -2 and dx(*args(dx_a, m=-1)) == -2
    # alignment: 16 bytes for what goes HBM -> LDS a row at a time and for the packed weights, 4 for the rest
    assert pack(*args(pack_a, packed=fake + 4)) == -3 and pack(*args(pack_a, w_ih=fake + 2)) == -3
    assert fwd(*args(fwd_a, w_packed=fake + 4)) == -3 and fwd(*args(fwd_a, h0=fake + 8)) == -3
    assert fwd(*args(fwd_a, x=fake + 4)) == -3 and fwd(*args(fwd_a, hs=fake + 1)) == -3 and fwd(*args(fwd_a, c0=fake + 2)) == -3
    assert fwd(*args(fwd_a, save_gates=fake + 2, save_c=fake)) == -3
    assert dx(*args(dx_a, dgates=fake + 4)) == -3 and dx(*args(dx_a, wiht_packed=fake + 8)) == -3
    assert dx(*args(dx_a, dx_out=fake + 2)) == -3 and dx(*args(dx_a, db_out=fake + 1)) == -3


def _kernels(tmp_path, unit):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / (unit + ".s")
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, unit + ".hip")],
        check=True, capture_output=True, timeout=600,
    )
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_compile_without_scratch_and_with_dynamic_lds_only(tmp_path):
    kernels = _kernels(tmp_path, "lstm_stack256_kernels")
    want = {f"lstm_wide_in_forward_kernelILi33ELb{save}EE" for save in (0, 1)}
    want |= {"lstm_stack256_pack_kernel", "lstm_stack256_dx_kernel", "lstm_stack256_db_reduce_kernel"}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    assert len(kernels) == len(want), sorted(kernels)
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        # all LDS is dynamic: what rl8_lstm_stack256_lds_bytes reports is all a workgroup takes
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name


# --- the host route, on stubbed envelope queries ---------------------------------------------------------------------------
@pytest.fixture
def envelopes(monkeypatch):
    """The build's envelope queries stubbed with what ``include/rl8_amd.h`` documents."""
    monkeypatch.setattr(hip, "lstm_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_split_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: hidden in (64, 128) and 1 <= d_in <= 16)
    monkeypatch.setattr(hip, "lstm_stack_supports", lambda hidden: hidden in (64, 128))
    monkeypatch.setattr(hip, "lstm_wide_in_supports", lambda d_in: 8 <= d_in <= 128)
    monkeypatch.setattr(hip, "lstm_stack256_supports", lambda: True)
    for name in ("RL8_AMD_WIDE_INPUT_LSTM", "RL8_AMD_LSTM_STACK_256"):
        monkeypatch.delenv(name, raising=False)
    caches = (fused_lstm._narrow_supported, fused_lstm._planes_supported, fused_lstm._wide_input_supported)
    for c in caches:
        c.cache_clear()
    yield
    for c in caches:  # (before the stubs go: nothing may keep their answers)
        c.cache_clear()


def _model():
    from rl8_amd import models_recurrent
    from rl8_amd.specs import Categorical as CategoricalSpec, Unbounded

    return models_recurrent.DefaultDiscreteRecurrentModel(
        Unbounded(shape=torch.Size([1]), device="cpu"), CategoricalSpec(2, shape=torch.Size([1]), device="cpu"), hidden_size=8)


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def test_stack256_family_truth_table(envelopes, monkeypatch):
    """Every clause ``_stack256_family`` names flipped, on one module whose attributes are set row by row; ``_family`` and
    ``_wide_input_family`` answer ``None`` wherever the new family says yes, and the lean rollout stays unavailable."""
    from rl8_amd.algorithms._recurrent import _LeanRollout
    from rl8_amd.distributions import Categorical
    from rl8_amd.env import DiscreteDummyEnv

    ns = types.SimpleNamespace
    model = _model()
    lstm = model.lstm
    algo = ns(policy=ns(model=model, distribution_cls=Categorical), _tm={DataKeys.OBS: torch.zeros(2, 1, 1)},
              env=object.__new__(DiscreteDummyEnv))
    yes = 0
    for (enabled, switch, wide_switch, hidden, layers, dropout, d_in, bias, batch_first, bidirectional,
         proj) in itertools.product((True, False), (None, "1", "0"), (None, "0"), (128, 256), (1, 2, 3), (0, 0.1),
                                    (0, 1, 7, 8, 128, 129), (True, False), (True, False), (False, True), (0, 16)):
        monkeypatch.setattr(fused_lstm, "ENABLED", enabled)
        _setenv(monkeypatch, "RL8_AMD_LSTM_STACK_256", switch)
        _setenv(monkeypatch, "RL8_AMD_WIDE_INPUT_LSTM", wide_switch)
        lstm.hidden_size, lstm.num_layers, lstm.input_size, lstm.bias, lstm.dropout = hidden, layers, d_in, bias, dropout
        lstm.batch_first, lstm.bidirectional, lstm.proj_size = batch_first, bidirectional, proj
        layer0 = 1 <= d_in <= 7 or (8 <= d_in <= 128 and wide_switch != "0")
        want = bool(enabled and switch != "0" and hidden == 256 and layers >= 2 and dropout == 0 and layer0 and bias
                    and batch_first and not bidirectional and proj == 0)
        got = fused_lstm._stack256_family(lstm)
        assert got == ("stack256" if want else None), (enabled, switch, wide_switch, vars(lstm))
        if want:
            yes += 1
            assert fused_lstm._family(lstm) is None and fused_lstm._wide_input_family(lstm) is None
            assert _LeanRollout.available(algo) is False
    # (switch unset / "1") x (2, 3 layers) x (d_in 1, 7 under either wide switch; 8, 128 under the wide switch unset)
    assert yes == 2 * 2 * (2 * 2 + 2)


def test_the_build_without_the_kernels_says_no(envelopes, monkeypatch):
    lstm = torch.nn.LSTM(4, 256, num_layers=2, batch_first=True)
    assert fused_lstm._stack256_family(lstm) == "stack256"
    monkeypatch.setattr(hip, "lstm_stack256_supports", lambda: False)
    assert fused_lstm._stack256_family(lstm) is None


def test_switch_is_read_per_call(envelopes, monkeypatch):
    lstm = torch.nn.LSTM(4, 256, num_layers=2, batch_first=True)
    assert fused_lstm._stack256_family(lstm) == "stack256" and fused_lstm.stack256_lstm_on()
    monkeypatch.setenv("RL8_AMD_LSTM_STACK_256", "0")
    assert fused_lstm._stack256_family(lstm) is None and not fused_lstm.stack256_lstm_on()
    monkeypatch.setenv("RL8_AMD_LSTM_STACK_256", "off")  # anything but "0" means the kernels
    assert fused_lstm._stack256_family(lstm) == "stack256"
    monkeypatch.delenv("RL8_AMD_LSTM_STACK_256")
    assert fused_lstm._stack256_family(lstm) == "stack256"


def test_the_entry_declines_without_a_kernel_call(envelopes, monkeypatch):
    """On the CPU every input fails ``_input_ok``; a device-like input that requires a gradient is declined under grad
    mode before anything of ``hip`` runs."""
    lstm = torch.nn.LSTM(4, 256, num_layers=2, batch_first=True)
    x, h0 = torch.zeros(3, 2, 4), torch.zeros(3, 2, 256)
    assert fused_lstm.lstm_stack256_forward(lstm, x, h0, h0) is None
    monkeypatch.setattr(fused_lstm, "_input_ok", lambda lstm, x: True)
    monkeypatch.setattr(fused_lstm, "_stack_apply", lambda *a: "ran")
    assert fused_lstm.lstm_stack256_forward(lstm, x, h0, h0) == "ran"
    for which in range(3):
        tensors = [x.clone(), h0.clone(), h0.clone()]
        tensors[which].requires_grad_()
        assert fused_lstm.lstm_stack256_forward(lstm, *tensors) is None
        with torch.no_grad():
            assert fused_lstm.lstm_stack256_forward(lstm, *tensors) == "ran"


def test_the_stack_node_keeps_its_signature_and_there_is_no_new_node():
    assert list(inspect.signature(fused_lstm._StackLSTM.forward).parameters) == ["ctx", "x", "h0", "c0", "grad_mode", "weights"]
    assert inspect.signature(fused_lstm._StackLSTM.forward).parameters["weights"].kind is inspect.Parameter.VAR_POSITIONAL
    nodes = {name for name, obj in vars(fused_lstm).items()
             if isinstance(obj, type) and issubclass(obj, torch.autograd.Function)}
    assert nodes == {"_FusedLSTM", "_NarrowLSTM", "_NarrowLSTMHeads", "_StackLSTM", "_Heads", "_FusedLSTMHeads"}


class _Ctx:
    """What ``_StackLSTM.forward`` / ``backward`` ask of an autograd context."""

    def __init__(self, n_weights):
        self.needs_input_grad = (False, False, False, False) + (True,) * n_weights
        self.saved_tensors = ()

    def set_materialize_grads(self, value):
        pass

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


@pytest.mark.parametrize("d_in,rows", [(4, True), (4, False), (24, True), (24, False)])
def test_the_node_runs_the_plans_its_forward_made(envelopes, monkeypatch, d_in, rows):
    """Width 256 selects the new per-layer calls inside ``_StackLSTM``: layer 0 on its own family's forward, the layers
    above on ``hip.lstm_stack256_forward``; the backward follows the plans kept on ``ctx`` after every switch has been
    flipped, from the top layer down, and hands each upper layer's dx to the layer below."""
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", "split")
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", rows)
    b, l, layers = 256, 2, 3
    z = torch.zeros
    packs, calls = [], []

    def layer_packs(params, kind):
        packs.append(kind)
        return (kind, kind) if kind == "split" else kind

    monkeypatch.setattr(fused_lstm, "_layer_packs", layer_packs)
    for name in ("RL8_AMD_LSTM_WGRAD_PLANES", "RL8_AMD_LSTM_WGRAD_GATES"):
        monkeypatch.delenv(name, raising=False)

    def forward(name):
        def run(x, h0, c0, *packed, save=False, state_out=None, **kw):
            calls.append((name, tuple(x.shape), save))
            return z(b, l, 256), z(b, 256), z(b, 256), z(b, l, 4, 256) if save else None, z(b, l, 256) if save else None
        return run

    for name in ("lstm_forward", "lstm_forward_split", "lstm_wide_in_forward", "lstm_stack256_forward"):
        monkeypatch.setattr(hip, name, forward(name))
    monkeypatch.setattr(fused_lstm, "_h0_planes", lambda h0: ("planes", "bound"))

    def upper_backward(below, h0, c0, hs, gates, cs, dhs, whht, wiht, *, wgrad, rows_packed=None, h0_bound=None):
        calls.append(("upper", wgrad, whht, wiht, rows_packed, float(dhs.flatten()[0])))
        return {"w_ih": None, "w_hh": None, "b": None, "dx": dhs + 1}

    def layer0_backward(x, h0, c0, hs, gates, cs, dhs, whht, *, wgrad, rows_packed=None, wide_in=False, h0_bound=None, **kw):
        calls.append(("layer0", wgrad, whht, rows_packed, wide_in, h0_bound, float(dhs.flatten()[0])))
        return {"w_ih": None, "w_hh": None, "b": None}

    monkeypatch.setattr(hip, "lstm_stack256_backward", upper_backward)
    monkeypatch.setattr(hip, "lstm_backward", layer0_backward)
    lstm = torch.nn.LSTM(d_in, 256, num_layers=layers, batch_first=True)
    weights = [getattr(lstm, f"{n}_l{k}") for k in range(layers) for n in fused_lstm._STACK_PARAMS]
    ctx = _Ctx(len(weights))
    out = fused_lstm._StackLSTM.forward(ctx, z(b, l, d_in), z(layers, b, 256), z(layers, b, 256), True, *weights)
    assert out[0].shape == (b, l, 256) and out[1].shape == (layers, b, 256) and out[2].shape == (layers, b, 256)
    wide = d_in > 7
    first = "lstm_wide_in_forward" if wide else "lstm_forward_split"
    assert calls == [(first, (b, l, d_in), True)] + [("lstm_stack256_forward", (b, l, 256), True)] * 2
    assert packs == ["wide" if wide else "split", "stack256", "stack256"]
    plan0, upper = ctx.plans
    assert plan0.wide_in is wide and upper.wide_in is True and upper.backward_rows is rows
    assert ctx.h0_bound == (None if wide else "bound")
    # every switch the other way before the backward
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", "f32")
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", not rows)
    monkeypatch.setenv("RL8_AMD_LSTM_WGRAD_GATES", "separate")
    packs.clear(), calls.clear()
    grads = fused_lstm._StackLSTM.backward(ctx, z(b, l, 256), None, None)
    assert len(grads) == 4 + 4 * layers and all(g is None for g in grads[:4])
    kind = "rows" if rows else "transposed"
    assert packs == [kind, "transposed-ih"] * 2 + [kind]
    through = (None, kind) if rows else (kind, None)
    upper_wgrad = "f16-gates" if rows else "f32"
    assert calls[:2] == [("upper", upper_wgrad, through[0], "transposed-ih", through[1], 0.0),
                         ("upper", upper_wgrad, through[0], "transposed-ih", through[1], 1.0)]
    assert calls[2] == ("layer0", plan0.wgrad, None if rows else "transposed", "rows" if rows else None, wide,
                        None if wide else "bound", 2.0)
    # a pass that wants no gradient saves nothing
    ctx2 = _Ctx(len(weights))
    calls.clear()
    fused_lstm._StackLSTM.forward(ctx2, z(b, l, d_in), z(layers, b, 256), z(layers, b, 256), False, *weights)
    assert [c[2] for c in calls] == [False] * 3 and ctx2.saved_tensors == () and not hasattr(ctx2, "plans")


def test_layer_packs_are_cached_on_the_layer_and_remade_when_a_parameter_changes(monkeypatch):
    made = []
    monkeypatch.setattr(hip, "lstm_stack256_pack", lambda *p: made.append("stack256") or object())
    monkeypatch.setattr(hip, "lstm_pack_transposed", lambda w: made.append(tuple(w.shape)) or object())
    lstm = torch.nn.LSTM(4, 256, num_layers=2, batch_first=True)
    params = tuple(getattr(lstm, f"{n}_l1") for n in fused_lstm._STACK_PARAMS)
    first = fused_lstm._layer_packs(params, "stack256")
    assert fused_lstm._layer_packs(params, "stack256") is first and made == ["stack256"]
    assert fused_lstm._layer_packs(params, "transposed-ih") is fused_lstm._layer_packs(params, "transposed-ih")
    assert fused_lstm._layer_packs(params, "transposed") is not fused_lstm._layer_packs(params, "transposed-ih")
    assert made == ["stack256", (1024, 256), (1024, 256)]
    with torch.no_grad():
        params[2].add_(1.0)  # a bias: every pack of the layer carries the stamp of all four parameters
    assert fused_lstm._layer_packs(params, "stack256") is not first
    other = tuple(getattr(lstm, f"{n}_l0") for n in fused_lstm._STACK_PARAMS)
    assert "_rl8_lstm_packs" not in other[1].__dict__  # a layer's packs live on its own weight_hh
