"""The narrow recurrent models' heads (rl8_amd/csrc/lstm_narrow_heads_kernels.hip), the backward through time with the
heads inside (lstm_narrow_kernels.hip) and the rollout tail with the heads inside (rollout_kernels.hip) compiled for
gfx950: every instantiation present, no scratch in the new file and in lstm_narrow_kernels.hip; the C entries
exported, bound, and refusing bad arguments before any launch; and the lean rollout's narrow route decided on the
CPU, without a device."""

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
ENTRIES = ("rl8_linear_heads_narrow_workspace_bytes", "rl8_linear_heads_narrow_forward_f32",
           "rl8_linear_heads_narrow_forward_pair_f32", "rl8_linear_heads_narrow_backward_f32",
           "rl8_lstm_narrow_backward_heads_f32", "rl8_rollout_step_dummy_heads_narrow_f32")


def _kernels(source: str, tmp_path) -> dict:
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / (source + ".s")
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, source)],
        check=True, capture_output=True, timeout=600,
    )
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))


def _no_scratch(name: str, body: str) -> None:
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
    assert "enable_private_segment 1" not in body, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_narrow_heads_kernels_compile_without_scratch(tmp_path):
    kernels = _kernels("lstm_narrow_heads_kernels.hip", tmp_path)
    want = {f"linear_heads_narrow_{kind}_kernelILi{h}ELi{n}EE" for kind in ("forward", "backward") for h in (64, 128)
            for n in range(1, 9)}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    assert any("linear_heads_narrow_reduce_kernel" in name for name in kernels)
    for name, body in kernels.items():
        _no_scratch(name, body)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_backward_through_time_with_the_heads_inside_compiles_without_scratch(tmp_path):
    kernels = _kernels("lstm_narrow_kernels.hip", tmp_path)
    for h in (64, 128):
        for kernel in ("lstm_narrow_backward_heads_kernel", "lstm_narrow_backward_kernel"):
            hits = [name for name in kernels if f"{kernel}ILi{h}EE" in name]
            assert len(hits) == 1, (kernel, h, hits)
            _no_scratch(hits[0], kernels[hits[0]])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_rollout_tail_with_the_narrow_heads_inside_compiles(tmp_path):
    """Both widths present beside the width-256 kernel, which stays; the sampler they share indexes its two
    log-probabilities by the drawn action (a few bytes of private memory in every kernel that draws), so the bar here
    is the width-256 kernel's own private segment, not zero."""
    kernels = _kernels("rollout_kernels.hip", tmp_path)
    private = lambda body: int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))  # noqa: E731
    wide = [body for name, body in kernels.items() if "rollout_step_dummy_heads_kernel" in name]
    assert len(wide) == 1
    for h in (64, 128):
        hits = [name for name in kernels if f"rollout_step_dummy_heads_narrow_kernelILi{h}EE" in name]
        assert len(hits) == 1, (h, hits)
        assert private(kernels[hits[0]]) <= private(wide[0]), hits[0]
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", kernels[hits[0]]), hits[0]


def test_narrow_heads_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    for name in ("linear_heads_narrow_forward", "linear_heads_narrow_forward_pair", "linear_heads_narrow_backward",
                 "rollout_step_dummy_heads_narrow"):
        assert callable(getattr(hip, name)), name
    assert hip.ABI_VERSION == 107 and hip.HEADS_MAX_OUT == 8 and hip.ROWS_BACKWARD_HEADS == 4


def test_narrow_heads_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    ws = lib.rl8_linear_heads_narrow_workspace_bytes
    fwd = lib.rl8_linear_heads_narrow_forward_f32
    pair = lib.rl8_linear_heads_narrow_forward_pair_f32
    bwd = lib.rl8_linear_heads_narrow_backward_f32
    bptt = lib.rl8_lstm_narrow_backward_heads_f32
    tail = lib.rl8_rollout_step_dummy_heads_narrow_f32

    def fwd_args(h=fake, m=10, hidden=64, w=fake, b=fake, n=3, out=fake):
        return h, m, hidden, w, b, n, out, None

    def pair_args(h=fake, m=10, hidden=64, w_a=fake, b_a=fake, n_a=2, out_a=fake, w_b=fake, b_b=fake, n_b=1, out_b=fake):
        return h, m, hidden, w_a, b_a, n_a, out_a, w_b, b_b, n_b, out_b, None

    def bwd_args(h=fake, dout=fake, m=10, hidden=64, w=fake, n=3, dh=fake, wsp=fake, grads=fake):
        return h, dout, m, hidden, w, n, dh, wsp, grads, None

    def bptt_args(x=fake, b=10, l=2, d_in=4, h0=fake, c0=fake, w_hh=fake, hidden=64, hs=fake, gates=fake, cs=fake,
                  dout=fake, w=fake, wsp=fake):
        return x, b, l, d_in, h0, c0, w_hh, hidden, hs, gates, cs, dout, w, wsp, None

    def tail_args(h=fake, hidden=64, w_pol=fake, b_pol=fake, w_vf=fake, b_vf=fake, noise=None, state=fake, act=fake,
                  logp=fake, val=fake, rew=fake, obs=fake, rdr_t=None, rdr_t1=None, n=10):
        return (h, hidden, w_pol, b_pol, w_vf, b_vf, noise, state, act, logp, val, rew, obs, rdr_t, rdr_t1, 0.99, n, 1,
                2, 0, 0, None)

    # the slabs: one per workgroup, a function of m alone
    assert ws(1, 64, 1) == 4 * 65 and ws(64, 128, 8) == 4 * 8 * 129 and ws(65, 64, 3) == 2 * 4 * 3 * 65
    assert ws(1 << 21, 64, 3) == 1024 * 4 * 3 * 65
    # NULL pointers
    for name in ("h", "w", "b", "out"):
        assert fwd(*fwd_args(**{name: None})) == -1, name
    for name in ("h", "w_a", "b_a", "out_a", "w_b", "b_b", "out_b"):
        assert pair(*pair_args(**{name: None})) == -1, name
    for name in ("h", "dout", "w", "wsp", "grads"):
        assert bwd(*bwd_args(**{name: None})) == -1, name
    for name in ("x", "h0", "c0", "w_hh", "hs", "gates", "cs", "dout", "w", "wsp"):
        assert bptt(*bptt_args(**{name: None})) == -1, name
    for name in ("h", "w_pol", "b_pol", "w_vf", "b_vf", "state", "act", "logp", "val", "rew", "obs"):
        assert tail(*tail_args(**{name: None})) == -1, name
    assert tail(*tail_args(rdr_t=fake)) == -1 and tail(*tail_args(rdr_t1=fake)) == -1  # both or neither
    # widths and sizes
    for hidden in (32, 96, 256):
        assert ws(10, hidden, 3) == -2, hidden
        assert fwd(*fwd_args(hidden=hidden)) == -2, hidden
        assert pair(*pair_args(hidden=hidden)) == -2, hidden
        assert bwd(*bwd_args(hidden=hidden)) == -2, hidden
        assert bptt(*bptt_args(hidden=hidden)) == -2, hidden
        assert tail(*tail_args(hidden=hidden)) == -2, hidden
    assert ws(0, 64, 3) == -2
    assert fwd(*fwd_args(m=0)) == -2 and pair(*pair_args(m=0)) == -2 and bwd(*bwd_args(m=0)) == -2
    assert bptt(*bptt_args(b=0)) == -2 and bptt(*bptt_args(l=0)) == -2 and bptt(*bptt_args(d_in=17)) == -2
    assert tail(*tail_args(n=0)) == -2
    for n in (0, 9):
        assert ws(10, 64, n) == -2, n
        assert fwd(*fwd_args(n=n)) == -2, n
        assert bwd(*bwd_args(n=n)) == -2, n
    assert pair(*pair_args(n_a=0)) == -2 and pair(*pair_args(n_b=0)) == -2 and pair(*pair_args(n_a=8, n_b=1)) == -2
    # alignment
    assert fwd(*fwd_args(h=fake + 4)) == -3 and fwd(*fwd_args(w=fake + 8)) == -3 and fwd(*fwd_args(out=fake + 2)) == -3
    assert pair(*pair_args(h=fake + 4)) == -3 and pair(*pair_args(w_b=fake + 4)) == -3
    assert pair(*pair_args(out_b=fake + 1)) == -3
    assert bwd(*bwd_args(h=fake + 2)) == -3 and bwd(*bwd_args(dh=fake + 1)) == -3 and bwd(*bwd_args(grads=fake + 2)) == -3
    assert bptt(*bptt_args(dout=fake + 4)) == -3 and bptt(*bptt_args(wsp=fake + 8)) == -3
    assert bptt(*bptt_args(w=fake + 2)) == -3 and bptt(*bptt_args(gates=fake + 1)) == -3
    assert tail(*tail_args(h=fake + 4)) == -3 and tail(*tail_args(w_vf=fake + 8)) == -3
    assert tail(*tail_args(noise=fake + 4)) == -3


# --- the lean rollout's narrow route, on CPU stand-ins (cf. tests/test_lstm_plan.py::_lean_rollout) ------------------
def _algo(monkeypatch, model, n: int = 64, horizon: int = 4, distribution=None):
    from rl8_amd.distributions import Categorical
    from rl8_amd.env import DiscreteDummyEnv

    d_in, hidden = model.lstm.input_size, model.lstm.hidden_size
    ns = types.SimpleNamespace
    tm = {k: torch.zeros(horizon + 1, n, w) for k, w in ((DataKeys.OBS, d_in), (DataKeys.ACTIONS, 1), (DataKeys.LOGP, 1),
                                                          (DataKeys.VALUES, 1), (DataKeys.REWARDS, 1))}
    stm = {k: torch.zeros(horizon + 1, n, model.lstm.num_layers, hidden)
           for k in (DataKeys.HIDDEN_STATES, DataKeys.CELL_STATES)}
    env = object.__new__(DiscreteDummyEnv)  # (a DummyEnv, which `available` type-checks; nothing of it is run)
    env.__dict__.update(state=torch.zeros(n), env_offset=0)
    return ns(policy=ns(model=model, distribution_cls=distribution or Categorical), _tm=tm, _tm_states=stm,
              local_num_envs=n, env=env, hparams=ns(gamma=0.99), noise=ns(seed=0))


def _model(kind: str = "discrete", **config):
    from rl8_amd import models_recurrent
    from rl8_amd.specs import Categorical, Unbounded

    obs = Unbounded(shape=torch.Size([1]), device="cpu")
    if kind == "discrete":
        return models_recurrent.DefaultDiscreteRecurrentModel(obs, Categorical(2, shape=torch.Size([1]), device="cpu"),
                                                              **config)
    return models_recurrent.DefaultContinuousRecurrentModel(obs, Unbounded(shape=torch.Size([1]), device="cpu"), **config)


@pytest.fixture
def no_device(monkeypatch):
    """``hip.load`` and the build's queries stubbed (and the memo of the narrow one dropped, before and after: nothing
    may keep a stub's answers); anything that would pack weights or make planes is recorded."""
    asked = {"packs": [], "planes": 0, "plans": 0}

    def planes(rows, device, copies=1):
        asked["planes"] += 1
        return torch.zeros(copies * 64, dtype=torch.uint8)

    def plan(d_in, b):
        asked["plans"] += 1
        raise AssertionError("the narrow route reads no plan")

    monkeypatch.setattr(hip, "load", lambda: None)
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: hidden in (64, 128) and 1 <= d_in <= 16)
    monkeypatch.setattr(hip, "lstm_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_stack_supports", lambda hidden: hidden in (64, 128))
    monkeypatch.setattr(hip, "lstm_state_planes", planes)
    monkeypatch.setattr(fused_lstm, "_packs", lambda lstm, kind: asked["packs"].append(kind) or torch.zeros(1))
    monkeypatch.setattr(fused_lstm, "_plan", plan)
    monkeypatch.setattr(fused_lstm, "ENABLED", True)
    fused_lstm._narrow_supported.cache_clear()
    yield asked
    fused_lstm._narrow_supported.cache_clear()


@pytest.mark.parametrize("hidden", [64, 128])
def test_lean_rollout_is_available_for_narrow_one_layer_discrete_models(no_device, monkeypatch, hidden):
    from rl8_amd.algorithms._recurrent import _LeanRollout

    algo = _algo(monkeypatch, _model(hidden_size=hidden))
    assert _LeanRollout.available(algo) is True
    for fuse in ("1", "0", None):
        if fuse is None:
            monkeypatch.delenv("RL8_AMD_ROLLOUT_FUSE_HEADS", raising=False)
        else:
            monkeypatch.setenv("RL8_AMD_ROLLOUT_FUSE_HEADS", fuse)
        lean = _LeanRollout(algo, False)
        assert lean.narrow and lean.hidden == hidden and not lean.split
        assert lean.fuse_heads == (fuse != "0")  # (read when the rollout is set up)
        assert tuple(lean.hs.shape) == (64, hidden) and lean.planes is None
    assert no_device == {"packs": [], "planes": 0, "plans": 0}
    # the state buffers' columns are dense [N][H] slabs: what the kernel writes h_t / c_t into
    assert lean.h[1] == lean.c[1] == 64 * hidden * 4


def test_lean_rollout_is_not_available_outside_the_narrow_envelope(no_device, monkeypatch):
    from rl8_amd.algorithms._recurrent import _LeanRollout
    from rl8_amd.distributions import Normal

    assert not _LeanRollout.available(_algo(monkeypatch, _model(hidden_size=64, num_layers=2)))
    assert not _LeanRollout.available(_algo(monkeypatch, _model(hidden_size=96)))
    assert not _LeanRollout.available(_algo(monkeypatch, _model(hidden_size=64, bias=False)))
    assert not _LeanRollout.available(_algo(monkeypatch, _model("continuous", hidden_size=64), distribution=Normal))
    assert not _LeanRollout.available(_algo(monkeypatch, _model("continuous", hidden_size=128)))
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: False)  # a build without this (hidden, d_in)
    fused_lstm._narrow_supported.cache_clear()
    assert not _LeanRollout.available(_algo(monkeypatch, _model(hidden_size=64)))
    monkeypatch.setattr(fused_lstm, "ENABLED", False)
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: True)
    fused_lstm._narrow_supported.cache_clear()
    assert not _LeanRollout.available(_algo(monkeypatch, _model(hidden_size=64)))


def test_width_256_still_takes_its_step_kernel_from_the_plan(no_device, monkeypatch):
    from rl8_amd.algorithms._recurrent import _LeanRollout

    monkeypatch.setattr(fused_lstm, "_plan", lambda d_in, b: types.SimpleNamespace(forward_planes=False))
    monkeypatch.setattr(fused_lstm, "_packs", lambda lstm, kind: no_device["packs"].append(kind) or torch.zeros(1))
    algo = _algo(monkeypatch, _model(hidden_size=256))
    assert _LeanRollout.available(algo)
    lean = _LeanRollout(algo, False)
    assert not lean.narrow and no_device["packs"] == ["step"] and no_device["planes"] == 1
