"""The stacked LSTM kernels (lstm_narrow_stack_* in rl8_amd/csrc/lstm_narrow_kernels.hip) compiled for gfx950: every
instantiation present, no scratch, no private segment; the rl8_lstm_stack_* entries exported, bound, and refusing
bad arguments before any launch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_lstm_stack_supports", "rl8_lstm_stack_workspace_bytes", "rl8_lstm_stack_forward_f32",
           "rl8_lstm_stack_backward_f32", "rl8_lstm_stack_reduce_f32")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_stack_lstm_kernels_compile_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "lstm_stack.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "lstm_narrow_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    want = {f"lstm_narrow_stack_proj_kernelILi{h}EE" for h in (64, 128)}
    want |= {f"lstm_narrow_stack_forward_kernelILi{h}ELb{save}EE" for h in (64, 128) for save in (0, 1)}
    want |= {f"lstm_narrow_stack_dx_kernelILi{h}EE" for h in (64, 128)}
    want |= {f"lstm_narrow_stack_wgrad_kernelILi{h}ELb{xpart}EE" for h in (64, 128) for xpart in (0, 1)}
    # the backward through time and the reduce are the one-layer ones: they must stay in the file for any layer
    want |= {f"lstm_narrow_backward_kernelILi{h}EE" for h in (64, 128)} | {"lstm_narrow_reduce_kernel"}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    stack = {name: body for name, body in kernels.items() if "lstm_narrow_stack" in name}
    assert len(stack) == 12, sorted(stack)
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name


def test_stack_lstm_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert hip.ABI_VERSION == 107


def test_stack_lstm_entries_leave_the_narrow_envelope_alone():
    lib = hip.load()
    assert lib.rl8_lstm_narrow_supports(64, 17) == 0 and lib.rl8_lstm_narrow_supports(128, 64) == 0
    assert lib.rl8_lstm_narrow_supports(64, 64) == 0 and lib.rl8_lstm_narrow_supports(128, 128) == 0


def test_stack_lstm_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    assert lib.rl8_lstm_stack_supports(64) == 1 and lib.rl8_lstm_stack_supports(128) == 1
    for h in (96, 256, 32, 0):
        assert lib.rl8_lstm_stack_supports(h) == 0, h
        assert lib.rl8_lstm_stack_workspace_bytes(100, 4, h) == -2, h
    assert lib.rl8_lstm_stack_workspace_bytes(0, 4, 64) == -2
    assert lib.rl8_lstm_stack_workspace_bytes(1, 0, 64) == -2
    assert lib.rl8_lstm_stack_workspace_bytes(1, 1 << 20, 128) == -2
    # dz (b l 4H floats) + one slab of 4H (H + H + 1) floats per sequence chunk
    assert lib.rl8_lstm_stack_workspace_bytes(1, 1, 64) == 4 * (256 + 256 * 129)
    assert lib.rl8_lstm_stack_workspace_bytes(1000, 3, 128) == 4 * (1000 * 3 * 512 + 125 * 512 * 257)
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    fwd = lib.rl8_lstm_stack_forward_f32
    bwd = lib.rl8_lstm_stack_backward_f32
    red = lib.rl8_lstm_stack_reduce_f32

    def fwd_args(**kw):
        a = dict(x=fake, b=10, l=2, h0=fake, c0=fake, w_ih=fake, w_hh=fake, b_ih=fake, b_hh=fake, hidden=64, zin=fake,
                 hs=fake, hn=fake, cn=fake, save_gates=None, save_c=None, stream=None)
        a.update(kw)
        return list(a.values())

    def bwd_args(**kw):
        a = dict(x=fake, b=10, l=2, h0=fake, c0=fake, w_ih=fake, w_hh=fake, hidden=64, hs=fake, gates=fake, cs=fake,
                 dhs=fake, workspace=fake, dx=fake, stream=None)
        a.update(kw)
        return list(a.values())

    # NULL pointers (save_gates / save_c: both or neither)
    for name in ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh", "zin", "hs", "hn", "cn"):
        assert fwd(*fwd_args(**{name: None})) == -1, name
    assert fwd(*fwd_args(save_gates=fake)) == -1
    assert fwd(*fwd_args(save_c=fake)) == -1
    for name in ("x", "h0", "c0", "w_ih", "w_hh", "hs", "gates", "cs", "dhs", "workspace", "dx"):
        assert bwd(*bwd_args(**{name: None})) == -1, name
    assert red(None, 10, 2, 64, fake, None) == -1
    assert red(fake, 10, 2, 64, None, None) == -1
    # sizes / widths
    for kw in ({"b": 0}, {"l": 0}, {"hidden": 96}, {"hidden": 256}, {"hidden": 32}, {"l": 1 << 20}):
        assert fwd(*fwd_args(**kw)) == -2, kw
        assert bwd(*bwd_args(**kw)) == -2, kw
    assert red(fake, 0, 2, 64, fake, None) == -2
    assert red(fake, 10, 0, 64, fake, None) == -2
    assert red(fake, 10, 2, 96, fake, None) == -2
    assert red(fake, 10, 2, 256, fake, None) == -2
    # alignment
    assert fwd(*fwd_args(x=fake + 2)) == -3
    assert fwd(*fwd_args(zin=fake + 4)) == -3
    assert fwd(*fwd_args(save_gates=fake + 1, save_c=fake)) == -3
    assert bwd(*bwd_args(workspace=fake + 4)) == -3
    assert bwd(*bwd_args(dx=fake + 2)) == -3
    assert bwd(*bwd_args(w_ih=fake + 1)) == -3
    assert red(fake + 8, 10, 2, 64, fake, None) == -3
    assert red(fake, 10, 2, 64, fake + 2, None) == -3
