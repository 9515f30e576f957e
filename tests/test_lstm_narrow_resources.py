"""The narrow LSTM kernels (rl8_amd/csrc/lstm_narrow_kernels.hip) compiled for gfx950: every instantiation present,
no scratch, no private segment; the C entries exported, bound, and refusing bad arguments before any launch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_lstm_narrow_supports", "rl8_lstm_narrow_workspace_bytes", "rl8_lstm_narrow_forward_f32",
           "rl8_lstm_narrow_backward_f32", "rl8_lstm_narrow_reduce_f32")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_narrow_lstm_kernels_compile_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "lstm_narrow.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "lstm_narrow_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    want = {f"lstm_narrow_forward_kernelILi{h}ELi{kin}ELb{save}EE" for h in (64, 128) for kin in (4, 16)
            for save in (0, 1)}
    want |= {f"lstm_narrow_wgrad_kernelILi{h}ELi{kin}EE" for h in (64, 128) for kin in (4, 16)}
    want |= {f"lstm_narrow_backward_kernelILi{h}EE" for h in (64, 128)}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    assert any("lstm_narrow_reduce_kernel" in name for name in kernels)
    for name, body in kernels.items():
        assert "lstm_narrow" in name, name
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name


def test_narrow_lstm_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert hip.LSTM_NARROW_HIDDEN == (64, 128)


def test_narrow_lstm_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    assert lib.rl8_lstm_narrow_supports(64, 1) == 1 and lib.rl8_lstm_narrow_supports(128, 16) == 1
    for h, d in ((96, 4), (256, 4), (64, 0), (64, 17), (32, 4)):
        assert lib.rl8_lstm_narrow_supports(h, d) == 0, (h, d)
        assert lib.rl8_lstm_narrow_workspace_bytes(100, 4, h, d) == -2, (h, d)
    assert lib.rl8_lstm_narrow_workspace_bytes(0, 4, 64, 1) == -2
    assert lib.rl8_lstm_narrow_workspace_bytes(1, 0, 64, 1) == -2
    assert lib.rl8_lstm_narrow_workspace_bytes(1, 1 << 20, 128, 1) == -2
    # dz (b l 4H floats) + one slab of 4H (H + d_in + 1) floats per sequence chunk
    assert lib.rl8_lstm_narrow_workspace_bytes(1, 1, 64, 1) == 4 * (256 + 256 * 66)
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    p6 = [fake] * 6
    fwd = lib.rl8_lstm_narrow_forward_f32
    bwd = lib.rl8_lstm_narrow_backward_f32
    red = lib.rl8_lstm_narrow_reduce_f32
    # NULL pointers (save_gates / save_c: both or neither)
    assert fwd(None, 10, 2, 4, *p6, 64, fake, fake, fake, None, None, None) == -1
    assert fwd(fake, 10, 2, 4, *p6, 64, fake, fake, None, None, None, None) == -1
    assert fwd(fake, 10, 2, 4, *p6, 64, fake, fake, fake, fake, None, None) == -1
    assert bwd(fake, 10, 2, 4, fake, fake, fake, 64, fake, fake, fake, None, fake, None) == -1
    assert bwd(fake, 10, 2, 4, fake, fake, fake, 64, fake, fake, fake, fake, None, None) == -1
    assert red(None, 10, 2, 64, 4, fake, None) == -1
    assert red(fake, 10, 2, 64, 4, None, None) == -1
    # sizes / widths
    assert fwd(fake, 0, 2, 4, *p6, 64, fake, fake, fake, None, None, None) == -2
    assert fwd(fake, 10, 0, 4, *p6, 64, fake, fake, fake, None, None, None) == -2
    assert fwd(fake, 10, 2, 17, *p6, 64, fake, fake, fake, None, None, None) == -2
    assert fwd(fake, 10, 2, 4, *p6, 256, fake, fake, fake, None, None, None) == -2
    assert fwd(fake, 10, 2, 4, *p6, 96, fake, fake, fake, None, None, None) == -2
    assert bwd(fake, 10, 2, 4, fake, fake, fake, 96, fake, fake, fake, fake, fake, None) == -2
    assert bwd(fake, 10, 2, 0, fake, fake, fake, 64, fake, fake, fake, fake, fake, None) == -2
    assert red(fake, 0, 2, 64, 4, fake, None) == -2
    assert red(fake, 10, 2, 128, 17, fake, None) == -2
    # alignment
    assert fwd(fake + 2, 10, 2, 4, *p6, 64, fake, fake, fake, None, None, None) == -3
    assert fwd(fake, 10, 2, 4, *p6, 64, fake, fake, fake, fake + 1, fake, None) == -3
    assert bwd(fake, 10, 2, 4, fake, fake, fake, 64, fake, fake, fake, fake, fake + 4, None) == -3
    assert bwd(fake, 10, 2, 4, fake, fake + 2, fake, 64, fake, fake, fake, fake, fake, None) == -3
    assert red(fake + 8, 10, 2, 64, 4, fake, None) == -3
    assert red(fake, 10, 2, 64, 4, fake + 2, None) == -3
