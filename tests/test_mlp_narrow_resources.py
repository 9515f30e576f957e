"""The narrow tower kernels (rl8_amd/csrc/mlp_narrow_kernels.hip) compiled for gfx950: every instantiation present,
no scratch, no private segment; the C entries exported, bound, and refusing bad arguments before any launch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_mlp_narrow_supports", "rl8_mlp_narrow_workspace_bytes", "rl8_mlp_narrow_forward_f32",
           "rl8_mlp_narrow_backward_f32", "rl8_mlp_narrow_reduce_f32")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_narrow_kernels_compile_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "narrow.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "mlp_narrow_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    want = {f"mlp_narrow_{kind}_kernelILi{h}ELi{kin}ELi{kout}E"
            for kind in ("forward", "backward") for h in (64, 128) for kin in (4, 16) for kout in (2, 8)}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want, sorted(want - found)
    assert any("mlp_narrow_reduce_kernel" in name for name in kernels)
    for name, body in kernels.items():
        if "mlp_narrow" not in name:
            continue
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name


def test_narrow_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name


def test_narrow_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    assert lib.rl8_mlp_narrow_supports(64, 1, 1) == 1 and lib.rl8_mlp_narrow_supports(128, 16, 8) == 1
    for h, d, n in ((96, 4, 2), (256, 4, 2), (64, 0, 2), (64, 17, 2), (128, 4, 0), (128, 4, 9)):
        assert lib.rl8_mlp_narrow_supports(h, d, n) == 0, (h, d, n)
        assert lib.rl8_mlp_narrow_workspace_bytes(100, h, d, n) == -2, (h, d, n)
    assert lib.rl8_mlp_narrow_workspace_bytes(0, 64, 1, 1) == -2
    assert lib.rl8_mlp_narrow_workspace_bytes(1, 64, 1, 1) > 0
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    ptrs = [fake] * 8
    # NULL pointers
    assert lib.rl8_mlp_narrow_forward_f32(None, 10, 4, *ptrs[:6], 2, 64, fake, None) == -1
    assert lib.rl8_mlp_narrow_forward_f32(fake, 10, 4, *ptrs[:6], 2, 64, None, None) == -1
    assert lib.rl8_mlp_narrow_backward_f32(fake, None, 10, 4, *ptrs[:5], 2, 64, fake, None) == -1
    assert lib.rl8_mlp_narrow_backward_f32(fake, fake, 10, 4, *ptrs[:5], 2, 64, None, None) == -1
    assert lib.rl8_mlp_narrow_reduce_f32(None, 10, 64, 4, 2, fake, None) == -1
    # sizes / widths
    assert lib.rl8_mlp_narrow_forward_f32(fake, 0, 4, *ptrs[:6], 2, 64, fake, None) == -2
    assert lib.rl8_mlp_narrow_forward_f32(fake, 10, 17, *ptrs[:6], 2, 64, fake, None) == -2
    assert lib.rl8_mlp_narrow_forward_f32(fake, 10, 4, *ptrs[:6], 9, 64, fake, None) == -2
    assert lib.rl8_mlp_narrow_forward_f32(fake, 10, 4, *ptrs[:6], 2, 256, fake, None) == -2
    assert lib.rl8_mlp_narrow_backward_f32(fake, fake, 10, 4, *ptrs[:5], 2, 96, fake, None) == -2
    assert lib.rl8_mlp_narrow_reduce_f32(fake, 0, 64, 4, 2, fake, None) == -2
    # alignment
    assert lib.rl8_mlp_narrow_forward_f32(fake + 2, 10, 4, *ptrs[:6], 2, 64, fake, None) == -3
    assert lib.rl8_mlp_narrow_backward_f32(fake, fake, 10, 4, *ptrs[:5], 2, 64, fake + 1, None) == -3
    assert lib.rl8_mlp_narrow_reduce_f32(fake, 10, 64, 4, 2, fake + 2, None) == -3
