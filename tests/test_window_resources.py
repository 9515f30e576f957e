"""The window kernels (gather_windows_kernel, window_last_kernel in rl8_amd/csrc/stats_gather_kernels.hip) compiled
for gfx950: both present, no scratch, no private segment, no LDS (they declare none); the rl8_gather_windows /
rl8_window_last entries exported, bound, and refusing bad arguments before any launch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_gather_windows", "rl8_window_last")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_window_kernels_compile_without_scratch_or_lds(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "stats_gather.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "stats_gather_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    window = {name: body for name, body in kernels.items() if "gather_windows_kernel" in name or "window_last_kernel" in name}
    assert len(window) == 2, sorted(kernels)
    for name, body in window.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name


def test_window_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert hip.ABI_VERSION == 107  # (new entries only: no bump)


def assert_error_statuses(src: int, dst: int) -> None:
    """Every argument check of the two entries, with ``src`` / ``dst`` as the (never dereferenced) pointers: each call
    fails its checks before a launch."""
    lib = hip.load()

    def fields(count: int = 1, **kw):
        f = dict(src=src, dst=dst, mask=dst, env_stride=1, time_stride=8, row_elems=1, elem_bytes=4, size=2)
        f.update(kw)
        out = (hip.WindowField * count)()
        for i in range(count):
            out[i] = hip.WindowField(*f.values())
        return out

    def both(status: int, count: int = 1, **kw) -> None:
        assert lib.rl8_gather_windows(None, 8, 4, fields(count, **kw), count, None) == status, kw
        assert lib.rl8_window_last(1, 8, fields(count, **kw), count, None) == status, kw

    # RL8_ENULL: fields, src, dst
    assert lib.rl8_gather_windows(None, 8, 4, None, 1, None) == -1
    assert lib.rl8_window_last(0, 8, None, 1, None) == -1
    both(-1, src=None)
    both(-1, dst=None)
    # RL8_ESIZE: rows, horizon, step, field count, row width, window length
    assert lib.rl8_gather_windows(None, 0, 4, fields(), 1, None) == -2
    assert lib.rl8_gather_windows(None, 8, 0, fields(), 1, None) == -2
    assert lib.rl8_window_last(-1, 8, fields(), 1, None) == -2
    assert lib.rl8_window_last(0, 0, fields(), 1, None) == -2
    assert lib.rl8_gather_windows(None, 8, 4, fields(), 0, None) == -2
    assert lib.rl8_window_last(0, 8, fields(), 0, None) == -2
    nine = hip.MAX_GATHER_FIELDS + 1
    assert lib.rl8_gather_windows(None, 8, 4, fields(nine), nine, None) == -2
    assert lib.rl8_window_last(0, 8, fields(nine), nine, None) == -2
    both(-2, row_elems=0)
    both(-2, size=0)
    both(-2, size=-1)
    # RL8_ECONFIG: element width other than 1, 4 or 8; a window without a mask
    for width in (0, 2, 3, 16):
        both(-4, elem_bytes=width)
    both(-4, mask=None)
    # RL8_EALIGN: src / dst not aligned to the element
    both(-3, src=src + 2)
    both(-3, dst=dst + 1)
    both(-3, elem_bytes=8, src=src + 4)
    both(-3, elem_bytes=8, dst=dst + 4)


def test_window_entries_refuse_bad_arguments_before_launching():
    fake = 4096  # (never dereferenced: every call fails its checks first)
    assert_error_statuses(fake, fake + 4096)
