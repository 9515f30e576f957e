"""The narrow LSTM kernels behind 17 to 128 input floats (rl8_amd/csrc/lstm_narrow_wide_in_kernels.hip) compiled for
gfx950 with the narrow file's flags (and the file's own of the Makefile: no packed fp32 VALU instructions): every
instantiation present, no scratch, no private segment; the C entries exported, bound, and refusing bad arguments
before any launch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PREFIX = "rl8_lstm_narrow_wide_in_"
ENTRIES = tuple(PREFIX + name for name in ("supports", "workspace_bytes", "forward_f32", "backward_f32",
                                           "backward_heads_f32", "reduce_f32", "input_grad_f32"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_compile_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "lstm_narrow_wide_in.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Xclang", "-target-feature", "-Xclang",
         "-packed-fp32-ops", f"-I{ROOT}/include", f"-I{csrc}", "-S", "--cuda-device-only", "-o", str(asm),
         os.path.join(csrc, "lstm_narrow_wide_in_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    want = {f"lstm_narrow_wide_in_proj_kernelILi{h}ELi{kg}EE" for h in (64, 128) for kg in (2, 4, 8)}
    want |= {f"lstm_narrow_wide_in_wgrad_kernelILi{h}ELi{nt}ELb0EE" for h in (64, 128) for nt in (3, 5, 9)}
    want |= {f"lstm_narrow_wide_in_wgrad_kernelILi{h}ELi{h // 16}ELb1EE" for h in (64, 128)}
    want |= {f"lstm_narrow_wide_in_dx_kernelILi{h}ELi{tpw}EE" for h, tpw in ((64, 1), (64, 2), (128, 1))}
    want |= {"lstm_narrow_wide_in_reduce_kernel"}
    found = {w for w in want if any(w in name for name in kernels)}
    assert found == want and len(kernels) == len(want), (sorted(want - found), sorted(kernels))
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 256, name  # two waves per SIMD


def test_entries_are_exported_and_bound():
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert hip.ABI_VERSION == 107 and hip.LSTM_NARROW_MAX_IN == 16


def test_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    supports, bytes_ = lib.rl8_lstm_narrow_wide_in_supports, lib.rl8_lstm_narrow_wide_in_workspace_bytes
    assert supports(64, 17) == 1 and supports(128, 128) == 1
    for h, d in ((64, 16), (64, 129), (96, 24), (256, 24)):
        assert supports(h, d) == 0 and bytes_(100, 4, h, d) == -2, (h, d)
    assert lib.rl8_lstm_narrow_supports(64, 17) == 0
    assert bytes_(0, 4, 64, 24) == -2 and bytes_(1, 0, 64, 24) == -2 and bytes_(1, 1 << 20, 128, 24) == -2
    # dz (b l 4H floats) + one slab of 4H (H + d_in + 1) floats per sequence chunk
    assert bytes_(1, 1, 64, 24) == 4 * (256 + 256 * 89)
    assert bytes_(1000, 3, 128, 128) == 4 * (1000 * 3 * 512 + 125 * 512 * 257)
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    fwd = dict(x=fake, b=10, l=2, d_in=24, h0=fake, c0=fake, w_ih=fake, w_hh=fake, b_ih=fake, b_hh=fake, hidden=64,
               zin=fake, hs=fake, hn=fake, cn=fake, save_gates=None, save_c=None, stream=None)
    bwd = dict(x=fake, b=10, l=2, d_in=24, h0=fake, c0=fake, w_hh=fake, hidden=64, hs=fake, gates=fake, cs=fake,
               dhs=fake, workspace=fake, stream=None)
    heads = {**{k: v for k, v in bwd.items() if k not in ("dhs", "workspace", "stream")}, "heads_dout": fake,
             "heads_w": fake, "workspace": fake, "stream": None}
    red = dict(workspace=fake, b=10, l=2, hidden=64, d_in=24, grads_out=fake, stream=None)
    dx = dict(workspace=fake, b=10, l=2, d_in=24, w_ih=fake, hidden=64, dx=fake, stream=None)
    cases = {"forward_f32": (fwd, {"save_gates", "save_c"}, ("zin",)), "backward_f32": (bwd, set(), ("workspace",)),
             "backward_heads_f32": (heads, set(), ("workspace", "heads_dout")), "reduce_f32": (red, set(), ("workspace",)),
             "input_grad_f32": (dx, set(), ("workspace",))}
    for name, (args, optional, aligned16) in cases.items():
        call = lambda **kw: getattr(lib, PREFIX + name)(*{**args, **kw}.values())  # noqa: E731
        pointers = [k for k, v in args.items() if v == fake or k in optional]
        for p in pointers:
            if p not in optional:
                assert call(**{p: None}) == -1, (name, p)
            assert call(**{p: fake + 2}) == (-1 if p in optional else -3), (name, p)  # (one of save_gates / save_c: NULL)
        for p in aligned16:
            assert call(**{p: fake + 4}) == -3, (name, p)
        for kw in ({"b": 0}, {"l": 0}, {"l": 1 << 20}, {"hidden": 96}, {"hidden": 256}, {"d_in": 16}, {"d_in": 129}):
            assert call(**kw) == -2, (name, kw)
    assert lib.rl8_lstm_narrow_wide_in_forward_f32(*{**fwd, "save_gates": fake + 1, "save_c": fake}.values()) == -3
