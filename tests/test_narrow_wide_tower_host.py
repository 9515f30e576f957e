"""The narrow-wide tower kernels (rl8_amd/csrc/mlp_narrow_wide_kernels.hip) compiled for gfx950: every instantiation
present, no scratch, LDS and registers as DESIGN.md states them; the envelope; every entry refusing bad arguments
before any launch; and the classifier ``fused_mlp._classify`` (family "narrow_wide") clause by clause on CPU modules."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import fused_mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLASSES = (1, 2, 4)  # 32-column tiles of the compiled d_in / n_out classes (32, 64, 128)


def _limits(backward, hidden, d_in, n_out):
    out = (ctypes.c_int * 2)()
    assert hip.load().rl8_mlp_narrow_wide_limits(backward, hidden, d_in, n_out, out) == 0
    return out[0], out[1]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_compile_without_scratch_inside_lds_and_registers(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "narrow_wide.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-S", "--cuda-device-only", "-o", str(asm),
         os.path.join(csrc, "mlp_narrow_wide_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    field = lambda body, name: int(re.search(rf"\.amdhsa_{name} (\d+)", body).group(1))  # noqa: E731
    seen = set()
    for name, body in kernels.items():
        assert "mlp_narrow_wide" in name, name
        assert field(body, "private_segment_fixed_size") == 0 and re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert field(body, "group_segment_fixed_size") == 0, name  # (all LDS is dynamic: rl8_mlp_narrow_wide_limits)
        inst = re.search(r"mlp_narrow_wide_(forward|backward)_kernelILi(\d+)ELi(\d)ELi(\d)E", name)
        if inst is None:
            seen.add(re.search(r"mlp_narrow_wide_(pack|reduce)_kernel", name).group(1))
            continue
        kind, h, ti, to = inst.group(1), *map(int, inst.groups()[1:])
        seen.add((kind, h, ti, to))
        lds, per_cu = _limits(int(kind == "backward"), h, 32 * ti, 32 * to)
        # activations only, 64 rows of (class + 4)-float tiles; two workgroups per CU where two fit
        want = 256 * ((32 * ti + 4) + 2 * (h + 4) + ((32 * to + 4) if kind == "backward" else 0))
        assert lds == want and lds * per_cu <= 160 * 1024, (name, lds, per_cu)
        # (registers per lane: 512 with one workgroup per CU, 256 with two; accumulators and vector registers together)
        assert field(body, "next_free_vgpr") <= 512 // per_cu, (name, field(body, "next_free_vgpr"))
    assert seen == {"pack", "reduce", *((k, h, ti, to) for k in ("forward", "backward") for h in (64, 128)
                                        for ti in CLASSES for to in CLASSES)}
    assert _limits(1, 128, 128, 128) == (135168, 1) and _limits(0, 128, 128, 128) == (101376, 1)
    assert _limits(1, 64, 24, 12) == (53248, 2) and _limits(0, 64, 24, 12) == (44032, 2)


def test_envelope_and_refusals_before_any_launch():
    lib = hip.load()
    for inside in ((64, 17, 1), (128, 128, 128), (64, 1, 9)):
        assert lib.rl8_mlp_narrow_wide_supports(*inside) == 1, inside
        assert lib.rl8_mlp_narrow_wide_workspace_bytes(100, *inside, 0) > 0
        assert lib.rl8_mlp_narrow_wide_workspace_bytes(100, *inside, 1) > lib.rl8_mlp_narrow_wide_workspace_bytes(100, *inside, 0)
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    w = [fake] * 5
    for h, d, n in ((64, 16, 8), (64, 129, 1), (64, 1, 129), (96, 24, 4), (256, 24, 4), (0, 24, 4), (64, 0, 9),
                    (64, 24, 0), (-64, 24, 4), (64, -1, 9), (64, 24, -3)):
        assert lib.rl8_mlp_narrow_wide_supports(h, d, n) == 0, (h, d, n)
        assert lib.rl8_mlp_narrow_wide_workspace_bytes(100, h, d, n, 1) == -2, (h, d, n)
        assert lib.rl8_mlp_narrow_wide_limits(1, h, d, n, (ctypes.c_int * 2)()) == -2, (h, d, n)
        assert lib.rl8_mlp_narrow_wide_forward_f32(fake, 10, d, *w, fake, n, h, fake, fake, None) == -2, (h, d, n)
        assert lib.rl8_mlp_narrow_wide_backward_f32(fake, fake, 10, d, *w, n, h, fake, fake, None) == -2, (h, d, n)
        assert lib.rl8_mlp_narrow_wide_reduce_f32(fake, 10, h, d, n, fake, None) == -2, (h, d, n)
    assert lib.rl8_mlp_narrow_wide_workspace_bytes(0, 64, 24, 4, 1) == -2
    assert lib.rl8_mlp_narrow_wide_workspace_bytes(10, 64, 24, 4, 2) == -4
    assert lib.rl8_mlp_narrow_wide_limits(0, 64, 24, 4, None) == -1
    # rows
    assert lib.rl8_mlp_narrow_wide_forward_f32(fake, 0, 24, *w, fake, 4, 64, fake, fake, None) == -2
    # NULL pointers (dx alone may be NULL)
    assert lib.rl8_mlp_narrow_wide_forward_f32(None, 10, 24, *w, fake, 4, 64, fake, fake, None) == -1
    assert lib.rl8_mlp_narrow_wide_backward_f32(fake, None, 10, 24, *w, 4, 64, fake, fake, None) == -1
    assert lib.rl8_mlp_narrow_wide_backward_f32(fake, fake, 10, 24, *w, 4, 64, None, None, None) == -1
    assert lib.rl8_mlp_narrow_wide_reduce_f32(None, 10, 64, 24, 4, fake, None) == -1
    # alignment: the workspace to 16 bytes, everything else to 4
    assert lib.rl8_mlp_narrow_wide_forward_f32(fake, 10, 24, *w, fake, 4, 64, fake + 4, fake, None) == -3
    assert lib.rl8_mlp_narrow_wide_backward_f32(fake, fake, 10, 24, *w, 4, 64, fake + 8, None, None) == -3
    assert lib.rl8_mlp_narrow_wide_reduce_f32(fake + 4, 10, 64, 24, 4, fake, None) == -3


def _trunk(d_in, h1, h2, bias=True, act=nn.ReLU):
    return nn.Sequential(nn.Sequential(nn.Linear(d_in, h1, bias=bias), act(), nn.Linear(h1, h2, bias=bias)), act())


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_the_classifier_clause_by_clause_and_cpu_tensors(switch, monkeypatch):
    monkeypatch.delenv("RL8_AMD_NARROW_WIDE_TOWERS", raising=False) if switch is None else monkeypatch.setenv(
        "RL8_AMD_NARROW_WIDE_TOWERS", switch)
    def family(trunk, heads):  # ((layer 1, layer 2) of a narrow-wide tower, ``None`` for every other answer)
        found = fused_mlp._classify(trunk, heads)
        return (found.l1, found.l2) if found is not None and found.family == "narrow_wide" else None

    assert fused_mlp.narrow_wide_towers_on() == (switch == "1")
    for h in (64, 128):
        head = nn.Linear(h, 12)
        trunk = _trunk(24, h, h)
        assert family(trunk, [head]) == (trunk[0][0], trunk[0][2])
        assert family(trunk, [nn.Linear(h, 6), nn.Linear(h, 6)]) is not None  # (two heads: their outputs in all)
        assert family(trunk, [nn.Linear(h, 4)]) is not None and family(_trunk(4, h, h), [head]) is not None  # one side
        assert family(_trunk(16, h, h), [nn.Linear(h, 8)]) is None  # inside 16 x 8: the narrow kernels' own
        assert fused_mlp._classify(_trunk(16, h, h), [nn.Linear(h, 8)]).family == "narrow"
        assert family(_trunk(128, h, h), [nn.Linear(h, 128)]) is not None
        assert family(_trunk(129, h, h), [head]) is None and family(trunk, [nn.Linear(h, 129)]) is None
        assert family(trunk, []) is None and family(trunk, [nn.Linear(h, 12, bias=False)]) is None
        assert family(_trunk(24, h, h, bias=False), [head]) is None and family(_trunk(24, h, h, act=nn.Tanh), [head]) is None
        assert family(_trunk(24, h, 192 - h), [nn.Linear(192 - h, 12)]) is None  # mixed widths
        with_norm = nn.Sequential(nn.Sequential(trunk[0][0], nn.BatchNorm1d(h), nn.ReLU(), trunk[0][2]), nn.ReLU())
        assert fused_mlp._classify(with_norm, [head]) is None  # (a BatchNorm tower outside 16 x 8 is no family's)
        assert fused_mlp.tower_forward(trunk, [head], torch.randn(10, 24)) is None  # CPU tensors, whatever the switch
    for width in (96, 256):
        assert family(_trunk(24, width, width), [nn.Linear(width, 12)]) is None
