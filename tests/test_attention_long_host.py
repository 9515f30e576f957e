"""The streaming attention entries (``rl8_attention_long_*``) without a GPU: their envelope, one refusal of each code
before any launch, the Python route's opt-in switch ``RL8_AMD_LONG_ATTENTION``, and the unit's kernels without scratch."""

import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import fused_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_long_supports_at_the_envelope_s_edges():
    supports = hip.load().rl8_attention_long_supports
    assert supports(2048, 2048, 1, 64) == 1 and supports(1, 1, 1, 1) == 1
    assert supports(2049, 5, 1, 8) == 0 and supports(5, 2049, 1, 8) == 0 and supports(5, 5, 1, 65) == 0
    for args in ((0, 5, 4, 2), (5, 0, 4, 2), (5, 5, 0, 2), (5, 5, 4, 0)):
        assert supports(*args) == -2, args
    assert hip.attention_long_supports(129, 5, 4, 2) and not hip.attention_long_supports(2049, 5, 4, 2)
    with pytest.raises(ValueError):
        hip.attention_long_supports(5, 5, 4, 0)
    # the family hip.attention launches: short, then wide, then long
    assert [hip._attention_entries(t, t, 4, 2)[1] for t in (64, 65, 128, 129)] == [
        "attention", "attention_wide", "attention_wide", "attention_long"]


def test_long_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p = [4096 * (i + 1) for i in range(11)]  # (never dereferenced: every call fails its checks first)

    def forward(q=p[0], q_stride=102, tq=129, heads=2, d=17, out=p[3]):
        return lib.rl8_attention_long_f32(q, q_stride, p[1], p[2], 102, None, None, 8, tq, 129, heads, d, out, None, None)

    def backward(q=p[0], tq=129, heads=2, d=17, dq=p[6], dkv_stride=102):
        return lib.rl8_attention_long_backward_f32(q, 102, p[1], p[2], 102, None, None, p[3], p[4], p[5], 8, tq, 129,
                                                   heads, d, dq, 102, p[7], p[8], dkv_stride, p[9], None)

    assert forward(out=None) == -1 and backward(dq=None) == -1  # RL8_ENULL
    assert forward(tq=0) == -2 and forward(q_stride=33) == -2  # RL8_ESIZE
    assert backward(heads=0) == -2 and backward(dkv_stride=33) == -2
    assert forward(q=p[10] + 2) == -3 and backward(dq=p[10] + 1) == -3  # RL8_EALIGN
    assert forward(tq=2049) == -4 and backward(heads=1, d=65) == -4  # RL8_ECONFIG
    # in that order: the earlier refusal wins
    assert forward(out=None, tq=0) == -1 and forward(tq=0, q=p[10] + 2) == -2 and forward(q=p[10] + 2, tq=2049) == -3
    assert backward(dq=None, heads=0) == -1 and backward(heads=0, q=p[10] + 2) == -2
    assert backward(q=p[10] + 2, tq=2049) == -3


def test_the_route_takes_the_long_envelope_only_when_asked(monkeypatch):
    def core(*args):
        raise RuntimeError("reached the kernels")

    monkeypatch.setattr(fused_attention, "self_attention_core", core)
    monkeypatch.setattr(fused_attention, "cross_attention_core", core)
    monkeypatch.setattr(fused_attention, "_on_device", lambda t: not t.is_meta)  # (host tensors stand in for HIP ones)
    monkeypatch.delenv("RL8_AMD_ATTENTION_KERNELS", raising=False)
    monkeypatch.delenv("RL8_AMD_WIDE_ATTENTION", raising=False)

    def taken(embed, heads, shape) -> bool:
        x = torch.zeros(shape)
        try:
            return fused_attention.multihead_attention(nn.MultiheadAttention(embed, heads, batch_first=True), x, x, None,
                                                       None) is not None
        except RuntimeError as err:
            assert "reached the kernels" in str(err)
            return True

    long_only, wide_only, short = (8, 4, (3, 129, 8)), (8, 4, (3, 65, 8)), (8, 4, (3, 5, 8))
    monkeypatch.delenv("RL8_AMD_LONG_ATTENTION", raising=False)
    for value in (None, "0", "yes"):
        if value is not None:
            monkeypatch.setenv("RL8_AMD_LONG_ATTENTION", value)
        assert not taken(*long_only) and not taken(*wide_only) and taken(*short), value
    monkeypatch.setenv("RL8_AMD_LONG_ATTENTION", "1")
    assert taken(*long_only) and not taken(*wide_only) and taken(*short)
    assert not taken(130, 2, (3, 5, 130)) and not taken(8, 4, (3, 2049, 8))  # (D = 65; 2049 cells)
    monkeypatch.setenv("RL8_AMD_WIDE_ATTENTION", "1")
    assert taken(*long_only) and taken(*wide_only)
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "0")
    assert not taken(*long_only) and not taken(*wide_only) and not taken(*short)


def test_the_long_kernels_compile_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "attention_long_kernels.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Xclang", "-target-feature", "-Xclang",
         "-packed-fp32-ops", f"-I{ROOT}/include", f"-I{csrc}", "-S", "--cuda-device-only", "-o", str(asm),
         os.path.join(csrc, "attention_long_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    for kind in ("forward", "backward_q", "backward_kv"):
        for nf in (1, 2, 3, 4):
            assert sum(f"attention_long_{kind}_kernelILi{nf}E" in name for name in kernels) == 1, (kind, nf)
    assert len(kernels) == 12
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
    assert "v_mfma_f32_16x16x4_f32" in text or "v_mfma_f32_16x16x4f32" in text
    assert not re.search(r"\b(global|flat|buffer|ds)_(atomic|add_f|pk_add)\w*", text)  # the same bits on every run
