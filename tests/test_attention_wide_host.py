"""The MFMA attention entries (``rl8_attention_wide_*``) without a GPU: their envelope, one refusal of each code before
any launch, and the Python route's opt-in switch ``RL8_AMD_WIDE_ATTENTION``."""

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import fused_attention


def test_wide_supports_at_the_envelope_s_edges():
    supports = hip.load().rl8_attention_wide_supports
    assert supports(128, 128, 1, 64) == 1 and supports(1, 1, 1, 1) == 1
    assert supports(129, 5, 1, 8) == 0 and supports(5, 129, 1, 8) == 0 and supports(5, 5, 1, 65) == 0
    for args in ((0, 5, 4, 2), (5, 0, 4, 2), (5, 5, 0, 2), (5, 5, 4, 0)):
        assert supports(*args) == -2, args
    # what the short entry leaves
    for args in ((5, 5, 2, 17), (65, 65, 4, 2)):
        assert supports(*args) == 1 and hip.load().rl8_attention_supports(*args) == 0, args
    assert hip.attention_wide_supports(65, 5, 4, 2) and not hip.attention_wide_supports(129, 5, 4, 2)
    with pytest.raises(ValueError):
        hip.attention_wide_supports(5, 5, 4, 0)


def test_wide_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p = [4096 * (i + 1) for i in range(11)]  # (never dereferenced: every call fails its checks first)

    def forward(q=p[0], q_stride=102, tq=65, heads=2, d=17, out=p[3]):
        return lib.rl8_attention_wide_f32(q, q_stride, p[1], p[2], 102, None, None, 8, tq, 65, heads, d, out, None, None)

    def backward(q=p[0], tq=65, heads=2, d=17, dq=p[6], dkv_stride=102):
        return lib.rl8_attention_wide_backward_f32(q, 102, p[1], p[2], 102, None, None, p[3], p[4], p[5], 8, tq, 65, heads,
                                                   d, dq, 102, p[7], p[8], dkv_stride, p[9], None)

    assert forward(out=None) == -1 and backward(dq=None) == -1  # RL8_ENULL
    assert forward(tq=0) == -2 and forward(q_stride=33) == -2  # RL8_ESIZE
    assert backward(heads=0) == -2 and backward(dkv_stride=33) == -2
    assert forward(q=p[10] + 2) == -3 and backward(dq=p[10] + 1) == -3  # RL8_EALIGN
    assert forward(tq=129) == -4 and backward(heads=1, d=65) == -4  # RL8_ECONFIG
    # in that order: the earlier refusal wins
    assert forward(out=None, tq=0) == -1 and forward(tq=0, q=p[10] + 2) == -2 and forward(q=p[10] + 2, tq=129) == -3


def test_the_route_takes_the_wide_envelope_only_when_asked(monkeypatch):
    def core(*args):
        raise RuntimeError("reached the kernels")

    monkeypatch.setattr(fused_attention, "self_attention_core", core)
    monkeypatch.setattr(fused_attention, "cross_attention_core", core)
    monkeypatch.setattr(fused_attention, "_on_device", lambda t: not t.is_meta)  # (host tensors stand in for HIP ones)
    monkeypatch.delenv("RL8_AMD_ATTENTION_KERNELS", raising=False)

    def taken(embed, heads, shape) -> bool:
        x = torch.zeros(shape)
        try:
            return fused_attention.multihead_attention(nn.MultiheadAttention(embed, heads, batch_first=True), x, x, None,
                                                       None) is not None
        except RuntimeError as err:
            assert "reached the kernels" in str(err)
            return True

    inside = ((34, 2, (3, 5, 34)), (8, 4, (3, 65, 8)))
    outside = ((8, 4, (3, 129, 8)), (130, 2, (3, 5, 130)))
    monkeypatch.delenv("RL8_AMD_WIDE_ATTENTION", raising=False)
    for value in (None, "0", "yes"):
        if value is not None:
            monkeypatch.setenv("RL8_AMD_WIDE_ATTENTION", value)
        assert not any(taken(*call) for call in inside + outside) and taken(8, 4, (3, 5, 8)), value
    monkeypatch.setenv("RL8_AMD_WIDE_ATTENTION", "1")
    assert all(taken(*call) for call in inside) and not any(taken(*call) for call in outside)
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "0")
    assert not any(taken(*call) for call in inside) and not taken(8, 4, (3, 5, 8))
