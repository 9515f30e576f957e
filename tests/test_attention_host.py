"""The short-sequence attention entries without a GPU: exported and bound, their envelope, their refusals before any
launch, the compiled kernels' resources, the torch yardstick ``attention_reference`` against ``nn.MultiheadAttention``
in float64, and the Python route's eligibility rules."""

import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rl8_amd import hip
from rl8_amd.nn import SelfAttention, fused_attention
from rl8_amd.nn.modules import attention as attention_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_attention_supports", "rl8_attention_f32", "rl8_attention_backward_f32")
#: (B, Tq, Tk, E, H)
SHAPES = ((7, 5, 5, 8, 4), (3, 1, 1, 4, 4), (5, 33, 64, 16, 1), (4, 2, 5, 12, 4))


# --- the C entries ------------------------------------------------------------------------------------------------
def test_attention_entries_are_exported_and_bound():
    lib = hip.load()
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        params = re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1))
        assert len(params.split(",")) == len(hip.SIGNATURES[name]), name
    assert hip.ABI_VERSION == 107  # (new entries only: no bump)


def test_attention_supports_at_the_envelope_s_edges():
    supports = hip.load().rl8_attention_supports
    assert supports(1, 1, 1, 1) == 1 and supports(64, 64, 4, 16) == 1 and supports(5, 5, 4, 2) == 1
    assert supports(65, 5, 4, 2) == 0 and supports(5, 65, 4, 2) == 0 and supports(5, 5, 4, 17) == 0
    for d in range(1, 17):
        assert supports(64, 1, 1, d) == 1
    for args in ((0, 5, 4, 2), (5, 0, 4, 2), (5, 5, 0, 2), (5, 5, 4, 0), (-1, 5, 4, 2), (65, 65, 4, -3)):
        assert supports(*args) == -2, args
    assert hip.attention_supports(5, 5, 4, 2) and not hip.attention_supports(5, 65, 4, 2)
    with pytest.raises(ValueError):
        hip.attention_supports(5, 5, 4, 0)


def test_attention_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p = [4096 * (i + 1) for i in range(12)]  # (never dereferenced: every call fails its checks first)

    def forward(q=p[0], q_stride=24, k=p[1], v=p[2], kv_stride=24, key_padding=None, bias=None, b=8, tq=5, tk=5,
                heads=4, d=2, out=p[3], lse=None):
        return lib.rl8_attention_f32(q, q_stride, k, v, kv_stride, key_padding, bias, b, tq, tk, heads, d, out, lse, None)

    def backward(q=p[0], q_stride=24, k=p[1], v=p[2], kv_stride=24, key_padding=None, bias=None, out=p[3], lse=p[4],
                 dout=p[5], b=8, tq=5, tk=5, heads=4, d=2, dq=p[6], dq_stride=24, dk=p[7], dv=p[8], dkv_stride=24,
                 delta_workspace=p[9]):
        return lib.rl8_attention_backward_f32(q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, b, tq, tk,
                                              heads, d, dq, dq_stride, dk, dv, dkv_stride, delta_workspace, None)

    # RL8_ENULL: every required pointer; key_padding, bias and the forward's lse are optional
    for name in ("q", "k", "v", "out"):
        assert forward(**{name: None}) == -1, name
    for name in ("q", "k", "v", "out", "lse", "dout", "dq", "dk", "dv", "delta_workspace"):
        assert backward(**{name: None}) == -1, name
    # RL8_ESIZE: a size < 1, a stride below heads * d
    for name in ("b", "tq", "tk", "heads", "d"):
        for bad in (0, -1):
            assert forward(**{name: bad}) == -2, name
            assert backward(**{name: bad}) == -2, name
    for name in ("q_stride", "kv_stride"):
        # (a stride of exactly heads * d passes the size check: shown by the NEXT refusal, RL8_ECONFIG for tq = 65 --
        # with every check passed the call would launch on the made-up pointers wherever a device is present)
        assert forward(**{name: 7}) == -2 and forward(**{name: 8}, tq=65) == -4 and forward(**{name: 7}, tq=65) == -2, name
    for name in ("q_stride", "kv_stride", "dq_stride", "dkv_stride"):
        assert backward(**{name: 7}) == -2 and backward(**{name: -24}) == -2, name
    # RL8_EALIGN: a float pointer off 4 bytes (the byte mask may sit anywhere)
    for name in ("q", "k", "v", "bias", "out", "lse"):
        assert forward(**{name: p[10] + 2}) == -3, name
    for name in ("q", "k", "v", "bias", "out", "lse", "dout", "dq", "dk", "dv", "delta_workspace"):
        assert backward(**{name: p[10] + 1}) == -3, name
    # RL8_ECONFIG: a shape outside rl8_attention_supports
    for shape in (dict(tq=65), dict(tk=65), dict(heads=1, d=17), dict(tq=128, tk=128)):
        assert forward(**shape) == -4, shape
        assert backward(**shape) == -4, shape


def test_wrappers_refuse_host_tensors():
    q, k = torch.zeros(2, 5, 8), torch.zeros(2, 3, 8)
    with pytest.raises(hip.HipExtensionError):
        hip.attention(q, k, k, None, None, 4)
    with pytest.raises(hip.HipExtensionError):
        hip.attention_backward(q, k, k, None, None, torch.zeros(2, 5, 8), torch.zeros(2, 4, 5), torch.zeros(2, 5, 8), 4,
                               torch.zeros(2, 5, 8), torch.zeros(2, 3, 8), torch.zeros(2, 3, 8))


def test_wrappers_check_layouts_before_the_library_sees_them():
    qkv = torch.zeros(2, 5, 24)
    q, k, v = qkv[..., :8], qkv[..., 8:16], qkv[..., 16:]
    assert hip._rows(q, (2, 5, 8), "q") == 24 and hip._rows(torch.zeros(2, 5, 8), (2, 5, 8), "q") == 8
    assert hip._rows(torch.zeros(3, 1, 24)[..., 8:16], (3, 1, 8), "k") == 24
    with pytest.raises(ValueError):
        hip._rows(torch.zeros(2, 8, 5).transpose(1, 2), (2, 5, 8), "q")
    with pytest.raises(ValueError):
        hip._rows(qkv[:, ::2, :8], (2, 3, 8), "q")
    with pytest.raises(TypeError):
        hip._rows(q.double(), (2, 5, 8), "q")
    with pytest.raises(ValueError, match="row stride"):
        hip.attention(q, k, torch.zeros(2, 5, 8), None, None, 4)
    with pytest.raises(ValueError, match="heads"):
        hip.attention(q, k, v, None, None, 3)
    with pytest.raises(TypeError):
        hip.attention(q, k, v, torch.zeros(2, 5), None, 4)
    with pytest.raises(ValueError):
        hip.attention(q, k, v, torch.zeros(2, 4, dtype=torch.bool), None, 4)
    with pytest.raises(ValueError):
        hip.attention(q, k, v, None, torch.zeros(5, 4), 4)


# --- the kernels' resources ---------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_attention_kernels_compile_without_scratch_stack_or_lds(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "attention.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "attention_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    # one instantiation of each of the three kernels per head width 1 .. 16 (Itanium mangling: ILi<D>E)
    wanted = [f"{name}ILi{d}E" for name in ("attention_forward_kernel", "attention_backward_q_kernel",
                                            "attention_backward_kv_kernel") for d in range(1, 17)]
    assert len(kernels) == len(wanted) == 48, sorted(kernels)
    for w in wanted:
        assert sum(w in name for name in kernels) == 1, w
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name


# --- the yardstick against torch ----------------------------------------------------------------------------------
def _masks(kind: str, b: int, tq: int, tk: int, g: torch.Generator):
    """``(key_padding_mask, attention_mask)``: random padding with batch row 0 fully padded, and a mask of ``kind``."""
    padding = torch.rand(b, tk, generator=g) < 0.4
    padding[0] = True
    if kind == "bool":
        return padding, torch.rand(tq, tk, generator=g) < 0.3
    if kind == "float":
        bias = torch.randn(tq, tk, generator=g, dtype=torch.float64)
        return padding, bias.masked_fill(torch.rand(tq, tk, generator=g) < 0.3, -math.inf)
    return padding, None


@pytest.mark.parametrize("kind", ["none", "bool", "float"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_reference_is_multihead_attention_s_core_in_float64(shape, kind):
    b, tq, tk, e, h = shape
    g = torch.Generator().manual_seed(b * 1000 + tq * 10 + len(kind))
    mha = nn.MultiheadAttention(e, h, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_bias.normal_(generator=g)
        mha.out_proj.bias.normal_(generator=g)
    padding, mask = _masks(kind, b, tq, tk, g)
    x = torch.randn(b, tq, e, generator=g, dtype=torch.float64)
    y = torch.randn(b, tk, e, generator=g, dtype=torch.float64)
    dout = torch.randn(b, tq, e, generator=g, dtype=torch.float64)
    results = []
    for route in ("torch", "reference"):
        xq, xkv = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        mha.zero_grad()
        if route == "torch":
            out, _ = mha(xq, xkv, xkv, key_padding_mask=padding, attn_mask=mask, need_weights=False)
        else:
            w, c = mha.in_proj_weight, mha.in_proj_bias
            q, kv = F.linear(xq, w[:e], c[:e]), F.linear(xkv, w[e:], c[e:])
            bias = mask if mask is None or mask.dtype != torch.bool else torch.zeros(tq, tk).masked_fill(mask, -math.inf)
            out = mha.out_proj(fused_attention.attention_reference(q, kv[..., :e], kv[..., e:], padding, bias, h))
        out.backward(dout)
        results.append([out.detach(), xq.grad, xkv.grad] + [p.grad.clone() for p in mha.parameters()])
    for got, want in zip(results[1], results[0]):
        assert not torch.isnan(want).any() and not torch.isnan(got).any()
        assert float((got - want).abs().max()) <= 1e-12
    # the fully padded batch row: out_proj's bias and nothing else, and no gradient into its inputs
    assert torch.equal(results[1][0][0], mha.out_proj.bias.detach().expand(tq, e))
    assert not results[1][1][0].any() and not results[1][2][0].any()


# --- the Python route ---------------------------------------------------------------------------------------------
def test_cpu_tensors_never_reach_a_wrapper(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("a kernel wrapper was called on CPU tensors")

    monkeypatch.setattr(hip, "attention", refuse)
    monkeypatch.setattr(hip, "attention_backward", refuse)
    monkeypatch.setattr(hip, "attention_supports", refuse)
    torch.manual_seed(0)
    layer = SelfAttention(8, num_heads=4, hidden_dim=16, skip_kind="residual")
    x = torch.randn(3, 5, 8, requires_grad=True)
    padding = torch.tensor([[True, True, False, False, False]]).expand(3, 5)
    assert fused_attention.multihead_attention(layer.attention, x, x, padding, None) is None
    out = layer(x, key_padding_mask=padding)
    out.sum().backward()
    assert out.shape == (3, 5, 8) and torch.isfinite(x.grad).all()
    assert all(p.grad is not None for p in layer.parameters())


def test_multihead_attention_declines_what_the_kernels_do_not_take(monkeypatch):
    """Each rule of the route on its own: the same call is taken (it reaches the in-projection) when the rule holds."""
    reached = []

    def core(*args):
        reached.append(args)
        raise RuntimeError("reached the kernels")

    monkeypatch.setattr(fused_attention, "self_attention_core", core)
    monkeypatch.setattr(fused_attention, "cross_attention_core", core)
    monkeypatch.setattr(fused_attention, "_on_device", lambda t: not t.is_meta)  # (host tensors stand in for HIP ones)
    monkeypatch.delenv("RL8_AMD_ATTENTION_KERNELS", raising=False)
    route = fused_attention.multihead_attention
    mha = nn.MultiheadAttention(8, 4, batch_first=True)
    x, y = torch.zeros(3, 5, 8), torch.zeros(3, 2, 8)
    pad_x, pad_y = torch.zeros(3, 5, dtype=torch.bool), torch.zeros(3, 2, dtype=torch.uint8)

    def taken(*args) -> bool:
        try:
            return route(*args) is not None
        except RuntimeError as err:
            assert "reached the kernels" in str(err)
            return True

    assert taken(mha, x, x, None, None) and taken(mha, x, x, pad_x, None) and taken(mha, x, y, pad_y, None)
    assert taken(mha, x, y, None, torch.zeros(5, 2, dtype=torch.bool))
    assert taken(mha, x, y, None, torch.zeros(5, 2))
    assert len(reached) == 5
    # inputs: host tensors, other dtypes, other ranks
    assert not taken(mha, torch.zeros(3, 5, 8, device="meta"), x, None, None)
    half = torch.zeros(3, 5, 8, dtype=torch.float16)
    assert not taken(mha, half, half, None, None)
    flat = torch.zeros(5, 8)
    assert not taken(mha, flat, flat, None, None)
    with monkeypatch.context() as m:
        m.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not taken(mha, x, x, None, None)
    # the module
    assert not taken(nn.MultiheadAttention(8, 4, batch_first=True, kdim=6, vdim=6), x, x, None, None)
    assert not taken(nn.MultiheadAttention(8, 4), x, x, None, None)
    assert not taken(nn.MultiheadAttention(8, 4, batch_first=True, add_bias_kv=True), x, x, None, None)
    assert not taken(nn.MultiheadAttention(8, 4, batch_first=True, add_zero_attn=True), x, x, None, None)
    dropping = nn.MultiheadAttention(8, 4, batch_first=True, dropout=0.1)
    assert not taken(dropping, x, x, None, None)
    assert taken(dropping.eval(), x, x, None, None)
    # key_padding_mask: float, wrong shape
    assert not taken(mha, x, x, torch.zeros(3, 5), None)
    assert not taken(mha, x, y, pad_x, None)
    # attention_mask: 3-D, wrong shape, float with a gradient, other float types
    assert not taken(mha, x, x, None, torch.zeros(12, 5, 5, dtype=torch.bool))
    assert not taken(mha, x, y, None, torch.zeros(5, 5, dtype=torch.bool))
    assert not taken(mha, x, x, None, torch.zeros(5, 5, requires_grad=True))
    assert not taken(mha, x, x, None, torch.zeros(5, 5, dtype=torch.float64))
    # the envelope: 65 cells, heads of 17 features
    long = torch.zeros(3, 65, 8)
    assert not taken(mha, long, long, None, None) and not taken(mha, x, long, None, None)
    wide = torch.zeros(3, 5, 34)
    assert not taken(nn.MultiheadAttention(34, 2, batch_first=True), wide, wide, None, None)
    # the switch, read on every call
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "0")
    assert not taken(mha, x, x, None, None)
    monkeypatch.setenv("RL8_AMD_ATTENTION_KERNELS", "1")
    assert taken(mha, x, x, None, None)


def test_attend_keeps_its_body_as_the_fallback(monkeypatch):
    """``_attend`` returns the fused result when there is one and calls the module itself otherwise."""
    mha = nn.MultiheadAttention(8, 4, batch_first=True)
    x = torch.randn(2, 5, 8)
    marker = torch.zeros(1)
    monkeypatch.setattr(fused_attention, "multihead_attention", lambda *a: marker)
    assert attention_module._attend(mha, x, x, None, None) is marker
    monkeypatch.setattr(fused_attention, "multihead_attention", lambda *a: None)
    want, _ = mha(x, x, x, need_weights=False)
    assert torch.equal(attention_module._attend(mha, x, x, None, None), want)
