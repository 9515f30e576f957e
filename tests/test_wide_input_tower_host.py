"""Wide-input towers (width 256 behind 17 to 128 inputs, rl8_amd/csrc/mlp_wide_in_kernels.hip) without a GPU: the C
entries declared, exported and bound; the structural classifier ``fused_mlp._wide_input_family`` beside ``_family``;
and every argument check of the entries, against the cross-compiled library with pointers that are never read."""

import os
import re

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import fused_mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rl8_mlp_wide_in_supports", "rl8_mlp_wide_in_lds_bytes", "rl8_mlp_wide_in_pack_floats",
           "rl8_mlp_wide_in_pack_w1_f32", "rl8_mlp_wide_in_forward_f32", "rl8_mlp_wide_in_partial_floats",
           "rl8_mlp_wide_in_max_rows", "rl8_mlp_wide_in_backward_f32", "rl8_mlp_wide_in_workspace_bytes",
           "rl8_mlp_wide_in_wgrad_f32")
NULL, SIZE, ALIGN = -1, -2, -3


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "rl8_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hip.load()
    for name in ENTRIES:
        declared = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, re.S)
        assert declared, f"include/rl8_amd.h does not declare {name}"
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        params = declared.group(2).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(hip.SIGNATURES[name]), name
        assert getattr(lib, name).restype is (hip.C.c_int64 if declared.group(1) == "int64_t" else hip.C.c_int), name
    assert hip.ABI_VERSION == 107 and re.search(r"#define RL8_ABI_VERSION 107\b", text)
    for wrapper in ("mlp_wide_in_supports", "mlp_wide_in_pack_w1", "mlp_wide_in_forward", "mlp_wide_in_backward",
                    "mlp_wide_in_wgrad"):
        assert callable(getattr(hip, wrapper)), wrapper


def test_the_envelopes_of_the_other_towers_have_not_moved():
    lib = hip.load()
    assert hip.MLP_MAX_IN == 16 and hip.MLP_MAX_OUT == 8
    assert lib.rl8_mlp_forward_f16_supports(17, 1) == 0 and lib.rl8_mlp_narrow_supports(64, 17, 2) == 0
    fake = 4096
    assert lib.rl8_mlp_tower_forward_f32(fake, 10, 17, *[fake] * 6, 2, fake, None, None, None) == SIZE


def _tower(d_in, width=256, *, act1=nn.ReLU, act2=nn.ReLU, bias1=True, bias2=True, outs=(2,), head_bias=True):
    trunk = nn.Sequential(nn.Sequential(nn.Linear(d_in, width, bias=bias1), act1(), nn.Linear(width, width, bias=bias2)),
                          act2())
    return trunk, [nn.Linear(width, n, bias=head_bias) for n in outs]


@pytest.mark.parametrize("d_in", [17, 24, 128])
@pytest.mark.parametrize("outs", [(2,), (3, 3), (8,), (1,)])
def test_the_classifier_accepts_the_default_structure(d_in, outs):
    trunk, heads = _tower(d_in, outs=outs)
    found = fused_mlp._wide_input_family(trunk, heads)
    assert found is not None and found[0] is trunk[0][0] and found[1] is trunk[0][2]
    assert fused_mlp._family(trunk, heads) is None


@pytest.mark.parametrize("case", ["d_in_16", "d_in_129", "width_64", "width_128", "width_512", "tanh_inner", "tanh_outer",
                                  "no_bias_1", "no_bias_2", "no_head_bias", "nine_outputs", "no_heads", "mixed_width",
                                  "three_layers"])
def test_the_classifier_refuses_everything_else(case):
    kw: dict = {}
    d_in, width = 24, 256
    if case.startswith("d_in_"):
        d_in = int(case[5:])
    elif case.startswith("width_"):
        width = int(case[6:])
    elif case == "tanh_inner":
        kw["act1"] = nn.Tanh
    elif case == "tanh_outer":
        kw["act2"] = nn.Tanh
    elif case == "no_bias_1":
        kw["bias1"] = False
    elif case == "no_bias_2":
        kw["bias2"] = False
    elif case == "no_head_bias":
        kw["head_bias"] = False
    elif case == "nine_outputs":
        kw["outs"] = (4, 5)
    elif case == "no_heads":
        kw["outs"] = ()
    trunk, heads = _tower(d_in, width, **kw)
    if case == "mixed_width":
        trunk[0][2] = nn.Linear(256, 128)
        heads = [nn.Linear(128, 2)]
    elif case == "three_layers":
        trunk[0].append(nn.ReLU())
        trunk[0].append(nn.Linear(256, 256))
    assert fused_mlp._wide_input_family(trunk, heads) is None
    if case != "d_in_16":  # (16 inputs at width 256 is _family's own "wide")
        assert fused_mlp._family(trunk, heads) is None
    else:
        assert fused_mlp._family(trunk, heads)[0] == "wide"


def test_the_upper_limit_is_asked_of_the_library_once_per_width(monkeypatch):
    asked = []
    monkeypatch.setattr(hip, "mlp_wide_in_supports", lambda d, n: asked.append((d, n)) or d <= 40)
    fused_mlp._wide_input_supported.cache_clear()
    try:
        for _ in range(3):
            assert fused_mlp._wide_input_family(*_tower(40)) is not None
            assert fused_mlp._wide_input_family(*_tower(41)) is None
        assert sorted(asked) == [(40, 2), (41, 2)]
        assert fused_mlp._wide_input_family(*_tower(16)) is None and len(asked) == 2  # (below the family: not asked)
    finally:
        fused_mlp._wide_input_supported.cache_clear()


def test_tower_forward_declines_a_cpu_tensor(monkeypatch):
    monkeypatch.setattr(hip, "mlp_wide_in_supports", lambda d, n: True)
    fused_mlp._wide_input_supported.cache_clear()
    try:
        trunk, heads = _tower(24)
        assert fused_mlp.tower_forward(trunk, heads, torch.randn(8, 24)) is None
    finally:
        fused_mlp._wide_input_supported.cache_clear()


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("RL8_AMD_WIDE_INPUT_TOWERS", raising=False)
    assert fused_mlp.wide_input_towers_on()
    monkeypatch.setenv("RL8_AMD_WIDE_INPUT_TOWERS", "0")
    assert not fused_mlp.wide_input_towers_on()
    monkeypatch.setenv("RL8_AMD_WIDE_INPUT_TOWERS", "1")
    assert fused_mlp.wide_input_towers_on()
    assert fused_mlp.WIDE_INPUT_SEGMENT_ROWS == 1 << 20  # two [rows, 256] fp32 scratch buffers: 2 GiB together


def test_helpers_follow_the_envelope():
    lib = hip.load()
    for d, n, ok in ((17, 1, 1), (24, 4, 1), (128, 8, 1), (16, 1, 0), (129, 1, 0), (24, 0, 0), (24, 9, 0), (0, 1, 0)):
        assert lib.rl8_mlp_wide_in_supports(d, n) == ok, (d, n)
    for d in (16, 129, 0, -1):
        assert lib.rl8_mlp_wide_in_pack_floats(d) == SIZE and lib.rl8_mlp_wide_in_workspace_bytes(d) == SIZE, d
        assert lib.rl8_mlp_wide_in_lds_bytes(0, d) == SIZE
    for d in (17, 24, 25, 128):
        assert lib.rl8_mlp_wide_in_pack_floats(d) == 256 * 8 * ((d + 7) // 8)
        assert lib.rl8_mlp_wide_in_workspace_bytes(d) == 256 * 256 * d * 4
    assert lib.rl8_mlp_wide_in_partial_floats(0) == SIZE and lib.rl8_mlp_wide_in_partial_floats(9) == SIZE
    assert lib.rl8_mlp_wide_in_partial_floats(3) == 512 + 3 * 256 + 3
    assert lib.rl8_mlp_wide_in_max_rows() == 512
    assert lib.rl8_mlp_wide_in_lds_bytes(3, 24) == SIZE and lib.rl8_mlp_wide_in_lds_bytes(-1, 24) == SIZE


def test_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    rows = hip.C.c_int(0)
    out = hip.C.byref(rows)

    def forward(x=fake, m=10, d_in=24, w1p=fake, b1=fake, w2p=fake, b2=fake, w3=fake, b3=fake, n_out=2, o=fake, h1=None,
                h2=None):
        return lib.rl8_mlp_wide_in_forward_f32(x, m, d_in, w1p, b1, w2p, b2, w3, b3, n_out, o, h1, h2, None)

    def backward(h1=fake, h2=fake, dout=fake, m=10, w2t=fake, w3=fake, n_out=2, dz1=fake, dz2=fake, partials=fake,
                 rows_out=out):
        return lib.rl8_mlp_wide_in_backward_f32(h1, h2, dout, m, w2t, w3, n_out, dz1, dz2, partials, rows_out, None)

    def wgrad(dz1=fake, x=fake, m=10, d_in=24, ws=fake, dw1=fake, accumulate=0):
        return lib.rl8_mlp_wide_in_wgrad_f32(dz1, x, m, d_in, ws, dw1, accumulate, None)

    def pack(w1=fake, d_in=24, packed=fake):
        return lib.rl8_mlp_wide_in_pack_w1_f32(w1, d_in, packed, None)

    # NULL pointers
    for name in ("x", "w1p", "b1", "w2p", "b2", "w3", "b3", "o"):
        assert forward(**{name: None}) == NULL, name
    assert forward(h1=fake) == NULL and forward(h2=fake) == NULL  # (both or neither)
    for name in ("h1", "h2", "dout", "w2t", "w3", "dz1", "dz2", "partials", "rows_out"):
        assert backward(**{name: None}) == NULL, name
    for name in ("dz1", "x", "ws", "dw1"):
        assert wgrad(**{name: None}) == NULL, name
    assert pack(w1=None) == NULL and pack(packed=None) == NULL
    # sizes / widths
    for bad in ({"m": 0}, {"m": -5}, {"d_in": 16}, {"d_in": 129}, {"n_out": 0}, {"n_out": 9}):
        assert forward(**bad) == SIZE, bad
    for bad in ({"m": 0}, {"n_out": 0}, {"n_out": 9}):
        assert backward(**bad) == SIZE, bad
    for bad in ({"m": 0}, {"d_in": 16}, {"d_in": 129}):
        assert wgrad(**bad) == SIZE, bad
    assert pack(d_in=16) == SIZE and pack(d_in=129) == SIZE
    # alignment: 16 bytes for what the kernels address through descriptors or direct-to-LDS loads, 4 for the rest
    for name in ("w1p", "w2p"):
        assert forward(**{name: fake + 4}) == ALIGN, name
    assert forward(h1=fake + 4, h2=fake) == ALIGN and forward(h1=fake, h2=fake + 8) == ALIGN
    for name in ("x", "b1", "b2", "w3", "b3", "o"):
        assert forward(**{name: fake + 2}) == ALIGN, name
    for name in ("h1", "h2", "w2t", "dz1", "dz2"):
        assert backward(**{name: fake + 4}) == ALIGN, name
    for name in ("dout", "w3", "partials"):
        assert backward(**{name: fake + 1}) == ALIGN, name
    assert wgrad(dz1=fake + 4) == ALIGN
    for name in ("x", "ws", "dw1"):
        assert wgrad(**{name: fake + 2}) == ALIGN, name
    assert pack(w1=fake + 2) == ALIGN and pack(packed=fake + 4) == ALIGN
    assert rows.value == 0  # (no refused call reported partial rows)
