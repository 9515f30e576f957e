"""Wide-head towers (width 256 with heads of 9 to 128 outputs in all, rl8_amd/csrc/mlp_wide_out_kernels.hip) without a
GPU: the C entries declared, exported and bound; the structural classifier ``fused_mlp._wide_head_family`` beside
``_family`` and ``_wide_input_family``; and every argument check of the entries, against the cross-compiled library
with pointers that are never read."""

import os
import re

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import fused_mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rl8_mlp_wide_out_supports", "rl8_mlp_wide_out_lds_bytes", "rl8_mlp_wide_out_pack_floats",
           "rl8_mlp_wide_out_pack_f32", "rl8_mlp_wide_out_forward_f32", "rl8_mlp_wide_out_partial_floats",
           "rl8_mlp_wide_out_max_rows", "rl8_mlp_wide_out_backward_f32", "rl8_mlp_wide_out_workspace_bytes",
           "rl8_mlp_wide_out_wgrad_f32")
NULL, SIZE, ALIGN = -1, -2, -3
SWITCH = "RL8_AMD_WIDE_HEAD_TOWERS"


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
    for wrapper in ("mlp_wide_out_supports", "mlp_wide_out_pack_w1", "mlp_wide_out_pack_w3", "mlp_wide_out_forward",
                    "mlp_wide_out_backward", "mlp_wide_out_wgrad"):
        assert callable(getattr(hip, wrapper)), wrapper
    assert "mlp_wide_out_kernels.hip" in open(os.path.join(ROOT, "rl8_amd", "csrc", "Makefile")).read()


def test_the_supports_table_at_its_edges():
    lib = hip.load()
    for d, n, ok in ((1, 9, 1), (128, 128, 1), (4, 100, 1), (16, 9, 1), (17, 9, 1), (24, 12, 1),
                     (4, 8, 0), (4, 129, 0), (129, 9, 0), (0, 9, 0), (-1, 9, 0), (4, 0, 0)):
        assert lib.rl8_mlp_wide_out_supports(d, n) == ok, (d, n)
        assert hip.mlp_wide_out_supports(d, n) is bool(ok)
    # the envelopes of the other towers have not moved
    assert hip.MLP_MAX_IN == 16 and hip.MLP_MAX_OUT == 8
    assert lib.rl8_mlp_wide_in_supports(24, 9) == 0 and lib.rl8_mlp_wide_in_supports(16, 2) == 0
    fake = 4096
    assert lib.rl8_mlp_wide_in_wgrad_f32(fake, fake, 10, 16, fake, fake, 0, None) == SIZE  # (still refuses d_in <= 16)


def test_helpers_follow_the_envelope():
    lib = hip.load()
    for n in (8, 129, 0, -1):
        assert lib.rl8_mlp_wide_out_partial_floats(n) == SIZE, n
        assert lib.rl8_mlp_wide_out_pack_floats(1, n) == SIZE and lib.rl8_mlp_wide_out_pack_floats(2, n) == SIZE, n
    for d in (0, 129, -1):
        assert lib.rl8_mlp_wide_out_pack_floats(0, d) == SIZE and lib.rl8_mlp_wide_out_workspace_bytes(d) == SIZE, d
        assert lib.rl8_mlp_wide_out_lds_bytes(0, d) == SIZE
    assert lib.rl8_mlp_wide_out_pack_floats(3, 24) == SIZE and lib.rl8_mlp_wide_out_pack_floats(-1, 24) == SIZE
    for d in (1, 8, 9, 24, 128):
        assert lib.rl8_mlp_wide_out_pack_floats(0, d) == 256 * 8 * ((d + 7) // 8)
        assert lib.rl8_mlp_wide_out_workspace_bytes(d) == 256 * 256 * d * 4
    for n in (9, 32, 33, 100, 128):
        assert lib.rl8_mlp_wide_out_pack_floats(1, n) == 32 * ((n + 31) // 32) * 256  # at most 128 KiB
        assert lib.rl8_mlp_wide_out_pack_floats(2, n) == 256 * 8 * ((n + 7) // 8)
        assert lib.rl8_mlp_wide_out_partial_floats(n) == 512 + n
    assert lib.rl8_mlp_wide_out_max_rows() == 512
    tile = 64 * 257 * 4
    assert lib.rl8_mlp_wide_out_lds_bytes(0, 24) == tile and lib.rl8_mlp_wide_out_lds_bytes(1, 100) == tile
    assert 2 * tile <= 160 * 1024
    for c, want in ((1, 98304), (32, 98304), (33, 106496), (96, 114688), (128, 122880)):
        assert lib.rl8_mlp_wide_out_lds_bytes(2, c) == want
    assert lib.rl8_mlp_wide_out_lds_bytes(3, 24) == SIZE and lib.rl8_mlp_wide_out_lds_bytes(-1, 24) == SIZE


def test_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    fake = 4096  # (never dereferenced: every call below fails its checks first)
    rows = hip.C.c_int(0)
    out = hip.C.byref(rows)

    def forward(x=fake, m=10, d_in=24, w1p=fake, b1=fake, w2p=fake, b2=fake, w3p=fake, b3=fake, n_out=12, o=fake, h1=None,
                h2=None):
        return lib.rl8_mlp_wide_out_forward_f32(x, m, d_in, w1p, b1, w2p, b2, w3p, b3, n_out, o, h1, h2, None)

    def backward(h1=fake, h2=fake, dout=fake, m=10, w2t=fake, w3t=fake, n_out=12, dz1=fake, dz2=fake, partials=fake,
                 rows_out=out):
        return lib.rl8_mlp_wide_out_backward_f32(h1, h2, dout, m, w2t, w3t, n_out, dz1, dz2, partials, rows_out, None)

    def wgrad(a=fake, b=fake, m=10, c=24, ws=fake, o=fake, accumulate=0, transpose=0):
        return lib.rl8_mlp_wide_out_wgrad_f32(a, b, m, c, ws, o, accumulate, transpose, None)

    def pack(w=fake, matrix=1, n=12, packed=fake):
        return lib.rl8_mlp_wide_out_pack_f32(w, matrix, n, packed, None)

    # NULL pointers
    for name in ("x", "w1p", "b1", "w2p", "b2", "w3p", "b3", "o"):
        assert forward(**{name: None}) == NULL, name
    assert forward(h1=fake) == NULL and forward(h2=fake) == NULL  # (both or neither)
    for name in ("h1", "h2", "dout", "w2t", "w3t", "dz1", "dz2", "partials", "rows_out"):
        assert backward(**{name: None}) == NULL, name
    for name in ("a", "b", "ws", "o"):
        assert wgrad(**{name: None}) == NULL, name
    assert pack(w=None) == NULL and pack(packed=None) == NULL
    # sizes / widths
    for bad in ({"m": 0}, {"m": -5}, {"d_in": 0}, {"d_in": 129}, {"n_out": 8}, {"n_out": 129}, {"n_out": 0}):
        assert forward(**bad) == SIZE, bad
    for bad in ({"m": 0}, {"n_out": 8}, {"n_out": 129}):
        assert backward(**bad) == SIZE, bad
    for bad in ({"m": 0}, {"c": 0}, {"c": 129}):
        assert wgrad(**bad) == SIZE, bad
    for bad in ({"matrix": 0, "n": 0}, {"matrix": 0, "n": 129}, {"matrix": 1, "n": 8}, {"matrix": 2, "n": 129},
                {"matrix": 3}, {"matrix": -1}):
        assert pack(**bad) == SIZE, bad
    # alignment: 16 bytes for what the kernels address through descriptors or direct-to-LDS loads, 4 for the rest
    for name in ("w1p", "w2p", "w3p"):
        assert forward(**{name: fake + 4}) == ALIGN, name
    assert forward(h1=fake + 4, h2=fake) == ALIGN and forward(h1=fake, h2=fake + 8) == ALIGN
    for name in ("x", "b1", "b2", "b3", "o"):
        assert forward(**{name: fake + 2}) == ALIGN, name
    for name in ("h1", "h2", "w2t", "w3t", "dz1", "dz2"):
        assert backward(**{name: fake + 4}) == ALIGN, name
    for name in ("dout", "partials"):
        assert backward(**{name: fake + 1}) == ALIGN, name
    assert wgrad(a=fake + 4) == ALIGN
    for name in ("b", "ws", "o"):
        assert wgrad(**{name: fake + 2}) == ALIGN, name
    assert pack(w=fake + 2) == ALIGN and pack(packed=fake + 4) == ALIGN
    assert rows.value == 0  # (no refused call reported partial rows)


def _tower(d_in, width=256, *, act1=nn.ReLU, act2=nn.ReLU, bias1=True, bias2=True, outs=(12,), head_bias=True):
    trunk = nn.Sequential(nn.Sequential(nn.Linear(d_in, width, bias=bias1), act1(), nn.Linear(width, width, bias=bias2)),
                          act2())
    return trunk, [nn.Linear(width, n, bias=head_bias) for n in outs]


@pytest.mark.parametrize("d_in", [1, 4, 16, 17, 128])
@pytest.mark.parametrize("outs", [(9,), (6, 6), (8, 1), (100,), (128,), (64, 64)])
def test_the_classifier_accepts_every_edge_of_the_envelope(d_in, outs):
    trunk, heads = _tower(d_in, outs=outs)
    found = fused_mlp._wide_head_family(trunk, heads)
    assert found is not None and found[0] is trunk[0][0] and found[1] is trunk[0][2]
    assert fused_mlp._family(trunk, heads) is None and fused_mlp._wide_input_family(trunk, heads) is None


@pytest.mark.parametrize("case", ["width_64", "width_128", "width_512", "tanh_inner", "tanh_outer", "no_bias_1",
                                  "no_bias_2", "no_head_bias", "head_reads_128", "eight_outputs", "outputs_129",
                                  "d_in_129", "no_heads", "three_layers"])
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
    elif case == "eight_outputs":
        kw["outs"] = (4, 4)
    elif case == "outputs_129":
        kw["outs"] = (64, 65)
    elif case == "no_heads":
        kw["outs"] = ()
    trunk, heads = _tower(d_in, width, **kw)
    if case == "head_reads_128":
        heads = [nn.Linear(256, 6), nn.Linear(128, 6)]
    elif case == "three_layers":
        trunk[0].append(nn.ReLU())
        trunk[0].append(nn.Linear(256, 256))
    assert fused_mlp._wide_head_family(trunk, heads) is None
    if case == "eight_outputs":  # (8 outputs behind 24 inputs is the wide-input family's)
        assert fused_mlp._wide_input_family(trunk, heads) is not None
    else:
        assert fused_mlp._wide_input_family(trunk, heads) is None
    assert fused_mlp._family(trunk, heads) is None


@pytest.mark.parametrize("d_in,outs", [(4, (2,)), (4, (4, 4)), (16, (8,)), (1, (1,)), (24, (8,)), (128, (1,)), (17, (3, 3))])
def test_towers_of_at_most_8_outputs_are_classified_as_before(d_in, outs):
    trunk, heads = _tower(d_in, outs=outs)
    assert fused_mlp._wide_head_family(trunk, heads) is None
    if d_in <= hip.MLP_MAX_IN:
        found = fused_mlp._family(trunk, heads)
        assert found is not None and found[0] == "wide" and found[1] is trunk[0][0] and found[2] is trunk[0][2]
        assert fused_mlp._wide_input_family(trunk, heads) is None
    else:
        assert fused_mlp._family(trunk, heads) is None
        found = fused_mlp._wide_input_family(trunk, heads)
        assert found is not None and found[0] is trunk[0][0] and found[1] is trunk[0][2]


def test_the_upper_limit_is_asked_of_the_library_once_per_width(monkeypatch):
    asked = []
    monkeypatch.setattr(hip, "mlp_wide_out_supports", lambda d, n: asked.append((d, n)) or n <= 40)
    fused_mlp._wide_head_supported.cache_clear()
    try:
        for _ in range(3):
            assert fused_mlp._wide_head_family(*_tower(4, outs=(40,))) is not None
            assert fused_mlp._wide_head_family(*_tower(4, outs=(41,))) is None
        assert sorted(asked) == [(4, 40), (4, 41)]
        assert fused_mlp._wide_head_family(*_tower(4, outs=(8,))) is None and len(asked) == 2  # (below: not asked)
    finally:
        fused_mlp._wide_head_supported.cache_clear()


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert fused_mlp.wide_head_towers_on()
    monkeypatch.setenv(SWITCH, "0")
    assert not fused_mlp.wide_head_towers_on()
    assert fused_mlp.wide_input_towers_on()  # (each family has its own switch)
    monkeypatch.setenv(SWITCH, "1")
    assert fused_mlp.wide_head_towers_on()


def test_tower_forward_declines_a_cpu_tensor(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    trunk, heads = _tower(4, outs=(18,))
    assert fused_mlp._wide_head_family(trunk, heads) is not None
    assert fused_mlp.tower_forward(trunk, heads, torch.randn(8, 4)) is None


def test_no_new_autograd_node():
    nodes = [name for name, obj in vars(fused_mlp).items()
             if isinstance(obj, type) and issubclass(obj, torch.autograd.Function)]
    assert "_WideInputTower" in nodes and not any("head" in n.lower() and "wide" in n.lower() for n in nodes), nodes
