"""The fused feedforward entries without a GPU: exported and bound, their envelope, their refusals before any launch,
the compiled kernels' resources, the torch yardstick ``feedforward_reference`` against the modules themselves in
float64, and the Python route's eligibility rules and fallback."""

import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from rl8_amd import hip
from rl8_amd.nn import SelfAttention, fused_feedforward
from rl8_amd.nn.functional import skip_connection
from rl8_amd.nn.modules.attention import _feedforward
from rl8_amd.nn.modules.skip import SequentialSkipConnection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INT_ENTRIES = ("rl8_feedforward_supports", "rl8_feedforward_limits", "rl8_feedforward_f32", "rl8_feedforward_backward_f32")
#: (B, T, F, H)
SHAPES = ((1, 1, 1, 1), (3, 5, 8, 64), (2, 7, 32, 256), (67, 1, 2, 65))


# --- the C entries ------------------------------------------------------------------------------------------------
def test_feedforward_entries_are_declared_exported_and_bound():
    lib = hip.load()
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        header = f.read()
    declared = [(name, re.search(rf"\bint {name}\((.*?)\);", header, re.S)) for name in INT_ENTRIES]
    declared.append(("rl8_feedforward_workspace_floats",
                     re.search(r"\bint64_t rl8_feedforward_workspace_floats\((.*?)\);", header, re.S)))
    for name, declaration in declared:
        assert declaration is not None, f"{name} is not declared"
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        params = re.sub(r"/\*.*?\*/", "", declaration.group(1))
        assert len(params.split(",")) == len(hip.SIGNATURES[name]), name
    assert hip.ABI_VERSION == 107  # (new entries only: no bump)
    for name in ("feedforward_supports", "feedforward", "feedforward_backward", "feedforward_limits",
                 "feedforward_workspace_floats"):
        assert callable(getattr(hip, name)), name


def test_feedforward_supports_at_the_envelope_s_edges():
    supports = hip.load().rl8_feedforward_supports
    assert supports(1, 1) == 1 and supports(32, 256) == 1 and supports(8, 64) == 1
    assert supports(33, 1) == 0 and supports(1, 257) == 0 and supports(33, 257) == 0
    for args in ((0, 1), (1, 0), (-1, 64), (8, -64), (0, 0), (33, -1)):
        assert supports(*args) == -2, args
    assert hip.feedforward_supports(32, 256) and not hip.feedforward_supports(33, 1)
    assert not hip.feedforward_supports(1, 257)
    with pytest.raises(ValueError):
        hip.feedforward_supports(0, 64)


def test_limits_and_workspace_size():
    limits = hip.feedforward_limits()
    assert limits.block == 256 and limits.grid_cap >= 256 and limits.wgrad_grid_cap >= 256 and limits.wgrad_rows >= 64
    assert hip.load().rl8_feedforward_limits(None) == -1
    floats = hip.feedforward_workspace_floats
    # one weight-gradient workgroup and one row-per-lane workgroup: at least one partial row of each kind
    assert floats(1, 8, 64) >= (2 * 8 * 64 + 64 + 8) + 2 * 8
    assert floats(1, 32, 256) >= (2 * 32 * 256 + 256 + 32) + 2 * 32
    # a function of the shape only that stops growing once both grids are capped
    assert floats(5, 8, 64) == floats(5, 8, 64) and floats(10 ** 6, 8, 64) > floats(1, 8, 64)
    assert floats(10 ** 9, 8, 64) == floats(10 ** 10, 8, 64) < 2 ** 26
    assert floats(10 ** 10, 32, 256) < 2 ** 26
    for args in ((0, 8, 64), (-1, 8, 64), (5, 0, 64), (5, 8, 0)):
        with pytest.raises(ValueError, match="out of range"):
            floats(*args)
    for args in ((5, 33, 64), (5, 8, 257)):
        with pytest.raises(ValueError, match="unsupported"):
            floats(*args)


def test_feedforward_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p = [4096 * (i + 1) for i in range(20)]  # (never dereferenced: every call fails its checks first)

    def forward(x=p[0], gamma=p[1], beta=p[2], w1=p[3], b1=p[4], w2=p[5], b2=p[6], rows=8, f=8, hidden=64, out=p[7]):
        return lib.rl8_feedforward_f32(x, gamma, beta, 1e-5, w1, b1, w2, b2, rows, f, hidden, 1, out, None)

    def backward(x=p[0], dout=p[8], gamma=p[1], beta=p[2], w1=p[3], b1=p[4], w2=p[5], rows=8, f=8, hidden=64, dx=p[9],
                 dgamma=p[10], dbeta=p[11], dw1=p[12], db1=p[13], dw2=p[14], db2=p[15], workspace=p[16]):
        return lib.rl8_feedforward_backward_f32(x, dout, gamma, beta, 1e-5, w1, b1, w2, rows, f, hidden, 1, dx, dgamma,
                                                dbeta, dw1, db1, dw2, db2, workspace, None)

    inputs = ("x", "gamma", "beta", "w1", "b1", "w2")
    outputs = ("dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")
    # RL8_ENULL: every input and the forward's output; the workspace as soon as one parameter gradient is wanted
    for name in inputs + ("b2", "out"):
        assert forward(**{name: None}) == -1, name
    for name in inputs + ("dout", "workspace"):
        assert backward(**{name: None}) == -1, name
    for name in outputs[1:]:
        only = {other: None for other in outputs if other != name}
        assert backward(workspace=None, **only) == -1, name
    # RL8_ESIZE
    for name in ("rows", "f", "hidden"):
        for bad in (0, -1):
            assert forward(**{name: bad}) == -2, name
            assert backward(**{name: bad}) == -2, name
    # RL8_EALIGN: any pointer off 4 bytes
    for name in inputs + ("b2", "out"):
        assert forward(**{name: p[17] + 2}) == -3, name
    for name in inputs + ("dout", "workspace") + outputs:
        assert backward(**{name: p[17] + 1}) == -3, name
    # RL8_ECONFIG: a shape outside rl8_feedforward_supports
    for shape in (dict(f=33), dict(hidden=257), dict(f=64, hidden=1024)):
        assert forward(**shape) == -4, shape
        assert backward(**shape) == -4, shape
    # no output wanted: nothing to do, and no workspace needed (checked after the arguments)
    nothing = {name: None for name in outputs}
    assert backward(workspace=None, **nothing) == 0
    assert backward(workspace=None, f=33, **nothing) == -4 and backward(workspace=None, x=None, **nothing) == -1


def _operands(f=8, hidden=64, shape=(3, 5)):
    return dict(x=torch.zeros(*shape, f), gamma=torch.ones(f), beta=torch.zeros(f), w1=torch.zeros(hidden, f),
                b1=torch.zeros(hidden), w2=torch.zeros(f, hidden), b2=torch.zeros(f))


def _forward(o, **changed):
    o = {**o, **changed}
    return hip.feedforward(o["x"], o["gamma"], o["beta"], 1e-5, o["w1"], o["b1"], o["w2"], o["b2"], True)


def _backward(o, dout, **changed):
    o = {**o, **changed}
    return hip.feedforward_backward(o["x"], dout, o["gamma"], o["beta"], 1e-5, o["w1"], o["b1"], o["w2"], True)


def test_wrappers_refuse_host_tensors():
    o = _operands()
    with pytest.raises(hip.HipExtensionError):
        _forward(o)
    with pytest.raises(hip.HipExtensionError):
        _backward(o, torch.zeros(3, 5, 8))


def test_wrappers_check_layouts_before_the_library_sees_them(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the operands were checked")

    monkeypatch.setattr(hip, "load", refuse)
    o = _operands()
    with pytest.raises(TypeError):
        _forward(o, x=o["x"].double())
    with pytest.raises(TypeError):
        _forward(o, w2=o["w2"].half())
    with pytest.raises(ValueError, match="contiguous"):
        _forward(o, x=torch.zeros(3, 8, 5).transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        _forward(o, w2=torch.zeros(64, 8).t())
    with pytest.raises(ValueError):
        _forward(o, x=torch.zeros(0, 8))
    for name, wrong in (("gamma", torch.ones(7)), ("beta", torch.zeros(8, 1)), ("w1", torch.zeros(64, 7)),
                        ("w1", torch.zeros(64 * 8)), ("b1", torch.zeros(63)), ("w2", torch.zeros(64, 8)),
                        ("b2", torch.zeros(9))):
        with pytest.raises(ValueError):
            _forward(o, **{name: wrong})
    with pytest.raises(ValueError):
        _backward(o, torch.zeros(3, 5, 7))
    with pytest.raises(ValueError):
        _backward(o, torch.zeros(5, 3, 8).transpose(0, 1))
    with pytest.raises(TypeError):
        _backward(o, torch.zeros(3, 5, 8, dtype=torch.float64))
    with pytest.raises(hip.HipExtensionError):  # (all layouts right: the device is what is left to refuse)
        _backward(o, torch.zeros(3, 5, 8))


# --- the kernels' resources ---------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_feedforward_kernels_compile_without_scratch_or_stack(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "feedforward.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "feedforward_kernels.hip")],
        check=True, capture_output=True, timeout=900,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    # per feature count 1 .. 32 (Itanium mangling: ILi<F>E...): the forward, the dx kernel with and without the
    # LayerNorm partials (...Lb1E / ...Lb0E), the weight-gradient kernel; and the one final sum
    per_lane = [f"feedforward_forward_kernelILi{f}ENS" for f in range(1, 33)]
    per_lane += [f"feedforward_backward_x_kernelILi{f}ENS0_4ReluELb{ln}E" for f in range(1, 33) for ln in (0, 1)]
    wgrad = [f"feedforward_wgrad_kernelILi{f}ENS" for f in range(1, 33)]
    assert len(kernels) == len(per_lane) + len(wgrad) + 1 == 129, sorted(kernels)
    for w in per_lane + wgrad + ["feedforward_sum_kernelE"]:
        assert sum(w in name for name in kernels) == 1, w
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        if any(w in name for w in per_lane):
            assert lds == 0, name
        else:
            assert lds <= 65536, name


# --- the yardstick against the modules ----------------------------------------------------------------------------
def _skip_block(kind, f, hidden, g, activation="relu", dropout=0.0) -> SequentialSkipConnection:
    skip = SequentialSkipConnection(f, kind=kind)
    skip.append(_feedforward(skip, hidden, activation, dropout))
    norm = skip._layers[1][0]
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5, generator=g)
        norm.bias.normal_(generator=g)
    return skip


@pytest.mark.parametrize("kind", ["residual", "cat", None])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feedforward_reference_is_the_modules_block_in_float64(shape, kind):
    b, t, f, hidden = shape
    g = torch.Generator().manual_seed(b * 1000 + t * 10 + f)
    skip = _skip_block(kind, f, hidden, g).double()
    block = skip._layers[1]
    norm, up, _, _, down = block
    y = torch.randn(b, t, f, generator=g, dtype=torch.float64)
    want_shape = (b, t, 2 * f if kind == "cat" else f)
    dout = torch.randn(want_shape, generator=g, dtype=torch.float64)
    results = []
    for route in ("modules", "reference"):
        x = y.clone().requires_grad_(True)
        block.zero_grad()
        if route == "modules":
            out = skip_connection(x, block(x), kind=kind)  # (what SequentialSkipConnection.forward does at an odd place)
        else:
            ff = fused_feedforward.feedforward_reference(x, norm.weight, norm.bias, norm.eps, up.weight, up.bias,
                                                         down.weight, down.bias, kind == "residual")
            out = torch.cat([x, ff], dim=-1) if kind == "cat" else ff
        assert tuple(out.shape) == want_shape
        out.backward(dout)
        results.append([out.detach(), x.grad] + [p.grad.clone() for p in block.parameters()])
    assert len(results[0]) == 8
    for got, want in zip(results[1], results[0]):
        assert torch.isfinite(want).all() and torch.isfinite(got).all()
        assert float((got - want).abs().max()) <= 1e-12


# --- the Python route ---------------------------------------------------------------------------------------------
def test_cpu_tensors_never_reach_a_wrapper(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("a kernel wrapper was called on CPU tensors")

    for name in ("feedforward", "feedforward_backward", "feedforward_supports"):
        monkeypatch.setattr(hip, name, refuse)
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "1")
    torch.manual_seed(0)
    layer = SelfAttention(8, num_heads=4, hidden_dim=16, skip_kind="residual")
    x = torch.randn(3, 5, 8, requires_grad=True)
    assert fused_feedforward.skip_feedforward(layer.skip_connection._layers[1], x, "residual") is None
    out = layer(x)
    out.sum().backward()
    assert out.shape == (3, 5, 8) and torch.isfinite(x.grad).all()
    assert all(p.grad is not None for p in layer.parameters())


def test_skip_feedforward_declines_what_the_kernels_do_not_take(monkeypatch):
    """Each rule of the route on its own: the same call is taken (it reaches the autograd node) when the rule holds."""
    reached = []

    class Reached:
        @staticmethod
        def apply(*args):
            reached.append(args)
            raise RuntimeError("reached the kernels")

    monkeypatch.setattr(fused_feedforward, "_FeedforwardBlock", Reached)
    monkeypatch.setattr(fused_feedforward, "_on_device", lambda t: not t.is_meta)  # (host tensors stand in for HIP ones)
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "1")
    g = torch.Generator().manual_seed(1)

    def block(f=8, hidden=64, **kwargs) -> nn.Sequential:
        return _skip_block("residual", f, hidden, g, **kwargs)._layers[1]

    def taken(module, y, kind="residual") -> bool:
        try:
            return fused_feedforward.skip_feedforward(module, y, kind) is not None
        except RuntimeError as err:
            assert "reached the kernels" in str(err)
            return True

    y = torch.zeros(3, 5, 8)
    plain = block()
    assert taken(plain, y) and taken(plain, y, "cat") and taken(plain, y, None) and taken(plain, torch.zeros(8))
    assert taken(block(32, 256), torch.zeros(2, 32)) and taken(block(1, 1), torch.zeros(4, 1))
    assert len(reached) == 6
    # what the node is given: the input, the six parameters, eps and whether the sum is the kernel's
    args = reached[0]
    assert args[0] is y and args[1] is plain[0].weight and args[6] is plain[4].bias and args[7:] == (plain[0].eps, True)
    assert reached[1][8] is False and reached[2][8] is False
    # the module
    assert not taken(block(activation="gelu"), y)
    dropping = block(dropout=0.1)
    assert not taken(dropping, y)
    assert taken(dropping.eval(), y)
    no_affine = block()
    no_affine[0] = nn.LayerNorm(8, elementwise_affine=False)
    assert not taken(no_affine, y)
    no_norm_bias = block()
    no_norm_bias[0] = nn.LayerNorm(8, bias=False)
    assert not taken(no_norm_bias, y)
    for place, layer in ((1, nn.Linear(8, 64, bias=False)), (4, nn.Linear(64, 8, bias=False))):
        unbiased = block()
        unbiased[place] = layer
        assert not taken(unbiased, y)
    assert not taken(nn.Sequential(*plain, nn.Identity()), y) and not taken(plain[1], y)
    assert not taken(nn.Sequential(plain[0], plain[1], plain[2], plain[3], nn.Linear(64, 4)), y)
    # the envelope
    assert not taken(block(33, 64), torch.zeros(3, 33)) and not taken(block(8, 257), y)
    # the input: other dtypes, host tensors, autocast, strided, empty, another width
    assert not taken(block().double(), y.double()) and not taken(plain, y.double()) and not taken(block().double(), y)
    assert not taken(plain, torch.zeros(3, 5, 8, device="meta"))
    with monkeypatch.context() as m:
        m.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not taken(plain, y)
    assert not taken(plain, torch.zeros(3, 8, 5).transpose(1, 2)) and not taken(plain, torch.zeros(3, 5, 16)[..., :8])
    assert not taken(plain, torch.zeros(0, 8)) and not taken(plain, torch.zeros(3, 5, 4))
    assert not taken(plain, y, "sum")
    # the switch, read on every call: the route is opt-in, so only "1" turns it on
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "0")
    assert not taken(plain, y)
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "1")
    assert taken(plain, y)
    monkeypatch.delenv("RL8_AMD_FEEDFORWARD_KERNELS")
    assert not taken(plain, y)


@pytest.mark.parametrize("kind", ["residual", "cat", None])
def test_sequential_skip_connection_keeps_its_body_as_the_fallback(monkeypatch, kind):
    """``forward`` returns the fused result for an appended module when there is one, and otherwise the bits it gave
    before the route existed."""
    g = torch.Generator().manual_seed(2)
    skip = _skip_block(kind, 8, 64, g)
    x, y = torch.randn(3, 5, 8, generator=g), torch.randn(3, 5, 8, generator=g)

    def old_body(x, y):
        y = skip_connection(x, y, kind=kind)
        for i, layer in enumerate(skip._layers):
            y = skip_connection(y, layer(y), kind=kind) if i % 2 else layer(y)
        return y

    want = old_body(x, y)
    calls = []
    monkeypatch.setattr(fused_feedforward, "skip_feedforward", lambda *a: calls.append(a))  # (returns None)
    assert torch.equal(skip(x, y), want)
    assert len(calls) == 1 and calls[0][0] is skip._layers[1] and calls[0][2] == kind  # (odd places only)
    marker = torch.randn(3, 5, 16 if kind == "cat" else 8, generator=g)
    monkeypatch.setattr(fused_feedforward, "skip_feedforward", lambda *a: marker)
    assert torch.equal(skip(x, y), skip._layers[2](marker))
