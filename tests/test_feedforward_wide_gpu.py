"""The MFMA feedforward kernels (``rl8_feedforward_wide_f32`` / ``rl8_feedforward_wide_backward_f32``) on the GPU, and
the modules that reach them with ``RL8_AMD_WIDE_FEEDFORWARD=1``.

Yardsticks, bars and helpers are those of ``tests/test_feedforward_kernels_gpu.py`` (its docstring has the two bars and
how a case is made tie-free): each case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor before it asserts
(measured on an MI355X: out 0.82 .. 1.28, dx 0.81 .. 1.38, dgamma 0.56 .. 1.41, dbeta 0.33 .. 1.32, dw1 0.10 .. 1.22,
db1 0.52 .. 1.32, dw2 0.12 .. 1.76, db2 0.09 .. 1.27 at R >= 15; the parameter gradients 5.6 .. 8.8 at R = 1, where the
floor carries the bar).
"""

import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402
from rl8_amd.nn import SelfAttention  # noqa: E402

from .test_feedforward_kernels_gpu import (DEV, EPS, NAMES, assert_guards, gen, guarded, launches, parameters,  # noqa: E402
                                           placed, pre_activations, ptr, stream, tie_free, window_padding, with_grads)

SWITCH = "RL8_AMD_WIDE_FEEDFORWARD"
NUM_CASES = 12
CORNER = 7  # (its 17 tiles are more than its 16 slices: the weight-gradient workgroups stride)


def cases() -> list[tuple[int, int, int, bool, float, int]]:
    """(R, F, H, residual, offset added to x, elements every base pointer sits into its allocation).  The sizes that
    depend on the kernels' launch shapes take them from the library."""
    lim = hip.feedforward_wide_limits()
    tile, chunk = lim.tile_rows, lim.chunk
    stride = lim.grid_cap * tile + 77  # (beyond one pass of all three kernels: the weight-gradient kernel's is less)
    assert stride > lim.wgrad_grid_cap * tile
    return [
        (1, 33, 1, True, 0.0, 0), (15, 40, 15, False, 0.0, 0), (17, 64, 17, True, 0.0, 0),
        (tile - 1, 100, chunk - 1, False, 0.0, 0), (tile, 64, chunk, True, 0.0, 0),
        (tile + 1, 128, chunk + 1, False, 0.0, 0),
        (2051, 64, 128, True, 30.0, 0),  # rows of mean 30: the two-pass variance
        (1027, 128, 512, True, 0.0, 0),  # the envelope's corner
        (67, 100, 128, False, 0.0, 1),
        (4099, 40, 64, False, 0.0, 0),
        (259, 33, 512, True, 0.0, 0),
        (stride, 33, 1, True, 0.0, 0),
    ]


@functools.lru_cache(maxsize=None)
def case(index: int) -> dict:
    """Inputs (CPU, float32), ``ref64`` and ``torch32`` of ``cases()[index]``: computed once, shared, never modified."""
    r, f, h, residual, offset, shift = cases()[index]
    g = gen(501 + index)
    p = parameters(f, h, 601 + index)
    x = tie_free(torch.randn(r, f, generator=g) + offset, p, g, offset)
    assert bool((pre_activations(x, p) > 0).any()), "every gate is closed: the case would compare zeros"
    dout = torch.randn(r, f, generator=g)
    ref64 = with_grads(x.double(), {k: v.double() for k, v in p.items()}, dout.double(), residual)
    torch32 = with_grads(x.to(DEV), {k: v.to(DEV) for k, v in p.items()}, dout.to(DEV), residual)
    return dict(x=x, dout=dout, p=p, residual=residual, shift=shift, ref64=ref64,
                torch32=tuple(t.double().cpu() for t in torch32))


def run_case(c: dict, *, want_dx=True, want_params=True):
    """The raw wide entries on device copies: ``(out, dx, dgamma, dbeta, dw1, db1, dw2, db2)``, a piece that was not
    asked for ``None``; every output, and the workspace, between guard words that are checked."""
    x, p, shift = c["x"], c["p"], c["shift"]
    (r, f), h, lib = x.shape, p["w1"].shape[0], hip.load()
    xd, gd = placed(x, shift), placed(c["dout"], shift)
    d = {k: placed(v, shift) for k, v in p.items()}
    weights = [ptr(d[k]) for k in ("gamma", "beta")] + [EPS] + [ptr(d[k]) for k in ("w1", "b1", "w2")]
    obuf, out = guarded(r * f, shift)
    assert lib.rl8_feedforward_wide_f32(ptr(xd), *weights, ptr(d["b2"]), r, f, h, int(c["residual"]), ptr(out),
                                        stream()) == 0
    shapes = dict(dx=(r, f), dgamma=(f,), dbeta=(f,), dw1=(h, f), db1=(h,), dw2=(f, h), db2=(f,))
    wanted = {name: (want_dx if name == "dx" else want_params) for name in shapes}
    grads = {name: guarded(math.prod(shape), shift) for name, shape in shapes.items()}
    wbuf, workspace = guarded(hip.feedforward_wide_workspace_floats(r, f, h), shift)
    assert lib.rl8_feedforward_wide_backward_f32(
        ptr(xd), ptr(gd), *weights, r, f, h, int(c["residual"]),
        *(ptr(grads[n][1]) if wanted[n] else None for n in shapes), ptr(workspace) if want_params else None,
        stream()) == 0
    results = [out.view(r, f)]
    for name, (buf, inner) in [("out", (obuf, out)), ("workspace", (wbuf, workspace))] + list(grads.items()):
        assert_guards(buf, inner, name)
        if not wanted.get(name, want_params if name == "workspace" else True):
            assert bool((buf == -77).all()), f"{name}: written though it was not asked for"
        elif name != "workspace":
            assert not bool((inner == -77).any()), f"{name}: an element was not written"
        if name in shapes:
            results.append(inner.view(shapes[name]) if wanted[name] else None)
    return tuple(results)


@pytest.mark.parametrize("index", range(NUM_CASES))
def test_wide_kernels_against_float64_within_three_times_torch_s_own_error(index):
    assert len(cases()) == NUM_CASES
    c = case(index)
    first = run_case(c)
    got = [t.double().cpu() for t in first]
    figures = []
    for name, g, want, t32 in zip(NAMES, got, c["ref64"], c["torch32"]):
        assert g.shape == want.shape, name
        assert not torch.isnan(g).any() and not torch.isnan(t32).any(), name
        figures.append((name, float((g - want).abs().max()), float((t32 - want).abs().max())))
    print(f"{cases()[index]}: " + "  ".join(f"{n} {err:.2e} / {te:.2e} = {err / te if te else math.nan:.2f}"
                                            for n, err, te in figures))
    for (name, _, torch_err), g, want in zip(figures, got, c["ref64"]):
        floor = 1e-6 + 1e-5 * want.abs() if name == "out" else 2e-5 * float(want.abs().max()) + 1e-9
        excess = (g - want).abs() - (3 * torch_err + floor)
        assert bool((excess <= 0).all()), (name, float(excess.max()))
    for name, a, b in zip(NAMES, first, run_case(c)):  # a second run: the same bits
        assert torch.equal(a, b), name
    if index == CORNER:  # an output that is not wanted is not formed (run_case checks that it stays untouched)
        only_dx, only_params = run_case(c, want_params=False), run_case(c, want_dx=False)
        assert torch.equal(only_dx[1], first[1]) and all(t is None for t in only_dx[2:]) and only_params[1] is None
        for name, a, b in zip(NAMES[2:], only_params[2:], first[2:]):
            assert torch.equal(a, b), name
        run_case(c, want_dx=False, want_params=False)


# --- the modules through the public route -------------------------------------------------------------------------
def module_run(monkeypatch, module, x, padding, dout, switch):
    """``([output, input gradient, parameter gradients ...], feedforward launches)`` of one forward + backward."""
    monkeypatch.setenv(SWITCH, switch)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        x = x.clone().requires_grad_(True)
        module.zero_grad()
        out = module(x, key_padding_mask=padding)
        out.backward(dout)
        ran = launches()
    finally:
        hip.timer.enabled = False
    return [out.detach(), x.grad] + [p.grad.clone() for p in module.parameters()], ran


@pytest.mark.parametrize("kind", ["residual", "cat"])
def test_modules_on_the_wide_kernels_against_float64(monkeypatch, kind):
    torch.manual_seed(9)
    b, t, e = 67, 33, 64
    layer = (SelfAttention(e, num_heads=2, hidden_dim=128, skip_kind="residual") if kind == "residual"
             else SelfAttention(e, num_heads=2))  # (the default "cat" skip: the sum outside the launch, a torch.cat behind)
    x, padding = torch.randn(b, t, e, generator=gen(91)), window_padding(b, t)
    reference = copy.deepcopy(layer).double()
    with torch.no_grad():
        dout = torch.randn(reference(x.double(), key_padding_mask=padding.cpu()).shape, generator=gen(92))
    want, _ = module_run(monkeypatch, reference, x.double(), padding.cpu(), dout.double(), "0")
    layer = layer.to(DEV)
    off, ran_off = module_run(monkeypatch, layer, x.to(DEV), padding, dout.to(DEV), "0")
    on, ran_on = module_run(monkeypatch, layer, x.to(DEV), padding, dout.to(DEV), "1")
    assert ran_on == {"feedforward_wide": 1, "feedforward_wide_backward": 1} and ran_off == {}
    names = ["out", "input"] + [n for n, _ in layer.named_parameters()]
    for name, got, base, ref in zip(names, on, off, want):
        diff, off_err = (got.double().cpu() - ref).abs(), float((base.double().cpu() - ref).abs().max())
        print(f"{name}: on {float(diff.max()):.2e}, off {off_err:.2e}")
        floor = 1e-6 + 1e-5 * ref.abs() if name == "out" else 2e-5 * float(ref.abs().max()) + 1e-9
        assert bool((diff <= 3 * off_err + floor).all()), name


def test_transformer_trader_with_wide_heads_collects_and_steps_on_the_wide_feedforward_kernels(monkeypatch):
    monkeypatch.setenv("RL8_AMD_WIDE_ATTENTION", "1")
    monkeypatch.setenv(SWITCH, "1")
    torch.manual_seed(0)
    algo = AlgorithmConfig(num_envs=64, horizon=8, model_cls=TransformerTrader,
                           model_config={"price_embed_dim": 64, "num_heads": 2, "seq_len": 64}).build(AlgoTrading)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        stats = dict(algo.collect())
        stats.update(algo.step())
        ran = launches()
    finally:
        hip.timer.enabled = False
    assert ran.get("feedforward_wide", 0) > 0 and ran.get("feedforward_wide_backward", 0) > 0
    assert "feedforward" not in ran
    for name, value in stats.items():
        assert math.isfinite(float(value)), name
