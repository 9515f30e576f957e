"""The masked sequence kernels (``rl8_amd/csrc/masked_kernels.hip``) and the functions of ``rl8_amd.nn.functional`` that
run them, on an MI355X.

Yardstick: the torch expression of the reference's formula (``rl8_amd.nn.functional`` on CPU tensors, itself pinned to
the reference by ``tests/test_nn_surface_host.py``), in float64 where a tolerance is given and in float32 where
equality or "as the fp32 reference does" is asked for; for the Python layer, the same expression on the device with
``RL8_AMD_MASKED_KERNELS=0``.

Bars.
* AVG forward: ``|got - ref64| <= (T + 2) 2^-24 sum_t|m x| / count`` elementwise: T - 1 additions in any order and one
  division, each within half an ulp of a partial result no larger than ``sum|m x|`` (resp. its quotient), plus the
  rounding of the result itself. NaN exactly where the fp32 reference is NaN.
* AVG backward, MAX forward (values and indices) and backward: equal to the fp32 reference (one division and a
  multiplication by 0 or 1; a selection).
* Log-softmax forward ``rtol=1e-5, atol=1e-6`` (the categorical sampler's bars, tests/test_hip_kernels.py), backward
  ``rtol=2e-5, atol=1e-6 max|want|`` (the loss kernels' gradient bars).
* Sampler: the float64 argmax of ``p / q`` on every row whose best and second-best ratios differ by more than 1e-5
  relative; at most 1 % of the rows may be that close (with standard-normal logits and Exp(1) noise far fewer than one
  row in 4099 is expected to be).

What ``index_out`` holds on a row without a valid cell: every cell reads as ``-FLT_MAX``, all tie, the first wins:
index 0, value ``-FLT_MAX`` -- and the same when ``x`` itself holds ``-FLT_MAX`` in a valid cell behind padded ones: a
padded cell and that value are not told apart, by the reference's ``masked_fill`` + ``argmax`` either, so the index is
that of the first cell of the two kinds. Both are compared with the reference below."""

from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402
from rl8_amd.distributions import NoiseStream  # noqa: E402
from rl8_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
FLT_MAX = torch.finfo(torch.float32).max
GUARD = 64  # elements in front of and behind every kernel output
MASKS = ("none", "valid", "random", "window")
#: rows x T x E: every rows in {1, 63, 64, 65, 4099}, T in {1, 2, 5, 33}, E in {1, 3, 8, 65} at least twice
POOL_SHAPES = [(1, 1, 1), (1, 5, 8), (63, 2, 3), (63, 33, 65), (64, 5, 8), (64, 1, 3), (65, 2, 65), (65, 33, 1),
               (4099, 5, 8), (4099, 2, 1), (4099, 33, 3)]
#: rows x K: every K in {1, 2, 3, 64 (the last of the lane route), 65 (the first of the wave route), 1000} at least twice
ROW_SHAPES = [(1, 3), (1, 65), (63, 1), (63, 64), (63, 1000), (64, 2), (64, 1000), (65, 3), (65, 65), (4099, 1),
              (4099, 2), (4099, 64), (4099, 65)]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def make_mask(kind: str, rows: int, t: int, seed: int) -> None | torch.Tensor:
    """CPU bool ``[rows, t]``, True = VALID. ``window``: row i has ``i % t`` leading cells padded (a padded rolling
    window: the last cell is always valid). ``random`` may pad a whole row."""
    if kind == "none":
        return None
    if kind == "valid":
        return torch.ones(rows, t, dtype=torch.bool)
    if kind == "random":
        return torch.rand(rows, t, generator=gen(seed)) > 0.4
    assert kind == "window"
    return torch.arange(t).expand(rows, t) >= (torch.arange(rows) % t).unsqueeze(1)


def dev(x: None | torch.Tensor) -> None | torch.Tensor:
    return None if x is None else x.to(DEV)


def guarded(numel: int, dtype: torch.dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """A sentinel-filled buffer and the ``numel`` elements in its middle that a kernel may write."""
    buf = torch.full((numel + 2 * GUARD,), -77, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def assert_guards(buf: torch.Tensor, what: str) -> None:
    assert bool((buf[:GUARD] == -77).all()) and bool((buf[-GUARD:] == -77).all()), f"{what}: wrote outside its output"


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: None | torch.Tensor) -> None | int:
    return None if t is None else t.data_ptr()


def raw_pool(x, mask, mode):
    """``rl8_masked_pool_f32`` on device tensors, its outputs between guard words: ``(out, index or None)``."""
    rows, t, e = x.shape
    obuf, out = guarded(rows * e, torch.float32)
    ibuf, index = guarded(rows * e, torch.int64) if mode == hip.POOL_MAX else (None, None)
    status = hip.load().rl8_masked_pool_f32(ptr(x), ptr(mask), rows, t, e, mode, ptr(out), ptr(index), stream())
    assert status == 0
    assert_guards(obuf, "pool out")
    if ibuf is not None:
        assert_guards(ibuf, "pool index")
    return out.view(rows, e), None if index is None else index.view(rows, e)


def raw_pool_backward(dout, mask, index, t, mode):
    rows, e = dout.shape
    buf, dx = guarded(rows * t * e, torch.float32)
    status = hip.load().rl8_masked_pool_backward_f32(ptr(dout), ptr(mask), ptr(index), rows, t, e, mode, ptr(dx), stream())
    assert status == 0
    assert_guards(buf, "pool dx")
    return dx.view(rows, t, e)


def raw_log_softmax(x, mask):
    rows, k = x.shape
    buf, out = guarded(rows * k, torch.float32)
    assert hip.load().rl8_masked_log_softmax_f32(ptr(x), ptr(mask), rows, k, ptr(out), stream()) == 0
    assert_guards(buf, "log-softmax out")
    return out.view(rows, k)


def raw_log_softmax_backward(dout, out):
    rows, k = dout.shape
    buf, dx = guarded(rows * k, torch.float32)
    assert hip.load().rl8_masked_log_softmax_backward_f32(ptr(dout), ptr(out), rows, k, ptr(dx), stream()) == 0
    assert_guards(buf, "log-softmax dx")
    return dx.view(rows, k)


def raw_sample(x, mask, noise, seed=0, step=0, row_offset=0):
    rows, k = x.shape
    vbuf, value = guarded(rows, torch.float32)
    ibuf, index = guarded(rows, torch.int64)
    status = hip.load().rl8_masked_categorical_sample_f32(ptr(x), ptr(mask), ptr(noise), rows, k, seed, step, row_offset,
                                                          ptr(value), ptr(index), stream())
    assert status == 0
    assert_guards(vbuf, "sample value")
    assert_guards(ibuf, "sample index")
    return value, index


def reference_grad(fn, x: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    x = x.clone().requires_grad_(True)
    fn(x).backward(dout)
    return x.grad


def add_log_mask(x: torch.Tensor, mask: None | torch.Tensor) -> torch.Tensor:
    """``z`` of the reference: ``x + clamp(log(mask), FINFO.min, FINFO.max)``."""
    return x if mask is None else x + torch.clamp(torch.log(mask), -FLT_MAX, FLT_MAX)


# --- pooling ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_case(rows: int, t: int, e: int, kind: str):
    """Inputs and CPU references of one pooling case, made once and never written to afterwards."""
    seed = 1000 * rows + 10 * t + e
    x = torch.randn(rows, t, e, generator=gen(seed))
    mask = make_mask(kind, rows, t, seed + 1)
    dout = torch.randn(rows, e, generator=gen(seed + 2))
    m64 = torch.ones(rows, t, 1, dtype=torch.float64) if mask is None else mask.unsqueeze(-1).double()
    return dict(
        x=x, mask=mask, dout=dout,
        avg64=F.masked_avg(x.double(), mask=mask),
        avg_scale=(m64 * x.double()).abs().sum(1) / m64.sum(1),
        avg32=F.masked_avg(x, mask=mask),
        avg_grad=reference_grad(lambda v: F.masked_avg(v, mask=mask), x, dout),
    )


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("rows,t,e", POOL_SHAPES)
def test_avg_forward_and_backward(rows, t, e, kind):
    c = pool_case(rows, t, e, kind)
    x, mask, dout = dev(c["x"]), dev(c["mask"]), dev(c["dout"])
    out, _ = raw_pool(x, mask, hip.POOL_AVG)
    got = out.cpu().double()
    nan = torch.isnan(c["avg32"])  # (rows of the random mask without a valid cell: 0 / 0)
    assert torch.equal(torch.isnan(got), nan)
    err = (got - c["avg64"]).abs()[~nan]
    bound = ((t + 2) * 2.0 ** -24 * c["avg_scale"])[~nan]
    if err.numel():
        print(f"avg {rows}x{t}x{e} {kind}: max error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    dx = raw_pool_backward(dout, mask, None, t, hip.POOL_AVG)
    torch.testing.assert_close(dx.cpu(), c["avg_grad"], rtol=0, atol=0, equal_nan=True)


def test_avg_propagates_nan_and_inf_of_padded_cells_as_mask_times_x_does():
    rows, t, e = 65, 5, 3
    x = torch.randn(rows, t, e, generator=gen(3))
    mask = make_mask("window", rows, t, 0).clone()
    mask[5] = False                      # no valid cell: 0 / 0
    x[7, 0] = float("nan")               # row 7 pads cells 0 and 1: 0 * NaN
    x[8, 1, 1] = float("inf")            # row 8 pads cells 0 .. 2: 0 * inf
    x[9, 0, 2] = float("-inf")           # row 9 pads cells 0 .. 3
    x[10, 0, 0] = float("inf")           # row 10 pads nothing: a valid inf stays inf
    assert not mask[7, 0] and not mask[8, 1] and not mask[9, 0] and mask[10, 0]
    want = F.masked_avg(x, mask=mask)
    assert torch.isnan(want[5]).all() and torch.isnan(want[7]).all() and torch.isnan(want[8, 1]) and torch.isnan(want[9, 2])
    out, _ = raw_pool(dev(x), dev(mask), hip.POOL_AVG)
    got = out.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    finite = torch.isfinite(want)
    m64, x64 = mask.unsqueeze(-1).double(), x.double()
    err = (got.double() - F.masked_avg(x64, mask=mask)).abs()[finite]
    assert bool((err <= ((t + 2) * 2.0 ** -24 * ((m64 * x64).abs().sum(1) / m64.sum(1)))[finite]).all())
    dout = torch.randn(rows, e, generator=gen(4))
    dx = raw_pool_backward(dev(dout), dev(mask), None, t, hip.POOL_AVG)
    want_dx = reference_grad(lambda v: F.masked_avg(v, mask=mask), x, dout)
    assert torch.isnan(want_dx[5]).all()  # (dout / 0 times 0)
    torch.testing.assert_close(dx.cpu(), want_dx, rtol=0, atol=0, equal_nan=True)


@functools.lru_cache(maxsize=None)
def max_case(rows: int, t: int, e: int, kind: str):
    seed = 2000 * rows + 10 * t + e
    # few distinct values: ties within most columns (the first maximal cell must win)
    x = torch.randint(-2, 3, (rows, t, e), generator=gen(seed)).float() * 0.5
    mask = make_mask(kind, rows, t, seed + 1)
    dout = torch.randn(rows, e, generator=gen(seed + 2))
    values, index = F.masked_max(x, mask=mask)
    grad = reference_grad(lambda v: F.masked_max(v, mask=mask)[0], x, dout.unsqueeze(1))
    return dict(x=x, mask=mask, dout=dout, values=values.squeeze(1), index=index.squeeze(1), grad=grad)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("rows,t,e", POOL_SHAPES)
def test_max_forward_and_backward(rows, t, e, kind):
    c = max_case(rows, t, e, kind)
    x, mask, dout = dev(c["x"]), dev(c["mask"]), dev(c["dout"])
    out, index = raw_pool(x, mask, hip.POOL_MAX)
    assert torch.equal(index.cpu(), c["index"]) and torch.equal(out.cpu(), c["values"])
    dx = raw_pool_backward(dout, mask, index, t, hip.POOL_MAX)
    torch.testing.assert_close(dx.cpu(), c["grad"], rtol=0, atol=0)


def test_max_on_nan_padded_rows_and_the_lowest_float():
    rows, t, e = 65, 5, 3
    x = torch.randn(rows, t, e, generator=gen(5))
    mask = make_mask("window", rows, t, 0).clone()
    mask[5] = False                       # no valid cell: -FLT_MAX at index 0
    x[6, 2] = float("nan")                # row 6 pads cell 0 only: cell 2 is valid, the first NaN wins
    x[6, 4, 0] = float("nan")
    x[7, 0] = float("nan")                # row 7 pads cells 0, 1: a padded NaN is not seen
    x[8, 3] = -FLT_MAX                    # row 8 pads cells 0 .. 2 and holds -FLT_MAX in its valid cells: they tie with
    x[8, 4] = -FLT_MAX                    # the padded ones, and index 0 (a padded cell) is what the reference gives
    values, index = F.masked_max(x, mask=mask)
    assert (index[5] == 0).all() and (values[5] == -FLT_MAX).all() and (index[6, 0] == 2).all() and (index[8] == 0).all()
    out, got_index = raw_pool(dev(x), dev(mask), hip.POOL_MAX)
    assert torch.equal(got_index.cpu(), index.squeeze(1))
    torch.testing.assert_close(out.cpu(), values.squeeze(1), rtol=0, atol=0, equal_nan=True)
    dout = torch.randn(rows, e, generator=gen(6))
    dx = raw_pool_backward(dev(dout), dev(mask), got_index, t, hip.POOL_MAX)
    want_dx = reference_grad(lambda v: F.masked_max(v, mask=mask)[0], x, dout.unsqueeze(1))
    assert (want_dx[5] == 0).all() and (want_dx[8] == 0).all()  # (nothing flows into a padded cell, chosen or not)
    torch.testing.assert_close(dx.cpu(), want_dx, rtol=0, atol=0)


# --- log-softmax --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_case(rows: int, k: int, kind: str):
    seed = 3000 * rows + k
    x = torch.randn(rows, k, generator=gen(seed))
    mask = make_mask(kind, rows, k, seed + 1)
    if kind == "random":
        mask = mask.clone()
        mask[0] = False  # a row with every class masked: uniform, by the same additions
    dout = torch.randn(rows, k, generator=gen(seed + 2))
    x64 = x.double()
    out64 = F.masked_log_softmax(x64, mask=mask)
    grad64 = reference_grad(lambda v: F.masked_log_softmax(v, mask=mask), x64, dout.double())
    return dict(x=x, mask=mask, dout=dout, out64=out64, grad64=grad64)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("rows,k", ROW_SHAPES)
def test_log_softmax_forward_and_backward(rows, k, kind):
    c = rows_case(rows, k, kind)
    assert hip.masked_rows_route(k) == (hip.MASKED_ROWS_LANE if k <= 64 else hip.MASKED_ROWS_WAVE)
    x, mask, dout = dev(c["x"]), dev(c["mask"]), dev(c["dout"])
    out = raw_log_softmax(x, mask)
    if kind == "random":
        torch.testing.assert_close(out[0].cpu(), torch.full((k,), -float(torch.log(torch.tensor(float(k))))),
                                   rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out.cpu(), c["out64"].float(), rtol=1e-5, atol=1e-6)
    dx = raw_log_softmax_backward(dout, out)
    want = c["grad64"].float()
    torch.testing.assert_close(dx.cpu(), want, rtol=2e-5, atol=1e-6 * float(want.abs().max()))


@pytest.mark.parametrize("k", [3, 64, 65, 1000])
def test_log_softmax_at_large_logits_behaves_as_the_fp32_reference(k):
    rows = 65
    x = torch.randn(rows, k, generator=gen(k))
    x[:, 0] = 80.0
    x[:, 1] = -80.0
    x[1::2, 0] = -80.0                 # (rows whose largest logit is an ordinary one)
    x[:, 2] = -3.0e38                  # masked below: -3e38 + -FLT_MAX overflows to -inf, as in the reference
    mask = torch.ones(rows, k, dtype=torch.bool)
    mask[:, 2] = False
    mask[3, 0] = False                 # a masked +80
    want = F.masked_log_softmax(x, mask=mask)
    assert torch.isinf(want[:, 2]).all() and torch.isfinite(want[:, :2]).all()
    out = raw_log_softmax(dev(x), dev(mask)).cpu()
    assert torch.equal(torch.isinf(out), torch.isinf(want)) and not torch.isnan(out).any()
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-6)


# --- sampler ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sample_case(rows: int, k: int, kind: str):
    seed = 4000 * rows + k
    x = torch.randn(rows, k, generator=gen(seed))
    mask = make_mask(kind, rows, k, seed + 1)
    if mask is not None and kind == "random":
        mask = mask.clone()
        mask[torch.arange(rows), torch.randint(0, k, (rows,), generator=gen(seed + 3))] = True  # a valid class per row
    q = torch.empty(rows, k).exponential_(generator=gen(seed + 2)).clamp_min(1e-30)
    z64 = add_log_mask(x.double(), mask)
    ratio = torch.softmax(z64, dim=-1) / q.double()
    if k > 1:
        top = ratio.topk(2, dim=-1)
        decided = (top.values[:, 0] - top.values[:, 1]) > 1e-5 * top.values[:, 0]
    else:
        decided = torch.ones(rows, dtype=torch.bool)
    return dict(x=x, mask=mask, q=q, want=ratio.argmax(dim=-1), decided=decided, z32=add_log_mask(x, mask))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("rows,k", ROW_SHAPES)
def test_sampler_with_injected_noise(rows, k, kind):
    c = sample_case(rows, k, kind)
    value, index = raw_sample(dev(c["x"]), dev(c["mask"]), dev(c["q"]))
    index, decided = index.cpu(), c["decided"]
    excluded = int((~decided).sum())
    print(f"sampler {rows}x{k} {kind}: {excluded} of {rows} rows closer than 1e-5")
    assert excluded <= rows // 100
    assert torch.equal(index[decided], c["want"][decided])
    assert bool(((index >= 0) & (index < k)).all())
    if c["mask"] is not None:  # (every row of these masks has a valid class: a masked one is never drawn)
        assert bool(c["mask"].gather(1, index.unsqueeze(1)).all())
    assert torch.equal(value.cpu(), c["z32"].gather(1, index.unsqueeze(1)).squeeze(1))


@pytest.mark.parametrize("k", [3, 64, 65, 1000])
def test_sampler_picks_the_first_valid_class_of_an_all_tied_row(k):
    rows = 65
    x = torch.full((rows, k), 0.25)
    q = torch.ones(rows, k)
    mask = torch.ones(rows, k, dtype=torch.bool)
    first = torch.arange(rows) % (k - 1)        # classes in front of `first` are masked
    mask[torch.arange(k).expand(rows, k) < first.unsqueeze(1)] = False
    _, index = raw_sample(dev(x), dev(mask), dev(q))
    assert torch.equal(index.cpu(), first)
    _, index = raw_sample(dev(x), None, dev(q))
    assert bool((index == 0).all())


@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("kind", ["none", "random"])
def test_sampler_on_philox_picks_the_classes_of_the_categorical_sampler(k, kind):
    """Same ``z``, seed, step and row offset: the same classes, bit for bit, as ``rl8_categorical_sample_logp_f32``."""
    rows = 4099
    c = sample_case(rows, k, kind)
    x, mask = dev(c["x"]), dev(c["mask"])
    z = dev(c["z32"])
    seed, step, row_offset = 0x1234_5678_9ABC, 7, 1_000_003
    want, _ = hip.categorical_sample_logp(z.unsqueeze(1).contiguous(), None, seed=seed, step=step, row_offset=row_offset)
    value, index = raw_sample(x, mask, None, seed, step, row_offset)
    assert torch.equal(index, want.squeeze(1))
    assert torch.equal(value, z.gather(1, index.unsqueeze(1)).squeeze(1))
    _, other = raw_sample(x, mask, None, seed, step + 1, row_offset)
    assert not torch.equal(other, index)  # (another step: other noise)


# --- the Python layer ---------------------------------------------------------------------------------------------
def grads_on_and_off(monkeypatch, fn, x: torch.Tensor, dout: torch.Tensor):
    """Output and input gradient of ``fn`` on the kernels and with ``RL8_AMD_MASKED_KERNELS=0``, and the launches of
    the first run."""
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("RL8_AMD_MASKED_KERNELS", switch)
        hip.timer.reset()
        hip.timer.enabled = True
        try:
            v = x.clone().requires_grad_(True)
            y = fn(v)
            y.backward(dout)
            out[switch] = (y.detach(), v.grad, set(hip.timer.summary()))
        finally:
            hip.timer.enabled = False
    return out["1"], out["0"]


@pytest.mark.parametrize("kind", ["valid", "random", "window"])
def test_masked_avg_gradient_with_the_switch_on_and_off(monkeypatch, kind):
    """(Masked cases: without a mask the torch route is ``x.mean``, which on the device multiplies by a rounded
    ``1 / T`` in both directions where the reference's CPU run, and the kernel, divide by ``T``; the unmasked kernel is
    held to the CPU's division in ``test_avg_forward_and_backward``.)"""
    rows, t, e = 4099, 5, 8
    x = torch.randn(rows, t, 2, e // 2, generator=gen(21)).to(DEV)  # (trailing dimensions are flattened to E)
    mask = dev(make_mask(kind, rows, t, 22))
    dout = torch.randn(rows, 1, 2, e // 2, generator=gen(23)).to(DEV)
    (y1, g1, ran1), (y0, g0, ran0) = grads_on_and_off(
        monkeypatch, lambda v: F.masked_avg(v, mask=mask, dim=1, keepdim=True), x, dout)
    assert {"masked_pool", "masked_pool_backward"} <= ran1 and not any(n.startswith("masked_") for n in ran0)
    assert y1.shape == y0.shape == (rows, 1, 2, e // 2)
    # (two fp32 results, each within (T + 2) 2^-24 sum|m x| / count <= (T + 2) 2^-24 max|x| of the exact one)
    torch.testing.assert_close(y1, y0, rtol=0, atol=(t + 2) * 2.0 ** -23 * float(x.abs().max()), equal_nan=True)
    torch.testing.assert_close(g1, g0, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("kind", MASKS)
def test_masked_max_gradient_with_the_switch_on_and_off(monkeypatch, kind):
    rows, t = 4099, 5
    x = (torch.randint(-2, 3, (rows, t, 3), generator=gen(31)).float() * 0.5).to(DEV)
    mask = dev(make_mask(kind, rows, t, 32))
    dout = torch.randn(rows, 1, 3, generator=gen(33)).to(DEV)
    (y1, g1, ran1), (y0, g0, ran0) = grads_on_and_off(monkeypatch, lambda v: F.masked_max(v, mask=mask)[0], x, dout)
    assert {"masked_pool", "masked_pool_backward"} <= ran1 and not any(n.startswith("masked_") for n in ran0)
    assert torch.equal(y1, y0) and torch.equal(g1, g0)
    monkeypatch.setenv("RL8_AMD_MASKED_KERNELS", "1")
    on_host = F.masked_max(x.cpu(), mask=None if mask is None else mask.cpu())[1]
    assert torch.equal(F.masked_max(x, mask=mask)[1].cpu(), on_host)


@pytest.mark.parametrize("k", [3, 1000])
@pytest.mark.parametrize("kind", MASKS)
def test_masked_log_softmax_gradient_with_the_switch_on_and_off(monkeypatch, kind, k):
    rows = 65
    x = torch.randn(4, rows, k, generator=gen(41)).to(DEV)  # (a 3-D input with a mask of its shape)
    mask = make_mask(kind, 4 * rows, k, 42)
    mask = None if mask is None else mask.view(4, rows, k).to(DEV)
    dout = torch.randn(4, rows, k, generator=gen(43)).to(DEV)
    (y1, g1, ran1), (y0, g0, ran0) = grads_on_and_off(monkeypatch, lambda v: F.masked_log_softmax(v, mask=mask), x, dout)
    assert {"masked_log_softmax", "masked_log_softmax_backward"} <= ran1 and not any(n.startswith("masked_") for n in ran0)
    torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(g1, g0, rtol=2e-5, atol=1e-6 * float(g0.abs().max()))


def test_masked_categorical_sample_through_the_public_function(monkeypatch):
    monkeypatch.setenv("RL8_AMD_MASKED_KERNELS", "1")
    c = sample_case(4099, 3, "random")
    x, mask, q = dev(c["x"]), dev(c["mask"]), dev(c["q"])
    v = x.clone().requires_grad_(True)
    values, index = F.masked_categorical_sample(v, mask=mask, dim=1, noise=q)
    assert values.shape == index.shape == (4099, 1) and index.dtype == torch.int64 and not index.requires_grad
    assert torch.equal(index.squeeze(1).cpu()[c["decided"]], c["want"][c["decided"]])
    dout = torch.randn(4099, 1, generator=gen(51)).to(DEV)
    values.backward(dout)
    assert torch.equal(v.grad, torch.zeros_like(x).scatter_(1, index, dout))  # (a one-hot scatter)
    # the Philox route: the stream given, at its address, and one step further afterwards
    noise = NoiseStream(99)
    noise.step, noise.row_offset = 4, 17
    _, drawn = F.masked_categorical_sample(x, mask=mask, noise_stream=noise)
    assert noise.step == 5
    want, _ = hip.categorical_sample_logp(dev(c["z32"]).unsqueeze(1).contiguous(), None, seed=99, step=4, row_offset=17)
    assert torch.equal(drawn, want)


def test_inputs_outside_the_kernels_take_the_torch_route(monkeypatch):
    monkeypatch.setenv("RL8_AMD_MASKED_KERNELS", "1")
    rows, t, e = 65, 5, 8
    x = torch.randn(rows, t, e, generator=gen(61)).to(DEV)
    mask = dev(make_mask("window", rows, t, 0))
    strided = torch.randn(rows, e, t, generator=gen(62)).to(DEV).transpose(1, 2)  # [rows, t, e], not contiguous
    logits = torch.randn(rows, t, generator=gen(63)).to(DEV)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        calls = [
            (lambda: F.masked_avg(strided, mask=mask), lambda: F.masked_avg(strided.cpu(), mask=mask.cpu())),
            (lambda: F.masked_avg(x, mask=mask.float()), lambda: F.masked_avg(x.cpu(), mask=mask.cpu().float())),
            (lambda: F.masked_avg(x, mask=None, dim=2), lambda: F.masked_avg(x.cpu(), mask=None, dim=2)),
            (lambda: F.masked_avg(x.double(), mask=mask), lambda: F.masked_avg(x.cpu().double(), mask=mask.cpu())),
            (lambda: F.masked_max(strided, mask=mask)[0], lambda: F.masked_max(strided.cpu(), mask=mask.cpu())[0]),
            (lambda: F.masked_max(x, mask=mask.float())[1], lambda: F.masked_max(x.cpu(), mask=mask.cpu().float())[1]),
            (lambda: F.masked_max(x, dim=2)[1], lambda: F.masked_max(x.cpu(), dim=2)[1]),
            (lambda: F.masked_log_softmax(logits, mask=mask.float()),
             lambda: F.masked_log_softmax(logits.cpu(), mask=mask.cpu().float())),
            (lambda: F.masked_log_softmax(logits, mask=mask, dim=0), lambda: F.masked_log_softmax(logits.cpu(), mask=mask.cpu(), dim=0)),
            (lambda: F.masked_log_softmax(x, mask=mask, dim=-1), lambda: F.masked_log_softmax(x.cpu(), mask=mask.cpu(), dim=-1)),
        ]
        for on_device, on_host in calls:
            torch.testing.assert_close(on_device().cpu(), on_host(), rtol=1e-5, atol=1e-6)
        ran = set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
    assert not any(name.startswith("masked_") for name in ran), ran


def test_what_the_autograd_functions_save(monkeypatch):
    """``masked_avg`` saves the mask only, ``masked_max`` indices (and its mask), ``masked_log_softmax`` its output;
    under ``no_grad`` nothing is saved and nothing is attached."""
    monkeypatch.setenv("RL8_AMD_MASKED_KERNELS", "1")
    rows, t, e = 65, 5, 8
    x = torch.randn(rows, t, e, generator=gen(71)).to(DEV).requires_grad_(True)
    logits = torch.randn(rows, t, generator=gen(72)).to(DEV).requires_grad_(True)
    mask = dev(make_mask("window", rows, t, 0))
    saved: list[torch.Tensor] = []

    def pack(tensor):
        saved.append(tensor)
        return tensor

    def run(fn):
        saved.clear()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda tensor: tensor):
            out = fn()
        return out, [(s.dtype, tuple(s.shape)) for s in saved]

    out, kept = run(lambda: F.masked_avg(x, mask=mask))
    assert out.requires_grad and kept == [(torch.bool, (rows, t))]
    out, kept = run(lambda: F.masked_avg(x))
    assert out.requires_grad and kept == []
    (out, _), kept = run(lambda: F.masked_max(x, mask=mask))
    assert out.requires_grad and sorted(kept, key=str) == sorted([(torch.int64, (rows, e)), (torch.bool, (rows, t))], key=str)
    out, kept = run(lambda: F.masked_log_softmax(logits, mask=mask))
    assert out.requires_grad and kept == [(torch.float32, (rows, t))] and saved[0].data_ptr() == out.data_ptr()
    with torch.no_grad():
        for fn in (lambda: F.masked_avg(x, mask=mask), lambda: F.masked_max(x, mask=mask)[0],
                   lambda: F.masked_log_softmax(logits, mask=mask),
                   lambda: F.masked_categorical_sample(logits, mask=mask)[0]):
            out, kept = run(fn)
            assert kept == [] and out.grad_fn is None and not out.requires_grad
