"""``rl8_gather_windows`` and ``rl8_window_last`` against ``rl8_amd/views.py`` (itself pinned to the reference by
``tests/golden/views.npz``) on the same buffers: ``PaddedRollingWindow.apply_all`` followed by an index,
``pad_last_sequence`` on the first ``t + 1`` steps, and a plain gather for ``size == 1``.  The kernels only move
data, so inputs and masks must be bit-equal: every comparison is ``torch.equal``."""

from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.views import PaddedRollingWindow, pad_last_sequence  # noqa: E402

from .test_window_resources import assert_error_statuses  # noqa: E402

DEV = "cuda"
ENVS = [1, 255, 257, 4099]   # one lane, below / above one block of 256, several blocks with a ragged tail
HORIZONS = [1, 5, 32]
#: (name, dtype, trailing shape): 4-byte rows of one and five elements, an 8-byte row, a 3-byte row (no word alignment)
LEAVES = [("f1", torch.float32, 1), ("f5", torch.float32, 5), ("i1", torch.int64, 1), ("b3", torch.bool, 3)]


def sizes_for(h: int) -> list[int]:
    """1 (plain gather), 2, 5, the whole history, and longer than the history (all but one cell padded at t = 0)."""
    return sorted({1, 2, 5, h, h + 3})


def random_slab(h: int, n: int, dtype: torch.dtype, d: int, seed: int, offset: int = 0) -> torch.Tensor:
    """A time-major ``[h + 1, n, d]`` slab; ``offset`` elements into a larger allocation (element-aligned only)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    numel = (h + 1) * n * d
    if dtype == torch.float32:
        flat = torch.randn(numel + offset, device=DEV, generator=g)
        flat[::7] = -0.0  # (a bit pattern a float comparison would not tell from +0)
    elif dtype == torch.int64:
        flat = torch.randint(-2**62, 2**62, (numel + offset,), device=DEV, generator=g)
    else:
        flat = torch.rand(numel + offset, device=DEV, generator=g) > 0.5
    return flat[offset:].view(h + 1, n, d)


def bits(x: torch.Tensor) -> torch.Tensor:
    """Floats as their bit patterns: ``torch.equal`` on them tells -0.0 from 0.0 and compares NaNs."""
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@functools.lru_cache(maxsize=None)
def case(n: int, h: int):
    """Buffers and references of one (N, H), made once and shared: the env-major views of the time-major slabs, and
    per leaf and size the windows of every sample from views.py.  Nothing here is written to afterwards."""
    leaves = {name: random_slab(h, n, dtype, d, seed=17 * n + h + i).transpose(0, 1)
              for i, (name, dtype, d) in enumerate(LEAVES)}
    want = {}
    for name, leaf in leaves.items():
        for size in sizes_for(h):
            if size == 1:
                want[name, size] = (leaf[:, :h].reshape(n * h, -1), None)
            else:
                windows = PaddedRollingWindow.apply_all(leaf[:, :h], size)
                want[name, size] = (windows[DataKeys.INPUTS].contiguous(), windows[DataKeys.PADDING_MASK].contiguous())
    return leaves, want


def launches(h: int) -> list[list[tuple[str, int]]]:
    """Every (leaf, size) pair, eight fields to a launch with the sizes mixed within each."""
    pairs = [(name, size) for size in sizes_for(h) for name, _, _ in LEAVES]
    return [pairs[i:i + hip.MAX_GATHER_FIELDS] for i in range(0, len(pairs), hip.MAX_GATHER_FIELDS)]


def indices(n: int, h: int) -> dict[str, None | torch.Tensor]:
    perm = torch.randperm(n * h, generator=torch.Generator().manual_seed(n + h)).to(DEV)
    envs = torch.arange(n, device=DEV).flip(0)
    return {
        "null": None,
        "permutation": perm,
        "ragged-slice": perm[: max(1, (n * h) // 3 | 1)].contiguous(),  # (an odd length: no multiple of the block)
        "only-t0": envs * h,
        "only-last-t": envs * h + (h - 1),
    }


@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("n", ENVS)
def test_gather_windows_equals_apply_all_then_index(n, h):
    leaves, want = case(n, h)
    assert any(len(fields) == hip.MAX_GATHER_FIELDS for fields in launches(h))
    for label, index in indices(n, h).items():
        rows = n * h if index is None else index.numel()
        for fields in launches(h):
            outs = hip.gather_windows(index, h, [leaves[name] for name, _ in fields], [size for _, size in fields])
            for (name, size), (inputs, mask) in zip(fields, outs):
                want_inputs, want_mask = want[name, size]
                if index is not None:
                    want_inputs = want_inputs[index]
                    want_mask = None if want_mask is None else want_mask[index]
                where = (label, name, size)
                assert inputs.dtype == want_inputs.dtype and inputs.shape == want_inputs.shape, where
                assert inputs.shape[0] == rows, where
                assert torch.equal(bits(inputs), bits(want_inputs)), where
                if size == 1:
                    assert mask is None, where
                else:
                    assert mask.dtype == torch.bool and torch.equal(mask, want_mask), where
                    assert torch.equal(mask.view(torch.uint8), want_mask.view(torch.uint8)), where  # (bytes 0 / 1 only)


def last_steps(h: int, size: int) -> list[int]:
    """t = 0, the last step with padding (size - 2), the first without (size - 1), and the bootstrap column H."""
    return sorted({t for t in (0, size - 2, size - 1, h) if 0 <= t <= h})


@pytest.mark.parametrize("offset", [0, 1], ids=["slab", "offset-in-a-larger-allocation"])
@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("n", ENVS)
def test_window_last_equals_pad_last_sequence(n, h, offset):
    if offset == 0:
        leaves, _ = case(n, h)
    else:  # (slabs that start one element into their allocation: aligned to the element, to nothing wider)
        leaves = {name: random_slab(h, n, dtype, d, seed=3 * n + h + i, offset=1).transpose(0, 1)
                  for i, (name, dtype, d) in enumerate(LEAVES)}
        assert leaves["b3"].data_ptr() % 2 == 1 and leaves["f1"].data_ptr() % 8 == 4
    for fields in launches(h):
        for t in sorted({t for _, size in fields for t in last_steps(h, size)}):
            outs = hip.window_last(t, [leaves[name] for name, _ in fields], [size for _, size in fields])
            for (name, size), (inputs, mask) in zip(fields, outs):
                where = (name, size, t)
                if size == 1:
                    assert mask is None and torch.equal(bits(inputs), bits(leaves[name][:, t].contiguous())), where
                    continue
                want = pad_last_sequence(leaves[name][:, : t + 1], size)
                assert inputs.shape == want[DataKeys.INPUTS].shape and inputs.dtype == want[DataKeys.INPUTS].dtype, where
                assert torch.equal(bits(inputs), bits(want[DataKeys.INPUTS].contiguous())), where
                assert torch.equal(mask, want[DataKeys.PADDING_MASK]), where


def test_rows_beyond_m_are_left_alone():
    """Guard words behind the ``m`` rows of every destination and mask, through the C entries themselves."""
    n, h, m, guard = 257, 5, 300, 64
    leaves, want = case(n, h)
    index = torch.randperm(n * h, generator=torch.Generator().manual_seed(9))[:m].to(DEV)
    lib = hip.load()
    specs = [("f5", 5), ("b3", 2), ("i1", 1), ("f1", h + 3)]

    def run(rows: int, launch) -> None:
        fields = (hip.WindowField * len(specs))()
        held = []
        for i, (name, size) in enumerate(specs):
            leaf = leaves[name]
            d = leaf.shape[2]
            dst = torch.empty(rows * size * d + guard, dtype=leaf.dtype, device=DEV)
            dst_bytes = dst.view(torch.uint8)
            dst_bytes.fill_(0xA5)
            mask = torch.full((rows * size + guard,), 0xA5, dtype=torch.uint8, device=DEV)
            fields[i] = hip.WindowField(leaf.data_ptr(), dst.data_ptr(), mask.data_ptr() if size > 1 else None,
                                        leaf.stride(0), leaf.stride(1), d, leaf.element_size(), size)
            held.append((name, size, d, dst, dst_bytes, mask))
        assert launch(fields) == 0
        torch.cuda.synchronize()
        for name, size, d, dst, dst_bytes, mask in held:
            written = rows * size * d * dst.element_size()
            assert bool((dst_bytes[written:] == 0xA5).all()), (name, size)
            assert bool((mask[rows * size if size > 1 else 0:] == 0xA5).all()), (name, size)
            yield name, size, dst[: rows * size * d], mask[: rows * size]

    stream = torch.cuda.current_stream().cuda_stream
    for name, size, dst, mask in run(m, lambda f: lib.rl8_gather_windows(index.data_ptr(), m, h, f, len(specs), stream)):
        want_inputs, want_mask = want[name, size]
        assert torch.equal(bits(dst), bits(want_inputs[index].reshape(-1))), (name, size)
        if size > 1:
            assert torch.equal(mask, want_mask[index].reshape(-1).view(torch.uint8)), (name, size)
    t = 3
    for name, size, dst, mask in run(n, lambda f: lib.rl8_window_last(t, n, f, len(specs), stream)):
        if size == 1:
            assert torch.equal(bits(dst), bits(leaves[name][:, t].reshape(-1))), name
            continue
        ref = pad_last_sequence(leaves[name][:, : t + 1], size)
        assert torch.equal(bits(dst), bits(ref[DataKeys.INPUTS].reshape(-1))), (name, size)
        assert torch.equal(mask, ref[DataKeys.PADDING_MASK].reshape(-1).view(torch.uint8)), (name, size)


def test_each_error_status_is_returned_with_real_pointers():
    """The argument checks of tests/test_window_resources.py, here with device pointers: nothing is launched, and the
    destination keeps its bytes."""
    dst = torch.full((64,), 0x5A, dtype=torch.uint8, device=DEV)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert_error_statuses(src.data_ptr(), dst.data_ptr())
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())


def test_wrappers_refuse_what_the_kernels_cannot_take():
    leaf = torch.zeros(4, 3, 2, device=DEV)
    with pytest.raises(ValueError, match="one window length each"):
        hip.gather_windows(None, 2, [leaf], [1, 2])
    with pytest.raises(ValueError, match="one window length each"):
        hip.gather_windows(None, 2, [leaf] * 9, [1] * 9)
    with pytest.raises(ValueError, match="at least 1"):
        hip.window_last(0, [leaf], [0])
    with pytest.raises(ValueError, match="outside the leaves"):
        hip.window_last(3, [leaf], [2])
    with pytest.raises(TypeError, match="1, 4 or 8 bytes"):
        hip.gather_windows(None, 2, [leaf.to(torch.float16)], [2])
    with pytest.raises(ValueError, match="trailing dims must be dense"):
        hip.gather_windows(None, 2, [torch.zeros(4, 3, 4, device=DEV)[:, :, ::2]], [2])
    assert C.sizeof(hip.WindowField) == 56
