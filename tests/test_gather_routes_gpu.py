"""Every route of the minibatch gathers (``rl8_gather_minibatch``, ``rl8_pack_samples``, ``rl8_gather_packed``;
``rl8_amd/csrc/stats_gather_kernels.hip``) at its boundaries, through the C ABI, byte for byte against torch indexing.

Sources and destinations live inside larger device buffers filled with a bit pattern no source word holds: the guard
words of both, every source word and the padding between strided source rows must come back untouched, and the
destination must equal ``leaf[:, :h].reshape(n * h, ...)[index]`` in every byte. Each case names the routes it is meant
for and asserts that ``hip.gather_minibatch_plan`` / ``hip.pack_plan`` agree, so a shape that moves to another kernel
fails instead of passing for the wrong reason. Both buffer layouts, time-major and env-major, run everywhere."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from rl8_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF
GUARD = 64       # words of guard on each side, at least
ALIGNED = 64     # word offset of a view into its buffer: 256 bytes
F32, I64 = torch.float32, torch.int64
LAYOUTS = ("time", "env")
GENERAL, WIDE, TILED = "GATHER_GENERAL", "GATHER_WIDE_ROWS", "GATHER_TILED"


class Guarded:
    """``words`` 4-byte words at word offset ``offset`` of a sentinel-filled device buffer."""

    def __init__(self, words: int, offset: int = ALIGNED) -> None:
        self.words, self.offset = words, offset
        self.bits = torch.full((offset + words + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.bits[offset:offset + words]
        assert self.view.data_ptr() % 16 == (offset * 4) % 16

    def ptr(self) -> int:
        return self.view.data_ptr()

    def guards_untouched(self) -> bool:
        lo, hi = self.bits[:self.offset], self.bits[self.offset + self.words:]
        assert lo.numel() >= GUARD and hi.numel() >= GUARD
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())


class Leaf:
    """A [N, T, *trailing] buffer leaf of ``dtype`` inside a guarded buffer: time-major ([T][N][row]) or env-major
    ([N][T][row]), the view ``shift`` elements past a 256-byte boundary, ``env_pad`` / ``time_pad`` elements of padding
    (sentinel words, never to be read or written) behind every env's / timestep's run. Data words are random bits."""

    def __init__(self, n, t, trailing, dtype=F32, layout="time", shift=0, env_pad=0, time_pad=0, seed=0):
        self.trailing = tuple(trailing)
        self.row = int(np.prod(self.trailing, dtype=np.int64)) if self.trailing else 1
        self.ew = 2 if dtype == I64 else 1
        row = self.row
        if layout == "time":
            self.es = row + env_pad
            self.ts = n * self.es + time_pad
        else:
            self.ts = row + time_pad
            self.es = t * self.ts + env_pad
        span = (n - 1) * self.es + (t - 1) * self.ts + row  # elements
        self.buf = Guarded(span * self.ew, ALIGNED + shift * self.ew)
        elems = self.buf.view.view(dtype) if dtype == I64 else self.buf.view.view(F32)
        self.tensor = torch.as_strided(elems, (n, t, row), (self.es, self.ts, 1))
        gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
        data = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, t, row * self.ew), dtype=torch.int64, device=DEV, generator=gen)
        data = data.to(torch.int32)
        data[data == SENTINEL] = 0
        torch.as_strided(self.buf.view, (n, t, row * self.ew), (self.es * self.ew, self.ts * self.ew, 1)).copy_(data)
        self.before = self.buf.bits.clone()
        self.dtype, self.n, self.t = dtype, n, t

    def ptr(self) -> int:
        return self.tensor.data_ptr()

    def intact(self) -> bool:
        return bool((self.buf.bits == self.before).all())

    def samples(self, h: int) -> torch.Tensor:
        """[N * h, row] in the reference's sample order s = env * h + t, by torch."""
        return self.tensor[:, :h].reshape(self.n * h, self.row)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32).reshape(-1)


def indexes(n: int, h: int, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(seed)
    total = n * h
    out = {
        "arange": torch.arange(total),
        "permutation": torch.randperm(total, generator=g),
        "repeats": torch.randint(0, total, (max(total // 2, 3),), generator=g).repeat_interleave(2)[:-1],
        "extremes": torch.tensor([0, total - 1]),
        "one": torch.tensor([total // 2]),
    }
    return {k: v.to(torch.int64).to(DEV) for k, v in out.items()}


def field_array(leaves, dsts):
    fields = (hip.GatherField * len(leaves))()
    for i, (leaf, dst) in enumerate(zip(leaves, dsts)):
        fields[i] = hip.GatherField(leaf.ptr(), dst.ptr() if dst is not None else None, leaf.es, leaf.ts, leaf.row,
                                    4 * leaf.ew)
    return fields


def gather(leaves, h, index, routes, groups=None, launches=None):
    """``rl8_gather_minibatch`` on guarded destinations; checks the plan, the bytes, the guards and the sources."""
    n = leaves[0].n
    m = n * h if index is None else index.numel()
    dsts = [Guarded(m * leaf.row * leaf.ew) for leaf in leaves]
    fields = field_array(leaves, dsts)
    plan = hip.gather_minibatch_plan(index is not None, m, h, fields, len(leaves))
    where = (n, h, m, [(leaf.row, leaf.ew, leaf.es, leaf.ts) for leaf in leaves], plan)
    assert plan.routes == tuple(routes), where
    assert groups is None or plan.groups == tuple(groups), where
    assert launches is None or plan.launches == launches, where
    st = hip.load().rl8_gather_minibatch(index.data_ptr() if index is not None else None, m, h, fields, len(leaves),
                                         torch.cuda.current_stream().cuda_stream)
    assert st == 0, (st, where)
    torch.cuda.synchronize()
    for f, (leaf, dst) in enumerate(zip(leaves, dsts)):
        want = leaf.samples(h) if index is None else leaf.samples(h)[index]
        assert torch.equal(dst.view, bits(want)), (f, where)
        assert dst.guards_untouched() and leaf.intact(), (f, where)
    return plan


# --------------------------------------------------------------------------- #
# indexed: general and wide rows
# --------------------------------------------------------------------------- #
WIDE_CASES = [  # trailing dims, dtype, route of the aligned view
    ((63,), F32, GENERAL),    # 252 bytes
    ((64,), F32, WIDE),       # 256: the boundary, the recurrent state of a width-64 LSTM
    ((65,), F32, GENERAL),    # 260: no whole 16-byte pieces
    ((68,), F32, WIDE),       # 272: one piece past the first 256 bytes
    ((32,), I64, WIDE),       # 256 bytes of 8-byte elements
    ((33,), I64, GENERAL),    # 264
    ((2, 64), F32, WIDE),     # 512: a two-layer width-64 state
    ((1, 128), F32, WIDE),    # 512: a width-128 state
    ((1,), F32, GENERAL), ((3,), I64, GENERAL),
]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("trailing,dtype,route", WIDE_CASES)
def test_rows_around_the_wide_boundary(trailing, dtype, route, layout):
    n, h = 5, 7
    for shift in (0, 1):  # the view one element past the boundary is not 16-byte aligned: general
        leaf = Leaf(n, h + 1, trailing, dtype, layout, shift=shift, seed=shift)
        assert (leaf.ptr() % 16 == 0) == (shift == 0)
        for kind, index in indexes(n, h).items():
            gather([leaf], h, index, [route if shift == 0 else GENERAL], launches=1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("env_pad,time_pad", [(1, 0), (0, 1), (4, 4), (0, 0)])
def test_wide_rows_need_strides_of_whole_sixteen_byte_pieces(env_pad, time_pad, layout):
    n, h = 5, 7
    leaf = Leaf(n, h + 1, (64,), F32, layout, env_pad=env_pad, time_pad=time_pad)
    route = WIDE if env_pad % 4 == 0 and time_pad % 4 == 0 else GENERAL
    for index in indexes(n, h, 1).values():
        gather([leaf], h, index, [route])
    if route == WIDE:  # a destination one float off sends the same leaf to the general kernel
        dst = Guarded(2 * 64, ALIGNED + 1)
        fields = field_array([leaf], [dst])
        assert hip.gather_minibatch_plan(True, 2, h, fields, 1).routes == (GENERAL,)
        index = torch.tensor([n * h - 1, 0], device=DEV)
        assert hip.load().rl8_gather_minibatch(index.data_ptr(), 2, h, fields, 1, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.view, bits(leaf.samples(h)[index])) and dst.guards_untouched() and leaf.intact()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_and_narrow_fields_in_one_call(layout):
    n, h = 6, 5
    mk = lambda trailing, dtype, seed, **kw: Leaf(n, h + 1, trailing, dtype, layout, seed=seed, **kw)  # noqa: E731
    wide_a, narrow_a, wide_b, narrow_b = mk((2, 64), F32, 1), mk((3,), F32, 2), mk((32,), I64, 3), mk((1,), I64, 4)
    off = mk((64,), F32, 5, shift=1)
    for index in indexes(n, h, 2).values():
        gather([wide_a, narrow_a, wide_b, narrow_b], h, index, [WIDE, GENERAL, WIDE, GENERAL], launches=3)
        gather([narrow_b, wide_b, off, narrow_a, wide_a], h, index, [GENERAL, WIDE, GENERAL, GENERAL, WIDE], launches=3)
    # index = NULL: narrow fields ride the tiles, wide ones keep their kernel with the implicit index
    gather([wide_a, narrow_a, wide_b, narrow_b], h, None, [WIDE, TILED, WIDE, TILED], groups=[-1, 0, -1, 1], launches=4)


# --------------------------------------------------------------------------- #
# index = NULL: tiled groups
# --------------------------------------------------------------------------- #
def _leaves(spec, n, t, layout):
    return [Leaf(n, t, (row,), dtype, layout, seed=i) for i, (row, dtype) in enumerate(spec)]


GROUPINGS = {
    "32 words": ([(16, F32), (4, I64), (8, F32)], [0, 0, 0], None),
    "33 words": ([(16, F32), (4, I64), (9, F32)], [0, 0, 1], None),
    "32 + 32": ([(32, F32), (16, I64)], [0, 1], None),
    "a 33-word field between": ([(3, F32), (33, F32), (2, F32)], [0, -1, 1], [TILED, GENERAL, TILED]),
    "eight": ([(1, F32), (1, I64), (5, F32), (1, F32), (1, F32), (2, I64), (19, F32), (1, F32)], [0] * 6 + [1, 1], None),
}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(GROUPINGS))
def test_every_sample_in_order_goes_in_tiled_groups(name, layout):
    spec, groups, routes = GROUPINGS[name]
    routes = routes or [TILED] * len(spec)
    for n, h in ((65, 7), (3, 1), (64, 33)):
        leaves = _leaves(spec, n, h + 1, layout)
        gather(leaves, h, None, routes, groups=groups, launches=max(groups) + 1 + routes.count(GENERAL))
    # the same fields through an index: no tiles
    leaves = _leaves(spec, 5, 4, layout)
    gather(leaves, 3, indexes(5, 3)["permutation"], [GENERAL] * len(spec), launches=1)


def test_every_sample_in_order_needs_whole_envs():
    leaf = Leaf(4, 4, (2,))
    dst = Guarded(13 * 2)
    fields = field_array([leaf], [dst])
    assert hip.load().rl8_gather_minibatch(None, 13, 3, fields, 1, None) == -2
    with pytest.raises(ValueError):
        hip.gather_minibatch_plan(False, 13, 3, fields, 1)
    torch.cuda.synchronize()
    assert bool((dst.view == SENTINEL).all()) and dst.guards_untouched()


# --------------------------------------------------------------------------- #
# pack_samples / gather_packed: all eight instantiations
# --------------------------------------------------------------------------- #
def _packed_specs(words: int):
    """Field lists of ``words`` words with one 8-byte field first, in the middle and last."""
    rest = words - 2
    if rest <= 0:
        return [[(words, F32)]] if words < 2 else [[(1, I64)]]
    a = max(rest // 2, 1)
    f32s = [(a, F32)] + ([(rest - a, F32)] if rest - a > 0 else [])
    lists = [[(1, I64)] + f32s, f32s + [(1, I64)]]
    if len(f32s) == 2:
        lists.insert(1, [f32s[0], (1, I64), f32s[1]])
    return lists


def pack_and_gather(spec, n, h, layout, row_words, seed):
    leaves = _leaves(spec, n, h + 1, layout)
    words = sum(leaf.row * leaf.ew for leaf in leaves)
    assert row_words - 4 < words <= row_words
    plan = hip.pack_plan(n, h, row_words)
    packed = Guarded(n * h * row_words)
    lib, stream = hip.load(), torch.cuda.current_stream().cuda_stream
    where = (spec, n, h, layout, row_words, plan)
    assert lib.rl8_pack_samples(field_array(leaves, [None] * len(leaves)), len(leaves), n, h, packed.ptr(), row_words,
                                stream) == 0, where
    torch.cuda.synchronize()
    rows = torch.cat([leaf.samples(h).contiguous().view(torch.int32).reshape(n * h, -1) for leaf in leaves], dim=1)
    want = torch.zeros((n * h, row_words), dtype=torch.int32, device=DEV)   # padding words are zero
    want[:, :words] = rows
    assert torch.equal(packed.view, want.reshape(-1)), where
    assert packed.guards_untouched() and all(leaf.intact() for leaf in leaves), where
    idx = indexes(n, h, seed)
    for index in (torch.cat([idx["permutation"], idx["repeats"], idx["extremes"]]), idx["one"]):
        m = index.numel()
        dsts = [Guarded(m * leaf.row * leaf.ew) for leaf in leaves]
        assert lib.rl8_gather_packed(index.data_ptr(), m, packed.ptr(), row_words, field_array(leaves, dsts),
                                     len(leaves), stream) == 0, where
        torch.cuda.synchronize()
        for leaf, dst in zip(leaves, dsts):
            assert torch.equal(dst.view, bits(leaf.samples(h)[index])) and dst.guards_untouched(), where
        assert torch.equal(packed.view, want.reshape(-1)) and packed.guards_untouched(), where
    return plan


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("row_words", range(4, 33, 4))
def test_packed_rows_of_every_width(row_words, layout):
    """``gather_packed_kernel<1..8>``; rows filled to the last word and one word short of it; tiles of 1, 63, 64 and 65
    envs, of one step, and horizons one under, at and one over the tile's steps."""
    tile_steps = hip.pack_plan(1, 1000, row_words).tile_steps
    assert tile_steps >= 2
    case = 0
    for words in (row_words, row_words - 1):
        specs = _packed_specs(words)
        for n in (1, 63, 64, 65):
            for h in (1, tile_steps - 1, tile_steps, tile_steps + 1):
                plan = pack_and_gather(specs[case % len(specs)], n, h, layout, row_words, case)
                assert plan.tile_steps == min(h, tile_steps) and plan.tiles == -(-n // 64) * (1 + (h > tile_steps))
                case += 1
    assert case >= 3 * len(_packed_specs(row_words))  # every placement of the 8-byte field ran


# --------------------------------------------------------------------------- #
# grid-stride loops, at the smallest shapes the plans give
# --------------------------------------------------------------------------- #
MAX_GRID, BLOCK, WAVES = 2048, 256, 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_general_and_packed_gathers_take_a_second_trip(layout):
    n, h, m = 64, 8, MAX_GRID * BLOCK + 5
    leaf = Leaf(n, h + 1, (1,), F32, layout)
    index = torch.randint(0, n * h, (m,), device=DEV)
    index[0], index[-1] = n * h - 1, 0
    gather([leaf], h, index, [GENERAL], launches=1)
    packed = Guarded(n * h * 4)
    lib, stream = hip.load(), torch.cuda.current_stream().cuda_stream
    assert lib.rl8_pack_samples(field_array([leaf], [None]), 1, n, h, packed.ptr(), 4, stream) == 0
    dst = Guarded(m)
    assert lib.rl8_gather_packed(index.data_ptr(), m, packed.ptr(), 4, field_array([leaf], [dst]), 1, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.view, bits(leaf.samples(h)[index])) and dst.guards_untouched() and packed.guards_untouched()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_rows_take_a_second_trip(layout):
    n, h, m = 16, 8, MAX_GRID * WAVES + 3   # one wave per row, 2048 workgroups of four
    leaf = Leaf(n, h + 1, (64,), F32, layout)
    index = torch.randint(0, n * h, (m,), device=DEV)
    index[0], index[-1] = n * h - 1, 0
    gather([leaf], h, index, [WIDE], launches=1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tiled_kernel_loops_over_more_tiles_than_workgroups(layout):
    """The smallest buffer of 32-word rows with more tiles than workgroups: a horizon one over the tile's steps doubles
    the tiles (the second of each pair holds one step), then envs are added until ``rl8_pack_plan`` reports a loop."""
    row_words = 32
    h = hip.pack_plan(1, 1000, row_words).tile_steps + 1
    n = 1
    while hip.pack_plan(n, h, row_words).tiles <= hip.pack_plan(n, h, row_words).grid:
        n += 64
    plan = hip.pack_plan(n, h, row_words)
    assert plan.tiles == plan.grid + 2 and hip.pack_plan(n - 64, h, row_words).tiles == plan.grid   # the smallest
    leaves = [Leaf(n, h + 1, (24,), F32, layout, seed=1), Leaf(n, h + 1, (4,), I64, layout, seed=2)]
    gather(leaves, h, None, [TILED, TILED], groups=[0, 0], launches=1)
    packed = Guarded(n * h * row_words)
    assert hip.load().rl8_pack_samples(field_array(leaves, [None, None]), 2, n, h, packed.ptr(), row_words,
                                       torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    want = torch.cat([leaf.samples(h).contiguous().view(torch.int32).reshape(n * h, -1) for leaf in leaves], dim=1)
    assert torch.equal(packed.view, want.reshape(-1)) and packed.guards_untouched()
    assert all(leaf.intact() for leaf in leaves)


def _byte_leaf(n, t, layout):
    data = torch.randint(0, 256, (n, t), dtype=torch.uint8, device=DEV)
    return data if layout == "env" else data.T.contiguous().T


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sequence_gather_takes_a_second_trip(layout):
    n, h, seq_len = 16, 8, 4
    leaf = _byte_leaf(n, h + 1, layout)
    num_seqs = MAX_GRID * BLOCK // seq_len + 1
    seq_index = torch.randint(0, n * h // seq_len, (num_seqs,), device=DEV)
    seq_index[0], seq_index[-1] = n * h // seq_len - 1, 0
    assert num_seqs * seq_len > MAX_GRID * BLOCK
    (got,) = hip.gather_sequences(seq_index, seq_len, h, [leaf])
    torch.cuda.synchronize()
    want = leaf[:, :h].reshape(n * h // seq_len, seq_len)[seq_index].reshape(-1)
    assert torch.equal(got, want)


def _windows(leaf, env, t, size):
    """[rows, size] cells and padding mask of the windows ending at (env, t), by torch."""
    steps = t[:, None] - (size - 1) + torch.arange(size, device=DEV)[None, :]
    padded = steps < 0
    cells = leaf[env[:, None], steps.clamp(min=0)]
    return torch.where(padded, torch.zeros_like(cells), cells), padded


@pytest.mark.parametrize("layout", LAYOUTS)
def test_window_gathers_take_a_second_trip(layout):
    n, h, size = 16, 8, 2
    leaf = _byte_leaf(n, h + 1, layout)
    m = MAX_GRID * BLOCK // size + 1
    index = torch.randint(0, n * h, (m,), device=DEV)
    index[0], index[-1] = n * h - 1, 0
    assert m * size > MAX_GRID * BLOCK
    ((got, mask),) = hip.gather_windows(index, h, [leaf], [size])
    torch.cuda.synchronize()
    want, want_mask = _windows(leaf, index // h, index % h, size)
    assert torch.equal(got, want) and torch.equal(mask, want_mask)
    # window_last: lanes run over envs within a cell
    envs = MAX_GRID * BLOCK // size + 1
    wide = _byte_leaf(envs, 3, layout)
    for t in (0, 2):
        ((got, mask),) = hip.window_last(t, [wide], [size])
        torch.cuda.synchronize()
        want, want_mask = _windows(wide, torch.arange(envs, device=DEV), torch.full((envs,), t, device=DEV), size)
        assert torch.equal(got, want) and torch.equal(mask, want_mask)
