"""The launch plans of ``rl8_amd/csrc/stats_gather_kernels.hip`` on the CPU: ``rl8_rollout_stats_plan``,
``rl8_gather_minibatch_plan`` and ``rl8_pack_plan`` are host arithmetic of the library, swept here over shapes, strides,
alignments and element widths and held to a plain restatement of the predicates as they stood while the entries decided
inline. The pointers in a field list are made-up addresses: the plans judge them for alignment and never read through
them. (``RL8_STATS_GRID_CAP`` and ``RL8_PACK_TILE_KIB`` are read once per process and are not part of these tables: the
sweeps describe the defaults.)"""

from __future__ import annotations

import ctypes as C
import itertools

import pytest

from rl8_amd import hip

# constants of rl8_amd/csrc/common.hip.h and stats_gather_kernels.hip
WAVE, BLOCK, CUS, MAX_GRID = 64, 256, 256, 2048
WAVES_PER_BLOCK = BLOCK // WAVE
PACK_ENVS, PACK_STEPS, TILE_WORDS, TILE_KIB, LDS_CU = 64, 32, 32, 36, 160 * 1024
BASE = 0x7F0000001000  # a 4 KiB-aligned made-up address


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _grid_for(items: int, per_block: int, cap: int = MAX_GRID) -> int:
    return min(max(_ceil_div(items, per_block), 1), cap)


# --------------------------------------------------------------------------- #
# statistics
# --------------------------------------------------------------------------- #
def _inline_stats(n, h, es, ts, aligned):
    vec = es == 1 and n % 4 == 0 and ts % 4 == 0 and aligned
    grid = _grid_for(n, BLOCK * 4) if vec else _grid_for(n, BLOCK)
    return ("STATS_VEC4" if vec else "STATS_VEC1", grid, _ceil_div(n, grid * BLOCK * (4 if vec else 1)))


STATS_N = tuple(range(1, 70)) + (255, 256, 257, 1023, 1024, 1025, 1028, 4096, 2048 * 256, 2048 * 256 + 3, 2048 * 1024,
                                 2048 * 1024 + 4, 2048 * 1024 + 5, 3 * 2048 * 1024)
STATS_H = (1, 2, 7, 8, 9, 16, 17, 32, 33)


def test_stats_plan_matches_the_inline_dispatch_it_replaced():
    lib, p, seen = hip.load(), hip.StatsPlanStruct(), set()
    for n, h, aligned in itertools.product(STATS_N, STATS_H, (True, False)):
        layouts = [(1, n), (1, n + 1), (1, n + 2), (1, n + 4), (1, (n + 3) // 4 * 4), (h + 1, 1), (h + 2, 1), (2, 2 * n)]
        for es, ts in layouts:
            assert lib.rl8_rollout_stats_plan(n, h, es, ts, int(aligned), C.byref(p)) == 0
            got = (hip.STATS_ROUTES[p.route], p.grid, p.trips)
            assert got == _inline_stats(n, h, es, ts, aligned), (n, h, es, ts, aligned)
            assert 1 <= p.grid <= MAX_GRID                 # one partial row per workgroup: RL8_MAX_PARTIALS of them
            per_trip = p.grid * BLOCK * (4 if got[0] == "STATS_VEC4" else 1)
            assert (p.trips - 1) * per_trip < n <= p.trips * per_trip   # every env visited, no idle trip
            if got[0] == "STATS_VEC4":                     # what the 16-byte loads rely on
                assert es == 1 and n % 4 == 0 and ts % 4 == 0 and aligned
            seen.add((got[0], p.trips > 1))
    assert seen == {("STATS_VEC4", False), ("STATS_VEC4", True), ("STATS_VEC1", False), ("STATS_VEC1", True)}


def test_stats_plan_edges():
    plan = hip.rollout_stats_plan
    assert plan(1024, 8, 1, 1024) == hip.StatsPlan("STATS_VEC4", 1, 1)
    assert plan(1028, 8, 1, 1028) == hip.StatsPlan("STATS_VEC4", 2, 1)
    assert plan(1024, 8, 1, 1024, False).route == "STATS_VEC1"      # a view one float into its slab
    assert plan(1024, 8, 1, 1026).route == "STATS_VEC1"             # padded columns, not whole 16-byte pieces
    assert plan(1023, 8, 1, 1023).route == "STATS_VEC1" == plan(1, 8, 1, 1).route
    assert plan(1024, 8, 9, 1).route == "STATS_VEC1"                # env-major
    assert plan(2048 * 256, 2, 3, 1) == hip.StatsPlan("STATS_VEC1", 2048, 1)
    assert plan(2048 * 256 + 3, 2, 3, 1) == hip.StatsPlan("STATS_VEC1", 2048, 2)
    assert plan(2048 * 1024 + 4, 2, 1, 2048 * 1024 + 4) == hip.StatsPlan("STATS_VEC4", 2048, 2)


def test_stats_plan_argument_checks_need_no_device():
    lib, p = hip.load(), hip.StatsPlanStruct()
    assert lib.rl8_rollout_stats_plan(8, 4, 1, 8, 1, None) == -1
    for bad in ((0, 4, 1, 8), (8, 0, 1, 8), (8, 4, 0, 8), (8, 4, 1, 0), (-1, 4, 1, 8)):
        assert lib.rl8_rollout_stats_plan(*bad, 1, C.byref(p)) == -2, bad
    # the entry itself: NULL pointers, then the plan's size checks, before any launch
    assert lib.rl8_rollout_stats_f32(None, None, 8, 4, 1, 8, None, None, None) == -1
    assert lib.rl8_rollout_stats_f32(16, None, 0, 4, 1, 8, 16, 16, None) == -2
    assert lib.rl8_rollout_stats_f32(16, None, 8, 4, 0, 8, 16, 16, None) == -2


# --------------------------------------------------------------------------- #
# gather_minibatch
# --------------------------------------------------------------------------- #
def _fields(specs):
    """specs: (row_elems, elem_bytes, src offset, dst offset, env_stride, time_stride), offsets in bytes from 4 KiB
    boundaries."""
    fields = (hip.GatherField * len(specs))()
    for i, (row, eb, so, do, es, ts) in enumerate(specs):
        fields[i] = hip.GatherField(BASE + 0x10000 * i + so, BASE + 0x1000000 + 0x10000 * i + do, es, ts, row, eb)
    return fields


def _inline_gather(indexed, specs):
    """The body of ``rl8_gather_minibatch`` before the plan existed: (routes, groups, launches)."""
    routes, groups = [], []
    n_groups, words, wide, general = 0, 0, 0, 0
    for row, eb, so, do, es, ts in specs:
        row_bytes = row * eb
        if not indexed and row_bytes // 4 <= TILE_WORDS:
            w = row_bytes // 4
            if words == 0 or words + w > TILE_WORDS:
                n_groups, words = n_groups + 1, 0
            words += w
            routes.append("GATHER_TILED")
            groups.append(n_groups - 1)
            continue
        words = 0
        is_wide = (row_bytes >= 256 and row_bytes % 16 == 0 and so % 16 == 0 and do % 16 == 0
                   and (es * eb) % 16 == 0 and (ts * eb) % 16 == 0)
        routes.append("GATHER_WIDE_ROWS" if is_wide else "GATHER_GENERAL")
        groups.append(-1)
        wide, general = wide + is_wide, general + (not is_wide)
    return tuple(routes), tuple(groups), n_groups + wide + (1 if general else 0)


def test_gather_plan_single_fields_over_widths_alignments_and_strides():
    seen = set()
    for eb in (4, 8):
        for row_bytes in (4, 8, 16, 124, 128, 132, 136, 248, 252, 256, 260, 264, 272, 512, 1024, 1028, 4096):
            if row_bytes % eb:
                continue
            row = row_bytes // eb
            for so, do in ((0, 0), (eb, 0), (0, eb), (eb, eb), (16, 32)):
                for es, ts in ((row * 9, row), (row, row * 7), (row * 9 + 1, row), (row, row * 7 + 1), (row * 9 + 2, row * 2)):
                    for indexed in (True, False):
                        spec = [(row, eb, so, do, es, ts)]
                        got = hip.gather_minibatch_plan(indexed, 12, 3, _fields(spec), 1)
                        assert tuple(got) == _inline_gather(indexed, spec), (spec, indexed)
                        assert got.launches == 1
                        seen.add(got.routes[0])
                        if got.routes[0] == "GATHER_WIDE_ROWS":   # what the 16-byte pieces of a wave rely on
                            assert row_bytes >= 256 and row_bytes % 16 == 0 and so % 16 == 0 and do % 16 == 0
                            assert (es * eb) % 16 == 0 and (ts * eb) % 16 == 0
                        if got.routes[0] == "GATHER_TILED":
                            assert not indexed and row_bytes <= 128 and got.groups == (0,)
    assert seen == set(hip.GATHER_ROUTES)


def test_gather_plan_field_lists_and_groups():
    f4 = lambda row: (row, 4, 0, 0, row * 5, row)  # noqa: E731
    i8 = lambda row: (row, 8, 0, 0, row * 5, row)  # noqa: E731
    lists = {
        "32 words": [f4(16), i8(4), f4(8)],
        "33 words": [f4(16), i8(4), f4(9)],
        "32 + 32": [f4(32), i8(16)],
        "33-word field between": [f4(3), f4(33), f4(2)],
        "eight": [f4(1), i8(1), f4(5), f4(1), f4(1), i8(2), f4(19), f4(1)],
        "wide and narrow": [f4(64), f4(1), i8(32), f4(3)],
        "narrow and wide": [f4(1), f4(128), i8(1), (64, 4, 4, 0, 320, 64)],
    }
    for name, spec in lists.items():
        for indexed in (True, False):
            got = hip.gather_minibatch_plan(indexed, 24, 4, _fields(spec), len(spec))
            assert tuple(got) == _inline_gather(indexed, spec), (name, indexed)
    plan = lambda name, indexed=False: hip.gather_minibatch_plan(indexed, 24, 4, _fields(lists[name]), len(lists[name]))  # noqa: E731
    assert plan("32 words") == (("GATHER_TILED",) * 3, (0, 0, 0), 1)
    assert plan("33 words") == (("GATHER_TILED",) * 3, (0, 0, 1), 2)
    assert plan("32 + 32") == (("GATHER_TILED",) * 2, (0, 1), 2)
    assert plan("33-word field between") == (("GATHER_TILED", "GATHER_GENERAL", "GATHER_TILED"), (0, -1, 1), 3)
    assert plan("eight").groups == (0, 0, 0, 0, 0, 0, 1, 1) and plan("eight").launches == 2
    assert plan("wide and narrow", True) == (("GATHER_WIDE_ROWS", "GATHER_GENERAL", "GATHER_WIDE_ROWS", "GATHER_GENERAL"),
                                            (-1,) * 4, 3)
    assert plan("narrow and wide", True).routes == ("GATHER_GENERAL", "GATHER_WIDE_ROWS", "GATHER_GENERAL", "GATHER_GENERAL")
    assert plan("wide and narrow").routes == ("GATHER_WIDE_ROWS", "GATHER_TILED", "GATHER_WIDE_ROWS", "GATHER_TILED")
    assert plan("wide and narrow").groups == (-1, 0, -1, 1)


def test_gather_plan_argument_checks_need_no_device():
    lib = hip.load()
    routes, groups, launches = (C.c_int * 8)(), (C.c_int * 8)(), C.c_int()
    ok = [(4, 4, 0, 0, 20, 4)]

    def call(indexed, m, h, fields, n_fields, r=routes, g=groups, l=launches):  # noqa: E741
        return lib.rl8_gather_minibatch_plan(indexed, m, h, fields, n_fields, r, g, C.byref(l) if l is not None else None)

    assert call(1, 12, 3, _fields(ok), 1) == 0
    assert call(1, 12, 3, None, 1) == -1 and call(1, 12, 3, _fields(ok), 1, None) == -1
    assert call(1, 12, 3, _fields(ok), 1, routes, None) == -1 and call(1, 12, 3, _fields(ok), 1, routes, groups, None) == -1
    assert call(1, 0, 3, _fields(ok), 1) == -2 and call(1, 12, 0, _fields(ok), 1) == -2
    assert call(1, 12, 3, _fields(ok), 0) == -2 and call(1, 12, 3, _fields(ok * 9), 9) == -2
    assert call(1, 13, 3, _fields(ok), 1) == 0 and call(0, 13, 3, _fields(ok), 1) == -2   # index = NULL: m % h
    for bad, code in (((4, 2, 0, 0, 20, 4), -4), ((4, 1, 0, 0, 20, 4), -4), ((0, 4, 0, 0, 20, 4), -2)):
        for indexed in (0, 1):
            assert call(indexed, 12, 3, _fields(ok + [bad]), 2) == code, (bad, indexed)
    null_src, null_dst = _fields(ok * 2), _fields(ok * 2)
    null_src[1].src, null_dst[1].dst = None, None
    for indexed in (0, 1):
        assert call(indexed, 12, 3, null_src, 2) == -1 and call(indexed, 12, 3, null_dst, 2) == -1
    # the entry returns the same codes before any launch: a bad LAST field behind good ones launches nothing
    for indexed_ptr in (None, 16):
        assert lib.rl8_gather_minibatch(indexed_ptr, 12, 3, _fields(ok + [(4, 2, 0, 0, 20, 4)]), 2, None) == -4
        assert lib.rl8_gather_minibatch(indexed_ptr, 12, 3, null_dst, 2, None) == -1
    assert lib.rl8_gather_minibatch(None, 13, 3, _fields(ok), 1, None) == -2


# --------------------------------------------------------------------------- #
# pack_samples / the tiled index = NULL path
# --------------------------------------------------------------------------- #
def _inline_pack(n, h, rw):
    per_step = PACK_ENVS * (rw + 1) * 4
    tile_steps = min(max(_ceil_div(TILE_KIB * 1024, per_step), 1), PACK_STEPS)
    tile_steps = min(tile_steps, h)
    tiles = _ceil_div(n, PACK_ENVS) * _ceil_div(h, tile_steps)
    lds = tile_steps * per_step
    per_cu = max(LDS_CU // (lds + 512), 1)
    return tile_steps, lds, tiles, min(tiles, per_cu * CUS)


def test_pack_plan_matches_the_inline_launch_it_replaced():
    modes = set()
    for rw in range(4, 33, 4):
        full = _inline_pack(1, 1000, rw)[0]
        for n in (1, 63, 64, 65, 1000, 64 * 192 + 1, 64 * 200 + 1, 1 << 20):
            for h in (1, 2, full - 1, full, full + 1, 20, 32, 33, 128):
                p = hip.pack_plan(n, h, rw)
                assert tuple(p) == _inline_pack(n, h, rw), (n, h, rw)
                assert 1 <= p.tile_steps <= min(h, PACK_STEPS)
                assert p.lds_bytes == p.tile_steps * PACK_ENVS * (rw + 1) * 4 <= LDS_CU - 1024   # static LDS beside it
                assert 1 <= p.grid <= p.tiles == _ceil_div(n, PACK_ENVS) * _ceil_div(h, p.tile_steps)
                modes.add(p.tiles > p.grid)
    assert modes == {False, True}   # a tile per workgroup, and workgroups that loop over tiles


def test_pack_plan_argument_checks_need_no_device():
    lib, p = hip.load(), hip.PackPlanStruct()
    assert lib.rl8_pack_plan(8, 4, 8, None) == -1
    for bad in ((0, 4, 8), (8, 0, 8), (8, 4, 0), (8, 4, 6), (8, 4, 36), (8, 4, -4)):
        assert lib.rl8_pack_plan(*bad, C.byref(p)) == -2, bad
    with pytest.raises(ValueError):
        hip.pack_plan(8, 4, 36)
    fields = _fields([(3, 4, 0, 0, 15, 3)])
    assert lib.rl8_pack_samples(fields, 1, 8, 4, None, 4, None) == -1
    assert lib.rl8_pack_samples(fields, 1, 8, 4, 32, 0, None) == -2       # fewer row words than the fields hold
    assert lib.rl8_pack_samples(fields, 1, 8, 4, 32, 36, None) == -2
    assert lib.rl8_pack_samples(fields, 1, 8, 4, 36, 4, None) == -3       # packed rows not 16-byte aligned
    assert lib.rl8_gather_packed(None, 8, 32, 4, fields, 1, None) == -1
    assert lib.rl8_gather_packed(16, 8, 32, 40, fields, 1, None) == -2
