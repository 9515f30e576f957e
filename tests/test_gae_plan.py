"""The GAE scan's launch plan (``rl8_gae_plan``) and the normalise route (``rl8_advantage_normalise_route``) on the
CPU: host arithmetic of the library, swept over shapes, layouts and alignments. Every plan is held to what the kernels
of ``rl8_amd/csrc/gae_kernels.hip`` rely on -- each bound below is read off the kernel it protects, not off the plan --
and to the dispatch as it stood while ``rl8_gae_scan_f32`` decided inline. (The ``RL8_GAE_*`` tuning variables are read
once per process and are not part of this table: the sweep describes the defaults.)"""

from __future__ import annotations

import ctypes as C

from rl8_amd import hip

ENV, TIME = hip.LAYOUT_ENV_MAJOR, hip.LAYOUT_TIME_MAJOR

# constants of rl8_amd/csrc/common.hip.h and gae_kernels.hip
WAVE, BLOCK, CUS, MAX_GRID = 64, 256, 256, 2048
KMAX = 9                    # gae_scan_env_major_pipelined_kernel<9>: sixteen-byte pieces a lane holds per array
LDS_OPT_IN = 160 * 1024     # allow_dynamic_lds(..., 160 * 1024)

LARGE_N = (511, 512, 513, 1000, 4096, 65535, 65536, 65537, 65536 + 129, 2 * 65536 + 3, 262144, 393413, 524287, 524288,
           524289, 524288 + 4, 1 << 20, (1 << 20) + 1, 1 << 21, (1 << 21) + 5)
ALL_N = tuple(range(1, 301)) + LARGE_N
ALL_H = tuple(range(1, 601))


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _grid_for(items: int, per_block: int, cap: int = MAX_GRID) -> int:
    return min(max(_ceil_div(items, per_block), 1), cap)


def _inline_dispatch(n: int, h: int, layout: int, aligned: bool) -> tuple:
    """The body of ``rl8_gae_scan_f32`` before the plan existed, clause for clause: (route, envs per block or None,
    chunk, LDS stride, dynamic LDS bytes, grid)."""
    if layout == TIME:
        vec = n % 4 == 0 and aligned
        return ("TIME_VEC4" if vec else "TIME_VEC1", None, 0, 0, 0, _grid_for(n, BLOCK * (4 if vec else 1), 2 * CUS))
    cols = h + 1
    chunk = cols if cols < 127 else 127
    lds_stride = chunk | 1
    e = 73728 // (lds_stride * 8) // WAVE * WAVE
    e = min(e, 256)
    pipelined_shape = chunk == cols and cols & 1 == 1 and cols <= 36
    if pipelined_shape and e > 128:
        e = 128
    e = max(e, WAVE)
    lds_bytes = 2 * e * lds_stride * 4
    flat = chunk == cols and lds_stride == cols and e % 4 == 0 and aligned
    rows = _grid_for(n, e)
    if flat and pipelined_shape:
        per_cu = max(min(LDS_OPT_IN // (lds_bytes + 16 + 1024), 2), 1)
        return "ENV_PIPELINED", e, chunk, lds_stride, lds_bytes + 16, min(rows, CUS * per_cu)
    return "ENV_FLAT" if flat else "ENV_CHUNKED", e, chunk, lds_stride, lds_bytes, rows


def _inline_normalise(n: int, h: int, layout: int, aligned: bool) -> str:
    if layout == TIME:
        return "FLAT_VEC4" if (n * h) % 4 == 0 and aligned else "FLAT_VEC1"
    return "ENV_MAJOR"


def _sweep():
    lib, p = hip.load(), hip.GaePlanStruct()
    for layout in (ENV, TIME):
        for aligned in (True, False):
            for h in ALL_H:
                for n in ALL_N:
                    assert lib.rl8_gae_plan(n, h, layout, int(aligned), C.byref(p)) == 0
                    yield n, h, layout, aligned, p


def test_every_plan_keeps_what_its_kernel_relies_on():
    reached = set()
    for n, h, layout, aligned, p in _sweep():
        route, e, cols, where = hip.GAE_ROUTES[p.route], p.envs_per_block, h + 1, (n, h, layout, aligned)
        reached.add(route)
        assert 1 <= p.grid <= MAX_GRID, where        # one partial row per workgroup: RL8_MAX_PARTIALS of them
        if layout == TIME:
            assert route in ("TIME_VEC4", "TIME_VEC1"), where
            vec = 4 if route == "TIME_VEC4" else 1
            # float4 accesses at column starts t * n + e0: n and e0 multiples of 4, all bases aligned
            assert vec == 1 or (n % 4 == 0 and aligned), where
            assert e == BLOCK * vec and p.grid <= _ceil_div(n, e), where
            assert (p.chunk, p.lds_stride, p.lds_bytes) == (0, 0, 0), where
            continue
        assert route in ("ENV_PIPELINED", "ENV_FLAT", "ENV_CHUNKED"), where
        # one lane per env in whole waves; block_reduce and __launch_bounds__(256) hold up to four
        assert e % WAVE == 0 and WAVE <= e <= 256, where
        assert 1 <= p.chunk <= 127 and p.chunk <= cols, where
        # lanes walk columns of consecutive rows: an odd stride spreads them over the banks; rows hold a chunk
        assert p.lds_stride % 2 == 1 and p.lds_stride >= p.chunk, where
        tiles = 2 * e * p.lds_stride * 4
        assert tiles <= p.lds_bytes <= LDS_OPT_IN, where
        assert p.grid <= _ceil_div(n, e), where      # no workgroup without a tile
        if route == "ENV_CHUNKED":
            assert p.lds_bytes == tiles, where
            continue
        # both flat routes copy a tile as ONE run of e * (H+1) floats in 16-byte pieces: whole rows in one chunk, the
        # LDS row stride equal to the global one, every tile's base 16-byte aligned (e * (H+1) * 4 bytes apart)
        assert aligned and p.chunk == cols and p.lds_stride == cols and cols % 2 == 1, where
        assert e % 4 == 0, where
        if route == "ENV_FLAT":
            assert 37 <= cols <= 127 and p.lds_bytes == tiles, where
        else:
            # KMAX pieces per lane must cover a full tile; the last piece of a ragged tile is written to LDS whole
            # (up to 12 bytes past ne * cols floats, behind the second tile when ne == e): one vector more
            assert _ceil_div(e * cols, 4) <= KMAX * e and 3 <= cols <= 35, where
            assert p.lds_bytes == tiles + 16, where
            assert e * cols * 4 < 1 << 31, where     # a tile's buffer descriptor counts bytes in 32 bits
            # only resident workgroups (two per CU at most): a later round would start with nothing requested
            assert p.grid <= 2 * CUS and 2 * (p.lds_bytes + 1024) <= LDS_OPT_IN, where
    assert reached == set(hip.GAE_ROUTES)


def test_a_misaligned_call_never_gets_a_sixteen_byte_route():
    lib, p = hip.load(), hip.GaePlanStruct()
    for layout in (ENV, TIME):
        for h in ALL_H:
            for n in ALL_N:
                assert lib.rl8_gae_plan(n, h, layout, 0, C.byref(p)) == 0
                assert hip.GAE_ROUTES[p.route] in ("TIME_VEC1", "ENV_CHUNKED"), (n, h, layout)
                assert hip.advantage_normalise_route(n, h, layout, False) in ("FLAT_VEC1", "ENV_MAJOR"), (n, h, layout)


def test_plan_matches_the_inline_dispatch_it_replaced():
    scan_routes, norm_routes, rows = set(), set(), 0
    lib = hip.load()
    for n, h, layout, aligned, p in _sweep():
        route, e, chunk, lds_stride, lds_bytes, grid = _inline_dispatch(n, h, layout, aligned)
        got = (hip.GAE_ROUTES[p.route], p.envs_per_block if e is not None else None, p.chunk, p.lds_stride, p.lds_bytes,
               p.grid)
        assert got == (route, e, chunk, lds_stride, lds_bytes, grid), (n, h, layout, aligned)
        norm = hip.NORMALISE_ROUTES[lib.rl8_advantage_normalise_route(n, h, layout, int(aligned))]
        assert norm == _inline_normalise(n, h, layout, aligned), (n, h, layout, aligned)
        scan_routes.add(route)
        norm_routes.add(norm)
        rows += 1
    assert scan_routes == set(hip.GAE_ROUTES) and norm_routes == set(hip.NORMALISE_ROUTES)
    assert rows == len(ALL_N) * len(ALL_H) * 4


def test_route_boundaries_named_by_the_kernels():
    """The edges of the table, one by one: H+1 = 35 / 37 around the pipelined kernel's nine pieces per lane, 127 / 128
    around one chunk, and the grids at which the tile loops start to stride."""
    plan = hip.gae_plan
    assert [plan(1000, c - 1, ENV).route for c in (2, 3, 4, 35, 36, 37, 38, 127, 128, 129)] == [
        "ENV_CHUNKED", "ENV_PIPELINED", "ENV_CHUNKED", "ENV_PIPELINED", "ENV_CHUNKED", "ENV_FLAT", "ENV_CHUNKED",
        "ENV_FLAT", "ENV_CHUNKED", "ENV_CHUNKED"]
    assert [plan(1000, c - 1, ENV).envs_per_block for c in (3, 35, 37, 65, 127, 128, 401)] == [128, 128, 192, 128, 64, 64, 64]
    assert (plan(1, 126, ENV).chunk, plan(1, 127, ENV).chunk, plan(1, 400, ENV).chunk) == (127, 127, 127)
    assert plan(65536, 32, ENV).grid == 512 == plan(65536 + 129, 32, ENV).grid      # two workgroups per CU, then tiles queue
    assert plan(2048 * 192, 36, ENV).grid == 2048 == plan(2048 * 192 + 197, 36, ENV).grid
    assert plan(524288, 1, TIME).grid == 512 == plan(524288 + 4, 1, TIME).grid      # 2 per CU x 256 lanes x 4 envs
    assert plan(524288 + 1, 1, TIME) == hip.GaePlan("TIME_VEC1", 256, 0, 0, 0, 512)


def test_argument_checks_need_no_device():
    lib, p = hip.load(), hip.GaePlanStruct()
    assert lib.rl8_gae_plan(8, 4, 0, 1, None) == -1
    assert lib.rl8_gae_plan(0, 4, 0, 1, C.byref(p)) == -2 and lib.rl8_gae_plan(8, 0, 1, 1, C.byref(p)) == -2
    assert lib.rl8_gae_plan(8, 4, 2, 1, C.byref(p)) == -4
    assert lib.rl8_advantage_normalise_route(0, 4, 1, 1) == -2 and lib.rl8_advantage_normalise_route(8, 4, 2, 1) == -4
