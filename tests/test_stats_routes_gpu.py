"""Every launch route of the rollout statistics (``rl8_rollout_stats_f32``, ``rl8_amd/csrc/stats_gather_kernels.hip``) at
its boundaries, against numpy in fp64 over the same float32 data.

Each case names the route it is meant for and asserts that ``hip.rollout_stats_plan`` agrees. Rewards, rdr and the twelve
outputs live inside larger device buffers filled with a NaN bit pattern (compared as int32, so payloads count); the
padding between the columns of a padded slab holds the same pattern, so a load from it turns a sum into NaN. Every case
runs twice: the twelve outputs must be bit-identical, every guard word and every input word untouched.

Tolerances. Counts and extrema are exact. The per-env returns are accumulated in float32 in ascending t (as the C
oracle and ``torch.sum`` do), so they are exact too, and ``oracle.rollout_stats`` checks their extrema. The fp64 sums
are held to ``D * u`` (``u = 2^-53``) relative to ``sum |x|`` and ``sum x^2``, where ``D`` is the number of fp64
additions on the longest path from a term to the result, counted from the plan in ``depth`` below; the terms themselves
are exact in fp64 (a product of two 24-bit significands has 48 bits). The host's ``std = sqrt((S2 - S1^2/n)/(n-1))`` is
held to numpy's two-pass fp64 ``std(ddof=1)`` within ``2 * D * u * (1 + mean^2/var)``: with both sums inside ``D * u``,
``S1^2/n`` is off by at most ``2 D u S2`` (Cauchy-Schwarz), the difference by ``3 D u S2`` plus the host's three
roundings, and ``S2 / ((n-1) var) = 1 + mean^2/var`` up to ``1/n``; halved by the square root. No measured number is
involved."""

from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle  # noqa: E402  (checker only)

from rl8_amd import hip  # noqa: E402
from rl8_amd.algorithms._feedforward import _collect_stats_from_raw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload no kernel produces
GUARD = 64             # words of guard on each side, at least
ALIGNED, MISALIGNED = 64, 65  # word offsets of the view into its buffer: 256 bytes, 260 bytes
U = 2.0 ** -53
WAVE, BLOCK = 64, 256
HORIZONS = (1, 7, 8, 9, 16, 17)  # around the 8-step load batch (kStatsBatch)


class Guarded:
    """``cells`` 4-byte words at word offset ``offset`` of a sentinel-filled device buffer."""

    def __init__(self, cells: int, offset: int, bits: None | np.ndarray = None) -> None:
        self.cells, self.offset = cells, offset
        self.bits = torch.full((offset + cells + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.bits[offset:offset + cells]
        assert self.view.data_ptr() % 16 == (offset * 4) % 16
        self.want = None
        if bits is not None:
            self.want = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).reshape(-1)).to(DEV)
            self.view.copy_(self.want)

    def ptr(self) -> int:
        return self.view.data_ptr()

    def guards_untouched(self) -> bool:
        lo, hi = self.bits[:self.offset], self.bits[self.offset + self.cells:]
        assert lo.numel() >= GUARD and hi.numel() >= GUARD
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())

    def unchanged(self) -> bool:
        return bool((self.view == self.want).all())


def strides(kind: str, n: int, h: int) -> tuple[int, int, int]:
    """(env_stride, time_stride, words of the slab) of a [N, H+1] leaf."""
    if kind == "env":
        return h + 1, 1, n * (h + 1)
    pad = {"time": 0, "time_pad1": 1, "time_pad2": 2, "time_pad4": 4}[kind]
    return 1, n + pad, h * (n + pad) + n


def slab(a: np.ndarray, kind: str) -> np.ndarray:
    """[N, H+1] float32 as the int32 words of its slab, the sentinel in the padding."""
    n, h = a.shape[0], a.shape[1] - 1
    es, ts, cells = strides(kind, n, h)
    flat = np.full(cells, SENTINEL, np.int32)
    flat[(np.arange(n)[:, None] * es + np.arange(h + 1)[None, :] * ts).reshape(-1)] = a.view(np.int32).reshape(-1)
    return flat


def depth(plan: hip.StatsPlan, per_env_terms: int) -> int:
    """fp64 additions on the longest path of a sum, read off ``rollout_stats_kernel``: a lane adds ``per_env_terms``
    terms for each of its ``trips * VEC`` envs into one accumulator; ``block_reduce`` folds 64 lanes in 6 shuffle steps
    and then the block's 4 waves in 3 additions; the last block's thread t adds rows t, t + 256, ... and one more
    ``block_reduce`` follows."""
    vec = 4 if plan.route == "STATS_VEC4" else 1
    block_fold = int(math.log2(WAVE)) + (BLOCK // WAVE - 1)
    return plan.trips * vec * per_env_terms + block_fold + -(-plan.grid // BLOCK) + block_fold


def reference(r: np.ndarray, d: None | np.ndarray) -> dict:
    """Exactly rounded sums (``math.fsum``), exact extrema, the float32 returns in ascending t. ``r``, ``d``: [N, H+1]."""
    n, h = r.shape[0], r.shape[1] - 1
    ret = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(h):
            ret = ret + r[:, t]

    def moments(x):
        x = x.astype(np.float64).reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            if np.isfinite(x).all():
                return math.fsum(x), math.fsum(x * x), math.fsum(np.abs(x))
            return float(np.sum(x)), float(np.sum(x * x)), float("nan")   # IEEE: inf, or NaN from inf - inf / a NaN

    with np.errstate(invalid="ignore"):
        out = {"ret": moments(ret), "ret_min": float(np.min(ret)), "ret_max": float(np.max(ret)),
               "r": moments(r[:, :h]), "r_min": float(np.min(r[:, :h])), "r_max": float(np.max(r[:, :h])),
               "rdr": moments(d[:, 1:]) if d is not None else None, "ret_values": ret}
    return out


def same(got: float, want: float) -> bool:
    return (math.isnan(got) and math.isnan(want)) or got == want


def check_sum(got_s, got_sq, want, d, where):
    s, sq, abs_s = want
    if math.isfinite(s) and math.isfinite(sq):
        assert abs(got_s - s) <= d * U * abs_s, (got_s, s, d, where)
        assert abs(got_sq - sq) <= d * U * sq, (got_sq, sq, d, where)
    else:
        assert same(got_s, s) and same(got_sq, sq), (got_s, s, got_sq, sq, where)


def std_band(x: np.ndarray, d: int) -> tuple[float, float]:
    """numpy's two-pass fp64 ``std(ddof=1)`` of ``x`` and the relative band the raw-moment form is held to."""
    x = x.astype(np.float64).reshape(-1)
    mean, var = x.mean(), x.var(ddof=1)
    return math.sqrt(var), 2.0 * d * U * (1.0 + mean * mean / var)


def check_host_stats(raw, r, rdr, d_ret, d_r, where):
    """What ``collect()`` reports from the twelve raw numbers, against two passes in fp64."""
    n, h = r.shape[0], r.shape[1] - 1
    stats, scale = _collect_stats_from_raw([float(v) for v in raw])
    ret = reference(r, None)["ret_values"]
    for key, x, d in (("returns/std", ret, d_ret), ("rewards/std", r[:, :h], d_r)) + (
            (("scale", rdr[:, 1:], d_r),) if rdr is not None else ()):
        got = scale if key == "scale" else stats[key]
        if x.size < 2:
            assert math.isnan(got), (key, got, where)   # one sample: 0/0, as the reference's unbiased std
            continue
        want, band = std_band(x, d)
        assert want > 0.0, (key, where)
        print(f"{where} {key}: got {got!r} want {want!r} rel {abs(got - want) / want:.3e} band {band:.3e} D {d}")
        assert abs(got - want) <= band * want, (key, got, want, band, where)
    assert stats["returns/mean"] == raw[1] / n and stats["rewards/mean"] == raw[6] / (n * h)


def run_case(r: np.ndarray, rdr: None | np.ndarray, kind: str, offset: int, route: str, finite: bool = True):
    """One shape through the C ABI inside guarded buffers, twice; everything above checked. Returns (raw, plan)."""
    n, h = r.shape[0], r.shape[1] - 1
    es, ts, cells = strides(kind, n, h)
    gr = Guarded(cells, offset, slab(r, kind))
    gd = Guarded(cells, offset, slab(rdr, kind)) if rdr is not None else None
    out = Guarded(24, ALIGNED)
    aligned = gr.ptr() % 16 == 0 and (gd is None or gd.ptr() % 16 == 0)
    assert aligned == (offset == ALIGNED)
    plan = hip.rollout_stats_plan(n, h, es, ts, aligned)
    where = (n, h, kind, offset, rdr is not None, plan)
    assert plan.route == route, where
    lib, scratch = hip.load(), hip.scratch(torch.device(DEV))
    runs = []
    for _ in range(2):
        out.view.fill_(SENTINEL)
        st = lib.rl8_rollout_stats_f32(gr.ptr(), gd.ptr() if gd is not None else None, n, h, es, ts, out.ptr(),
                                       scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, (st, where)
        torch.cuda.synchronize()
        runs.append(out.view.cpu().numpy().copy())
        for name, g in (("rewards", gr), ("rdr", gd), ("out", out)):
            assert g is None or g.guards_untouched(), (name, where)
        assert gr.unchanged() and (gd is None or gd.unchanged()), where
    assert runs[0].tobytes() == runs[1].tobytes(), where
    raw = runs[0].view(np.float64)
    want = reference(r, rdr)
    d_ret, d_r = depth(plan, 1), depth(plan, h)
    assert raw[0] == n and raw[5] == n * h, where
    check_sum(raw[1], raw[2], want["ret"], d_ret, where + ("returns",))
    check_sum(raw[6], raw[7], want["r"], d_r, where + ("rewards",))
    for i, key in ((3, "ret_min"), (4, "ret_max"), (8, "r_min"), (9, "r_max")):
        assert same(raw[i], want[key]), (key, raw[i], want[key], where)
    if rdr is not None:
        check_sum(raw[10], raw[11], want["rdr"], d_r, where + ("rdr",))
    else:
        assert raw[10] == 0.0 and raw[11] == 0.0, where
    if finite:
        check_host_stats(raw, r, rdr, d_ret, d_r, where)
        if n * h <= 1 << 16:  # the C oracle on the same rollout: the float32 returns and their extrema, its own two passes
            o = oracle.rollout_stats(r[:, :, None], rdr[:, :, None] if rdr is not None else None)
            assert same(o["returns/min"], raw[3]) and same(o["returns/max"], raw[4]), where
            assert o["rewards/min"] == raw[8] and o["rewards/max"] == raw[9], where
    return raw, plan


def inputs(n: int, h: int, seed: int, mean: float = 0.0, std: float = 1.0):
    rng = np.random.default_rng(seed)
    r = (mean + std * rng.standard_normal((n, h + 1))).astype(np.float32)
    d = (mean + std * rng.standard_normal((n, h + 1))).astype(np.float32)
    return r, d


def sweep_horizons(n: int, kind: str, offset: int, route: str):
    for h in HORIZONS:
        r, d = inputs(n, h, 1000 * n + h, mean=0.5, std=2.0)
        for rdr in (d, None):
            run_case(r, rdr, kind, offset, route)


# --------------------------------------------------------------------------- #
# routes x horizons x envs, with and without rdr
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8, 1024, 1028])
def test_time_major_four_envs_per_lane(n):
    sweep_horizons(n, "time", ALIGNED, "STATS_VEC4")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5, 1023])
def test_time_major_env_count_not_a_multiple_of_four(n):
    """One env per lane. At n = 1 the unbiased std of the returns is 0/0 on the host, as the reference's; at
    n * h = 1 that of the rewards too."""
    sweep_horizons(n, "time", ALIGNED, "STATS_VEC1")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 1024, 1028])
def test_time_major_view_one_float_into_its_slab(n):
    assert hip.rollout_stats_plan(n, 8, 1, n, True).route == "STATS_VEC4"
    sweep_horizons(n, "time", MISALIGNED, "STATS_VEC1")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("time_pad1", "STATS_VEC1"), ("time_pad2", "STATS_VEC1"), ("time_pad4", "STATS_VEC4")])
@pytest.mark.parametrize("n", [8, 1028])
def test_time_major_padded_columns(n, kind, route):
    """A time stride that is no multiple of 4 takes the one-env kernel; one that is keeps the 16-byte loads and must
    step over the padding (which holds NaNs)."""
    sweep_horizons(n, kind, ALIGNED, route)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [ALIGNED, MISALIGNED])
@pytest.mark.parametrize("n", [1, 4, 8, 1023, 1024, 1028])
def test_env_major(n, offset):
    sweep_horizons(n, "env", offset, "STATS_VEC1")


# --------------------------------------------------------------------------- #
# grid-stride trips
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["time", "env"])
def test_one_env_per_lane_takes_a_second_trip(kind):
    n, h = 2048 * 256 + 3, 2
    r, d = inputs(n, h, 5)
    _, plan = run_case(r, d, kind, ALIGNED, "STATS_VEC1")
    assert plan == hip.StatsPlan("STATS_VEC1", 2048, 2)


VEC4_TRIP_SHAPES = (4 * 256 * 2 + 4, 4 * 256 * 3)


def child_main(cap: int) -> None:
    """Runs in a child process with RL8_STATS_GRID_CAP = cap (the library reads it once per process)."""
    for n in VEC4_TRIP_SHAPES:
        for h in (8, 9):
            r, d = inputs(n, h, 31 * n + h, mean=0.5, std=2.0)
            for rdr in (d, None):
                _, plan = run_case(r, rdr, "time", ALIGNED, "STATS_VEC4")
                assert plan.grid == cap and plan.trips == -(-n // (cap * BLOCK * 4)), plan
        print("TRIPS", n, plan.grid, plan.trips)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 2])
def test_four_envs_per_lane_takes_further_trips_under_a_capped_grid(cap):
    """A lane's second and third group of four envs, a last trip that only lane 0 takes (n = 2 * 1024 + 4), and partial
    rows of one or two workgroups in the last block's fold."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_stats_routes_gpu as t; t.child_main({cap})")
    env = dict(os.environ, RL8_STATS_GRID_CAP=str(cap))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    trips = [tuple(int(v) for v in line.split()[1:]) for line in res.stdout.splitlines() if line.startswith("TRIPS")]
    want = {1: [(2052, 1, 3), (3072, 1, 3)], 2: [(2052, 2, 2), (3072, 2, 2)]}[cap]
    assert trips == want, trips


# --------------------------------------------------------------------------- #
# accuracy of the raw-moment form, derived
# --------------------------------------------------------------------------- #
MOMENT_INPUTS = ((0.0, 1.0), (1e2, 1.0), (1e3, 1.0), (1e3, 1e-1), (-1e3, 1.0))
MOMENT_SHAPES = ((1024, 16, "time", "STATS_VEC4"), (1023, 17, "time", "STATS_VEC1"), (1024, 9, "env", "STATS_VEC1"))


@pytest.mark.parametrize("mean,std", MOMENT_INPUTS)
def test_numpy_alone_stays_inside_the_derived_bands(mean, std):
    """No GPU: raw moments summed by numpy in fp64 (pairwise, fewer additions per term than the kernel's ``D``), through
    the host's formula, against two passes. If this failed the band would be wrong, not the kernel."""
    for n, h, kind, route in MOMENT_SHAPES:
        r, d = inputs(n, h, 7, mean, std)
        es, ts, _ = strides(kind, n, h)
        plan = hip.rollout_stats_plan(n, h, es, ts, True)
        assert plan.route == route
        ret = reference(r, None)["ret_values"].astype(np.float64)
        x, y = r[:, :h].astype(np.float64), d[:, 1:].astype(np.float64)
        raw = [n, ret.sum(), (ret * ret).sum(), ret.min(), ret.max(), n * h, x.sum(), (x * x).sum(), x.min(), x.max(),
               y.sum(), (y * y).sum()]
        want = reference(r, d)
        check_sum(raw[1], raw[2], want["ret"], depth(plan, 1), (mean, std, n, h))
        check_sum(raw[6], raw[7], want["r"], depth(plan, h), (mean, std, n, h))
        check_host_stats(raw, r, d, depth(plan, 1), depth(plan, h), (mean, std, n, h, kind))


def test_a_float32_accumulator_or_square_would_leave_the_band():
    """No GPU: the same data with the squares formed, or the sums taken, in float32 misses the bands by orders of
    magnitude, so a kernel that did either cannot pass the test below."""
    n, h = 1024, 16
    r, _ = inputs(n, h, 7, 1e3, 1.0)
    plan = hip.rollout_stats_plan(n, h, 1, n, True)
    x = r[:, :h].reshape(-1)
    want, band = std_band(x, depth(plan, h))
    x64 = x.astype(np.float64)
    sq32 = (x * x).astype(np.float64).sum()                  # fp32 square, fp64 sums
    acc32 = float(np.cumsum(x * x, dtype=np.float32)[-1])    # fp32 accumulator
    for s2 in (sq32, acc32):
        got = _collect_stats_from_raw([n, 0, 0, 0, 0, n * h, x64.sum(), s2, 0, 0, 0, 0])[0]["rewards/std"]
        assert abs(got - want) > 100 * band * want, (got, want, band)


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,kind,route", MOMENT_SHAPES)
@pytest.mark.parametrize("mean,std", MOMENT_INPUTS)
def test_ill_conditioned_moments(mean, std, n, h, kind, route):
    r, d = inputs(n, h, 7, mean, std)
    run_case(r, d, kind, ALIGNED, route)


# --------------------------------------------------------------------------- #
# rewards that are not finite
# --------------------------------------------------------------------------- #
def _non_finite(case: str, n: int, h: int):
    r, d = inputs(n, h, 13, mean=0.5, std=2.0)
    if case == "inf":
        r[n // 2, h // 2] = np.inf
    elif case == "inf and -inf":
        r[1, 0], r[n - 2, h - 1] = np.inf, -np.inf
    elif case == "nan":
        r[n - 1, h - 1] = np.nan
    elif case == "nan in rdr":
        d[n // 3, h] = np.nan
    return r, d


@pytest.mark.parametrize("case", ["inf", "inf and -inf", "nan", "nan in rdr", "finite"])
def test_oracle_extrema_follow_the_reference(case):
    """No GPU: the C oracle's min / max against numpy's (which keep a NaN, as ``torch.min`` / ``torch.max`` do), with
    the odd element first, in the middle and last of the scan; its means and stds follow IEEE 754."""
    for n, h in ((7, 5), (1, 4), (64, 1)):
        r, d = _non_finite(case, n, h) if n > 2 and h > 1 else inputs(n, h, 3)
        if case == "nan":
            for e, t in ((0, 0), (n // 2, h // 2), (n - 1, h - 1)):
                r2 = inputs(n, h, 13)[0]
                r2[e, t] = np.nan
                o = oracle.rollout_stats(r2[:, :, None], d[:, :, None])
                assert all(math.isnan(o[k]) for k in oracle.STAT_KEYS[:8]) and math.isfinite(o["reward_scale"]), (e, t, o)
        want = reference(r, d)
        o = oracle.rollout_stats(r[:, :, None], d[:, :, None])
        for key, ref in (("returns/min", "ret_min"), ("returns/max", "ret_max"), ("rewards/min", "r_min"),
                         ("rewards/max", "r_max")):
            assert same(o[key], want[ref]), (case, n, h, key, o[key], want[ref])
        assert math.isnan(o["rewards/mean"]) == math.isnan(want["r"][0]), (case, n, h)
        assert math.isnan(o["reward_scale"]) == (case == "nan in rdr" and n > 2 and h > 1), (case, n, h)


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,kind,route", [(1024, 9, "time", "STATS_VEC4"), (1023, 9, "time", "STATS_VEC1"),
                                            (1024, 9, "env", "STATS_VEC1"), (2052, 3, "time", "STATS_VEC4")])
@pytest.mark.parametrize("case", ["inf", "inf and -inf", "nan", "nan in rdr"])
def test_non_finite_rewards_follow_the_reference(case, n, h, kind, route):
    """Sums follow IEEE 754, min / max of a set that holds a NaN are NaN (``torch.min`` / ``torch.max``), infinities are
    ordinary extrema -- in every lane, wave, block and last-block fold: the odd element sits in the first, a middle
    and the last env, so it reaches the result through different lanes and workgroups."""
    r, d = _non_finite(case, n, h)
    raw, _ = run_case(r, d, kind, ALIGNED, route, finite=False)
    stats, scale = _collect_stats_from_raw([float(v) for v in raw])
    o = oracle.rollout_stats(r[:, :, None], d[:, :, None])
    for key in ("returns/min", "returns/max", "rewards/min", "rewards/max"):
        assert same(stats[key], o[key]), (key, stats[key], o[key])
    if case == "inf":
        assert stats["rewards/max"] == math.inf == stats["returns/max"] and math.isfinite(stats["rewards/min"])
        assert stats["rewards/mean"] == math.inf and math.isnan(stats["rewards/std"]) and math.isfinite(scale)
    elif case == "inf and -inf":
        assert (stats["rewards/min"], stats["rewards/max"]) == (-math.inf, math.inf)
        assert (stats["returns/min"], stats["returns/max"]) == (-math.inf, math.inf)
        assert math.isnan(stats["rewards/mean"]) and math.isnan(stats["returns/mean"])
    elif case == "nan":
        assert all(math.isnan(stats[k]) for k in stats) and math.isfinite(scale)
    else:
        assert all(math.isfinite(stats[k]) for k in stats) and math.isnan(scale)
        clean, _ = run_case(r, None, kind, ALIGNED, route)
        assert raw[:10].tobytes() == clean[:10].tobytes()   # the rewards' statistics do not see rdr
