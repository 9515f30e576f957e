"""Every launch route of the GAE scan and of the advantage normalisation (``rl8_amd/csrc/gae_kernels.hip``) at its
boundaries: bit for bit against the C oracle, inside guarded buffers, through aligned and misaligned views, twice.

Each case names the route it is meant for and asserts that ``hip.gae_plan`` agrees, so a shape that moves to another
route fails instead of passing for the wrong reason. All four arrays live inside larger device buffers filled with a
NaN bit pattern (compared as int32, so payloads count): a store past either end of ``rewards``, ``adv`` or ``ret``,
or any store to ``values``, fails the case.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle  # noqa: E402  (checker only)

from rl8_amd import hip  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.nn import generalized_advantage_estimate  # noqa: E402
from rl8_amd.nn.functional import gae_launch  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402

DEV = "cuda:0"
ENV, TIME = hip.LAYOUT_ENV_MAJOR, hip.LAYOUT_TIME_MAJOR
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload no kernel produces
GUARD = 64             # floats of guard on each side, at least
ALIGNED, MISALIGNED = 64, 65  # float offsets of the view into its buffer: 256 bytes, 260 bytes
GAMMA, LAMBDA, SCALE = 0.95, 0.9, 41.5
EPS53 = 2.0 ** -53


class Guarded:
    """``cells`` floats at float offset ``offset`` of a sentinel-filled device buffer."""

    def __init__(self, cells: int, offset: int, fill: None | np.ndarray = None) -> None:
        self.cells, self.offset = cells, offset
        self.bits = torch.full((offset + cells + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.bits.view(torch.float32)[offset:offset + cells]
        assert self.view.data_ptr() % 16 == (offset * 4) % 16
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))

    def guards_untouched(self) -> bool:
        lo, hi = self.bits[:self.offset], self.bits[self.offset + self.cells:]
        assert lo.numel() >= GUARD and hi.numel() >= GUARD
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())

    def same_bits(self, want: np.ndarray) -> bool:
        """Bit for bit; where the oracle holds a NaN (0/0, whose sign and payload IEEE 754 leaves to the machine: x86
        sets the sign bit) any NaN but the sentinel will do."""
        want = torch.from_numpy(np.ascontiguousarray(want, np.float32).reshape(-1)).to(DEV)
        got = self.view
        same = got.view(torch.int32) == want.view(torch.int32)
        return bool((same | (want.isnan() & got.isnan() & (got.view(torch.int32) != SENTINEL))).all())

    def host(self) -> np.ndarray:
        return self.view.cpu().numpy()


def _inputs(n: int, h: int, seed: int):
    rng = np.random.default_rng(seed)
    rewards = -np.abs(rng.uniform(-100, 100, (n, h + 1, 1))).astype(np.float32)
    values = rng.standard_normal((n, h + 1, 1)).astype(np.float32)
    return rewards, values


def _arranged(a: np.ndarray, layout: int) -> np.ndarray:
    """env-major [N, H+1, 1] as the flat array the layout stores."""
    a = a.reshape(a.shape[0], a.shape[1])
    return np.ascontiguousarray(a.T if layout == TIME else a).reshape(-1)


def launch(rewards, values, *, layout, offset, write_back, route, norm_route=None, gamma=GAMMA, lam=LAMBDA, scale=SCALE,
           norm=True):
    """One scan (+ normalise) inside guarded buffers. Returns the four buffers and the scan's moments (host)."""
    n, h = rewards.shape[0], rewards.shape[1] - 1
    cells = n * (h + 1)
    r = Guarded(cells, offset, _arranged(rewards, layout))
    v = Guarded(cells, offset, _arranged(values, layout))
    adv, ret = Guarded(cells, offset), Guarded(cells, offset)
    aligned = all(g.view.data_ptr() % 16 == 0 for g in (r, v, adv, ret))
    assert aligned == (offset == ALIGNED)
    plan = hip.gae_plan(n, h, layout, aligned)
    assert plan.route == route, (plan, n, h, layout, offset)
    if norm_route is not None:
        assert hip.advantage_normalise_route(n, h, layout, aligned) == norm_route
    moments = hip.gae_scan(
        r.view, v.view, adv.view, ret.view, layout=layout, n=n, h=h, gamma=float(np.float32(gamma)),
        gamma_lambda=float(np.float32(gamma * lam)), reward_denominator=float(np.float32(scale + 1e-8)),
        write_scaled_rewards=write_back,
    )
    scan_moments = moments.clone()
    if norm:
        hip.advantage_normalise(adv.view, layout=layout, n=n, h=h, moments=moments)
    torch.cuda.synchronize()
    return r, v, adv, ret, scan_moments.cpu().numpy(), plan


def check_case(n, h, layout, offset, route, norm_route=None, seed=None):
    """The case three times: twice writing the scaled rewards back (identical bits, moments included), once without
    (rewards untouched, everything else the same). Every run: outputs bit-equal to the oracle on all H+1 columns,
    ``values`` bit-identical, every guard word of the four buffers untouched."""
    rewards, values = _inputs(n, h, seed if seed is not None else n * 1000 + h)
    want = oracle.gae(rewards, values, gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=True)
    raw = oracle.gae(rewards, values, gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=False)
    assert not want["advantages"][:, h].any() and np.array_equal(want["returns"][:, h], values[:, h])
    first = None
    for write_back in (True, True, False):
        r, v, adv, ret, moments, plan = launch(rewards, values, layout=layout, offset=offset, write_back=write_back,
                                               route=route, norm_route=norm_route)
        where = (n, h, layout, offset, write_back, plan)
        for name, g in (("rewards", r), ("values", v), ("adv", adv), ("ret", ret)):
            assert g.guards_untouched(), (name, where)
        assert v.same_bits(_arranged(values, layout)), where
        assert r.same_bits(_arranged(want["scaled_rewards"] if write_back else rewards, layout)), where
        assert ret.same_bits(_arranged(want["returns"], layout)), where
        assert adv.same_bits(_arranged(want["advantages"], layout)), where
        assert moments[0] == n * h, where
        if first is None:
            first = moments
            if n * h <= 1 << 21:
                check_moments(moments, raw["advantages"], where)
        else:
            assert first.tobytes() == moments.tobytes(), where
    return plan


def check_moments(moments, raw_adv, where):
    """(count, sum, sum of squares) against exactly rounded sums of the oracle's un-normalised fp32 advantages. The
    terms are exact in fp64 (a product of two 24-bit significands has 48 bits), so all of the kernel's error is
    summation error, in any order at most that of a recursive sum: n * u * sum |term|, u = 2^-53."""
    a = raw_adv[:, :-1].astype(np.float64).reshape(-1)
    cnt = a.size
    want_s, want_sq, abs_s = math.fsum(a), math.fsum(a * a), math.fsum(np.abs(a))
    assert moments[0] == cnt, where
    assert abs(moments[1] - want_s) <= cnt * EPS53 * abs_s, (moments[1], want_s, where)
    assert abs(moments[2] - want_sq) <= cnt * EPS53 * want_sq, (moments[2], want_sq, where)


# --------------------------------------------------------------------------- #
# env-major, pipelined: odd H+1 in 3..35, tiles of 128 envs, at most 512 workgroups
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cols", [3, 5, 33, 35])
@pytest.mark.parametrize("n", [1, 3, 127, 128, 129, 131, 65536 + 129, 2 * 65536 + 3])
def test_pipelined_ragged_tiles(n, cols):
    """Last tiles whose float count is no multiple of 4 (a lane's last 16-byte piece reaches past the tile and the
    buffer range check must drop the excess), alone, behind full tiles, and as a workgroup's second and third tile."""
    plan = check_case(n, cols - 1, ENV, ALIGNED, "ENV_PIPELINED", "ENV_MAJOR")
    assert plan.envs_per_block == 128
    last = n % 128
    assert n in (128,) or (last * cols) % 4 != 0           # every other case ends ragged
    if n > 65536:
        assert plan.grid == 512 < -(-n // 128)              # some workgroup takes a further tile


# --------------------------------------------------------------------------- #
# env-major, flat: odd H+1 in 37..127
# --------------------------------------------------------------------------- #
def _flat_ns():
    for cols in (37, 65, 127):
        e = hip.gae_plan(1, cols - 1, ENV).envs_per_block
        for n in (1, 63, e, e + 1, 5 * e + 3):
            yield cols, n
    yield 37, 2048 * hip.gae_plan(1, 36, ENV).envs_per_block + 192 + 5  # more tiles than workgroups: the tile loop strides


@pytest.mark.parametrize("cols,n", list(_flat_ns()))
def test_flat_staging_groups_and_leftovers(cols, n):
    """The 4-deep staging loop, its partial last group and the `< 4 leftovers` loop: tiles of 1, 63, e and ragged
    envs give vector counts below, at and above 4 * e, and float counts of every residue modulo 4."""
    plan = check_case(n, cols - 1, ENV, ALIGNED, "ENV_FLAT", "ENV_MAJOR")
    assert plan.envs_per_block == {37: 192, 65: 128, 127: 64}[cols]
    if n > 2048 * plan.envs_per_block:
        assert plan.grid == 2048 < -(-n // plan.envs_per_block)


# --------------------------------------------------------------------------- #
# env-major, chunked: even H+1, H+1 > 127 (chunks of 127 columns), misaligned views
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cols", [2, 4, 34, 36, 128, 129, 254, 255, 401])
@pytest.mark.parametrize("n", [1, 65, 777])
def test_chunked_rows_and_chunk_boundaries(n, cols):
    """127 columns is the last single chunk; 128 leaves a second chunk of one column, 254 two full ones, 255 a third of
    one column; `prev` and `v_next` cross every boundary in registers."""
    plan = check_case(n, cols - 1, ENV, ALIGNED, "ENV_CHUNKED", "ENV_MAJOR")
    assert plan.chunk == min(cols, 127)


@pytest.mark.parametrize("cols", [33, 65])
@pytest.mark.parametrize("n", [65, 777])
def test_misaligned_env_major_falls_back_to_the_element_copy(n, cols):
    assert hip.gae_plan(n, cols - 1, ENV, True).route in ("ENV_PIPELINED", "ENV_FLAT")
    check_case(n, cols - 1, ENV, MISALIGNED, "ENV_CHUNKED", "ENV_MAJOR")


# --------------------------------------------------------------------------- #
# time-major: 4 envs per lane / 1 env per lane; the env loop strides above 512 workgroups
# --------------------------------------------------------------------------- #
def _time_cases():
    for h in (1, 32, 33):
        for n in (4, 1000):
            yield n, h, ALIGNED, "TIME_VEC4"
        for n in (1, 5, 777):
            yield n, h, ALIGNED, "TIME_VEC1"
        yield 1000, h, MISALIGNED, "TIME_VEC1"
    for h in (1, 5):  # (the largest sizes with few columns: a few million cells for the oracle)
        yield 524288 + 4, h, ALIGNED, "TIME_VEC4"
        yield 524288 + 1, h, ALIGNED, "TIME_VEC1"


@pytest.mark.parametrize("n,h,offset,route", list(_time_cases()))
def test_time_major_vector_widths_tails_and_strides(n, h, offset, route):
    norm_route = "FLAT_VEC4" if (n * h) % 4 == 0 and offset == ALIGNED else "FLAT_VEC1"
    plan = check_case(n, h, TIME, offset, route, norm_route)
    if n > 524288:
        assert plan.grid == 512 < -(-n // plan.envs_per_block)  # a second, partial round of the env loop


@pytest.mark.parametrize("n,h,layout,offset,norm_route", [
    (1000, 32, TIME, ALIGNED, "FLAT_VEC4"),        # N H a multiple of 4, aligned
    (4, 3, TIME, ALIGNED, "FLAT_VEC4"),
    (1001, 33, TIME, ALIGNED, "FLAT_VEC1"),        # N H not a multiple of 4
    (1000, 32, TIME, MISALIGNED, "FLAT_VEC1"),     # misaligned
    (2048 * 1024 // 32 + 4, 32, TIME, ALIGNED, "FLAT_VEC4"),  # more than 2048 x 256 x 4 cells: the grid strides
    (1000, 32, ENV, ALIGNED, "ENV_MAJOR"),
    (1000, 33, ENV, MISALIGNED, "ENV_MAJOR"),
])
def test_normalise_routes(n, h, layout, offset, norm_route):
    check_case(n, h, layout, offset, hip.gae_plan(n, h, layout, offset == ALIGNED).route, norm_route)


# --------------------------------------------------------------------------- #
# the moments an env-sharded run all-reduces, on every route
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,h,layout,offset,route", [
    (65536 + 129, 4, ENV, ALIGNED, "ENV_PIPELINED"),
    (4099, 32, ENV, ALIGNED, "ENV_PIPELINED"),
    (4099, 64, ENV, ALIGNED, "ENV_FLAT"),
    (4099, 64, ENV, MISALIGNED, "ENV_CHUNKED"),
    (777, 400, ENV, ALIGNED, "ENV_CHUNKED"),
    (65536, 32, TIME, ALIGNED, "TIME_VEC4"),
    (65537, 31, TIME, ALIGNED, "TIME_VEC1"),
])
def test_moments_on_every_route(n, h, layout, offset, route):
    rewards, values = _inputs(n, h, 17 * n + h)
    raw = oracle.gae(rewards, values, gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=False)
    *_, moments, plan = launch(rewards, values, layout=layout, offset=offset, write_back=True, route=route, norm=False)
    check_moments(moments, raw["advantages"], (n, h, layout, offset, plan))


# --------------------------------------------------------------------------- #
# conditioning of the one-pass variance
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("layout,route", [(ENV, "ENV_PIPELINED"), (TIME, "TIME_VEC4")])
@pytest.mark.parametrize("ratio", [1.0, 10.0, 1e2, 1e3, 1e4])
def test_one_pass_variance_conditioning(ratio, layout, route):
    """Advantages whose mean is ``ratio`` times their spread. With zero values, ``gae_lambda = 0`` and
    ``reward_scale = 1`` (the denominator rounds to 1.0f) the advantage IS the reward, so the ratio is set directly.

    ``norm_consts`` forms var = (sq - s * mean) / (cnt - 1) in fp64 from the three moments; the oracle and
    ``torch.std_mean`` take two passes. With s and sq each within cnt * u of exact (u = 2^-53, see ``check_moments``;
    s * mean = s^2 / cnt <= sq by Cauchy-Schwarz), the difference of the two is off by at most 2 * cnt * u * sq, so
    |var_got - var_want| <= 2 * cnt * u * sq / (cnt - 1). No measured number is involved.

    Where that bound, carried through sqrt and the cast, stays under half an fp32 ulp of the standard deviation, the
    normalised advantages must equal the oracle's bit for bit as well; beyond it the bound alone is required."""
    n, h = 4096, 32
    rng = np.random.default_rng(int(ratio) + layout)
    rewards = (-ratio + rng.standard_normal((n, h + 1, 1))).astype(np.float32)
    values = np.zeros_like(rewards)
    kw = dict(gamma=GAMMA, gae_lambda=0.0, reward_scale=1.0)
    raw = oracle.gae(rewards, values, normalize_advantages=False, **kw)
    want = oracle.gae(rewards, values, normalize_advantages=True, **kw)
    assert np.array_equal(raw["advantages"][:, :h], rewards[:, :h])
    a = raw["advantages"][:, :h].astype(np.float64).reshape(-1)
    cnt = a.size
    mean_want, var_want = a.mean(), a.var(ddof=1)  # two passes, fp64
    assert 0.5 * ratio <= abs(mean_want) / math.sqrt(var_want) <= 2.0 * ratio
    sq = math.fsum(a * a)
    bound = 2.0 * cnt * EPS53 * sq / (cnt - 1)
    sd_want = math.sqrt(var_want)
    sd_bound = math.sqrt(var_want + bound) - sd_want
    half_ulp = float(np.spacing(np.float32(sd_want))) / 2
    # the oracle alone, its fp32 result against fp64: inside the bound (plus the rounding of its own cast)
    assert abs(want["std"] - sd_want) <= sd_bound + half_ulp
    assert abs(want["mean"] - mean_want) <= float(np.spacing(np.float32(abs(mean_want)))) / 2 + EPS53 * math.fsum(np.abs(a))

    r, v, adv, ret, moments, plan = launch(rewards, values, layout=layout, offset=ALIGNED, write_back=True, route=route,
                                           gamma=GAMMA, lam=0.0, scale=1.0)
    c, s, q = (float(x) for x in moments)
    mean_got = s / c
    var_got = (q - s * mean_got) / (c - 1.0)  # as norm_consts
    print(f"ratio {ratio:g} layout {layout}: var_got {var_got!r} var_want {var_want!r} bound {bound:.3e}"
          f" sd_bound/half_ulp {sd_bound / half_ulp:.3e}")
    assert c == cnt
    assert abs(var_got - var_want) <= bound, (var_got, var_want, bound)
    assert ret.same_bits(_arranged(want["returns"], layout))
    if sd_bound < half_ulp:
        assert adv.same_bits(_arranged(want["advantages"], layout)), (ratio, sd_bound, half_ulp)
    else:  # the advantages follow from (mean, sd): hold sd to the carried bound, in fp32
        sd_got = float(np.float32(math.sqrt(max(var_got, 0.0))))
        assert abs(sd_got - sd_want) <= sd_bound + half_ulp


# --------------------------------------------------------------------------- #
# one sample
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("layout,route,norm_route", [(ENV, "ENV_CHUNKED", "ENV_MAJOR"), (TIME, "TIME_VEC1", "FLAT_VEC1")])
def test_one_sample_normalises_to_nan_as_the_reference(layout, route, norm_route):
    """N H = 1: the unbiased standard deviation of one element is 0/0. The oracle (and the reference's
    ``std_mean``) give a NaN advantage there; column H stays 0 and the returns are not normalised at all."""
    rewards, values = _inputs(1, 1, 11)
    want = oracle.gae(rewards, values, gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=True)
    assert np.isnan(want["advantages"][0, 0, 0]) and want["advantages"][0, 1, 0] == 0.0 and np.isnan(want["std"])
    r, v, adv, ret, moments, _ = launch(rewards, values, layout=layout, offset=ALIGNED, write_back=True, route=route,
                                        norm_route=norm_route)
    for g in (r, v, adv, ret):
        assert g.guards_untouched()
    got = adv.host()
    assert np.isnan(got[0]) and got[1] == 0.0, got
    assert ret.same_bits(_arranged(want["returns"], layout)) and r.same_bits(_arranged(want["scaled_rewards"], layout))
    assert moments[0] == 1.0


# --------------------------------------------------------------------------- #
# the public path
# --------------------------------------------------------------------------- #
def test_public_gae_on_an_env_sliced_batch():
    """``batch[1:]`` of an env-major batch with odd H+1 starts 4 * (H+1) bytes into the allocation: misaligned. It
    must match the oracle on the slice and leave row 0 of every leaf alone."""
    n, h = 300, 32
    rewards, values = _inputs(n, h, 3)
    full = TensorDict({DataKeys.REWARDS: torch.from_numpy(rewards).to(DEV), DataKeys.VALUES: torch.from_numpy(values).to(DEV)},
                      batch_size=[n, h + 1])
    batch = full[1:]
    assert batch[DataKeys.REWARDS].data_ptr() % 16 != 0 and batch[DataKeys.VALUES].data_ptr() % 16 != 0
    assert hip.buffer_layout(batch[DataKeys.REWARDS])[0] == ENV
    assert hip.gae_plan(n - 1, h, ENV, False).route == "ENV_CHUNKED" != hip.gae_plan(n - 1, h, ENV, True).route
    out = generalized_advantage_estimate(batch, gae_lambda=LAMBDA, gamma=GAMMA, reward_scale=SCALE)
    torch.cuda.synchronize()
    want = oracle.gae(rewards[1:], values[1:], gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=True)
    assert np.array_equal(out[DataKeys.ADVANTAGES].cpu().numpy(), want["advantages"])
    assert np.array_equal(out[DataKeys.RETURNS].cpu().numpy(), want["returns"])
    assert np.array_equal(full[DataKeys.REWARDS][1:].cpu().numpy(), want["scaled_rewards"])  # scaled in place, as the reference
    assert np.array_equal(full[DataKeys.REWARDS][0].cpu().numpy(), rewards[0])
    assert np.array_equal(full[DataKeys.VALUES].cpu().numpy(), values)


def test_time_major_batch_sliced_along_envs_is_refused_by_the_launch():
    """A time-major leaf sliced along envs is neither layout (its columns are no longer N apart): ``gae_launch`` raises
    the documented ``ValueError``, and the public function works on a dense copy instead."""
    n, h = 64, 8
    rewards, values = _inputs(n, h, 4)

    def time_major(a):
        return torch.from_numpy(a.reshape(n, h + 1).T.copy()).to(DEV).T.unsqueeze(-1)

    full = TensorDict({DataKeys.REWARDS: time_major(rewards), DataKeys.VALUES: time_major(values)}, batch_size=[n, h + 1])
    assert hip.buffer_layout(full[DataKeys.REWARDS])[0] == TIME
    batch = full[1:]
    r, v = batch[DataKeys.REWARDS], batch[DataKeys.VALUES]
    assert hip.buffer_layout(r)[0] < 0
    with pytest.raises(ValueError, match="env-major or time-major dense"):
        gae_launch(r, v, torch.empty_like(r), torch.empty_like(r), gae_lambda=LAMBDA, gamma=GAMMA, reward_scale=SCALE,
                   normalize_advantages=True, write_scaled_rewards=True)
    out = generalized_advantage_estimate(batch, gae_lambda=LAMBDA, gamma=GAMMA, reward_scale=SCALE)
    torch.cuda.synchronize()
    want = oracle.gae(rewards[1:], values[1:], gamma=GAMMA, gae_lambda=LAMBDA, reward_scale=SCALE, normalize_advantages=True)
    assert np.array_equal(out[DataKeys.ADVANTAGES].cpu().numpy(), want["advantages"])
    assert np.array_equal(out[DataKeys.RETURNS].cpu().numpy(), want["returns"])
    assert np.array_equal(full[DataKeys.VALUES].cpu().numpy(), values)
