"""The wave-per-row categorical kernels (rl8_amd/csrc/categorical_wide_kernels.hip) against fp64 torch and, at
k <= 64, against the lane-per-row kernels they stand beside.

Shapes: k around the 64-class chunks of a wave (63, 64, 65, 127, 128, 129), one register-held row of several chunks
(1000) and one that is read again (4099, above the 1024 classes kept in registers); a in {1, 2, 5}; m around the four
waves of a workgroup (1, 3, 4, 5) and 4099 (1025 workgroups, a last one with a single row).  One loss case runs in a
child process with RL8_LOSS_GRID_CAP=3, where a wave strides over ~340 rows, and one sampler case has more rows than
the grid has waves.

Yardsticks and bars
* sampler picks: fp64 ``argmax(softmax(z) / q)`` on the injected Exp(1) noise.  Wherever the fp64 top two ratios
  differ by more than 1e-4 relative -- 100x the fp32 rounding of p / q, which is a few 1e-7 -- the class must be
  the yardstick's; elsewhere one of the two; at most 0.5 % of a case's draws may fall under the gap.
* sampler logp: fp64 log-softmax at the picked classes, rtol 1e-5 / atol 1e-6 (tests/test_hip_kernels.py) on the
  rows of N(0, 1) logits.  The rows of five times that have an lse near 20, where one fp32 rounding is 9.5e-7: they
  are held to rtol 1e-5 plus twice what the lane-per-row kernel leaves on such rows at k = 64 (``check_logp``).
* loss: fp64 autograd of the reference expression; means at rel 1e-5 / abs 1e-7 (1e-6 under 16 samples), gradients
  entrywise at 2e-5 relative with a floor of 1e-6 of the tensor's largest entry, rows within 1e-5 of a clip boundary
  exempt and at most 8 (tests/test_ppo_loss_edges_gpu.py, whose ``assert_means`` is used as it is; ``assert_grad``
  is restated on the device because the largest case has 84 M entries).
"""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import oracle  # noqa: E402  (checker only: the Philox draws of a disputed row)

from rl8_amd import hip  # noqa: E402

from .test_ppo_loss_edges_gpu import GAS, HPS, assert_means  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.finfo(torch.float32)

KS = [2, 63, 64, 65, 127, 128, 129, 1000, 4099]
AS = [1, 2, 5]
MS = [1, 3, 4, 5, 4099]
GAP = 1e-4


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def seed_of(k, a, m):
    return k * 1000 + a * 100 + m % 97


def sampler_inputs(m, a, k, seed):
    """z ~ N(0, 1), every other row times 5; q ~ Exp(1)."""
    g = gen(seed)
    scale = torch.where((torch.arange(m, device=DEV) + k) % 2 == 0, 1.0, 5.0).reshape(m, 1, 1)
    z = (torch.randn(m, a, k, generator=g, device=DEV) * scale).contiguous()
    q = torch.empty(m, a, k, device=DEV).exponential_(1.0, generator=g)
    return z, q


def check_picks(actions, z, q):
    """The rule of the module docstring; returns the number of draws under the gap."""
    v = torch.softmax(z.double(), -1) / q.double()
    top, idx = v.topk(2, dim=-1)
    clear = (top[..., 0] - top[..., 1]) > GAP * top[..., 0]
    assert torch.equal(actions[clear], idx[..., 0][clear]), int((actions[clear] != idx[..., 0][clear]).sum())
    near = ~clear
    assert ((actions[near] == idx[..., 0][near]) | (actions[near] == idx[..., 1][near])).all()
    assert int(near.sum()) <= 0.005 * actions.numel(), (int(near.sum()), actions.numel())
    return int(near.sum())


def unit_rows(m, k):
    """The rows of ``sampler_inputs`` whose logits are N(0, 1) (the others are five times that)."""
    return (torch.arange(m, device=DEV) + k) % 2 == 0


def logp_excess(logp, actions, z):
    """Per row, the error of ``logp`` against fp64 beyond rtol 1e-5 of the fp64 value."""
    want = torch.log_softmax(z.double(), -1).gather(-1, actions.unsqueeze(-1)).squeeze(-1).sum(-1, keepdim=True)
    assert torch.isfinite(logp).all()
    return ((logp.double() - want).abs() - 1e-5 * want.abs()).reshape(-1)


@functools.lru_cache(maxsize=None)
def lane_kernel_excess(a):
    """What the lane-per-row sampler itself leaves beyond rtol 1e-5 on the x5 rows of the same inputs at k = 64,
    4099 rows: the rounding of lse = max + log(sum) in fp32, half an ulp of a number near 13."""
    z, q = sampler_inputs(4099, a, 64, 640 + a)
    actions, logp = hip.categorical_sample_logp(z, q)
    excess = float(logp_excess(logp, actions, z)[~unit_rows(4099, 64)].max())
    print(f"lane kernel, k = 64, a = {a}, x5 rows: logp error beyond rtol 1e-5: {excess:.3e}")
    return excess


def check_logp(logp, actions, z, unit=None):
    """rtol 1e-5 / atol 1e-6 (tests/test_hip_kernels.py) on every row in ``unit`` (all rows when None).  The other
    rows have logits of +-20 and an lse near 20, where one fp32 rounding of lse is 9.5e-7 by itself: they are held
    to rtol 1e-5 plus twice what the lane kernel leaves at k = 64 on inputs of the same kind (lse near 13, half
    the ulp), never less than 1e-6."""
    excess = logp_excess(logp, actions, z)
    if unit is None:
        unit = torch.ones_like(excess, dtype=torch.bool)
    assert (excess[unit] <= 1e-6).all(), float(excess[unit].max())
    if not unit.all():
        bar = max(1e-6, 2.0 * lane_kernel_excess(actions.shape[1]))
        worst = float(excess[~unit].max())
        print(f"wide kernel, k = {z.shape[-1]}, a = {actions.shape[1]}, x5 rows: {worst:.3e} (bar {bar:.3e})")
        assert worst <= bar, (worst, bar)


# --------------------------------------------------------------------------- #
# Sampler
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("k", KS)
def test_sampler_picks_and_logp_against_fp64(k, a, m):
    z, q = sampler_inputs(m, a, k, seed_of(k, a, m))
    actions, logp = hip.categorical_sample_logp_wide(z, q)
    assert actions.shape == (m, a) and actions.dtype == torch.int64 and logp.shape == (m, 1)
    assert ((actions >= 0) & (actions < k)).all()
    check_picks(actions, z, q)
    check_logp(logp, actions, z, unit_rows(m, k))
    again = hip.categorical_sample_logp_wide(z, q)
    assert torch.equal(again[0], actions) and torch.equal(again[1], logp)


def test_sampler_with_more_rows_than_the_grid_has_waves():
    """2048 workgroups of four waves: from row 8192 on a wave takes a second row."""
    m, a, k = 8192 + 5, 1, 65
    z, q = sampler_inputs(m, a, k, 7)
    actions, logp = hip.categorical_sample_logp_wide(z, q)
    check_picks(actions, z, q)
    check_logp(logp, actions, z, unit_rows(m, k))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("k", [2, 63, 64])
def test_sampler_agrees_with_the_lane_kernel_up_to_64_classes(k, a, m):
    """Same operations, sums in another order: on injected noise both kernels obey the fp64 rule, so they differ only
    under the gap; on Philox (same seed, step and row offset, hence the same draws) every draw they disagree on is
    looked up -- its Exp(1) values come from the oracle's Philox -- and must sit under the gap too."""
    z, q = sampler_inputs(m, a, k, seed_of(k, a, m) + 1)
    wide, wide_lp = hip.categorical_sample_logp_wide(z, q)
    lane, lane_lp = hip.categorical_sample_logp(z, q)
    check_picks(wide, z, q)
    check_picks(lane, z, q)
    check_logp(wide_lp, wide, z, unit_rows(m, k))
    addr = dict(seed=11, step=3, row_offset=1000)
    wide, wide_lp = hip.categorical_sample_logp_wide(z, None, **addr)
    lane, lane_lp = hip.categorical_sample_logp(z, None, **addr)
    differ = (wide != lane).nonzero().tolist()
    assert len(differ) <= 0.005 * wide.numel(), len(differ)
    for i, d in differ:
        qs = torch.tensor([oracle.exponential(addr["seed"], i + addr["row_offset"], addr["step"], d * k + j)
                           for j in range(k)], dtype=torch.float64, device=DEV)
        v = torch.softmax(z[i, d].double(), -1) / qs
        top, idx = v.topk(2)
        assert (top[0] - top[1]) <= GAP * top[0], (i, d)
        assert {int(wide[i, d]), int(lane[i, d])} <= set(idx.tolist()), (i, d)
    check_logp(wide_lp, wide, z, unit_rows(m, k))


@pytest.mark.parametrize("k", [65, 129, 1000, 4099])
def test_deterministic_mode_picks_the_first_maximum(k):
    m, a = 37, 2
    z, _ = sampler_inputs(m, a, k, k)
    want = z.argmax(-1)
    rows = torch.arange(m, device=DEV)
    # duplicated maxima: a second one 64 classes on (the same lane, the next chunk), a third in the last class
    first = torch.randint(0, k - 64, (m, a), generator=gen(k + 1), device=DEV)
    top = z.amax(-1) + 1.0
    for d in range(a):
        z[rows, d, first[:, d]] = top[:, d]
        z[rows, d, first[:, d] + 64] = top[:, d]
        z[rows, d, k - 1] = top[:, d]
    actions, logp = hip.categorical_sample_logp_wide(z, None, deterministic=True)
    assert torch.equal(actions, first) and not torch.equal(first, want)
    check_logp(logp, actions, z, unit_rows(m, k))
    # one maximum alone, wherever it is
    z2, _ = sampler_inputs(m, a, k, k + 2)
    actions, _ = hip.categorical_sample_logp_wide(z2, None, deterministic=True)
    assert torch.equal(actions, z2.argmax(-1))
    # noise is not read in deterministic mode
    assert torch.equal(hip.categorical_sample_logp_wide(z2, torch.rand_like(z2), deterministic=True)[0], actions)


@pytest.mark.parametrize("k", [65, 100, 1000, 4099])
def test_masked_classes_are_never_picked(k):
    m, a = 259, 2
    z, q = sampler_inputs(m, a, k, k + 5)
    r = torch.rand(m, a, k, generator=gen(k + 6), device=DEV)
    r[..., k // 2] = 1.0  # one class stays live
    masked = r < 1.0 / 3.0
    z = torch.where(r < 1.0 / 6.0, -torch.inf, torch.where(masked, F32.min, z)).contiguous()
    assert torch.isinf(z).any() and (z == F32.min).any()
    for noise in (q, None):
        actions, logp = hip.categorical_sample_logp_wide(z, noise, seed=5, step=1)
        assert not masked.gather(-1, actions.unsqueeze(-1)).any(), "a masked class was drawn"
        check_logp(logp, actions, z, unit_rows(m, k))
    check_picks(hip.categorical_sample_logp_wide(z, q)[0], z, q)


@pytest.mark.parametrize("k", [65, 129, 1000, 4099])
def test_the_last_class_can_be_picked(k):
    m, a = 5, 2
    z, q = sampler_inputs(m, a, k, k + 9)
    z[..., k - 1] = z.amax(-1) + 40.0
    actions, logp = hip.categorical_sample_logp_wide(z, q)
    assert (actions == k - 1).all()
    check_logp(logp, actions, z)
    # ... and by the noise alone, on equal logits
    flat = torch.zeros(m, a, k, device=DEV)
    q2 = torch.ones(m, a, k, device=DEV)
    q2[..., k - 1] = 0.25
    assert (hip.categorical_sample_logp_wide(flat, q2)[0] == k - 1).all()


@pytest.mark.parametrize("k,a", [(65, 2), (1000, 1), (4099, 1)])
def test_row_offset_reproduces_a_slice_of_the_full_call(k, a):
    m, r0, n = 300, 131, 70
    z, _ = sampler_inputs(m, a, k, k + 3)
    full_a, full_lp = hip.categorical_sample_logp_wide(z, None, seed=9, step=4, row_offset=2000)
    part_a, part_lp = hip.categorical_sample_logp_wide(z[r0:r0 + n].contiguous(), None, seed=9, step=4,
                                                       row_offset=2000 + r0)
    assert torch.equal(part_a, full_a[r0:r0 + n]) and torch.equal(part_lp, full_lp[r0:r0 + n])
    again = hip.categorical_sample_logp_wide(z, None, seed=9, step=4, row_offset=2000)
    assert torch.equal(again[0], full_a) and torch.equal(again[1], full_lp)
    other = hip.categorical_sample_logp_wide(z, None, seed=9, step=5, row_offset=2000)
    assert not torch.equal(other[0], full_a)
    check_logp(full_lp, full_a, z, unit_rows(m, k))


# --------------------------------------------------------------------------- #
# Loss
# --------------------------------------------------------------------------- #
def loss_inputs(m, a, k, seed, kind="plain"):
    """Logits N(0, 1.5), actions drawn from the policy, logp_old at a log-ratio ~ N(0, 0.3), values around returns.
    ``kind="likely"``: one class per row and dimension is raised by log(k) + 3, so that it holds most of the mass and
    a taken action is a likely one, as in training.  A uniform-looking policy over 4099 classes and five dimensions
    has log-probabilities near -42, where one fp32 rounding is 1.9e-6 of the ratio whatever the kernel does: the
    bars were set on log-probabilities of a few units (tests/test_ppo_loss_edges_gpu.py: ``cat_inputs``), and a
    handful of samples does not average that rounding down."""
    g = gen(seed)
    x = torch.randn(m, a, k, generator=g, device=DEV) * 1.5
    if kind == "likely":
        fav = torch.randint(0, k, (m, a, 1), generator=g, device=DEV)
        x = x + (math.log(k) + 3.0) * (torch.arange(k, device=DEV) == fav)
    masked = torch.zeros(m, a, k, dtype=torch.bool, device=DEV)
    u = torch.rand(m, a, generator=g, device=DEV).double()
    if kind == "masked":
        r = torch.rand(m, a, k, generator=g, device=DEV)
        masked = r < 0.4
    cdf = torch.softmax(torch.where(masked, -torch.inf, x).double(), -1).cumsum(-1)
    actions = (cdf < u.unsqueeze(-1)).sum(-1).clamp(max=k - 1)
    if kind == "masked":  # -inf on some classes, finfo.min on others, never on the taken action
        masked &= ~F.one_hot(actions, k).bool()
        x = torch.where(masked & (r < 0.2), -torch.inf, torch.where(masked, F32.min, x))
    if kind == "saturated":  # row 0: all of its mass on one class (spread 1e3, the runners-up 32 below the top or more)
        row = torch.round(torch.randn(a, k, generator=g, device=DEV) * 1e3)
        top = row.amax(-1, keepdim=True)
        row = torch.where((row > top - 32) & (row < top), row - 32, row) - top
        x[0] = row
        actions[0] = row.argmax(-1)
    x = x.float().contiguous()
    logp = torch.log_softmax(x.double(), -1).gather(-1, actions.unsqueeze(-1)).squeeze(-1).sum(-1, keepdim=True)
    ret = torch.randn(m, 1, generator=g, device=DEV) * 3
    values = ret + torch.randn(m, 1, generator=g, device=DEV) * 2
    logp_old = (logp - torch.randn(m, 1, generator=g, device=DEV).double() * 0.3).float()
    adv = torch.randn(m, 1, generator=g, device=DEV) * 2
    return dict(logits=x, values=values.contiguous(), actions=actions.contiguous(), logp_old=logp_old, adv=adv,
                ret=ret), masked


def ref_loss(inp, kw):
    """fp64 autograd of the reference expression (tests/test_ppo_loss_edges_gpu.py: ``ref_categorical`` / ``_ppo``)
    on the device: loss means, the gradients the kernel writes (of the mean loss / GAS) and the rows on a clip edge."""
    x = inp["logits"].double().requires_grad_(True)
    values = inp["values"].double().requires_grad_(True)
    logp_old, adv, ret = inp["logp_old"].double(), inp["adv"].double(), inp["ret"].double()
    m = values.shape[0]
    dist = torch.distributions.Categorical(logits=x, validate_args=False)
    logp = dist.log_prob(inp["actions"]).sum(-1, keepdim=True)
    ent = dist.entropy().sum(-1, keepdim=True)
    lr = logp - logp_old
    ratio = torch.exp(lr)
    huber = F.smooth_l1_loss(values, ret, reduction="none")
    vf = torch.clamp(huber, 0.0, kw["vf_clip_param"])
    s1 = adv * ratio
    s2 = adv * torch.clamp(ratio, 1 - kw["clip_param"], 1 + kw["clip_param"])
    clip1 = torch.min(s1, s2)
    pol = torch.where(adv < 0, torch.max(clip1, kw["dual_clip_param"] * adv), clip1) if kw["dual_clip_param"] else clip1
    total = kw["vf_coeff"] * vf.sum() - pol.sum()
    if kw["entropy_coeff"] != 0:
        total = total - kw["entropy_coeff"] * ent.sum()
    (total / (m * GAS)).backward()
    with torch.no_grad():
        kl = (ratio - 1) - lr
        means = {"entropy": float(ent.mean()) if kw["entropy_coeff"] != 0 else 0.0, "policy": float(pol.mean()),
                 "vf": float(vf.mean()), "kl": float(kl.mean())}
        means["total"] = kw["vf_coeff"] * means["vf"] - means["policy"] - kw["entropy_coeff"] * means["entropy"]
        lo, hi = 1 - kw["clip_param"], 1 + kw["clip_param"]
        r = ratio.reshape(-1)
        edge = ((r - lo).abs() < 1e-5) | ((r - hi).abs() < 1e-5) | ((huber.reshape(-1) - kw["vf_clip_param"]).abs() < 1e-5)
        if kw["dual_clip_param"]:
            edge |= (r - kw["dual_clip_param"]).abs() < 1e-5
    return means, x.grad, values.grad, ent.detach(), edge


def assert_grad(got, want, edge, name):
    """``assert_grad`` of tests/test_ppo_loss_edges_gpu.py, on the device."""
    got = got.double()
    assert torch.isfinite(got).all(), name
    err = (got - want).abs()
    bad = err > 2e-5 * want.abs() + 1e-6 * float(want.abs().max())
    bad_rows = bad.reshape(bad.shape[0], -1).any(-1)
    off_edge = bad_rows & ~edge
    assert not off_edge.any(), (name, int(off_edge.sum()), float(err[off_edge].max()))
    assert int(bad_rows.sum()) <= 8, (name, int(bad_rows.sum()))


def hp_of(kw, m):
    return hip.ppo_hparams(grad_scale=1.0 / (m * GAS), **kw)


def run_wide(inp, kw):
    m = inp["values"].shape[0]
    d = [inp[n] for n in ("logits", "values", "actions", "logp_old", "adv", "ret")]
    hp = hp_of(kw, m)
    sums, g_logits, g_value = hip.ppo_loss_categorical_wide(*d, hp)
    means, wg_logits, wg_value, ent, edge = ref_loss(inp, kw)
    assert_means(sums, m, means, kw)
    assert_grad(g_logits, wg_logits, edge, "logits")
    assert_grad(g_value, wg_value, edge, "values")
    sums_ng, n1, n2 = hip.ppo_loss_categorical_wide(*d, hp, with_grad=False)
    assert n1 is None and n2 is None and torch.equal(sums_ng, sums)
    sums2, g2, v2 = hip.ppo_loss_categorical_wide(*d, hp)
    assert torch.equal(sums2, sums) and torch.equal(g2, g_logits) and torch.equal(v2, g_value)
    return sums, g_logits, g_value, ent


HNAMES = ["plain", "dual", "ent", "dual_ent"]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("k", KS)
def test_loss_against_fp64_autograd(k, a, m):
    inp, _ = loss_inputs(m, a, k, seed_of(k, a, m), "likely")
    run_wide(inp, HPS[HNAMES[(KS.index(k) + AS.index(a) + MS.index(m)) % 4]])


@pytest.mark.parametrize("hname", HNAMES)
@pytest.mark.parametrize("k,a", [(65, 2), (1000, 1), (4099, 1)])
def test_loss_hyperparameters_at_every_row_route(k, a, hname):
    """... on a policy without a favoured class: log-probabilities of -4 to -17 per sample, 515 samples."""
    inp, _ = loss_inputs(515, a, k, k + len(hname))
    run_wide(inp, HPS[hname])


@pytest.mark.parametrize("hname", ["ent", "dual_ent", "plain"])
@pytest.mark.parametrize("k,a", [(65, 2), (100, 1), (1000, 2), (4099, 1)])
def test_loss_masked_classes_get_gradient_zero_and_a_finite_entropy(k, a, hname):
    inp, masked = loss_inputs(259, a, k, k + 17, "masked")
    assert masked.any() and torch.isinf(inp["logits"]).any() and (inp["logits"] == F32.min).any()
    sums, g_logits, _, ent = run_wide(inp, HPS[hname])
    assert (g_logits[masked] == 0).all()
    assert torch.isfinite(sums).all() and torch.isfinite(ent).all()


@pytest.mark.parametrize("k", [65, 1000, 4099])
def test_loss_with_a_row_of_all_its_mass_on_one_class(k):
    inp, _ = loss_inputs(259, 1, k, k + 23, "saturated")
    p0 = torch.softmax(inp["logits"][0, 0].double(), -1)
    assert float(p0.max()) > 1 - 1e-12 and float(inp["logits"][0, 0].min()) < -1e3
    _, g_logits, _, _ = run_wide(inp, HPS["dual_ent"])
    assert torch.isfinite(g_logits[0]).all()


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("k", [2, 63, 64])
def test_loss_agrees_with_the_lane_kernel_up_to_64_classes(k, a, m):
    """Both kernels at the bars of the fp64 comparison, against each other."""
    inp, _ = loss_inputs(m, a, k, seed_of(k, a, m) + 2)
    kw = HPS[HNAMES[(k + a + m) % 4]]
    d = [inp[n] for n in ("logits", "values", "actions", "logp_old", "adv", "ret")]
    sums, g_logits, g_value = hip.ppo_loss_categorical_wide(*d, hp_of(kw, m))
    lane_sums, lane_g, lane_v = hip.ppo_loss_categorical(*d, hp_of(kw, m))
    s = lane_sums.cpu().numpy()
    lane_means = {"entropy": s[0] / m if kw["entropy_coeff"] != 0 else 0.0, "policy": s[1] / m, "vf": s[2] / m,
                  "kl": s[4] / m}
    lane_means["total"] = kw["vf_coeff"] * lane_means["vf"] - lane_means["policy"] - kw["entropy_coeff"] * lane_means["entropy"]
    assert_means(sums, m, lane_means, kw)
    edge = ref_loss(inp, kw)[4]
    assert_grad(g_logits, lane_g.double(), edge, "logits")
    assert_grad(g_value, lane_v.double(), edge, "values")
    if k == 2:  # (the lane kernel's exact antisymmetry is not a promise of the wide one: it never feeds a pair head)
        assert torch.isfinite(g_logits).all()


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from rl8_amd import hip
d = np.load(sys.argv[2])
t = [torch.from_numpy(d[n]).to("cuda:0") for n in ("logits", "values", "actions", "logp_old", "adv", "ret")]
hp = hip.ppo_hparams(clip_param=0.2, dual_clip_param=3.0, entropy_coeff=0.01, vf_clip_param=2.0, vf_coeff=0.5,
                     grad_scale=float(d["grad_scale"]))
sums, g, v = hip.ppo_loss_categorical_wide(*t, hp)
np.savez(sys.argv[3], sums=sums.cpu().numpy(), g=g.cpu().numpy(), v=v.cpu().numpy())
"""


def test_loss_under_a_small_grid_cap_strides_over_rows(tmp_path):
    """RL8_LOSS_GRID_CAP=3 (read once per process, so set in a child): 12 waves take 4099 samples, ~340 each.  The
    per-sample results are those of the uncapped grid bit for bit; the sums are the same terms in another order."""
    m, a, k = 4099, 2, 129
    inp, _ = loss_inputs(m, a, k, 99)
    kw = HPS["dual_ent"]
    assert kw == dict(clip_param=0.2, dual_clip_param=3.0, entropy_coeff=1e-2, vf_clip_param=2.0, vf_coeff=0.5)
    src, out = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, grad_scale=np.float64(1.0 / (m * GAS)), **{n: t.cpu().numpy() for n, t in inp.items()})
    env = dict(os.environ, RL8_LOSS_GRID_CAP="3")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(src), str(out)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    child = np.load(out)
    sums, g_logits, g_value, _ = run_wide(inp, kw)
    assert np.array_equal(child["g"], g_logits.cpu().numpy()) and np.array_equal(child["v"], g_value.cpu().numpy())
    np.testing.assert_allclose(child["sums"], sums.cpu().numpy(), rtol=1e-12, atol=0)
    means, wg_logits, _, _, edge = ref_loss(inp, kw)
    assert_means(torch.from_numpy(child["sums"]), m, means, kw)
    assert_grad(torch.from_numpy(child["g"]).to(DEV), wg_logits, edge, "logits under the cap")


# --------------------------------------------------------------------------- #
# Routing one level up
# --------------------------------------------------------------------------- #
def _launched(fn):
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        out = fn()
        return out, set(hip.timer.summary())
    finally:
        hip.timer.enabled = False
        hip.timer.reset()


@pytest.mark.parametrize("k,wide", [(64, False), (65, True), (1000, True)])
def test_distribution_and_fused_loss_route_by_the_number_of_classes(k, wide):
    from rl8_amd.distributions import Categorical, NoiseStream
    from rl8_amd.nn.functional import fused_ppo_loss
    from rl8_amd.tensordict import TensorDict

    m, a = 33, 2
    inp, _ = loss_inputs(m, a, k, k)
    z, q = sampler_inputs(m, a, k, k)
    dist = Categorical(TensorDict({"logits": z}, batch_size=[m]), None)
    dist.noise = q
    (actions, logp), launched = _launched(dist.sample_with_logp)
    assert ("categorical_sample_logp_wide" in launched) == wide
    want = (hip.categorical_sample_logp_wide if wide else hip.categorical_sample_logp)(z, q)
    assert torch.equal(actions, want[0]) and torch.equal(logp, want[1])
    dist.noise, dist.noise_stream = None, NoiseStream(7)
    dist.noise_stream.row_offset = 50
    a1, _ = dist.sample_with_logp()
    direct = (hip.categorical_sample_logp_wide if wide else hip.categorical_sample_logp)(z, None, seed=7, step=0,
                                                                                         row_offset=50)
    assert torch.equal(a1, direct[0]) and dist.noise_stream.step == 1
    assert torch.equal(dist.deterministic_sample(), z.argmax(-1))

    kw = HPS["dual_ent"]
    logits = inp["logits"].clone().requires_grad_(True)
    (sums, inputs, grads), launched = _launched(lambda: fused_ppo_loss(
        Categorical, TensorDict({"logits": logits}, batch_size=[m]), inp["values"], inp["actions"], inp["logp_old"],
        inp["adv"], inp["ret"], grad_scale=1.0 / (m * GAS), **kw))
    assert ("ppo_loss_categorical_wide" in launched) == wide and ("ppo_loss_categorical" in launched) != wide
    d = [inp[n] for n in ("logits", "values", "actions", "logp_old", "adv", "ret")]
    want = (hip.ppo_loss_categorical_wide if wide else hip.ppo_loss_categorical)(*d, hp_of(kw, m))
    assert torch.equal(sums, want[0]) and inputs[0] is logits and torch.equal(grads[0], want[1])
    assert torch.equal(grads[1], want[2])


def test_more_classes_than_the_wide_limit_raise_a_value_error_that_names_it():
    from rl8_amd.distributions import Categorical
    from rl8_amd.nn.functional import fused_ppo_loss
    from rl8_amd.tensordict import TensorDict

    k = hip.MAX_WIDE_CLASSES + 1
    z = torch.zeros(2, 1, k, device=DEV)
    with pytest.raises(ValueError, match=str(hip.MAX_WIDE_CLASSES)):
        Categorical(TensorDict({"logits": z}, batch_size=[2]), None).sample()
    one = torch.zeros(2, 1, device=DEV)
    with pytest.raises(ValueError, match=str(hip.MAX_WIDE_CLASSES)):
        fused_ppo_loss(Categorical, TensorDict({"logits": z}, batch_size=[2]), one, one.long(), one, one, one,
                       clip_param=0.2, dual_clip_param=None, entropy_coeff=0.0, vf_clip_param=1.0, vf_coeff=1.0,
                       grad_scale=0.5)
    # the limit itself runs
    z = torch.zeros(2, 1, hip.MAX_WIDE_CLASSES, device=DEV)
    z[:, :, -1] = 50.0
    actions, _ = hip.categorical_sample_logp_wide(z, None, seed=1)
    assert (actions == hip.MAX_WIDE_CLASSES - 1).all()
