"""The fused PPO loss kernels (rl8_amd/csrc/ppo_loss_kernels.hip) against a plain fp64 reference, on every launch
path of the two launchers and at the numerical edges: saturated and masked softmax, ratios past the clip and the dual
clip, the Huber kink and the value-clip boundary, extreme log_std, squashed actions at +-1 and the -100 clamp.

The reference is written here from the formulas (torch.distributions in fp64 on the CPU, the clipped / dual-clipped
surrogate, clamp(smooth_l1, 0, vf_clip), the approximate KL, autograd for the gradients) and evaluated on the same
fp32 tensors the kernel gets.  Bars are those of tests/test_hip_kernels.py::test_ppo_loss_matches_reference_autograd:
loss means to rel 1e-5 / abs 1e-7, gradients entrywise to 2e-5 relative with a floor of 1e-6 of the tensor's largest
entry.  Inputs stay where an fp32 evaluation of the formula is well conditioned (see `cat_inputs`, `normal_inputs`):
the bar measures the kernel, not the fp32 rounding of its inputs.
"""

import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import oracle  # noqa: E402  (checker only)

from rl8_amd import hip  # noqa: E402

DEV = "cuda:0"
F32 = np.finfo(np.float32)
EPS = float(F32.eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HPS = {
    "dual_ent": dict(clip_param=0.2, dual_clip_param=3.0, entropy_coeff=1e-2, vf_clip_param=2.0, vf_coeff=0.5),
    "plain": dict(clip_param=0.2, dual_clip_param=None, entropy_coeff=0.0, vf_clip_param=2.0, vf_coeff=0.5),
    "dual": dict(clip_param=0.3, dual_clip_param=3.0, entropy_coeff=0.0, vf_clip_param=2.0, vf_coeff=1.0),
    "ent": dict(clip_param=0.1, dual_clip_param=None, entropy_coeff=1e-2, vf_clip_param=2.0, vf_coeff=2.0),
}
GAS = 2  # gradient accumulation steps: grad_scale = 1 / (m * GAS)


def dev(a, offset=False):
    """A device copy; ``offset``: a contiguous view 4 or 8 bytes past a 16-byte boundary."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if not offset:
        return t.to(DEV)
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = base[1:].view(t.shape)
    v.copy_(t.to(DEV))
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def host(t):
    return t.detach().cpu().numpy()


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


# --------------------------------------------------------------------------- #
# Launch paths, by the launchers' shape and alignment rules.
# --------------------------------------------------------------------------- #
def cat_path(ins, a, k, m):
    if a == 1 and k in (2, 3) and m >= 4 and aligned(*ins):
        return "vec" if m % 4 == 0 else "vec+tail"
    return "generic"


def normal_path(ins, a, m):
    if a == 1 and m >= 4 and aligned(*ins):
        return "vec" if m % 4 == 0 else "vec+tail"
    return "generic"


# --------------------------------------------------------------------------- #
# fp64 reference
# --------------------------------------------------------------------------- #
def _d(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def _ppo(logp, ent, inp, kw, feats):
    """Per-sample terms and autograd gradients of sum(vf_coeff * vf - policy - entropy_coeff * entropy) * grad_scale
    (= what the kernel writes: the gradient of the reference's mean loss divided by GAS)."""
    values, logp_old, adv, ret = (_d(inp["values"], True), _d(inp["logp_old"]), _d(inp["adv"]), _d(inp["ret"]))
    m = values.shape[0]
    lr = logp - logp_old
    ratio = torch.exp(lr)
    vf = torch.clamp(F.smooth_l1_loss(values, ret, reduction="none"), 0.0, kw["vf_clip_param"])
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
    r = ratio.detach().numpy().reshape(-1)
    huber = F.smooth_l1_loss(values, ret, reduction="none").detach().numpy().reshape(-1)
    edge = (np.abs(r - lo) < 1e-5) | (np.abs(r - hi) < 1e-5) | (np.abs(huber - kw["vf_clip_param"]) < 1e-5)
    if kw["dual_clip_param"]:
        edge |= np.abs(r - kw["dual_clip_param"]) < 1e-5
    grads = {name: f.grad.numpy() for name, f in feats.items()}
    grads["values"] = values.grad.numpy()
    return means, grads, edge


def ref_categorical(inp, kw):
    x = _d(inp["logits"], True)
    dist = torch.distributions.Categorical(logits=x, validate_args=False)
    act = torch.as_tensor(inp["actions"])
    logp = dist.log_prob(act).sum(-1, keepdim=True)
    ent = dist.entropy().sum(-1, keepdim=True)
    return _ppo(logp, ent, inp, kw, {"logits": x})


def ref_normal(inp, kw, squashed):
    mean, log_std = _d(inp["mean"], True), _d(inp["log_std"], True)
    dist = torch.distributions.Normal(mean, torch.exp(log_std), validate_args=False)
    a = inp["actions"]
    if squashed:
        c = np.clip(a.astype(np.float64), -1 + EPS, 1 - EPS)
        u = _d(0.5 * (np.log1p(c) - np.log1p(-c)))
        # 1 - s^2 near |s| = 1 is cancellation: s^2 is evaluated as the reference evaluates it, in fp32
        # (tests/test_hip_kernels.py::assert_logp_close); the rest of the formula in fp64.
        s2 = (a * a).astype(np.float32).astype(np.float64)
        logp = torch.clamp(dist.log_prob(u), -100, 100).sum(-1, keepdim=True) - \
            torch.log(_d(1 - s2 + EPS)).sum(-1, keepdim=True)
        ent = torch.zeros_like(logp)
    else:
        logp = dist.log_prob(_d(a)).sum(-1, keepdim=True)
        ent = dist.entropy().sum(-1, keepdim=True)
    return _ppo(logp, ent, inp, kw, {"mean": mean, "log_std": log_std})


# --------------------------------------------------------------------------- #
# Comparison
# --------------------------------------------------------------------------- #
def assert_grad(got, want, edge, name):
    """2e-5 relative with a floor of 1e-6 of the largest entry.  A sample whose fp64 ratio lies within 1e-5 of a
    clip boundary (or whose vf term lies within 1e-5 of vf_clip) has a one-sided gradient, so may differ in any
    evaluation order: those are exempt, must really sit on a boundary, and stay few."""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), name
    bad = np.abs(got - want) > 2e-5 * np.abs(want) + 1e-6 * float(np.abs(want).max())
    bad_rows = bad.reshape(bad.shape[0], -1).any(-1)
    assert not (bad_rows & ~edge).any(), (name, int((bad_rows & ~edge).sum()),
                                           float(np.abs(got - want)[bad_rows & ~edge].max()))
    assert bad_rows.sum() <= 8, (name, int(bad_rows.sum()))


def assert_means(sums, m, want, kw):
    """Loss means at rel 1e-5 / abs 1e-7.  ``want``: the fp64 reference from 1 024 samples on; below that the fp32
    oracle, because a single fp32 sample carries ~1e-7 of rounding in (ratio - 1) - log_ratio by itself -- and below
    16 samples that rounding is not averaged down at all, so the absolute floor there is 1e-6."""
    s = host(sums)
    assert np.isfinite(s).all(), s
    assert s[3] == m
    got = {"entropy": s[0] / m if kw["entropy_coeff"] != 0 else 0.0, "policy": s[1] / m, "vf": s[2] / m,
           "kl": s[4] / m}
    got["total"] = kw["vf_coeff"] * got["vf"] - got["policy"] - kw["entropy_coeff"] * got["entropy"]
    for name in oracle.LOSS_KEYS:
        assert got[name] == pytest.approx(want[name], rel=1e-5, abs=1e-7 if m >= 16 else 1e-6), \
            (name, got[name], want[name])


def _hp(kw, m):
    return hip.ppo_hparams(grad_scale=1.0 / (m * GAS), **kw)


def run_categorical(inp, kw, *, path, offset=(), exact_zero=None):
    """Launches the categorical loss, checks its path, the fp64 reference, the fp32 oracle, with_grad=False and a
    second launch; returns the device outputs."""
    m, a, k = inp["logits"].shape
    names = ("logits", "values", "actions", "logp_old", "adv", "ret")
    d = [dev(inp[n], n in offset) for n in names]
    assert cat_path(d, a, k, m) == path
    hp = _hp(kw, m)
    sums, g_logits, g_value = hip.ppo_loss_categorical(*d, hp)
    want, wg, edge = ref_categorical(inp, kw)
    if m < 1024:
        want = oracle.ppo_loss_categorical(inp["logits"], inp["values"], inp["actions"], inp["logp_old"], inp["adv"],
                                           inp["ret"], oracle.ppo_hparams(**kw))[0]
    assert_means(sums, m, want, kw)
    assert_grad(host(g_logits), wg["logits"], edge, "logits")
    assert_grad(host(g_value), wg["values"], edge, "values")
    if exact_zero is not None:  # masked classes, fully clipped value terms
        assert (host(g_logits)[exact_zero] == 0).all() and (wg["logits"][exact_zero] == 0).all()
    assert (host(g_value)[np.abs(inp["values"] - inp["ret"]) > 100] == 0).all()
    if k == 2:  # the pair weight-gradient kernel's premise, on every path
        gl = host(g_logits).reshape(-1, 2)
        assert np.array_equal(gl[:, 0], -gl[:, 1])
    if m * a * k <= 1 << 20:
        ow, og, ov = oracle.ppo_loss_categorical(inp["logits"], inp["values"], inp["actions"], inp["logp_old"],
                                                 inp["adv"], inp["ret"], oracle.ppo_hparams(grad_accumulation_steps=GAS,
                                                                                            **kw))
        assert_grad(host(g_logits), og.astype(np.float64), edge, "logits vs oracle")
        assert_grad(host(g_value), ov.astype(np.float64), edge, "values vs oracle")
    sums_ng, n1, n2 = hip.ppo_loss_categorical(*d, hp, with_grad=False)
    assert n1 is None and n2 is None and torch.equal(sums_ng, sums)
    sums2, g2, v2 = hip.ppo_loss_categorical(*d, hp)
    assert torch.equal(sums2, sums) and torch.equal(g2, g_logits) and torch.equal(v2, g_value)
    return sums, g_logits, g_value


def run_normal(inp, kw, *, squashed, path, offset=(), exact_zero=None):
    m, a = inp["mean"].shape
    names = ("mean", "log_std", "values", "actions", "logp_old", "adv", "ret")
    d = [dev(inp[n], n in offset) for n in names]
    assert normal_path(d, a, m) == path
    hp = _hp(kw, m)
    sums, g_mean, g_ls, g_value = hip.ppo_loss_normal(*d, hp, squashed=squashed)
    want, wg, edge = ref_normal(inp, kw, squashed)
    if m < 1024:
        want = oracle.ppo_loss_normal(inp["mean"], inp["log_std"], inp["values"], inp["actions"], inp["logp_old"],
                                      inp["adv"], inp["ret"], oracle.ppo_hparams(**kw), squashed=squashed)[0]
    assert_means(sums, m, want, kw)
    assert_grad(host(g_mean), wg["mean"], edge, "mean")
    assert_grad(host(g_ls), wg["log_std"], edge, "log_std")
    assert_grad(host(g_value), wg["values"], edge, "values")
    if exact_zero is not None:  # the -100 clamp engaged: no policy gradient through mean and log_std
        assert exact_zero.any()
        assert (host(g_mean)[exact_zero] == 0).all() and (wg["mean"][exact_zero] == 0).all()
        assert (host(g_ls)[exact_zero] == 0).all() and (wg["log_std"][exact_zero] == 0).all()
    assert (host(g_value)[np.abs(inp["values"] - inp["ret"]) > 100] == 0).all()
    if m * a <= 1 << 20:
        ow, om, ol, ov = oracle.ppo_loss_normal(inp["mean"], inp["log_std"], inp["values"], inp["actions"],
                                                inp["logp_old"], inp["adv"], inp["ret"],
                                                oracle.ppo_hparams(grad_accumulation_steps=GAS, **kw), squashed=squashed)
        for got, o, name in ((g_mean, om, "mean"), (g_ls, ol, "log_std"), (g_value, ov, "values")):
            assert_grad(host(got), o.astype(np.float64), edge, name + " vs oracle")
    sums_ng, *none = hip.ppo_loss_normal(*d, hp, squashed=squashed, with_grad=False)
    assert none == [None, None, None] and torch.equal(sums_ng, sums)
    sums2, m2, l2, v2 = hip.ppo_loss_normal(*d, hp, squashed=squashed)
    assert torch.equal(sums2, sums) and torch.equal(m2, g_mean) and torch.equal(l2, g_ls) and torch.equal(v2, g_value)
    return sums, g_mean, g_ls, g_value


# --------------------------------------------------------------------------- #
# Inputs
# --------------------------------------------------------------------------- #
def _softmax(x):
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(-1, keepdims=True)


def _value_side(rng, m, kind):
    ret = (rng.standard_normal((m, 1)) * 3).astype(np.float32)
    if kind == "vf":  # the Huber kink (|d| = 1), the vf_clip boundary (l = 2 at |d| = 2.5) and fully clipped terms
        d = np.array([0.5, 0.999, 1.0, 1.001, 1.5, 2.49, 2.51, 3.0, 1e6])[rng.integers(0, 9, (m, 1))]
        d = d * np.where(rng.random((m, 1)) < 0.5, -1.0, 1.0)
    else:
        d = rng.standard_normal((m, 1)) * 2
    values = (ret.astype(np.float64) + d).astype(np.float32)
    return values, ret


def _log_ratio(rng, m, kind):
    if kind == "wide":  # e^-20 .. e^20: past the clip and the dual clip, advantages of both signs
        return rng.uniform(-20, 20, (m, 1))
    if kind == "ulp":  # within a few ulp of 1
        return rng.integers(-3, 4, (m, 1)) * 6e-8
    return rng.standard_normal((m, 1)) * 0.3


def cat_inputs(m, a, k, kind="plain", seed=0):
    """Logits, actions sampled from the policy (a taken action is a likely one, as in training; uniform where the
    softmax saturates) and logp_old at a chosen log-ratio.  ``spread50`` / ``spread1e3`` subtract the row maximum (a categorical is shift invariant):
    an fp32 logp is only good to an ulp of the logits' magnitude, which at 1e3 is 6e-5 of the ratio; ``spread1e3``
    keeps its runner-up classes 32 below the maximum (probabilities of 0 and 1 to fp32)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, a, k))
    if kind == "spread50":
        x = x * 50
    elif kind == "spread1e3":
        x = np.round(x * 1e3)
        top = x.max(-1, keepdims=True)
        x = np.where((x > top - 32) & (x < top), x - 32, x)
    elif kind == "dominant":
        x = x + 40.0 * (np.arange(k) == rng.integers(0, k, (m, a, 1)))
    elif kind == "equal":
        x = np.repeat(x[..., :1], k, -1)
    else:
        x = x * 1.5
    if kind in ("spread50", "spread1e3"):
        x = x - x.max(-1, keepdims=True)
    x = x.astype(np.float32)
    if kind in ("spread50", "spread1e3", "dominant"):
        # not only the likeliest class: one whose probability rounds to 1 in fp32 has a gradient (1 - p) of rounding
        # residue.  Uniform over the classes within 20 of the maximum (the two largest at spread1e3): an fp32 logp
        # is good to an ulp of its own magnitude.
        order = np.argsort(-x, -1, kind="stable")
        near = {"spread50": (x >= x.max(-1, keepdims=True) - 20).sum(-1), "spread1e3": np.full((m, a), 2),
                "dominant": np.full((m, a), k)}[kind]
        near = np.maximum(np.minimum(near, k), 1)
        pick = np.minimum((rng.random((m, a)) * near).astype(np.int64), near - 1)
        actions = np.take_along_axis(order, pick[..., None], -1)[..., 0]
    else:
        cdf = np.cumsum(_softmax(x.astype(np.float64)), -1)
        actions = np.minimum((cdf < rng.random((m, a, 1))).sum(-1), k - 1)
    masked = np.zeros_like(x, dtype=bool)
    if kind.startswith("masked"):  # -inf on some classes, finfo.min on others, never on the taken action
        r = rng.random((m, a, k))
        taken = np.arange(k) == actions[..., None]
        masked = (r < 0.4) & ~taken
        x = np.where(masked & (r < 0.2), np.float32(-np.inf), np.where(masked, F32.min, x)).astype(np.float32)
    x64 = x.astype(np.float64)
    top = x64.max(-1, keepdims=True)
    nl = x64 - top - np.log(np.exp(x64 - top).sum(-1, keepdims=True))
    logp = nl[np.arange(m)[:, None], np.arange(a), actions].sum(-1, keepdims=True)
    values, ret = _value_side(rng, m, "vf" if kind in ("wide", "vf") else "plain")
    return dict(logits=x, values=values, actions=actions.astype(np.int64),
                logp_old=(logp - _log_ratio(rng, m, kind)).astype(np.float32),
                adv=(rng.standard_normal((m, 1)) * 2).astype(np.float32), ret=ret), masked


def normal_inputs(m, a, kind="plain", squashed=False, seed=0):
    """``wide``: log_std in [-20, 5]; a quarter of the rows at |action - mean| / std in [50, 1e4] with logp_old = -1
    (their ratio underflows to 0 in any precision: an fp32 z^2 / 2 of 5e7 carries an error of 4).  ``clamp``
    (squashed): actions at +-1, +-(1 - eps), +-(1 - 2 eps) and 0 next to ordinary draws (|tanh argument| <= 3), and a
    quarter of the rows with small std far from the action, where the -100 clamp engages."""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((m, a))
    # (log_std in [-20, 5] at one action dim; several dims sum logps of up to 60 in magnitude: [-5, 5] there)
    log_std = rng.uniform(-1.0, 0.5, (m, a)) if kind != "wide" else rng.uniform(-20 if a == 1 else -5, 5, (m, a))
    z = rng.standard_normal((m, a))
    far = np.zeros(m, bool)
    clamp = np.zeros((m, a), bool)
    if kind == "wide":
        far = rng.random(m) < 0.25
        z[far] = np.exp(rng.uniform(np.log(50), np.log(1e4), (far.sum(), a))) * np.sign(z[far])
    raw = mean + np.exp(log_std) * z
    if squashed:
        actions = np.tanh(np.clip(raw, -3, 3))
        if kind == "clamp":
            edges = np.array([1.0, -1.0, 1 - EPS, -(1 - EPS), 1 - 2 * EPS, -(1 - 2 * EPS), 0.0])
            pick = rng.random((m, a)) < 0.3
            actions = np.where(pick, edges[rng.integers(0, 7, (m, a))], actions)
            # (an edge action is drawn near its mean: a log-prob of -100 in fp32 carries 4e-6 of rounding per op)
            c = np.clip(actions, -1 + EPS, 1 - EPS)
            mean = np.where(pick, 0.5 * (np.log1p(c) - np.log1p(-c)) + np.exp(log_std) * z, mean)
            clamp = rng.random((m, a)) < 0.25
            log_std = np.where(clamp, rng.uniform(-6, -5, (m, a)), log_std)
            mean = np.where(clamp, np.where(actions > 0, -1.0, 1.0) * rng.uniform(1.0, 2.0, (m, a)), mean)
    else:
        actions = raw
    mean, log_std, actions = (v.astype(np.float32) for v in (mean, log_std, actions))
    inp = dict(mean=mean, log_std=log_std, actions=actions)
    values, ret = _value_side(rng, m, "vf" if kind in ("wide", "clamp") else "plain")
    inp.update(values=values, ret=ret, adv=(rng.standard_normal((m, 1)) * 2).astype(np.float32))
    lo = _fp64_logp(inp, squashed) - _log_ratio(rng, m, "wide" if kind == "wide" else kind)
    lo[far] = -1.0
    inp["logp_old"] = lo.astype(np.float32)
    return inp, clamp


def _fp64_logp(inp, squashed, s2_f32=True):
    """The reference's log-prob in fp64 (``s2_f32``: with s^2 rounded to fp32, as in `ref_normal`)."""
    mean, log_std, a = (np.asarray(inp[n], np.float64) for n in ("mean", "log_std", "actions"))
    sc = np.exp(log_std)
    if squashed:
        c = np.clip(a, -1 + EPS, 1 - EPS)
        u = 0.5 * (np.log1p(c) - np.log1p(-c))
        lp = np.clip(-((u - mean) ** 2) / (2 * sc * sc) - log_std - 0.5 * np.log(2 * np.pi), -100, 100)
        s2 = (inp["actions"] * inp["actions"]).astype(np.float32).astype(np.float64) if s2_f32 else a * a
        return lp.sum(-1, keepdims=True) - np.log(1 - s2 + EPS).sum(-1, keepdims=True)
    return (-((a - mean) ** 2) / (2 * sc * sc) - log_std - 0.5 * np.log(2 * np.pi)).sum(-1, keepdims=True)


# --------------------------------------------------------------------------- #
# Launch-path matrix
# --------------------------------------------------------------------------- #
CAT_MS = [1, 3, 4, 5, 7, 1025, 65539]


@pytest.mark.parametrize("m", CAT_MS)
@pytest.mark.parametrize("a", [1, 2, 5])
@pytest.mark.parametrize("k", [2, 3, 4, 7, 16, 33, 63, 64])
def test_categorical_launch_matrix(k, a, m):
    inp, _ = cat_inputs(m, a, k, seed=k * 1000 + a * 100 + m % 97)
    path = ("vec" if m % 4 == 0 else "vec+tail") if (a == 1 and k in (2, 3) and m >= 4) else "generic"
    run_categorical(inp, HPS["dual_ent" if (k + a + m) % 2 else "plain"], path=path)


def test_categorical_more_than_64_classes_is_refused():
    inp, _ = cat_inputs(8, 1, 65)
    d = [dev(inp[n]) for n in ("logits", "values", "actions", "logp_old", "adv", "ret")]
    with pytest.raises(ValueError):
        hip.ppo_loss_categorical(*d, _hp(HPS["plain"], 8))


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 7, 8, 1025, 65539])
@pytest.mark.parametrize("a", [1, 2, 3, 6])
@pytest.mark.parametrize("dist", ["normal", "squashed"])
def test_normal_launch_matrix(dist, a, m):
    squashed = dist == "squashed"
    inp, _ = normal_inputs(m, a, squashed=squashed, seed=a * 100 + m % 97)
    path = ("vec" if m % 4 == 0 else "vec+tail") if (a == 1 and m >= 4) else "generic"
    for hname in (("dual", "plain") if squashed else ("dual", "plain", "ent", "dual_ent")):
        run_normal(inp, HPS[hname], squashed=squashed, path=path)


@pytest.mark.parametrize("dist", ["normal", "squashed"])
def test_normal_grid_cap_fills_every_partial_row(dist):
    """2^21 + 3 samples at a = 1: the vector kernel's grid is capped at 2 047 workgroups and the 3-sample tail
    publishes row 2 047, the last row of the scratch."""
    m = (1 << 21) + 3
    inp, _ = normal_inputs(m, 1, squashed=dist == "squashed", seed=21)
    assert (m // 4 + 255) // 256 > 2047
    run_normal(inp, HPS["dual"], squashed=dist == "squashed", path="vec+tail")


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("which", ["logits", "values", "actions", "logp_old", "adv", "ret"])
def test_categorical_misaligned_input_takes_generic_kernel(which, k):
    """One input 4 (float) or 8 (int64) bytes off a 16-byte boundary sends a = 1, K = 2 / 3 to the generic kernel,
    which must meet the same bar (and keep g[:, 0] == -g[:, 1] at K = 2)."""
    inp, _ = cat_inputs(1027, 1, k, seed=k)
    run_categorical(inp, HPS["dual_ent"], path="generic", offset=(which,))


@pytest.mark.parametrize("squashed", [False, True])
@pytest.mark.parametrize("which", ["mean", "log_std", "values", "actions", "logp_old", "adv", "ret"])
def test_normal_misaligned_input_takes_generic_kernel(which, squashed):
    inp, _ = normal_inputs(1027, 1, squashed=squashed, seed=5)
    run_normal(inp, HPS["dual"], squashed=squashed, path="generic", offset=(which,))


# --------------------------------------------------------------------------- #
# Numerical edges, over the paths
# --------------------------------------------------------------------------- #
CAT_PATHS = {  # (a, k, m, misaligned input)
    "vec2": (1, 2, 1027, ()), "vec3": (1, 3, 1027, ()), "generic2_misaligned": (1, 2, 1027, ("logits",)),
    "generic3": (1, 3, 3, ()), "generic7": (1, 7, 515, ()), "generic64_a2": (2, 64, 257, ()),
}


# (a saturated softmax over 3 rows, or at spread 1e3 over two action dims, leaves gradient entries that are all fp32
# residue of 1 - p: those combinations are not held to the relative bar)
CAT_EDGES = [(path, kind) for path in CAT_PATHS
             for kind in ("spread50", "spread1e3", "dominant", "equal", "masked", "wide", "ulp", "vf")
             if not (kind.startswith("spread") and (CAT_PATHS[path][2] < 16
                                                    or (CAT_PATHS[path][0] > 1 and kind == "spread1e3")))]


@pytest.mark.parametrize("hname", ["dual_ent", "plain", "ent"])
@pytest.mark.parametrize("path,kind", CAT_EDGES)
def test_categorical_edges(path, kind, hname):
    a, k, m, offset = CAT_PATHS[path]
    inp, masked = cat_inputs(m, a, k, kind, seed=zlib.crc32(f"{path}/{kind}".encode()) % 1000)
    want_path = "generic" if path.startswith("generic") else ("vec" if m % 4 == 0 else "vec+tail")
    _, g_logits, _ = run_categorical(inp, HPS[hname], path=want_path, offset=offset,
                                     exact_zero=masked if kind == "masked" else None)
    if kind == "masked":
        assert masked.any() and np.isinf(inp["logits"]).any() and (inp["logits"] == F32.min).any()


NORMAL_PATHS = {  # (a, m, misaligned input)
    "vec": (1, 1027, ()), "generic1": (1, 3, ()), "generic1_misaligned": (1, 1027, ("mean",)), "generic3": (3, 515, ()),
}


@pytest.mark.parametrize("hname", ["dual", "plain", "ent", "dual_ent"])
@pytest.mark.parametrize("kind", ["wide", "ulp", "vf"])
@pytest.mark.parametrize("path", list(NORMAL_PATHS))
def test_normal_edges(path, kind, hname):
    a, m, offset = NORMAL_PATHS[path]
    inp, _ = normal_inputs(m, a, kind, seed=zlib.crc32(f"{path}/{kind}".encode()) % 1000)
    want_path = "generic" if path.startswith("generic") else "vec+tail"
    run_normal(inp, HPS[hname], squashed=False, path=want_path, offset=offset)


@pytest.mark.parametrize("hname", ["dual", "plain"])
@pytest.mark.parametrize("path", list(NORMAL_PATHS))
def test_squashed_edges(path, hname):
    a, m, offset = NORMAL_PATHS[path]
    if path == "generic1":
        m = 3
    inp, clamp = normal_inputs(max(m, 3), a, "clamp", squashed=True, seed=zlib.crc32(path.encode()) % 1000)
    want_path = "generic" if path.startswith("generic") else "vec+tail"
    run_normal(inp, HPS[hname], squashed=True, path=want_path, offset=offset,
               exact_zero=clamp if clamp.any() else None)


# --------------------------------------------------------------------------- #
# The tuning override of the categorical vector grid
# --------------------------------------------------------------------------- #
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
sums, g, v = hip.ppo_loss_categorical(*t, hp)
np.savez(sys.argv[3], sums=sums.cpu().numpy(), g=g.cpu().numpy(), v=v.cpu().numpy())
"""


def test_categorical_grid_cap_override_keeps_a_row_for_the_tail(tmp_path):
    """RL8_LOSS_GRID_CAP (read once per process, so set in a child) raises the vector grid to the scratch's 2 048
    rows at most; the m % 4 tail's row must still fit (it used to land on the arrival counter)."""
    m, k = (1 << 21) + 5, 2
    inp, _ = cat_inputs(m, 1, k, seed=77)
    kw = HPS["dual_ent"]
    src = tmp_path / "in.npz"
    np.savez(src, grad_scale=np.float64(1.0 / (m * GAS)), **inp)
    out = tmp_path / "out.npz"
    env = dict(os.environ, RL8_LOSS_GRID_CAP="4096")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(src), str(out)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    child = np.load(out)
    sums, g_logits, g_value = run_categorical(inp, kw, path="vec+tail")
    assert np.array_equal(child["g"], host(g_logits)) and np.array_equal(child["v"], host(g_value))
    np.testing.assert_allclose(child["sums"], host(sums), rtol=1e-12, atol=0)


# --------------------------------------------------------------------------- #
# Sampler -> loss consistency
# --------------------------------------------------------------------------- #
def _ratio_inside(run, m, clip):
    """True per sample iff the loss kernel's ratio exp(logp - logp_old) lies within [1 - clip, 1 + clip]: with the
    entropy bonus off, a sample's policy gradient vanishes on the clipped side -- above 1 + clip for a positive
    advantage, below 1 - clip for a negative one -- so it survives both launches only inside the band."""
    inside = np.ones(m, bool)
    for sign in (1.0, -1.0):
        g = run(np.full((m, 1), sign, np.float32), clip)
        inside &= (g.reshape(m, -1) != 0).any(-1)
    return inside


@pytest.mark.parametrize("k", [2, 3, 9, 64])
def test_categorical_sampler_matches_loss_logp(k):
    m, a, clip = 4099, 2 if k > 3 else 1, 2e-5
    rng = np.random.default_rng(k)
    x = (rng.standard_normal((m, a, k)) * 3).astype(np.float32)
    r = rng.random((m, a, k))
    r[..., 0] = 1.0  # class 0 stays live
    x = np.where(r < 0.15, np.float32(-np.inf), np.where(r < 0.3, F32.min, x)).astype(np.float32)
    actions, logp = hip.categorical_sample_logp(dev(x), None, seed=3, step=1)
    act, lp = host(actions), host(logp)
    assert (x[np.arange(m)[:, None], np.arange(a), act] > -1e38).all(), "a masked class was drawn"
    assert np.isfinite(lp).all()
    ref = torch.distributions.Categorical(logits=_d(x), validate_args=False).log_prob(torch.as_tensor(act)).sum(-1)
    np.testing.assert_allclose(lp.reshape(-1), ref.numpy(), rtol=1e-5, atol=1e-6)
    values = np.zeros((m, 1), np.float32)
    live = (1 - np.exp(ref.numpy())) > 1e-3  # rows whose taken class is not certain: a policy gradient to see

    def run(adv, c):
        kw = dict(HPS["plain"], clip_param=c)
        _, g, _ = hip.ppo_loss_categorical(dev(x), dev(values), actions, logp, dev(adv), dev(values), _hp(kw, m))
        return host(g)
    assert _ratio_inside(run, m, clip)[live].all()


@pytest.mark.parametrize("a", [1, 3])
@pytest.mark.parametrize("squashed", [False, True])
def test_normal_sampler_matches_loss_logp(squashed, a):
    from tests.test_hip_kernels import assert_logp_close

    m, clip = 4099, 2e-5
    rng = np.random.default_rng(a)
    mean = rng.standard_normal((m, a)).astype(np.float32)
    if squashed:  # saturated draws: tanh rounds to +-1 in fp32
        mean[: m // 2] = (np.sign(mean[: m // 2]) * rng.uniform(10, 15, (m // 2, a))).astype(np.float32)
    log_std = rng.uniform(-1.0, 0.5, (m, a)).astype(np.float32)
    actions, logp = hip.normal_sample_logp(dev(mean), dev(log_std), None, squashed=squashed, seed=4, step=2)
    act, lp = host(actions), host(logp)
    assert np.isfinite(lp).all() and (not squashed or (np.abs(act) <= 1).all())
    if squashed:
        assert (np.abs(act) == 1).any()
    # (s^2 in fp64 here: the band of assert_logp_close covers the fp32 rounding of 1 - s^2)
    want = _fp64_logp(dict(mean=mean, log_std=log_std, actions=act), squashed, s2_f32=False)
    assert_logp_close(lp, want, act, squashed=squashed)
    values = np.zeros((m, 1), np.float32)

    def run(adv, c):
        kw = dict(HPS["plain"], clip_param=c)
        _, gm, _, _ = hip.ppo_loss_normal(dev(mean), dev(log_std), dev(values), actions, logp, dev(adv), dev(values),
                                          _hp(kw, m), squashed=squashed)
        return host(gm)
    live = np.ones(m, bool)
    if squashed:  # rows whose clamp engaged (or nearly: the two evaluations may fall either side) have no gradient
        c = np.clip(act.astype(np.float64), -1 + EPS, 1 - EPS)
        z = (0.5 * (np.log1p(c) - np.log1p(-c)) - mean) / np.exp(log_std.astype(np.float64))
        live = ((-0.5 * z * z - log_std - 0.92) > -90).all(-1) & (np.abs(act) < 1).all(-1)
        assert live.sum() > m // 4
    assert _ratio_inside(run, m, clip)[live].all()


# --------------------------------------------------------------------------- #
# The reference's own edge fixture (tests/golden/generate_fixtures.py: gen_ppo_loss_edges)
# --------------------------------------------------------------------------- #
def test_ppo_loss_edges_match_reference_fixture(golden):
    """Masked logits, ratios past the dual clip, the Huber kink / vf_clip rows and clamp-engaged squashed rows, as
    the reference computed them: at the bars of test_hip_kernels.py::test_ppo_loss_matches_reference_autograd."""
    from tests.test_hip_kernels import _hp_from, _losses_from_sums

    g = golden("ppo_loss_edges.npz")
    # (the squashed cases are held to the oracle only, tests/test_oracle_golden.py: their saturated draws with a
    # std of e^-6 amplify the a = 1 vector kernel's one-logarithm atanh by 1/std, 1.4e-4 of a few mean gradients)
    for case in [c for c in g["cases"] if not c.startswith("squashed")]:
        m = g[f"{case}_values"].shape[0]
        kw, gscale = _hp_from(g[f"{case}_hparams"], m)
        hp = hip.ppo_hparams(grad_scale=gscale, **kw)
        tail = [dev(g[f"{case}_logp_old"]), dev(g[f"{case}_advantages"]), dev(g[f"{case}_returns"])]
        if case.startswith("cat"):
            sums, g_logits, g_value = hip.ppo_loss_categorical(
                dev(g[f"{case}_feat_logits"]), dev(g[f"{case}_values"]), dev(g[f"{case}_actions"]), *tail, hp)
            want = g[f"{case}_grad_logits"]
            np.testing.assert_allclose(host(g_logits), want, rtol=2e-5, atol=1e-8, err_msg=case)
            assert (host(g_logits)[g[f"{case}_feat_logits"] < -1e38] == 0).all(), case
        else:
            sums, g_mean, g_ls, g_value = hip.ppo_loss_normal(
                dev(g[f"{case}_feat_mean"]), dev(g[f"{case}_feat_log_std"]), dev(g[f"{case}_values"]),
                dev(g[f"{case}_actions"]), *tail, hp, squashed=case.startswith("squashed"))
            for got, name in ((g_mean, "grad_mean"), (g_ls, "grad_log_std")):
                want = g[f"{case}_{name}"]
                np.testing.assert_allclose(host(got), want, rtol=2e-5, atol=1e-6 * float(np.abs(want).max()),
                                           err_msg=f"{case} {name}")
        np.testing.assert_allclose(host(g_value), g[f"{case}_grad_values"], rtol=2e-5, atol=1e-9, err_msg=case)
        got = _losses_from_sums(host(sums), kw)
        for i, name in enumerate(oracle.LOSS_KEYS):
            assert got[i] == pytest.approx(g[f"{case}_losses"][i], rel=1e-5, abs=1e-7), (case, name)
