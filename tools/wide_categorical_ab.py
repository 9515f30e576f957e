#!/usr/bin/env python
"""A/B of the wave-per-row categorical kernels against the torch route of the same code, at ``--m`` samples (2^20) of
``--classes`` (128, 1024) classes and one action dimension.

There is no earlier kernel to compare with above 64 classes (the lane-per-row kernels refuse them), so the yardstick
is what a user would otherwise run:

* loss: ``ppo_losses(...)`` + ``total.backward()`` with the built-in ``Categorical`` (the fused wide kernel behind
  ``_AttachPrecomputedGrads``) against the same call with a subclass that overrides ``logp``, which sends
  ``ppo_losses`` through its torch composition and autograd;
* sampler: ``Categorical.sample_with_logp()`` against ``torch.distributions.Categorical(logits=...).sample()`` plus
  ``log_prob`` of the sample.

The two routes alternate call by call; after ``--warmup`` rounds each of ``--repeats`` rounds is timed with HIP events
around the whole call, and the report gives the median and the spread (max - min).  The bare loss launch
(``hip.ppo_loss_categorical_wide``) is timed the same way for the achieved bytes per second over the 2 x 4 x m x k
bytes of logits in and gradients out plus the per-sample columns (value, action, logp_old, advantage, return in;
grad_value out: 32 bytes).

    python tools/wide_categorical_ab.py --out profiles/wide_categorical_ab.txt
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn) -> float:
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def _stats(values: list[float]) -> tuple[float, float]:
    return statistics.median(values), max(values) - min(values)


def measure(m: int, k: int, warmup: int, repeats: int) -> list[str]:
    import torch

    from rl8_amd import hip
    from rl8_amd.data import DataKeys
    from rl8_amd.distributions import Categorical
    from rl8_amd.nn.functional import has_fused_loss, ppo_losses
    from rl8_amd.tensordict import TensorDict

    class TorchCategorical(Categorical):
        """The same distribution with a ``logp`` of its own: ``ppo_losses`` composes the loss from torch operations."""

        def logp(self, samples):
            return super().logp(samples)

    assert has_fused_loss(Categorical) and not has_fused_loss(TorchCategorical)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(k)
    logits = (torch.randn(m, 1, k, generator=g, device=dev) * 1.5).requires_grad_(True)
    values = torch.randn(m, 1, generator=g, device=dev).requires_grad_(True)
    with torch.no_grad():
        actions, logp = hip.categorical_sample_logp_wide(logits.detach(), None, seed=1)
    batch = TensorDict({DataKeys.ACTIONS: actions, DataKeys.LOGP: logp + 0.1 * torch.randn(m, 1, generator=g, device=dev),
                        DataKeys.ADVANTAGES: torch.randn(m, 1, generator=g, device=dev),
                        DataKeys.RETURNS: torch.randn(m, 1, generator=g, device=dev)}, batch_size=[m])
    sample_batch = TensorDict({DataKeys.VALUES: values}, batch_size=[m])
    kw = dict(clip_param=0.2, dual_clip_param=5.0, entropy_coeff=1e-2, vf_clip_param=1.0, vf_coeff=1.0)
    hp = hip.ppo_hparams(grad_scale=1.0 / m, **kw)

    def loss(dist_cls):
        def run():
            logits.grad = values.grad = None
            dist = dist_cls(TensorDict({"logits": logits}, batch_size=[m]), None)
            ppo_losses(batch, sample_batch, dist, **kw)["total"].backward()
        return run

    def bare_loss():
        hip.ppo_loss_categorical_wide(logits.detach(), values.detach(), actions, batch[DataKeys.LOGP],
                                      batch[DataKeys.ADVANTAGES], batch[DataKeys.RETURNS], hp)

    def sample_kernel():
        with torch.no_grad():
            Categorical(TensorDict({"logits": logits}, batch_size=[m]), None).sample_with_logp()

    def sample_torch():
        with torch.no_grad():
            dist = torch.distributions.Categorical(logits=logits)
            dist.log_prob(dist.sample()).sum(-1, keepdim=True)

    routes = {"loss, fused kernel": loss(Categorical), "loss, torch composition": loss(TorchCategorical),
              "loss, bare launch": bare_loss, "sampler, kernel": sample_kernel, "sampler, torch": sample_torch}
    times: dict[str, list[float]] = {name: [] for name in routes}
    for r in range(warmup + repeats):
        for name, fn in routes.items():  # (alternating: every round runs every route once)
            t = _timed(fn)
            if r >= warmup:
                times[name].append(t)
    # the two loss routes agree (a sanity check of the comparison, not a test)
    loss(Categorical)()
    fused = logits.grad.clone()
    loss(TorchCategorical)()
    worst = float((fused - logits.grad).abs().max() / logits.grad.abs().max())
    lines = [f"\nm = {m}, k = {k}, a = 1 ({warmup} warm-up + {repeats} timed rounds; median ms [spread = max - min])"]
    med = {}
    for name in routes:
        med[name], spread = _stats(times[name])
        lines.append(f"  {name:26s} {med[name]:10.3f} ms [{spread:.3f}]")
    lines.append(f"  loss: torch composition / fused kernel = {med['loss, torch composition'] / med['loss, fused kernel']:.1f}x;"
                 f" sampler: torch / kernel = {med['sampler, torch'] / med['sampler, kernel']:.1f}x")
    nbytes = 2 * 4 * m * k + 32 * m
    lines.append(f"  loss, bare launch: {nbytes / 1e9:.3f} GB moved (2 x 4 x m x k + 32 m) in {med['loss, bare launch']:.3f} ms"
                 f" = {nbytes / med['loss, bare launch'] / 1e9:.2f} TB/s")
    lines.append(f"  largest difference of the two loss routes' logit gradients: {worst:.1e} of the largest entry")
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--classes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 timed rounds")
    import torch

    lines = [f"wide categorical A/B on {torch.cuda.get_device_name(0)}: the wave-per-row kernels against the torch route of"
             " the same code"]
    for k in args.classes:
        lines += measure(args.m, k, args.warmup, args.repeats)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
