"""GAE, the PPO loss and the masked sequence functions, backed by the gfx950 kernels.

Signatures and semantics follow the reference's ``src/rl8/nn/functional.py``:
``generalized_advantage_estimate`` :50-123 and ``ppo_losses`` :259-363. Both take
and return tensordicts exactly as the reference does; what runs underneath is

* ``rl8_gae_scan_f32`` + ``rl8_advantage_normalise_f32`` -- one launch for the
  whole reverse scan (the reference issues 5H+6 strided ops), for both the
  reference's env-major ``[B, T+1, 1]`` layout (LDS-staged tiles) and this
  build's time-major rollout buffer (register scan);
* ``rl8_ppo_loss_*_fwd_bwd_f32`` -- loss terms, approximate KL and the gradients
  w.r.t. the distribution features and the value estimates in one launch, hooked
  into autograd so ``losses["total"].backward()`` keeps working.

For those two, tensors must live on a HIP device: there is no CPU fallback.

The mask helpers and the masked sequence functions (:13-47, :126-257, :366-400; the second half of this file) are
general-purpose: user models and host tests call them on any device. ``masked_avg``, ``masked_max``,
``masked_log_softmax`` and ``masked_categorical_sample`` run ``rl8_masked_*`` (``csrc/masked_kernels.hip``) on dense
float32 HIP tensors reduced along the dimension the kernels take, and the reference's torch expression everywhere else.

"""

from __future__ import annotations

import os
from typing import Any, Callable

import numpy as np
import torch

from .. import distributions, hip
from ..data import DataKeys
from ..distributions import Categorical, Distribution, Normal, SquashedNormal
from ..tensordict import TensorDict

MomentReduce = Callable[[torch.Tensor], torch.Tensor]


def _f32(x: float) -> float:
    """The value ``x`` takes when torch casts a Python scalar to float32."""
    return float(np.float32(x))


def _require_hip(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise hip.HipExtensionError(
            f"{what} is on {t.device}: rl8_amd runs this op on a HIP device only"
            " (no CPU fallback)."
        )


def gae_launch(
    rewards: torch.Tensor,
    values: torch.Tensor,
    advantages: torch.Tensor,
    returns: torch.Tensor,
    *,
    gae_lambda: float,
    gamma: float,
    reward_scale: float,
    normalize_advantages: bool,
    write_scaled_rewards: bool,
    moment_reduce: None | MomentReduce = None,
) -> torch.Tensor:
    """Scan + optional normalisation over ``[N, H+1, 1]`` leaves that share one
    layout (env-major or time-major). Returns the device moments
    ``(count, sum, sum_sq)`` of ``advantages[:, :H]`` (after ``moment_reduce``,
    which an env-sharded run uses to all-reduce them)."""
    layout, es, ts = hip.buffer_layout(rewards)
    if layout < 0:
        raise ValueError("GAE leaves must be env-major or time-major dense tensors")
    for name, t in (("values", values), ("advantages", advantages), ("returns", returns)):
        if t.shape != rewards.shape or t.stride() != rewards.stride() or t.dtype != torch.float32:
            raise ValueError(f"{name} must share shape, strides and dtype (float32) with rewards")
    n, h = rewards.shape[0], rewards.shape[1] - 1
    if h < 1:
        raise ValueError("GAE needs at least two columns ([B, T + 1, ...])")
    moments = hip.gae_scan(
        rewards,
        values,
        advantages,
        returns,
        layout=layout,
        n=n,
        h=h,
        gamma=_f32(gamma),
        gamma_lambda=_f32(gamma * gae_lambda),
        reward_denominator=_f32(reward_scale + 1e-8),
        write_scaled_rewards=write_scaled_rewards,
    )
    if normalize_advantages:
        if moment_reduce is not None:
            moments = moment_reduce(moments)
        hip.advantage_normalise(advantages, layout=layout, n=n, h=h, moments=moments)
    return moments


def generalized_advantage_estimate(
    batch: TensorDict,
    /,
    *,
    gae_lambda: float = 0.95,
    gamma: float = 0.95,
    inplace: bool = False,
    normalize_advantages: bool = True,
    return_returns: bool = True,
    reward_scale: float = 1.0,
) -> TensorDict:
    """Generalized Advantage Estimate (and returns) from rewards and values.

    Args:
        batch: Tensordict of batch size ``[B, T + 1, ...]`` with ``"rewards"``
            and ``"values"``. As in the reference, the rewards it holds are
            divided by ``reward_scale + 1e-8``.
        gae_lambda: GAE bias/variance trade-off.
        gamma: Discount factor.
        inplace: Store outputs in ``batch`` instead of a new tensordict.
        normalize_advantages: Standardise ``advantages[:, :-1]`` with their
            batch mean and (unbiased) standard deviation.
        return_returns: Also store ``"returns" = advantages + values``.
        reward_scale: Reward normaliser.

    Returns:
        Tensordict with ``"advantages"`` and, optionally, ``"returns"``.

    """
    rewards = batch[DataKeys.REWARDS]
    values = batch[DataKeys.VALUES]
    _require_hip(rewards, "rewards")
    _require_hip(values, "values")
    out = batch if inplace else TensorDict({}, batch_size=batch.batch_size, device=batch.device)

    work_rewards = rewards
    if rewards.dtype != torch.float32 or hip.buffer_layout(rewards)[0] < 0:
        work_rewards = rewards.to(torch.float32).contiguous()
    work_values = values
    if (
        values.dtype != torch.float32
        or values.stride() != work_rewards.stride()
        or values.shape != work_rewards.shape
    ):
        work_values = torch.empty_like(work_rewards)
        work_values.copy_(values)

    advantages = out[DataKeys.ADVANTAGES] if DataKeys.ADVANTAGES in out.keys() else None
    if (
        advantages is None
        or advantages.stride() != work_rewards.stride()
        or advantages.dtype != torch.float32
        or advantages.shape != work_rewards.shape
    ):
        advantages = torch.empty_like(work_rewards)
    returns = torch.empty_like(work_rewards)

    gae_launch(
        work_rewards,
        work_values,
        advantages,
        returns,
        gae_lambda=gae_lambda,
        gamma=gamma,
        reward_scale=reward_scale,
        normalize_advantages=normalize_advantages,
        write_scaled_rewards=True,
    )
    batch[DataKeys.REWARDS] = work_rewards
    out[DataKeys.ADVANTAGES] = advantages
    if return_returns:
        out[DataKeys.RETURNS] = returns
    return out


# --------------------------------------------------------------------------- #
# PPO loss.
# --------------------------------------------------------------------------- #
class PPOLossSums:
    """Raw fp64 sums from one fused loss launch: entropy, policy, vf, count, kl.
    Env shards add these with one all-reduce before anything is divided."""

    KEYS = ("entropy", "policy", "vf", "count", "kl")

    def __init__(self, sums: torch.Tensor) -> None:
        self.sums = sums

    def losses(
        self, *, entropy_coeff: float, vf_coeff: float, grad_accumulation_steps: int = 1
    ) -> dict[str, float]:
        """One device->host copy; returns entropy / policy / vf / total (each
        divided by ``grad_accumulation_steps``) and the unscaled kl."""
        ent_s, pol_s, vf_s, cnt, kl_s = self.sums.tolist()
        return losses_from_sums(
            ent_s, pol_s, vf_s, cnt, kl_s,
            entropy_coeff=entropy_coeff, vf_coeff=vf_coeff,
            grad_accumulation_steps=grad_accumulation_steps,
        )


def losses_from_sums(
    ent_s: float, pol_s: float, vf_s: float, cnt: float, kl_s: float, *,
    entropy_coeff: float, vf_coeff: float, grad_accumulation_steps: int = 1,
) -> dict[str, float]:
    entropy = ent_s / cnt if entropy_coeff != 0 else 0.0
    policy, vf = pol_s / cnt, vf_s / cnt
    total = vf_coeff * vf - policy
    if entropy_coeff != 0:
        total -= entropy_coeff * entropy
    g = grad_accumulation_steps
    return {
        "entropy": entropy / g,
        "policy": policy / g,
        "vf": vf / g,
        "total": total / g,
        "kl": kl_s / cnt,
    }


def fused_ppo_loss(
    distribution_cls: type[Distribution],
    features: TensorDict,
    values: torch.Tensor,
    actions: torch.Tensor,
    logp_old: torch.Tensor,
    advantages: torch.Tensor,
    returns: torch.Tensor,
    *,
    clip_param: float,
    dual_clip_param: None | float,
    entropy_coeff: float,
    vf_clip_param: float,
    vf_coeff: float,
    grad_scale: float,
    with_grad: bool = True,
) -> tuple[torch.Tensor, list[torch.Tensor], list[torch.Tensor]]:
    """One fused launch. Returns ``(sums, inputs, grads)`` where ``inputs`` are
    the differentiable tensors (features then values) and ``grads`` the matching
    ``d total / d input * grad_scale``; feed both to ``torch.autograd.backward``.

    ``grad_scale`` is ``1 / (global minibatch size * grad_accumulation_steps)``.

    """
    hp = hip.ppo_hparams(
        clip_param=clip_param, dual_clip_param=dual_clip_param, entropy_coeff=entropy_coeff,
        vf_clip_param=vf_clip_param, vf_coeff=vf_coeff, grad_scale=grad_scale,
    )
    flat = lambda t: t.detach().contiguous()  # noqa: E731
    if issubclass(distribution_cls, Categorical):
        logits = features["logits"]
        # (more classes than one lane's array holds: the wave-per-sample kernel; up to MAX_CLASSES nothing changes)
        wide = logits.shape[-1] > hip.MAX_CLASSES
        sums, g_logits, g_values = (hip.ppo_loss_categorical_wide if wide else hip.ppo_loss_categorical)(
            flat(logits).float(), flat(values).float(), flat(actions), flat(logp_old),
            flat(advantages), flat(returns), hp, with_grad=with_grad,
        )
        if not with_grad:
            return sums, [], []
        g_logits = g_logits.to(logits.dtype)
        if logits.shape[-1] == 2 and logits.numel() == 2 * values.numel() and g_logits.dtype == torch.float32:
            from . import fused_mlp

            fused_mlp.trust_pair_gradient(g_logits)  # (one action dimension, two classes: the kernel stored g and -g)
        return sums, [logits, values], [g_logits, g_values.to(values.dtype)]
    if issubclass(distribution_cls, Normal):
        if issubclass(distribution_cls, SquashedNormal) and entropy_coeff != 0:
            raise NotImplementedError(
                f"Entropy isn't defined for {distribution_cls.__name__}. Set the"
                " entropy coefficient to `0` to avoid this error during training."
            )
        mean, log_std = features["mean"], features["log_std"]
        sums, g_mean, g_ls, g_values = hip.ppo_loss_normal(
            flat(mean).float(), flat(log_std).float(), flat(values).float(), flat(actions),
            flat(logp_old), flat(advantages), flat(returns), hp,
            squashed=issubclass(distribution_cls, SquashedNormal), with_grad=with_grad,
        )
        if not with_grad:
            return sums, [], []
        return (
            sums,
            [mean, log_std, values],
            [g_mean.to(mean.dtype), g_ls.to(log_std.dtype), g_values.to(values.dtype)],
        )
    raise TypeError(f"{distribution_cls.__name__} has no fused loss kernel")


def has_fused_loss(distribution_cls: type[Distribution]) -> bool:
    """True when ``distribution_cls`` computes ``logp`` / ``entropy`` exactly as
    one of the built-in distributions (so the fused kernel restates it)."""
    for base in (Categorical, SquashedNormal, Normal):
        if issubclass(distribution_cls, base):
            return (
                distribution_cls.logp is base.logp and distribution_cls.entropy is base.entropy
            )
    return False


class _AttachPrecomputedGrads(torch.autograd.Function):
    """Scalar whose gradient w.r.t. ``inputs`` was already computed by the fused
    kernel; backward scales those gradients by the incoming scalar."""

    @staticmethod
    def forward(ctx: Any, total: torch.Tensor, n_inputs: int, *tensors: torch.Tensor) -> torch.Tensor:
        ctx.grads = tensors[n_inputs:]
        return total.clone()

    @staticmethod
    def backward(ctx: Any, grad_total: torch.Tensor) -> tuple[Any, ...]:
        scaled = tuple(g * grad_total.to(g.dtype) for g in ctx.grads)
        return (None, None, *scaled, *([None] * len(scaled)))


def ppo_losses(
    buffer_batch: TensorDict,
    sample_batch: TensorDict,
    sample_distribution: Distribution,
    /,
    *,
    clip_param: float = 0.2,
    dual_clip_param: None | float = 5.0,
    entropy_coeff: float = 0.0,
    vf_clip_param: float = 1.0,
    vf_coeff: float = 1.0,
) -> TensorDict:
    """Proximal Policy Optimization loss (dual-clipped surrogate, clamped Huber
    value loss, optional entropy bonus), mean-reduced.

    Args:
        buffer_batch: ``[B, ...]`` tensordict with ``"actions"``,
            ``"advantages"``, ``"logp"``, ``"returns"``.
        sample_batch: ``[B, ...]`` tensordict with ``"values"`` from the current
            policy.
        sample_distribution: Distribution built from the current policy's
            features.
        clip_param, dual_clip_param, entropy_coeff, vf_clip_param, vf_coeff:
            As in the reference (``dual_clip_param=None`` disables dual clip).

    Returns:
        Tensordict with scalar ``"entropy"``, ``"policy"``, ``"vf"``, ``"total"``;
        ``total.backward()`` propagates into the features and the values.

    Raises:
        ValueError: under grad mode, with a built-in distribution, a column of ``buffer_batch`` requires a gradient
            (the fused loss forms none for buffer data).

    """
    values = sample_batch[DataKeys.VALUES]
    _require_hip(values, "values")
    dist_cls = type(sample_distribution)
    device = values.device
    if has_fused_loss(dist_cls):
        m = values.shape[0]
        if torch.is_grad_enabled():
            # (the loss kernels form gradients for the features and the values alone: a buffer column that asks for
            # one is refused here, before any launch, never answered with ``None``)
            for key in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.ADVANTAGES, DataKeys.RETURNS):
                if buffer_batch[key].requires_grad:
                    raise ValueError(
                        f"buffer_batch[{key!r}] requires a gradient, which the fused PPO loss does not form: it is"
                        " rollout-buffer data here. Detach it, or compose the loss from torch operations."
                    )
        need_grad = torch.is_grad_enabled() and (
            values.requires_grad
            or any(f.requires_grad for f in sample_distribution.features.values())
        )
        sums, inputs, grads = fused_ppo_loss(
            dist_cls,
            sample_distribution.features,
            values,
            buffer_batch[DataKeys.ACTIONS],
            buffer_batch[DataKeys.LOGP],
            buffer_batch[DataKeys.ADVANTAGES],
            buffer_batch[DataKeys.RETURNS],
            clip_param=clip_param,
            dual_clip_param=dual_clip_param,
            entropy_coeff=entropy_coeff,
            vf_clip_param=vf_clip_param,
            vf_coeff=vf_coeff,
            grad_scale=1.0 / m,
            with_grad=need_grad,
        )
        means = sums / sums[3]
        policy_loss = means[1].float()
        vf_loss = means[2].float()
        total = vf_coeff * means[2] - means[1]
        if entropy_coeff != 0:
            entropy_loss = means[0].float()
            total = total - entropy_coeff * means[0]
        else:
            entropy_loss = torch.tensor([0.0])
        total = total.float()
        if need_grad:
            total = _AttachPrecomputedGrads.apply(total, len(inputs), *inputs, *grads)
        return TensorDict(
            {"entropy": entropy_loss, "policy": policy_loss, "vf": vf_loss, "total": total},
            batch_size=[],
        )

    # Custom distribution: compose the loss from its own logp / entropy with
    # tensor ops on the device (same operation order as the reference).
    import torch.nn.functional as F

    advantages = buffer_batch[DataKeys.ADVANTAGES]
    p_ratio = torch.exp(
        sample_distribution.logp(buffer_batch[DataKeys.ACTIONS]) - buffer_batch[DataKeys.LOGP]
    )
    vf_loss = torch.mean(
        torch.clamp(
            F.smooth_l1_loss(values, buffer_batch[DataKeys.RETURNS], reduction="none"),
            0.0,
            vf_clip_param,
        )
    )
    surr1 = advantages * p_ratio
    surr2 = advantages * torch.clamp(p_ratio, 1 - clip_param, 1 + clip_param)
    clip1 = torch.min(surr1, surr2)
    if dual_clip_param:
        clip2 = torch.max(clip1, dual_clip_param * advantages)
        policy_loss = torch.where(advantages < 0, clip2, clip1).mean()
    else:
        policy_loss = clip1.mean()
    total_loss = vf_coeff * vf_loss - policy_loss
    if entropy_coeff != 0:
        entropy_loss = sample_distribution.entropy().mean()
        total_loss = total_loss - entropy_coeff * entropy_loss
    else:
        entropy_loss = torch.tensor([0.0])
    del device
    return TensorDict(
        {"entropy": entropy_loss, "policy": policy_loss, "vf": vf_loss, "total": total_loss},
        batch_size=[],
    )


# --------------------------------------------------------------------------- #
# Masks, skip connections and the masked sequence functions.
# --------------------------------------------------------------------------- #
FINFO = torch.finfo(torch.float32)


def binary_mask_to_float_mask(mask: torch.Tensor, /) -> torch.Tensor:
    """``0`` / ``1`` -> ``-inf`` / ``0``: a float mask whose ``0`` marks a VALID cell."""
    out = mask.float()
    out = out.masked_fill(mask == 0, float("-inf"))
    return out.masked_fill(mask == 1, 0.0)


def float_mask_to_binary_mask(mask: torch.Tensor, /) -> torch.Tensor:
    """``0`` / ``-inf`` -> ``True`` / ``False``: a boolean mask whose ``True`` marks a VALID cell."""
    out = mask.float()
    out = out.masked_fill(mask == float("-inf"), False)
    return out.masked_fill(mask == 0, True).bool()


def mask_from_lengths(x: torch.Tensor, lengths: torch.Tensor, /) -> torch.Tensor:
    """``[B, T]`` boolean mask of the VALID cells of ``x [B, T, ...]`` whose sequences have ``lengths [B]``."""
    b, t = x.shape[:2]
    lengths = lengths.long().view(-1, 1).expand(b, t)
    steps = torch.arange(t, device=lengths.device, dtype=lengths.dtype).expand(b, t)
    return steps < lengths


def skip_connection(x: torch.Tensor, y: torch.Tensor, /, *, kind: None | str = "cat", dim: int = -1) -> torch.Tensor:
    """``x + y`` (``"residual"``), ``cat([x, y], dim)`` (``"cat"``) or ``y`` (``None``)."""
    if kind == "residual":
        return x + y
    if kind == "cat":
        return torch.cat([x, y], dim=dim)
    if kind is None:
        return y
    raise ValueError(f"No skip connection type for {kind}.")


def _masked_kernels_on() -> bool:
    """``RL8_AMD_MASKED_KERNELS=0`` (read on every call) puts the masked functions on their torch expressions."""
    return os.environ.get("RL8_AMD_MASKED_KERNELS", "1") != "0"


def _kernel_input(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0 and _masked_kernels_on()


def _kernel_mask(mask: None | torch.Tensor, shape: tuple) -> bool:
    return mask is None or (mask.is_cuda and mask.dtype in (torch.bool, torch.uint8)
                            and tuple(mask.shape) == tuple(shape))


def _expand_mask(mask: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    while mask.dim() < x.dim():
        mask = mask.unsqueeze(-1)
    return mask


def _add_log_mask(x: torch.Tensor, mask: None | torch.Tensor) -> torch.Tensor:
    """``x`` with ``clamp(log(mask))`` added: ``-FLT_MAX`` on the padded cells."""
    if mask is None:
        return x
    return x + torch.clamp(torch.log(_expand_mask(mask, x)), FINFO.min, FINFO.max)


def _wants_grad(x: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


class _MaskedAvg(torch.autograd.Function):
    """``rl8_masked_pool_f32`` / ``rl8_masked_pool_backward_f32`` in AVG mode on ``[B, T, ...]``: saves the mask only."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, mask: None | torch.Tensor) -> torch.Tensor:
        b, t = x.shape[:2]
        out, _ = hip.masked_pool(x.view(b, t, -1), mask, hip.POOL_AVG)
        ctx.shape = x.shape
        ctx.save_for_backward(*([] if mask is None else [mask]))
        return out.view(b, *x.shape[2:])

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor) -> tuple[Any, ...]:
        mask = ctx.saved_tensors[0] if ctx.saved_tensors else None
        b, t = ctx.shape[:2]
        dx = hip.masked_pool_backward(dout.contiguous().view(b, -1), mask, None, t, hip.POOL_AVG)
        return dx.view(ctx.shape), None


class _MaskedMax(torch.autograd.Function):
    """The same pair in MAX mode: saves the indices (and the mask, an input)."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, mask: None | torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        b, t = x.shape[:2]
        out, index = hip.masked_pool(x.view(b, t, -1), mask, hip.POOL_MAX)
        ctx.shape = x.shape
        ctx.save_for_backward(index, *([] if mask is None else [mask]))
        index = index.view(b, 1, *x.shape[2:])
        ctx.mark_non_differentiable(index)
        return out.view(b, 1, *x.shape[2:]), index

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor, _dindex: Any) -> tuple[Any, ...]:
        index, *rest = ctx.saved_tensors
        b, t = ctx.shape[:2]
        dx = hip.masked_pool_backward(dout.contiguous().view(b, -1), rest[0] if rest else None, index, t, hip.POOL_MAX)
        return dx.view(ctx.shape), None


class _MaskedLogSoftmax(torch.autograd.Function):
    """``rl8_masked_log_softmax_f32`` / ``..._backward_f32`` along the last dimension: saves its output."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, mask: None | torch.Tensor) -> torch.Tensor:
        k = x.shape[-1]
        out = hip.masked_log_softmax(x.view(-1, k), None if mask is None else mask.view(-1, k)).view(x.shape)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx: Any, dout: torch.Tensor) -> tuple[Any, ...]:
        (out,) = ctx.saved_tensors
        k = out.shape[-1]
        return hip.masked_log_softmax_backward(dout.contiguous().view(-1, k), out.view(-1, k)).view(out.shape), None


class _MaskedSample(torch.autograd.Function):
    """``rl8_masked_categorical_sample_f32`` on ``[B, K]``; the gathered logit's gradient is a one-hot scatter."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, mask: None | torch.Tensor, noise: None | torch.Tensor, seed: int, step: int,
                row_offset: int) -> tuple[torch.Tensor, torch.Tensor]:
        value, index = hip.masked_categorical_sample(x, mask, noise, seed=seed, step=step, row_offset=row_offset)
        index = index.unsqueeze(-1)
        ctx.shape = x.shape
        ctx.save_for_backward(index)
        ctx.mark_non_differentiable(index)
        return value.unsqueeze(-1), index

    @staticmethod
    def backward(ctx: Any, dvalue: torch.Tensor, _dindex: Any) -> tuple[Any, ...]:
        (index,) = ctx.saved_tensors
        dx = torch.zeros(ctx.shape, dtype=dvalue.dtype, device=dvalue.device).scatter_(1, index, dvalue)
        return dx, None, None, None, None, None


def masked_avg(x: torch.Tensor, /, *, mask: None | torch.Tensor = None, dim: int = 1, keepdim: bool = False) -> torch.Tensor:
    """Average of ``x [B, T, ...]`` along ``dim`` over the cells that ``mask [B, T]`` marks VALID (all of them without a
    mask). A row without a valid cell is ``0 / 0 = NaN``, as in the reference."""
    if x.dim() >= 2 and dim % x.dim() == 1 and _kernel_input(x) and _kernel_mask(mask, x.shape[:2]):
        if mask is not None:
            mask = mask.contiguous()
        if _wants_grad(x):
            avg = _MaskedAvg.apply(x, mask)
        else:
            b, t = x.shape[:2]
            avg = hip.masked_pool(x.view(b, t, -1), mask, hip.POOL_AVG)[0].view(b, *x.shape[2:])
        return avg.unsqueeze(1) if keepdim else avg
    if mask is not None:
        mask = _expand_mask(mask, x)
        count = mask.sum(dim=dim, keepdim=True)
        avg = (mask * x).sum(dim=dim, keepdim=True) / count
    else:
        avg = x.mean(dim=dim, keepdim=True)
    return avg if keepdim else avg.squeeze(dim)


def masked_max(x: torch.Tensor, /, *, mask: None | torch.Tensor = None, dim: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """Maximum of ``x [B, T, ...]`` along ``dim`` over the VALID cells (padded ones read as the lowest finite float)
    and its index, both with ``dim`` kept."""
    if x.dim() >= 2 and dim % x.dim() == 1 and _kernel_input(x) and _kernel_mask(mask, x.shape[:2]):
        if mask is not None:
            mask = mask.contiguous()
        if _wants_grad(x):
            return _MaskedMax.apply(x, mask)
        b, t = x.shape[:2]
        out, index = hip.masked_pool(x.view(b, t, -1), mask, hip.POOL_MAX)
        return out.view(b, 1, *x.shape[2:]), index.view(b, 1, *x.shape[2:])
    if mask is not None:
        x = x.masked_fill(~_expand_mask(mask, x).bool(), FINFO.min)
    index = x.argmax(dim=dim, keepdim=True)
    return x.gather(dim, index), index


def masked_log_softmax(x: torch.Tensor, /, *, mask: None | torch.Tensor = None, dim: int = -1) -> torch.Tensor:
    """Log-softmax of ``x`` along ``dim`` with ``clamp(log(mask))`` added first: padded cells sit at the lowest finite
    float, so a row that is padded throughout comes out uniform."""
    if x.dim() >= 1 and dim % x.dim() == x.dim() - 1 and _kernel_input(x) and _kernel_mask(mask, x.shape):
        if mask is not None:
            mask = mask.contiguous()
        if _wants_grad(x):
            return _MaskedLogSoftmax.apply(x, mask)
        k = x.shape[-1]
        return hip.masked_log_softmax(x.view(-1, k), None if mask is None else mask.view(-1, k)).view(x.shape)
    return torch.nn.functional.log_softmax(_add_log_mask(x, mask), dim=dim)


def masked_categorical_sample(
    x: torch.Tensor,
    /,
    *,
    mask: None | torch.Tensor = None,
    dim: int = 1,
    noise: None | torch.Tensor = None,
    noise_stream: None | "distributions.NoiseStream" = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """One categorical draw along the last dimension of the logits ``x`` (with ``clamp(log(mask))`` added), and the
    masked logits gathered along ``dim`` at the drawn classes: ``(logits, classes)``, the classes with a trailing 1.

    ``noise`` (the shape of ``x``) injects the Exp(1) draws ``q`` of ``argmax p / q``; otherwise a HIP ``[B, T]`` input
    draws from ``noise_stream`` (default: ``distributions.default_noise``, the stream ``Distribution.sample`` uses) and
    any other input from ``torch.distributions.Categorical``, as the reference does.

    """
    if (
        x.dim() == 2 and dim % 2 == 1 and _kernel_input(x) and _kernel_mask(mask, x.shape)
        # (a noise that asks for a gradient goes to the torch expression: the node forms none for it)
        and (noise is None or (_kernel_input(noise) and noise.shape == x.shape and not _wants_grad(noise)))
    ):
        seed = step = row_offset = 0
        if noise is None:
            stream = noise_stream or distributions.default_noise
            seed, step, row_offset = stream.seed, stream.next_step(), stream.row_offset
        if mask is not None:
            mask = mask.contiguous()
        if _wants_grad(x):
            return _MaskedSample.apply(x, mask, noise, seed, step, row_offset)
        value, index = hip.masked_categorical_sample(x, mask, noise, seed=seed, step=step, row_offset=row_offset)
        return value.unsqueeze(-1), index.unsqueeze(-1)
    x = _add_log_mask(x, mask)
    if noise is None:
        samples = torch.distributions.Categorical(logits=x).sample().unsqueeze(-1)
    else:
        probs = torch.distributions.Categorical(logits=x).probs
        samples = (probs / noise).argmax(dim=-1).unsqueeze(-1)
    return x.gather(dim, samples), samples
