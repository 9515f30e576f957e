"""The reference's ``rl8.nn`` surface: the functional ops (GAE, the PPO loss and the masked sequence functions, on the
gfx950 kernels where they have one) and the modules."""

from .functional import (
    binary_mask_to_float_mask,
    float_mask_to_binary_mask,
    generalized_advantage_estimate,
    mask_from_lengths,
    masked_avg,
    masked_categorical_sample,
    masked_log_softmax,
    masked_max,
    ppo_losses,
    skip_connection,
)
from .modules import (
    MLP,
    CrossAttention,
    Module,
    PerceiverIOLayer,
    PerceiverLayer,
    PositionalEmbedding,
    SelfAttention,
    SelfAttentionStack,
    SequentialSkipConnection,
    SquaredReLU,
    get_activation,
)

__all__ = [
    "MLP",
    "CrossAttention",
    "Module",
    "PerceiverIOLayer",
    "PerceiverLayer",
    "PositionalEmbedding",
    "SelfAttention",
    "SelfAttentionStack",
    "SequentialSkipConnection",
    "SquaredReLU",
    "binary_mask_to_float_mask",
    "float_mask_to_binary_mask",
    "generalized_advantage_estimate",
    "get_activation",
    "mask_from_lengths",
    "masked_avg",
    "masked_categorical_sample",
    "masked_log_softmax",
    "masked_max",
    "ppo_losses",
    "skip_connection",
]
