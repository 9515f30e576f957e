"""Recurrent PPO: ``RecurrentAlgorithmConfig`` / ``RecurrentAlgorithm``.

API follows the reference's ``src/rl8/algorithms/_recurrent.py``
(``RecurrentAlgorithmConfig`` :29-192, ``collect`` :325-479, ``step`` :481-652):
truncated BPTT over ``seq_len`` steps, recurrent states carried in the rollout
buffer, re-initialised every ``seqs_per_state_reset`` sequences, sequences (not
samples) shuffled into minibatches.

Built on :class:`Algorithm`: same time-major buffer (the ``states`` leaves are
``[H+1][N][layers][hidden]`` slabs, so the per-timestep state carry is a dense
copy, not the reference's strided one), same fused per-timestep launch, same GAE
and fused loss kernels. A minibatch of sequences is assembled by
``rl8_gather_minibatch``: per-sample leaves through the narrow path, the initial
states of each sequence (1 KiB rows) through the wave-per-row path. As in the
feed-forward algorithm, a minibatch that is the whole buffer (the default) is not
shuffled -- its mean does not depend on the order of the sequences: they are laid
sequence-major once per ``step()`` in buffer order and every SGD iteration reads
that copy (the reference draws ``randperm`` and gathers per iteration,
``src/rl8/_utils.py:211-225``; ``bench.py --recurrent --minibatches 4`` times the
shuffled path). Dict observations (a one-level ``Composite``, the feed-forward
algorithm's leaf rules) are held leaf by leaf; their sequences are gathered by
``rl8_gather_sequences``, which also takes byte-wide leaves (bool masks), and the
model receives a tensordict of ``[B, L, ...]`` leaves. A training pass through the
default models is ONE autograd node
(``nn/fused_lstm.py:lstm_heads_forward``: ``_FusedLSTMHeads`` at hidden width 256,
``_NarrowLSTMHeads`` at 64 / 128): the heads' data gradient is formed inside the
backward-through-time kernel.

"""

from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Any

import torch
import torch.amp as amp

from .. import hip
from .._utils import profile_ms
from ..data import (
    CollectStats,
    DataKeys,
    RecurrentAlgorithmHparams,
    RecurrentAlgorithmState,
)
from ..distributions import Categorical
from ..env import EnvFactory
from ..models_recurrent import RecurrentModel, RecurrentModelFactory
from ..nn.functional import fused_ppo_loss, has_fused_loss
from ..policies_recurrent import RecurrentPolicy
from ..specs import Composite
from ..tensordict import TensorDict
from ._feedforward import Algorithm, AlgorithmConfig, _collect_stats_from_raw

#: Rows (sequences x steps) of one forward / backward pass through the LSTM;
#: larger minibatches accumulate over several passes. 2^21 rows of the default
#: 256-wide LSTM keep the pass's activations around 20 GB.
RECURRENT_MAX_ROWS_PER_PASS = 1 << 21


_NO_TIMER = contextlib.nullcontext()


class _LeanRollout:
    """The per-timestep launches of ``collect()`` for the default discrete recurrent
    model on a dummy env, issued straight through the C ABI with addresses computed
    once: LSTM step (new states written into the buffer's next column -- no copies),
    the logits head, the value head, and the fused sampler + ``env.step`` +
    bookkeeping kernel. Same kernels, same arguments, same order as
    ``policy.sample()`` + ``_fused_step`` (tests/test_algorithm_gpu.py:
    ``test_recurrent_lean_and_plumbed_rollouts_agree``); what goes is ~150 us of
    tensordict / autograd-function / ``torch.cat`` host work per timestep, which at
    8192 environments per GPU (BASELINE configs[4]) was twice the kernels' time.
    ``step`` is one of three LSTM-step launches -- the plane step kernel or the fp32
    forward with l = 1 at width 256 (``fused_lstm._plan``), the narrow forward with
    l = 1 on the weights as they are at 64 / 128 (no packs, no planes, no plan) --
    and then ``_heads_and_env``, the same at every width."""

    TIMER_EVERY = 16  # with hip.timer enabled, only every 16th timestep is bracketed by events

    def __init__(self, algo: "RecurrentAlgorithm", deterministic: bool) -> None:
        from ..nn import fused_lstm

        self.lib = hip.load()
        model = algo.policy.model
        tm, stm = algo._tm, algo._tm_states
        self.n = n = algo.local_num_envs
        self.d_in = int(tm[DataKeys.OBS].shape[-1])
        self.k = int(model.feature_head.out_features)
        dev = tm[DataKeys.OBS].device
        lstm = model.lstm
        self.hidden = int(lstm.hidden_size)
        self.narrow = self.hidden in hip.LSTM_NARROW_HIDDEN  # (``available`` has said "narrow" or "256")
        self.split = not self.narrow and fused_lstm._plan(lstm.input_size, n).forward_planes
        # what the LSTM step reads, kept alive on self (parameters are leaf tensors: .detach() shares storage)
        if self.narrow:
            self.lstm_weights = [p.detach().contiguous() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0,
                                                                   lstm.bias_hh_l0)]
        elif self.split:  # bf16-plane step kernel: W_hh planes, [w_ih | bias] rows, planes of h_{t-1}
            self.lstm_weights = list(fused_lstm._packs(lstm, "split"))
        else:
            self.lstm_weights = [fused_lstm._packs(lstm, "step")]
        self.params = [p.detach().contiguous() for p in (model.feature_head.weight, model.feature_head.bias,
                                                         model.vf_head.weight, model.vf_head.bias)]
        # the heads' entries and the names they are timed under; below 256 they take the width after hs (and n)
        if self.narrow:
            self.width: tuple = (self.hidden,)
            self.sampler_heads = ("rl8_rollout_step_dummy_heads_narrow_f32", "rollout_step_dummy_heads_narrow")
            self.heads = ("rl8_linear_heads_narrow_forward_pair_f32", "rl8_linear_heads_narrow_forward_f32",
                          "linear_heads_narrow_forward")
        else:
            self.width = ()
            self.sampler_heads = ("rl8_rollout_step_dummy_heads_f32", "rollout_step_dummy")
            self.heads = ("rl8_linear_heads_forward_pair_f32", "rl8_linear_heads_forward_f32", "linear_heads_forward")
        cache = algo.__dict__.setdefault("_lean_scratch", {})
        key = (n, self.k, str(dev), self.hidden)
        if cache.get("key") != key:
            cache.update(key=key, hs=torch.empty(n, self.hidden, device=dev),
                         logits=torch.empty(n, self.k, device=dev), value=torch.empty(n, 1, device=dev),
                         planes=None if self.narrow else hip.lstm_state_planes(n, dev, copies=2))
        self.hs, self.logits, self.value, self.planes = cache["hs"], cache["logits"], cache["value"], cache["planes"]
        rdr = tm.get(DataKeys.REVERSED_DISCOUNTED_RETURNS)

        def column(t: torch.Tensor) -> tuple[int, int]:
            return t.data_ptr(), t.stride(0) * t.element_size()

        self.obs, self.act, self.logp = column(tm[DataKeys.OBS]), column(tm[DataKeys.ACTIONS]), column(tm[DataKeys.LOGP])
        self.val, self.rew = column(tm[DataKeys.VALUES]), column(tm[DataKeys.REWARDS])
        self.rdr = column(rdr) if rdr is not None else None
        self.h, self.c = column(stm[DataKeys.HIDDEN_STATES]), column(stm[DataKeys.CELL_STATES])
        self.state_ptr = algo.env.state.data_ptr()
        self.gamma = float(torch.tensor(algo.hparams.gamma, dtype=torch.float32))
        self.seed, self.env_offset = algo.noise.seed, algo.env.env_offset
        self.deterministic = int(deterministic)
        self.lstm_ptrs = [t.data_ptr() for t in self.lstm_weights]
        self.ptrs = [t.data_ptr() for t in (self.hs, self.logits, self.value, *self.params)]
        self.planes_ptr, self.planes_half = (self.planes.data_ptr(), self.planes.numel() // 2) if self.split else (None, 0)
        self.planes_of = -1   # timestep whose hidden state the planes buffer (t & 1) holds (-1: none)
        # two-way categorical + value head: evaluated inside the timestep's last kernel (switched off: two launches)
        self.fuse_heads = self.k == 2 and fused_lstm._rollout_fuse_heads()

    @staticmethod
    def available(algo: "RecurrentAlgorithm") -> bool:
        from ..env import DummyEnv
        from ..models_recurrent import DefaultDiscreteRecurrentModel
        from ..nn import fused_lstm

        model = algo.policy.model
        if DataKeys.OBS not in algo._tm:  # dict observations (held leaf by leaf): the lean launches read ONE slab
            return False
        if type(model) is not DefaultDiscreteRecurrentModel or not isinstance(algo.env, DummyEnv):
            return False
        if algo.policy.distribution_cls is not Categorical or model.action_spec.shape[0] != 1:
            return False
        # (the buffer may live on the CPU in tests of this rule: the module's family and the dtypes, not the device)
        return bool(fused_lstm._family(model.lstm) in ("256", "narrow")
                    and algo._tm[DataKeys.OBS].dtype == torch.float32 and model.vf_head.bias is not None
                    and all(p.dtype == torch.float32 for p in model.parameters()))

    def step(self, t: int, noise: None | torch.Tensor, step_id: int) -> None:
        lib, n, stream, H = self.lib, self.n, hip._stream(), self.hidden
        at = lambda col, i: col[0] + i * col[1]  # noqa: E731
        timed = hip.timer.enabled and t % self.TIMER_EVERY == 0
        hs = self.ptrs[0]
        if self.narrow:
            # h_t and c_t straight into the state buffers' next column, a dense [N][H] slab for one layer
            w_ih, w_hh, b_ih, b_hh = self.lstm_ptrs
            with hip._timed("lstm_narrow_forward", n) if timed else _NO_TIMER:
                hip._check(lib.rl8_lstm_narrow_forward_f32(at(self.obs, t), n, 1, self.d_in, at(self.h, t), at(self.c, t), w_ih,
                                                           w_hh, b_ih, b_hh, H, hs, at(self.h, t + 1), at(self.c, t + 1), None,
                                                           None, stream), "rl8_lstm_narrow_forward_f32")
        elif self.split:
            packed, wb = self.lstm_ptrs
            planes = self.planes_ptr
            p_in, p_out = planes + (t & 1) * self.planes_half, planes + ((t + 1) & 1) * self.planes_half
            if self.planes_of != t:
                # the first timestep, or one whose states were just re-initialised: planes of h_t
                # from the buffer; otherwise the previous step's kernel has left them
                hip._check(lib.rl8_lstm_split_state(at(self.h, t), H, n, p_in, stream), "rl8_lstm_split_state")
            with hip._timed("lstm_step", n) if timed else _NO_TIMER:
                hip._check(lib.rl8_lstm_step_split_f32(at(self.obs, t), self.d_in, self.d_in, p_in, at(self.c, t), H,
                                                       packed, wb, n, at(self.h, t + 1), H, at(self.c, t + 1), H, None,
                                                       0, p_out, stream), "rl8_lstm_step_split_f32")
            self.planes_of = t + 1
            hs = at(self.h, t + 1)  # the heads read h_t where the buffer keeps it
        else:
            (packed,) = self.lstm_ptrs
            with hip._timed("lstm_forward", n) if timed else _NO_TIMER:
                hip._check(lib.rl8_lstm_forward_f32(at(self.obs, t), n, 1, self.d_in, at(self.h, t), at(self.c, t), packed,
                                                    hs, at(self.h, t + 1), at(self.c, t + 1), None, None, stream),
                           "rl8_lstm_forward_f32")
        self._heads_and_env(t, hs, noise, step_id, timed, stream)

    def _heads_and_env(self, t: int, hs: int, noise: None | torch.Tensor, step_id: int, timed: bool, stream) -> None:
        """The rest of a timestep, from ``h_t`` at ``hs``: the two heads inside the sampler + env.step + bookkeeping
        kernel (one launch instead of two), or both heads in one pass over ``h_t`` (else one launch each) and then
        that kernel on their outputs."""
        lib, n, width = self.lib, self.n, self.width
        _, logits, value, w_pol, b_pol, w_vf, b_vf = self.ptrs
        at = lambda col, i: col[0] + i * col[1]  # noqa: E731
        env = (noise.data_ptr() if noise is not None else None, self.state_ptr, at(self.act, t), at(self.logp, t),
               at(self.val, t), at(self.rew, t), at(self.obs, t + 1), at(self.rdr, t) if self.rdr else None,
               at(self.rdr, t + 1) if self.rdr else None, self.gamma, n, self.seed, step_id, self.env_offset,
               self.deterministic, stream)
        if self.fuse_heads:
            entry, name = self.sampler_heads
            with hip._timed(name, n) if timed else _NO_TIMER:
                hip._check(getattr(lib, entry)(hs, *width, w_pol, b_pol, w_vf, b_vf, *env), entry)
            return
        pair, single, name = self.heads
        with hip._timed(name, n) if timed else _NO_TIMER:
            if self.k + 1 <= hip.HEADS_MAX_OUT:
                hip._check(getattr(lib, pair)(hs, n, *width, w_pol, b_pol, self.k, logits, w_vf, b_vf, 1, value, stream), pair)
            else:
                hip._check(getattr(lib, single)(hs, n, *width, w_pol, b_pol, self.k, logits, stream), single)
                hip._check(getattr(lib, single)(hs, n, *width, w_vf, b_vf, 1, value, stream), single)
        with hip._timed("rollout_step_dummy", n) if timed else _NO_TIMER:
            hip._check(lib.rl8_rollout_step_dummy_f32(1, 0, logits, None, value, *env), "rl8_rollout_step_dummy_f32")


@dataclass
class RecurrentAlgorithmConfig(AlgorithmConfig):
    """Configuration of a recurrent PPO algorithm: :class:`AlgorithmConfig` plus
    the truncated-BPTT settings."""

    model: None | RecurrentModel = None  # type: ignore[assignment]
    model_cls: None | RecurrentModelFactory = None  # type: ignore[assignment]
    #: Truncated backpropagation-through-time sequence length (a factor of
    #: ``horizon``).
    seq_len: int = 4
    #: Sequences collected between re-initialisations of the recurrent states
    #: (negative: never after the first).
    seqs_per_state_reset: int = 8

    def build(self, env_cls: EnvFactory) -> "RecurrentAlgorithm":  # type: ignore[override]
        algo = RecurrentAlgorithm(env_cls, config=self)
        algo.validate()
        return algo


class RecurrentAlgorithm(Algorithm):
    """Recurrent PPO (LSTM policies) with the usual stabilising tricks."""

    hparams: RecurrentAlgorithmHparams
    policy: RecurrentPolicy  # type: ignore[assignment]
    state: RecurrentAlgorithmState  # type: ignore[assignment]
    #: Issue the rollout's per-timestep launches through :class:`_LeanRollout` when the
    #: model / env pair allows it (False: always through ``policy.sample()``).
    lean_rollout: bool = True
    #: Dict observations under the feed-forward algorithm's leaf rules, with a model of the caller's (``model`` or
    #: ``model_cls``): there is no default recurrent model for a dict.
    composite_observations = True

    def __init__(self, env_cls: EnvFactory, /, config: None | RecurrentAlgorithmConfig = None) -> None:
        config = config or RecurrentAlgorithmConfig()
        self._recurrent_config = config
        super().__init__(env_cls, config=config)

    # -- construction hooks ---------------------------------------------------
    def _make_policy(self, config: Any, device: str) -> RecurrentPolicy:
        return RecurrentPolicy(
            self.env.observation_spec,
            self.env.action_spec,
            model=config.model,
            model_cls=config.model_cls,
            model_config=config.model_config,
            distribution_cls=config.distribution_cls,
            device=device,
        )

    def _extra_buffer_specs(self) -> dict[str, Any]:
        return {DataKeys.STATES: self.policy.state_spec}

    def _default_minibatch_size(self, config: Any, num_envs: int, horizon: int) -> int:
        return num_envs * (horizon // config.seq_len)

    def _make_hparams(self, **common: Any) -> RecurrentAlgorithmHparams:
        return RecurrentAlgorithmHparams(
            seq_len=self._recurrent_config.seq_len,
            seqs_per_state_reset=self._recurrent_config.seqs_per_state_reset,
            **common,
        )

    def _make_state(self) -> RecurrentAlgorithmState:
        return RecurrentAlgorithmState()

    def _composite_obs_leaves(self) -> None | list[str]:
        leaves = super()._composite_obs_leaves()
        config = self._recurrent_config
        if leaves is not None and config.model is None and config.model_cls is None:
            raise NotImplementedError(
                "rl8_amd has no default recurrent model for dict observations: pass `model` or `model_cls`"
                " (composite specs are outside the accelerated path)."
            )
        return leaves

    # -- helpers ----------------------------------------------------------------
    def _obs_batch(self, t: int) -> TensorDict:
        """Column ``t`` of the observations as the model's ``[N, 1]`` input batch: the slab, or a tensordict of the
        leaves' slabs for dict observations."""
        n = self.local_num_envs
        if self._tm_obs is None:
            return TensorDict({DataKeys.OBS: self._tm[DataKeys.OBS][t].unsqueeze(1)}, batch_size=[n, 1])
        obs = TensorDict({leaf: storage[t].unsqueeze(1) for leaf, storage in self._tm_obs.items()}, batch_size=[n, 1])
        return TensorDict({DataKeys.OBS: obs}, batch_size=[n, 1])

    def _state_slabs(self, t: int) -> TensorDict:
        """States at column ``t`` as a ``[N, 1, layers, hidden]`` tensordict."""
        n = self.local_num_envs
        return TensorDict(
            {k: v[t].unsqueeze(1) for k, v in self._tm_states.items()}, batch_size=[n, 1]
        )

    def _samples_per_minibatch(self) -> int:
        return self.hparams.sgd_minibatch_size * self.hparams.seq_len

    # -- collect ------------------------------------------------------------------
    def collect(
        self,
        *,
        env_config: None | dict[str, Any] = None,
        deterministic: bool = False,
    ) -> CollectStats:
        """As :meth:`Algorithm.collect`, additionally carrying the recurrent
        states from column to column and re-initialising them at sequence
        boundaries according to ``seqs_per_state_reset``."""
        hp = self.hparams
        H, N = hp.horizon, self.local_num_envs
        tm, stm = self._tm, self._tm_states
        rdr = tm.get(DataKeys.REVERSED_DISCOUNTED_RETURNS)
        self._flat_full = None  # (a sequence-major copy of the buffer this collect() overwrites)
        self._release_step_caches()
        with profile_ms() as collect_timer:
            env_was_reset = self._reset_or_carry(env_config)
            for v in stm.values():  # :380-382
                v[0].copy_(v[H])

            fused = self._fusable()
            lean = None
            if fused and self.lean_rollout and _LeanRollout.available(self):
                lean = _LeanRollout(self, deterministic)
            gamma = float(torch.tensor(hp.gamma, dtype=torch.float32))
            for t in range(H):
                if self.state.seqs and hp.seqs_per_state_reset < 0:
                    pass
                elif not (t % hp.seq_len) and not (self.state.seqs % hp.seqs_per_state_reset):
                    init = self.policy.init_states(N)  # :385-392
                    for k, v in stm.items():
                        v[t].copy_(init[k])
                    if lean is not None:
                        lean.planes_of = -1  # h_t was replaced: its planes must be re-made
                noise_t = self.injected_noise[t] if self.injected_noise is not None else None
                step_id = self.noise.next_step()
                if lean is not None:
                    lean.step(t, noise_t.contiguous() if noise_t is not None else None, step_id)
                    if not ((t + 1) % hp.seq_len):
                        self.state.seqs += 1
                    continue
                in_batch = self._obs_batch(t)
                if fused:
                    sample, new_states = self.policy.sample(
                        in_batch, self._state_slabs(t), deterministic=deterministic, inplace=False,
                        requires_grad=False, return_actions=False, return_logp=False, return_values=True,
                    )
                    self._fused_step(sample[DataKeys.FEATURES], sample[DataKeys.VALUES], noise_t, t, gamma,
                                     step_id, deterministic)
                else:
                    self.policy.injected_noise = noise_t
                    self.noise.step = step_id
                    sample, new_states = self.policy.sample(
                        in_batch, self._state_slabs(t), deterministic=deterministic, inplace=False,
                        requires_grad=False, return_actions=True, return_logp=True, return_values=True,
                    )
                    self._scatter_step(sample, self.env.step(sample[DataKeys.ACTIONS]), t, gamma)
                for k, v in stm.items():  # :428
                    v[t + 1].copy_(new_states[k])
                if not ((t + 1) % hp.seq_len):
                    self.state.seqs += 1

            # Bootstrap value at the last observation and state (:433-446).
            sample, _ = self.policy.sample(
                self._obs_batch(H), self._state_slabs(H), deterministic=deterministic, inplace=False,
                requires_grad=False, return_actions=False, return_logp=False, return_values=True,
            )
            tm[DataKeys.VALUES][H].copy_(sample[DataKeys.VALUES])

            # Stats.  The reference's recurrent variant slices rewards [:, 1:-1]
            # (:449), unlike the feed-forward [:, :-1]; reward_scale still uses
            # rdr[:, 1:].  Two passes of the stats kernel reproduce both.
            rewards = self.buffer[DataKeys.REWARDS]
            if H >= 2:
                raw = hip.rollout_stats(rewards[:, 1:], None)
            else:
                raw = torch.full((12,), float("nan"), dtype=torch.float64, device=rewards.device)
            if rdr is not None:
                raw_rdr = hip.rollout_stats(rewards, self.buffer[DataKeys.REVERSED_DISCOUNTED_RETURNS])
                raw = torch.cat([raw[:10], raw_rdr[10:]])
                rdr_count = float(N * H)
            values = self.shards.combine_rollout_stats(raw)
            collect_stats, _ = _collect_stats_from_raw(values)
            if rdr is not None:
                world = self.shards.world_size
                _, reward_scale = _collect_stats_from_raw(
                    values[:5] + [rdr_count * world] + values[6:]
                )
            else:
                reward_scale = 1.0
        return self._finish_collect(collect_stats, reward_scale, env_was_reset, collect_timer())

    # -- step ---------------------------------------------------------------------
    def _release_step_caches(self) -> None:
        from ..nn import fused_lstm

        super()._release_step_caches()

        fused_lstm.clear_state_cache()  # the planes of the initial hidden states, shared by the SGD iterations

    def _iter_minibatches(self, sgd_iter: int):
        """Minibatches of SEQUENCES: per-sample leaves as ``[B*L, ...]`` in
        (sequence, step) order (dict observations: a dict of such leaves), and each
        sequence's initial recurrent states ``[B, layers, hidden]``."""
        hp = self.hparams
        H, L = hp.horizon, hp.seq_len
        local_seqs = self.local_num_envs * (H // L)
        local_mb = hp.sgd_minibatch_size // self.shards.world_size
        state_keys = list(self._tm_states)
        whole = local_mb >= local_seqs and self.injected_permutations is None
        if whole:
            from ..nn import fused_lstm

            fused_lstm.SHARE_H0_PLANES = True  # until _release_step_caches(): every pass reads the same initial states
        if whole and self._flat_full is not None:
            yield self._flat_full
            return
        # One minibatch that is the whole buffer: its mean does not depend on the order of the sequences (the
        # feed-forward algorithm's full-buffer rule), so they are laid sequence-major ONCE per step() in buffer order
        # and every SGD iteration reads that copy -- no permutation, one gather instead of num_sgd_iters.
        perm = (torch.arange(local_seqs, device=self._tm[DataKeys.LOGP].device) if whole
                else self._permutation(sgd_iter, local_seqs))
        steps = torch.arange(L, device=perm.device)
        for seq_index in torch.split(perm, local_mb):
            # reference sequence id q = env * (H/L) + s  ->  sample ids q*L + j
            sample_ids = (seq_index[:, None] * L + steps[None, :]).reshape(-1).contiguous()
            # (the whole buffer in order: a transposition through LDS tiles, every byte moved once -- the indexed
            # gather reads a 64-byte sector per 4-byte cell of a time-major leaf)
            keys = [k for k in self.TRAIN_KEYS if k != DataKeys.OBS or self._tm_obs is None]
            gathered = hip.gather_minibatch(None if whole else sample_ids, H, [self.buffer[k] for k in keys])
            batch: dict[str, Any] = dict(zip(keys, gathered))
            if self._tm_obs is not None:
                # the leaves of a dict observation, byte-wide ones (bool masks) included: whole sequences in one launch
                obs = self.buffer[DataKeys.OBS]
                leaves = hip.gather_sequences(None if whole else seq_index.contiguous(), L, H,
                                              [obs[leaf] for leaf in self._tm_obs])
                batch[DataKeys.OBS] = dict(zip(self._tm_obs, leaves))
            first_ids = (seq_index * L).contiguous()
            states = hip.gather_minibatch(
                first_ids, H, [self.buffer[DataKeys.STATES][k] for k in state_keys]
            )
            batch["_states"] = dict(zip(state_keys, states))
            batch["_num_seqs"] = seq_index.numel()
            if whole:
                self._flat_full = batch  # (dropped at the end of step(), with the buffer it was read from)
            yield batch

    def _minibatch_forward_backward(
        self, batch: dict[str, Any], entropy_coeff: float, grad_scale: float
    ) -> torch.Tensor:
        hp = self.hparams
        L = hp.seq_len
        num_seqs = batch["_num_seqs"]
        dist_cls = self.policy.distribution_cls
        # A user's Distribution: the loss is composed from its own logp / entropy with device tensor ops, as the
        # reference does with whatever class it was given (src/rl8/algorithms/_recurrent.py:560-585) -- the
        # feed-forward algorithm's rule (Algorithm._composed_loss_backward), here per pass of sequences.
        fused = has_fused_loss(dist_cls)
        seqs_per_pass = max(1, min(self.max_rows_per_pass, RECURRENT_MAX_ROWS_PER_PASS) // L)
        total_sums: None | torch.Tensor = None
        scale = None
        if hp.enable_amp:
            scale = self.grad_scaler.scale(torch.ones((), device=batch[DataKeys.LOGP].device))
        for start in range(0, num_seqs, seqs_per_pass):
            stop = min(num_seqs, start + seqs_per_pass)
            b = stop - start
            rows = slice(start * L, stop * L)
            if self._tm_obs is None:
                obs = batch[DataKeys.OBS][rows].reshape(b, L, *batch[DataKeys.OBS].shape[1:])
            else:
                obs = TensorDict({leaf: v[rows].reshape(b, L, *v.shape[1:]) for leaf, v in batch[DataKeys.OBS].items()},
                                 batch_size=[b, L])
            states = TensorDict(
                {k: v[start:stop].unsqueeze(1) for k, v in batch["_states"].items()}, batch_size=[b, 1]
            )
            with amp.autocast("cuda", enabled=hp.enable_amp):
                sample, _ = self.policy.sample(
                    TensorDict({DataKeys.OBS: obs}, batch_size=[b, L]), states, deterministic=False,
                    inplace=False, requires_grad=True, return_actions=False, return_logp=False,
                    return_values=True,
                )
            if fused:
                sums, inputs, grads = fused_ppo_loss(
                    dist_cls, sample[DataKeys.FEATURES], sample[DataKeys.VALUES], batch[DataKeys.ACTIONS][rows],
                    batch[DataKeys.LOGP][rows], batch[DataKeys.ADVANTAGES][rows], batch[DataKeys.RETURNS][rows],
                    clip_param=hp.clip_param, dual_clip_param=hp.dual_clip_param, entropy_coeff=entropy_coeff,
                    vf_clip_param=hp.vf_clip_param, vf_coeff=hp.vf_coeff, grad_scale=grad_scale,
                )
                if scale is not None:
                    grads = [g * scale.to(g.dtype) for g in grads]
                torch.autograd.backward(inputs, grads)
            else:
                chunk = {k: batch[k][rows] for k in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.ADVANTAGES,
                                                     DataKeys.RETURNS)}
                sums = self._composed_loss_backward(sample[DataKeys.FEATURES], sample[DataKeys.VALUES], chunk,
                                                    entropy_coeff, grad_scale, scale)
            total_sums = sums if total_sums is None else total_sums + sums
        assert total_sums is not None
        return total_sums

    # -- validate -------------------------------------------------------------------
    def validate(self) -> None:
        """Shape checks on one reset / sample / step round trip (:654-756)."""
        n = self.local_num_envs
        obs = self.env.reset()
        self.env.observation_spec.assert_is_in(obs)
        try:
            self.buffer[DataKeys.OBS][:, 0, ...] = obs
        except RuntimeError as e:
            raise AssertionError(
                f"The observation from {self.env.reset.__qualname__} doesn't match the"
                " observation spec shape."
            ) from e
        states = self.policy.init_states(n)
        try:
            self.buffer[DataKeys.STATES][:, 0, ...] = states
        except RuntimeError as e:
            raise AssertionError(
                "The recurrent states from the policy don't match the state spec."
            ) from e
        sample_batch, out_states = self.policy.sample(
            self.buffer[:, :1, ...].select(DataKeys.OBS),
            self.buffer[DataKeys.STATES][:, :1, ...],
            deterministic=False, inplace=False, requires_grad=False, return_actions=True,
            return_logp=True, return_values=True,
        )
        actions = sample_batch[DataKeys.ACTIONS]
        assert actions.ndim >= 2, (
            "Actions must be at least 2D and have shape ``[N, ...]`` (where ``N`` is"
            " the number of independent elements or environment instances, and ``...``"
            " is any number of additional dimensions)."
        )
        self.env.action_spec.assert_is_in(actions)
        try:
            self.buffer[DataKeys.ACTIONS][:, 0, ...] = actions
            self.buffer[DataKeys.STATES][:, 1, ...] = out_states
        except RuntimeError as e:
            raise AssertionError(
                "The action or states sampled from the policy don't match their specs."
            ) from e
        assert sample_batch[DataKeys.LOGP].shape == torch.Size([n, 1]), (
            "Action log probabilities must be 2D and have shape ``[N, 1]`` (where ``N``"
            " is the number of independent elements or environment instances)."
        )
        assert sample_batch[DataKeys.VALUES].shape == torch.Size([n, 1]), (
            "Expected value estimates must be 2D and have shape ``[N, 1]`` (where ``N``"
            " is the number of independent elements or environment instances)."
        )
        out_batch = self.env.step(actions)
        self.env.observation_spec.assert_is_in(out_batch[DataKeys.OBS])
        assert out_batch[DataKeys.REWARDS].shape == torch.Size([n, 1]), (
            "Rewards must be 2D and have shape ``[N, 1]`` (where ``N`` is the number of"
            " independent elements or environment instances)."
        )
        # validate() must not leave anything behind in the buffer
        self._reset_buffer()
        for storage in (self._tm_obs or {None: self._tm[DataKeys.OBS]}).values():
            storage[self.hparams.horizon].zero_()
        for v in self._tm_states.values():
            v.zero_()


__all__ = ["RecurrentAlgorithm", "RecurrentAlgorithmConfig", "Composite"]
