"""The default policy / value tower as fused gfx950 kernels.

``Linear(d_in, 256) -> ReLU -> Linear(256, 256) -> ReLU -> Linear(256, n_out)``
(``src/rl8/models/_feedforward.py:336-362`` of the reference) runs as one forward
kernel and two backward kernels on the matrix cores -- fp16-plane products at fp32
accuracy where a plane kernel serves the width, fp32 MFMA elsewhere (``_plan`` decides
per call) -- instead of ~8 (forward) / ~20 (backward) eager launches whose 256-wide
activations each make an HBM round trip. Parameters stay ordinary ``torch.nn.Linear``
weights; this module only changes how the tower is evaluated.

Towers of hidden width 64 or 128 (same structure, ``d_in <= 16``, ``n_out <= 8``) run
their own kernel family (``mlp_narrow_kernels.hip``, ``_NarrowTower``): fp32 MFMA for
layer 2, nothing saved by the forward, activations recomputed by the one backward
kernel.  They are never recorded for rollout replay.  An input that asks for its
gradient (a tower behind a learned encoder) gets it from the same backward launch
(``rl8_mlp_narrow_backward_dx_f32``).

The same towers with an affine ``BatchNorm1d`` behind layer 1 (family ``"narrow_bn"``: the
two towers of ``MLPTrader`` and ``TransformerTrader``) run on those kernels too, opt-in with
``RL8_AMD_BATCHNORM_TOWERS=1``: the norm is folded into layer 1 from the batch's first and
second moments of x (``_NarrowBatchNormTower``; the algebra stands above it, and
``batchnorm_tower_reference`` is its torch expression).

Width-256 towers whose first layer reads 17 to 128 floats (family "wide input",
``mlp_wide_in_kernels.hip``, ``_WideInputTower``) run in fp32 MFMA throughout: layer 1 too is
a matrix-core product, the forward saves h1 and h2, and the backward walks the rows in
segments (dW2 alone on exact bf16 planes, ``WIDE_INPUT_DW2_PLANES``).  ``RL8_AMD_WIDE_INPUT_TOWERS=0`` sends them to the torch modules.

Width-256 towers whose heads have 9 to 128 outputs in all, behind 1 to 128 inputs (family "wide head",
``mlp_wide_out_kernels.hip``), run through the same node: there the head, ``dout @ W3`` and dW3 are
matrix-core products as well.  ``RL8_AMD_WIDE_HEAD_TOWERS=0`` sends them to the torch modules.

``tower_forward`` falls back to the module's own eager path whenever the tower
is none of these shapes (other widths, activations, other norm layers, non-HIP or
non-fp32 inputs), so custom models are unaffected.

Under ``enable_amp`` (torch autocast) the fused towers still run, at fp32 accuracy: that is
at least the precision autocast asks for, and on MI355X it is also ~5x faster than
the autocast path of the same modules (37 vs 8 M transitions/s on the headline
config), whose casts and elementwise launches dominate at this width.

"""

from __future__ import annotations

import contextlib
import dataclasses
import functools
import os
from typing import Sequence

import torch
import torch.nn as nn

from .. import hip
from . import piecewise_mlp

#: Set to False to evaluate towers with eager PyTorch (A/B comparisons).
ENABLED = True

#: How the 256x256 product of the forward kernel is formed: "f16" = both fp32
#: operands scaled by powers of two (per activation row / per weight matrix) and
#: split into two fp16 planes, three plane products per 16 k on the fp16 matrix
#: pipe, fp32 accumulate (fp32 accuracy: same fp64 bars as the others);
#: "f32" = v_mfma_f32_32x32x2_f32 (2.7x slower; also what widths without a plane
#: kernel run).  ``RL8_AMD_TOWER_GEMM`` / ``RL8_AMD_TOWER_FORWARD_GEMM`` /
#: ``RL8_AMD_TOWER_BACKWARD_GEMM`` override.  Read on every call (``_plan``): tests
#: and ``bench.py`` change them at run time.
FORWARD_GEMM = os.environ.get("RL8_AMD_TOWER_FORWARD_GEMM", os.environ.get("RL8_AMD_TOWER_GEMM", "f16"))
#: Same choice for the data-gradient product of the backward pass (the weight
#: gradient runs on fp16 planes scaled per output column, ``hip`` / mlp_split_kernels.hip).
BACKWARD_GEMM = os.environ.get("RL8_AMD_TOWER_BACKWARD_GEMM", os.environ.get("RL8_AMD_TOWER_GEMM", "f16"))
for _name, _value in (("forward", FORWARD_GEMM), ("backward", BACKWARD_GEMM)):
    if _value not in ("f16", "f32"):
        raise ValueError(f"RL8_AMD_TOWER_GEMM / RL8_AMD_TOWER_{_name.upper()}_GEMM = {_value!r}: the towers' {_name} product"
                         " runs as 'f16' (fp16 planes, default) or 'f32' (fp32 MFMA); 'split' no longer exists")


def _packed(layer: nn.Linear, transposed: bool, planes: bool) -> torch.Tensor:
    """MFMA-fragment-ordered copy of ``layer.weight`` (fp16 planes or fp32), cached ON
    the layer and re-made when the optimizer has changed the weight (version counter)
    or the weight tensor has been replaced / moved."""
    w2 = layer.weight
    cache = layer.__dict__.setdefault("_rl8_w2_packs", {})
    hit = cache.get((transposed, planes))
    if hit is not None and hit[0] == w2._version and hit[1] == w2.data_ptr():
        return hit[2]
    pack = hip.mlp_pack_w2_f16 if planes else hip.mlp_pack_w2
    packed = pack(w2, transposed=transposed)
    cache[(transposed, planes)] = (w2._version, w2.data_ptr(), packed)
    return packed


def _packed_gate(layer: nn.Linear, w3: torch.Tensor, w3_key: tuple) -> torch.Tensor:
    """``hip.mlp_pack_w2_f16_gate(layer.weight, w3)``, cached on the layer like ``_packed`` and re-made when
    either weight has changed. ``w3_key`` identifies the head PARAMETERS (version counters and addresses):
    ``w3`` itself is a fresh ``torch.cat`` temporary for multi-head towers, whose version is always 0 and whose
    address the caching allocator may hand out again."""
    w2 = layer.weight
    cache = layer.__dict__.setdefault("_rl8_w2_packs", {})
    hit = cache.get("gate")
    key = (w2._version, w2.data_ptr(), w3_key, tuple(w3.shape))
    if hit is not None and hit[0] == key:
        return hit[1]
    packed = hip.mlp_pack_w2_f16_gate(w2, w3)
    cache["gate"] = (key, packed)
    return packed


@functools.lru_cache(maxsize=None)
def _planes_supported(d_in: int, n_out: int) -> tuple[bool, bool]:
    """(plane forward, plane backward) compiled for this width: fixed by the build, asked once per width."""
    return hip.mlp_forward_f16_supports(d_in, n_out), hip.mlp_backward_f16_supports(d_in, n_out)


@dataclasses.dataclass(frozen=True)
class _TowerPlan:
    """The kernels one tower call runs, forward and backward: made once by ``_plan`` and saved on ``ctx`` so that the
    backward runs what its forward prepared for."""

    #: forward on fp16 planes (saves the gate bits of h2); else fp32 MFMA (saves h1 and h2)
    forward_planes: bool
    #: data gradient on fp16 planes (reads the plane forward's gate bits, recomputes h1); else fp32 MFMA
    backward_planes: bool
    #: dW2 on fp16 planes -- the fused weight-gradient kernel, or ``mlp_wgrad_split`` behind the fp32 data gradient
    wgrad_planes: bool
    #: the rank-one gate kernels may run (``hip.mlp_gates_on``)
    gates: bool
    #: one output, or two with the pair hint, and gates on: the backward is expected to take the gate kernels
    rank_one: bool

    @property
    def keep_h1(self) -> bool:
        """The plane forward stores h1: only the fp32 data gradient reads it."""
        return not self.backward_planes

    @property
    def gate_only(self) -> bool:
        """The forward keeps the gate bits of h2 alone (no h2 store, no h2 read)."""
        return self.backward_planes and self.rank_one

    @property
    def recordable(self) -> bool:
        """Planes both ways: the rollout record / replay path.  (The wide-input and wide-head families have no planes
        and no plan: ``tower_forward`` returns before the record and the replay are asked.)"""
        return self.backward_planes


def _plan(d_in: int, n_out: int, pair: bool) -> _TowerPlan:
    """The one place the tower routes are decided; reads the switches as they are now."""
    fwd_ok, bwd_ok = _planes_supported(d_in, n_out)
    forward_planes = FORWARD_GEMM == "f16" and fwd_ok
    gates = hip.mlp_gates_on()
    return _TowerPlan(forward_planes=forward_planes,
                      # (the plane data gradient reads the gate bits only the plane forward saves)
                      backward_planes=forward_planes and BACKWARD_GEMM == "f16" and bwd_ok,
                      wgrad_planes=BACKWARD_GEMM == "f16",
                      gates=gates,
                      rank_one=gates and (n_out == 1 or (n_out == 2 and pair)))


_PAIR_HINT = False


class expect_pair_gradients:
    """Context manager for callers that KNOW the gradients of a two-output tower evaluated inside it will be exact
    negatives of each other (``Algorithm``: a two-way ``Categorical`` policy under the fused PPO loss, whose kernel
    emits antisymmetric logit gradients by construction). Towers that ask (``pair_gradients=None`` resolves to
    this hint) then keep only the gate bits of h2 from the first iteration on. The promise is checked on the
    device in the backward (``rl8_mlp_dout_pair_check``); a broken one costs a re-run of the forward, never a
    wrong gradient. One exception: a gradient tensor registered by ``trust_pair_gradient`` -- the two-class loss
    kernel's own output, a pair by construction -- is taken on trust while its address, element count and version
    counter are the registered ones (any in-place change, copy or rescaling of it is checked again)."""

    def __enter__(self):
        global _PAIR_HINT
        self._before = _PAIR_HINT
        _PAIR_HINT = True
        return self

    def __exit__(self, *exc):
        global _PAIR_HINT
        _PAIR_HINT = self._before
        return False


def pair_hint() -> bool:
    return _PAIR_HINT


#: Gradient tensors known to be exact pairs BY CONSTRUCTION: the output of ``rl8_ppo_loss_categorical_fwd_bwd_f32`` for
#: two classes (the kernel stores ``g`` and ``-g``), registered by ``nn.functional.fused_ppo_loss`` under (address,
#: element count, version).  A backward that receives exactly such a tensor skips ``rl8_mlp_dout_pair_check`` -- a pass
#: over dOut and a host read per backward: with 8 shuffled minibatches 64 host round trips per ``step()`` -- and anything
#: else (a scaled copy under AMP, a custom loss) is still checked on the device.
_TRUSTED_PAIRS: dict[int, tuple[torch.Tensor, int]] = {}


def trust_pair_gradient(g: torch.Tensor) -> None:
    """Registers ``g`` (kept alive here until a backward consumes it or four newer ones arrive, so that its address
    cannot be handed to another tensor in between)."""
    while len(_TRUSTED_PAIRS) >= 4:
        _TRUSTED_PAIRS.pop(next(iter(_TRUSTED_PAIRS)))
    _TRUSTED_PAIRS[g.data_ptr()] = (g, g._version)


def _trusted_pair(g: torch.Tensor) -> bool:
    hit = _TRUSTED_PAIRS.pop(g.data_ptr(), None)
    return (hit is not None and hit[0].numel() == g.numel() and hit[0]._version == hit[1]
            and hit[0].untyped_storage().data_ptr() == g.untyped_storage().data_ptr())


class _FusedTower(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, layer2, grad_mode, plan, w3_key):  # type: ignore[override]
        # needs_input_grad reflects the parameters' requires_grad even when the
        # caller runs under no_grad (rollouts), and inside forward() grad mode is
        # always off: the caller's grad mode comes in as an argument, so that
        # activations are kept only when a backward can follow.
        need_grad = grad_mode and any(ctx.needs_input_grad[1:7])
        if plan.forward_planes:
            # Rank-one heads (one output; two outputs with exactly opposite gradients, as the last backward of
            # this tower found them) need only the gate bits of h2 in the backward pass: no h2 store, no h2
            # read.  Should a two-output head stop being rank-one, its backward re-runs this forward for h2.
            out, h1, h2, gate = hip.mlp_tower_forward_split(x, w1, b1, _packed(layer2, False, True), b2, w3, b3,
                                                            save=need_grad, save_h1=plan.keep_h1, save_gate=True,
                                                            save_h2=not plan.gate_only)
        else:
            out, h1, h2 = hip.mlp_tower_forward(x, w1, b1, _packed(layer2, False, False), b2, w3, b3, save=need_grad)
            gate = None
        if need_grad:
            ctx.layer2 = layer2
            ctx.w3_key = w3_key
            ctx.plan = plan
            # (w2 is saved although the kernels read its packed copies: autograd's version check then refuses a
            # backward after an in-place change of the weight, as it would for the eager modules)
            ctx.save_for_backward(x, h1, h2, w3, w1, b1, gate, b2, b3, w2)
        return out

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        return _tower_backward(ctx, dout) + (None,) * 4


def _tower_backward(ctx, dout):
    """Backward of ``_FusedTower`` and of ``_ReplayedTower`` (same saved tensors, same kernels, the forward's
    ``ctx.plan``): gradients of x (none) and of the six tower parameters."""
    x, h1, h2, w3, w1, b1, gate, b2, b3, w2 = ctx.saved_tensors
    plan: _TowerPlan = ctx.plan
    planes = plan.backward_planes
    layer2 = ctx.layer2
    w3_key = ctx.w3_key
    gate_pack = (lambda: _packed_gate(layer2, w3, w3_key)) if planes and w3.shape[0] <= 2 else None

    def h2_again():  # (a two-output head that is not rank-one after all: the forward once more, with h2)
        return hip.mlp_tower_forward_split(x, w1, b1, _packed(layer2, False, True), b2, w3, b3, save=True,
                                           save_h1=False, save_gate=True)[2]

    info: dict = {}
    # (a two-output head an earlier backward found NOT to be a pair -- mean / log_std of a normal -- is not asked again)
    known_general = w3.shape[0] == 2 and layer2.__dict__.get("_rl8_rank_one") is False
    known_pair = w3.shape[0] == 2 and dout.dtype == torch.float32 and dout.is_contiguous() and _trusted_pair(dout)
    g = hip.mlp_tower_backward(x, h1, h2, dout.contiguous().float(), _packed(layer2, True, planes), w3,
                               w1, b1, wgrad_split=plan.wgrad_planes, gate2=gate if planes else None,
                               gate_pack=gate_pack, w2=w2, b2=b2, h2_fn=h2_again, info=info, assume_general=known_general,
                               assume_pair=known_pair, gates_on=plan.gates)
    if w3.shape[0] == 2:  # what this backward found, for callers that give no hint (see tower_forward)
        layer2.__dict__["_rl8_rank_one"] = bool(info.get("rank_one", False))
    return None, g["w1"], g["b1"], g["w2"], g["b2"], g["w3"], g["b3"]


# --------------------------------------------------------------------------- #
# The rollout's forward passes, kept for the first SGD pass.
#
# ``Algorithm.collect()`` evaluates both towers on every observation of the buffer
# (reference ``algorithms/_feedforward.py:362-367``); SGD iteration 0 of ``step()``
# then evaluates them AGAIN on the same observations with the same weights
# (``:519-524``).  The forward kernel is deterministic per row, so that second pass
# reproduces numbers that already exist.  A ``RolloutRecord`` makes the rollout's
# launches run in the training forward's save mode (gate bits of h2, 32 B per row;
# h2 too for heads that are not rank-one) into ``[H][N]`` slabs -- the row order of
# the time-major buffer's flat full batch -- and ``replay`` hands those to autograd
# in place of a forward launch.  Used only while every parameter of the tower is
# what the rollout saw (version counters and addresses).
# --------------------------------------------------------------------------- #
#: Absolute cap on the h2 slabs a rollout record may hold (1 KiB per row and general-head tower: 34 GB at 2^25 rows),
#: besides "a third of what is free when the slab is made" (ADVICE r4).  ``RL8_AMD_RECORD_H2_GIB`` overrides; 0: never.
def _record_h2_budget_bytes() -> int:
    try:  # (a malformed value must not abort importing the package: ADVICE r5)
        gib = float(os.environ.get("RL8_AMD_RECORD_H2_GIB", "48"))
    except ValueError:
        gib = 48.0
    return int(max(gib, 0.0) * (1 << 30))


RECORD_H2_BUDGET_BYTES = _record_h2_budget_bytes()
#: ... and the slabs are given back when, at the end of a step(), less than this is free on the device.
RECORD_H2_KEEP_FREE_BYTES = 8 << 30


def _param_key(params) -> tuple:
    """What identifies the values of ``params``: version counters (in-place changes) and addresses (replacement)."""
    return tuple((p._version, p.data_ptr()) for p in params)


@dataclasses.dataclass(frozen=True)
class _RecordedRows:
    """One tower's part of a replay: the parameter key of its rows, their outputs, gate bits and h2 (if recorded)."""
    key: tuple
    out: torch.Tensor
    gate: torch.Tensor
    h2: None | torch.Tensor

    def slice(self, start: int, stop: int) -> "_RecordedRows":
        return _RecordedRows(self.key, self.out[start:stop], self.gate[start:stop],
                             None if self.h2 is None else self.h2[start:stop])


class _TowerRecord:
    def __init__(self, params: list[torch.Tensor], n_out: int, gate_only: bool, rows: int, device) -> None:
        self.params = params
        self.n_out, self.gate_only, self.rows = n_out, gate_only, rows
        self.out = torch.empty(rows, n_out, dtype=torch.float32, device=device)
        self.gate = torch.empty(rows, 8, dtype=torch.int32, device=device)
        self.h2 = None if gate_only else torch.empty(rows, hip.MLP_HIDDEN, dtype=torch.float32, device=device)
        self.seen: set[int] = set()
        #: address of the input each recorded timestep was evaluated on; a second evaluation of the same tower inside
        #: one ``record.at(t)`` (a model that runs it on obs AND next_obs) spoils the timestep: never replayed
        self.inputs: dict[int, int] = {}
        self.reset(None)

    def reset(self, key: None | tuple) -> None:
        """Nothing recorded yet, for the parameters ``key`` names (``None``: a rollout that has not reached it)."""
        self.key, self.spoiled = key, False
        self.seen.clear()
        self.inputs.clear()

    def current_key(self) -> tuple:
        return _param_key(self.params)


class RolloutRecord:
    """Outputs, gate bits (and h2 where needed) of the towers for the ``steps x rows_per_step`` observations of one
    rollout, in time-major row order. ``at(t)`` is the context ``collect()`` evaluates timestep ``t`` in (``record``
    takes the tower calls made inside it), ``seal`` ends the rollout, ``rows_for`` is all a training pass asks."""

    def __init__(self, steps: int, rows_per_step: int, *, keep_general: bool) -> None:
        self.steps, self.rows_per_step = steps, rows_per_step
        self.keep_general = keep_general
        self.towers: dict[int, _TowerRecord] = {}
        self.t = -1
        self.refused: set[int] = set()
        self._sealed: None | int = None  # version counter of the observations a finished rollout was recorded on

    def begin(self) -> None:
        self.unseal()
        for tr in self.towers.values():
            tr.reset(None)

    def seal(self, obs_tm: torch.Tensor) -> None:
        """End of the rollout that filled the record from the time-major observations ``obs_tm``."""
        self._sealed = obs_tm._version

    def unseal(self) -> None:
        """Nothing is replayed until the next ``seal``: a new rollout has begun, recording or not."""
        self._sealed = None

    @contextlib.contextmanager
    def at(self, t: int):
        global _RECORDING
        before, _RECORDING, self.t = _RECORDING, self, t
        try:
            yield self
        finally:
            _RECORDING = before

    def _tower(self, layer2: nn.Linear, params: list[torch.Tensor], n_out: int, gate_only: bool, device) -> None | _TowerRecord:
        tr = self.towers.get(id(layer2))
        rows = self.steps * self.rows_per_step
        if tr is not None and (tr.n_out, tr.gate_only, tr.rows) == (n_out, gate_only, rows) and tr.out.device == device:
            tr.params = params
            return tr
        if id(layer2) in self.refused:
            return None
        if not gate_only:
            # h2 is 1 KiB per row (34 GB per tower at 2^25 rows): only where every row is read back and it fits easily
            need = rows * (hip.MLP_HIDDEN * 4 + 32 + 4 * n_out)
            free, _ = torch.cuda.mem_get_info(device)
            held = sum(t.h2.numel() * 4 for t in self.towers.values() if t.h2 is not None)
            if not self.keep_general or need > free // 3 or held + need > RECORD_H2_BUDGET_BYTES:
                self.refused.add(id(layer2))
                return None
        self.towers.pop(id(layer2), None)
        try:
            tr = self.towers[id(layer2)] = _TowerRecord(params, n_out, gate_only, rows, device)
        except torch.cuda.OutOfMemoryError:  # (the tower is then evaluated without a record: one more forward per step())
            self.refused.add(id(layer2))
            return None
        return tr

    def record(self, l1: nn.Linear, l2: nn.Linear, heads: Sequence[nn.Linear], w3: torch.Tensor, b3: torch.Tensor,
               plan: _TowerPlan, x: torch.Tensor) -> None | torch.Tensor:
        """Timestep ``self.t`` of the tower, evaluated in the training forward's save mode straight into its slabs:
        the output, or ``None`` where nothing was recorded (the caller then runs the tower as usual)."""
        if not plan.recordable or x.shape[0] != self.rows_per_step:
            return None
        tr = self._tower(l2, _tower_params(l1, l2, heads), w3.shape[0], plan.gate_only, x.device)
        if tr is None:
            return None
        key = tr.current_key()
        if tr.key != key:
            tr.reset(key)
        if self.t in tr.seen:  # second evaluation in this timestep's context: the slab rows of t would be overwritten
            tr.spoiled = True
            return None
        tr.inputs[self.t] = x.data_ptr()
        sl = slice(self.t * self.rows_per_step, (self.t + 1) * self.rows_per_step)
        out = hip.mlp_tower_forward_split(
            x.contiguous(), l1.weight, l1.bias, _packed(l2, False, True), l2.bias, w3, b3, save=True,
            save_h1=False, save_gate=True, save_h2=not plan.gate_only, out=tr.out[sl], gate_out=tr.gate[sl],
            h2_out=None if plan.gate_only else tr.h2[sl], timer_name="mlp_tower_forward_record")[0]
        tr.seen.add(self.t)
        replay_stats["recorded_rows"] += self.rows_per_step
        return out

    def release_if_tight(self, device) -> int:
        """End of a ``step()``: give the h2 slabs back (and refuse new ones) when the device is short of memory --
        activations and workspaces allocated by ``step()`` come after the slabs and must not be what runs out.  Returns
        the bytes released."""
        if not any(tr.h2 is not None for tr in self.towers.values()):
            return 0  # (nothing to give back: no driver query -- hipMemGetInfo costs ~100 ms per call when several
            #            processes share the device, as the multi-rank rehearsals on one GPU do)
        free, _ = torch.cuda.mem_get_info(device)
        if free >= RECORD_H2_KEEP_FREE_BYTES:
            return 0
        released = 0
        for key in [k for k, tr in self.towers.items() if tr.h2 is not None]:
            released += self.towers[key].h2.numel() * 4
            del self.towers[key]
            self.refused.add(key)
        return released

    def _usable(self) -> list[tuple[int, _TowerRecord]]:
        """The towers that saw all the timesteps, once each, with the parameters they have now."""
        return [(k, tr) for k, tr in self.towers.items()
                if tr.key is not None and not tr.spoiled and len(tr.seen) == self.steps and tr.current_key() == tr.key]

    def require_inputs(self, base_ptr: int, step_bytes: int) -> None:
        """The caller replays the record against the rows of ONE dense array (the time-major observations, timestep t
        at ``base_ptr + t * step_bytes``): a tower recorded on anything else -- a model that feeds it a transformed or
        shifted view -- is never replayed."""
        for tr in self.towers.values():
            if any(ptr != base_ptr + t * step_bytes for t, ptr in tr.inputs.items()):
                tr.spoiled = True

    def valid(self) -> bool:
        """Some recorded tower can still be replayed."""
        return bool(self._usable())

    def rows(self, start: int, stop: int) -> dict[int, _RecordedRows]:
        """Record rows ``[start, stop)`` (time-major order) of every usable tower."""
        return {k: _RecordedRows(tr.key, tr.out, tr.gate, tr.h2).slice(start, stop) for k, tr in self._usable()}

    def gather(self, index: torch.Tensor) -> dict[int, _RecordedRows]:
        """The same for the samples ``index`` names (reference sample ids ``env * H + t``): one strided gather per
        tower (``rl8_gather_minibatch``) out of the ``[H][N]`` slabs seen as ``[N, H, ...]`` leaves."""
        H, N = self.steps, self.rows_per_step
        got: dict[int, _RecordedRows] = {}
        for k, tr in self._usable():
            leaves = [t.view(H, N, t.shape[1]).transpose(0, 1) for t in (tr.out, tr.gate, tr.h2) if t is not None]
            dense = hip.gather_minibatch(index, H, leaves)
            got[k] = _RecordedRows(tr.key, dense[0], dense[1], dense[2] if tr.h2 is not None else None)
        return got

    def rows_for(self, obs_tm: torch.Tensor, which: slice | torch.Tensor) -> None | dict[int, _RecordedRows]:
        """The recorded rows of a training batch out of ``obs_tm`` (``which``: a ``slice`` of its flat time-major rows, or
        sample ids for ``gather``); ``None``: no sealed rollout, observations written to since, or no tower left usable."""
        if self._sealed != obs_tm._version or not self.valid():
            return None
        self.require_inputs(obs_tm.data_ptr(), obs_tm.stride(0) * obs_tm.element_size())
        return (self.rows(which.start, which.stop) if isinstance(which, slice) else self.gather(which)) or None


_RECORDING: None | RolloutRecord = None
_REPLAY: None | "replay" = None


class replay:
    """Context for a grad-enabled pass over ``x`` (a dense ``[m, d]`` tensor): towers found in ``rows`` (from
    ``RolloutRecord.rows_for``) whose parameters are still the recorded ones skip their forward launch."""

    def __init__(self, rows: dict[int, _RecordedRows], x: torch.Tensor) -> None:
        self.rows, self.x = rows, x

    def __enter__(self):
        global _REPLAY
        self._before = _REPLAY
        _REPLAY = self
        return self

    def __exit__(self, *exc):
        global _REPLAY
        _REPLAY = self._before
        return False

    def hit(self, l1: nn.Linear, l2: nn.Linear, heads: Sequence[nn.Linear], x: torch.Tensor, n_out: int,
            plan: _TowerPlan) -> None | _RecordedRows:
        """The recorded rows that stand for this tower call (the context's own ``x``, the recorded parameters), or ``None``."""
        got = self.rows.get(id(l2))
        # (an x that asks for its gradient is never replayed: ``_ReplayedTower`` forms none, see ``tower_forward``)
        ok = (got is not None and not (x.requires_grad and torch.is_grad_enabled())
              and x.data_ptr() == self.x.data_ptr() and x.shape == self.x.shape and x.is_contiguous()
              and got.key == _param_key(_tower_params(l1, l2, heads))
              and got.out.shape == (x.shape[0], n_out)
              and (got.h2 is not None or plan.gate_only))  # (a record without h2 serves rank-one calls)
        return got if ok else None


#: Counts for tests / the bench line: towers evaluated from the record, rows recorded.
replay_stats = {"replayed_towers": 0, "replayed_rows": 0, "recorded_rows": 0}


class _ReplayedTower(torch.autograd.Function):
    """``_FusedTower`` whose forward already ran (during the rollout): returns the recorded output and saves the
    recorded gate bits / h2 for the same backward kernels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, layer2, plan, w3_key, out, gate, h2):  # type: ignore[override]
        ctx.layer2 = layer2
        ctx.w3_key = w3_key
        ctx.plan = plan
        ctx.save_for_backward(x, None, h2, w3, w1, b1, gate, b2, b3, w2)
        return out.detach()

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        return _tower_backward(ctx, dout) + (None,) * 6


def _tower_params(l1: nn.Linear, l2: nn.Linear, heads: Sequence[nn.Linear]) -> list[torch.Tensor]:
    return [l1.weight, l1.bias, l2.weight, l2.bias, *[h.weight for h in heads], *[h.bias for h in heads]]


def _family(trunk: nn.Module, heads: Sequence[nn.Linear]) -> None | tuple[str, nn.Linear, nn.Linear]:
    """The one place the module structure is inspected: (family, layer1, layer2) if ``trunk`` is
    ``Sequential(MLP(Linear, ReLU, Linear), ReLU)`` with biased layers of one width and biased heads (one at least) that
    read it -- "wide": 256, "narrow": a width in ``hip.MLP_NARROW_HIDDEN`` (``mlp_narrow_kernels.hip``) -- else ``None``.
    "narrow_bn": a narrow tower with an affine ``BatchNorm1d`` that tracks running statistics behind layer 1,
    ``Sequential(MLP(Linear, BatchNorm1d, ReLU, Linear), ReLU)`` (the norm is ``trunk[0][1]``)."""
    if not isinstance(trunk, nn.Sequential) or len(trunk) < 2:
        return None
    mlp, act = trunk[0], trunk[1]
    if not isinstance(mlp, nn.Sequential) or len(mlp) not in (3, 4) or not isinstance(act, nn.ReLU):
        return None
    norm = mlp[1] if len(mlp) == 4 else None
    l1, a1, l2 = mlp[0], mlp[-2], mlp[-1]
    if not (isinstance(l1, nn.Linear) and isinstance(a1, nn.ReLU) and isinstance(l2, nn.Linear)):
        return None
    width = l1.out_features
    family = "narrow" if width in hip.MLP_NARROW_HIDDEN else "wide" if width == hip.MLP_HIDDEN else None
    if norm is not None:
        if not (type(norm) is nn.BatchNorm1d and family == "narrow" and norm.num_features == width and norm.affine
                and norm.track_running_stats and norm.running_mean is not None):
            return None
        family = "narrow_bn"
    if family is None or l2.in_features != width or l2.out_features != width:
        return None
    if l1.in_features > hip.MLP_MAX_IN or l1.bias is None or l2.bias is None:
        return None
    if not heads or sum(h.out_features for h in heads) > hip.MLP_MAX_OUT or any(h.bias is None for h in heads):
        return None
    if any(h.in_features != width for h in heads):
        return None
    return family, l1, l2


class _NarrowTower(torch.autograd.Function):
    """A narrow tower (hidden width 64 / 128): one forward kernel that saves nothing, one backward kernel that
    recomputes the activations from x, and the fixed-order reduction of its partial gradients."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):  # type: ignore[override]
        ctx.save_for_backward(x, w1, b1, w2, b2, w3, b3)
        return hip.mlp_narrow_forward(x, w1, b1, w2, b2, w3, b3)

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        x, w1, b1, w2, b2, w3, _ = ctx.saved_tensors
        # (an input that asks for its gradient -- a tower behind a learned encoder -- takes the entry that forms dx)
        g = hip.mlp_narrow_backward(x, dout.contiguous().float(), w1, b1, w2, b2, w3, want_dx=ctx.needs_input_grad[0])
        return g.get("x"), g["w1"], g["b1"], g["w2"], g["b2"], g["w3"], g["b3"]


# --------------------------------------------------------------------------- #
# BatchNorm towers ("narrow_bn"): Linear -> BatchNorm1d -> ReLU -> Linear -> ReLU -> heads at width 64 / 128.
#
# A BatchNorm1d directly behind a Linear is an affine map of x.  In training mode, with mu = mean_i x_i and the biased
# covariance C = (1/B) sum_i (x_i - mu)(x_i - mu)^T of the batch, unit j of z1 = x W1^T + b1 has
#     batch mean  m_j = W1_j . mu + b1_j          batch variance  v_j = W1_j C W1_j^T
#     r_j = 1 / sqrt(v_j + eps),  s_j = gamma_j r_j
#     y_j = a_j . x + c_j,   a_j = s_j W1_j,   c_j = beta_j - s_j (W1_j . mu)                     (b1 cancels)
# so the tower is a plain narrow tower with W1' = A, b1' = c.  With GA = dL/dA and gc = dL/dc of that tower:
#     dbeta = gc                          ds_j = GA_j . W1_j - gc_j (W1_j . mu)
#     dgamma_j = r_j ds_j                 dv_j = -1/2 r_j^3 gamma_j ds_j
#     dW1_j = s_j GA_j - gc_j s_j mu + 2 dv_j (C W1_j)                     db1 = 0
#     dmu = - sum_j gc_j s_j W1_j         dC = sum_j dv_j W1_j W1_j^T
#     dx_i = dx_i(tower) + dmu / B + (2 / B) dC (x_i - mu)
# In eval mode a_j = gamma_j W1_j / sqrt(rv_j + eps) and c_j = beta_j + gamma_j (b1_j - rm_j) / sqrt(rv_j + eps).
# --------------------------------------------------------------------------- #
def _fold_training(mu, cov, w1, b1, gamma, beta, eps):
    """``(A, c, r, m_z, v)`` from the batch moments of x, in the dtype of the operands."""
    wm = w1 @ mu
    v = ((w1 @ cov) * w1).sum(-1).clamp_min(0.0)
    r = torch.rsqrt(v + eps)
    s = gamma * r
    return s[:, None] * w1, beta - s * wm, r, wm + b1, v


def _fold_training_backward(ga, gc, w1, gamma, mu, cov, r):
    """``(dW1, dgamma, dbeta, dmu, dC)`` from the gradients ``ga`` / ``gc`` of the folded layer."""
    s = gamma * r
    ds = (ga * w1).sum(-1) - gc * (w1 @ mu)
    dv = -0.5 * r ** 3 * gamma * ds
    dw1 = s[:, None] * ga - (gc * s)[:, None] * mu[None, :] + 2.0 * dv[:, None] * (w1 @ cov)
    return dw1, r * ds, gc, -(gc * s) @ w1, (w1 * dv[:, None]).t() @ w1


def _fold_eval(w1, b1, gamma, beta, running_mean, running_var, eps):
    """``(A, c, r)`` from the running statistics."""
    r = torch.rsqrt(running_var + eps)
    s = gamma * r
    return s[:, None] * w1, beta + s * (b1 - running_mean), r


def _fold_eval_backward(ga, gc, w1, shift, gamma, r):
    """``(dW1, db1, dgamma, dbeta)``; ``shift`` = b1 - running_mean."""
    s = gamma * r
    return s[:, None] * ga, s * gc, r * ((ga * w1).sum(-1) + gc * shift), gc


def _dx_statistics_term(dx: torch.Tensor, x: torch.Tensor, mu: torch.Tensor, dmu: torch.Tensor, dcov: torch.Tensor) -> None:
    """``dx += dmu / B + (2 / B) (x - mu) dC`` in place: one elementwise pass and one ``addmm_`` over ``[B, d_in]``.  The
    centring uses ``mu`` rounded to the dtype of x; what the rounding leaves goes into the constant row."""
    rows = x.shape[0]
    scaled = dcov * (2.0 / rows)
    mu_x = mu.to(x.dtype)
    const = dmu / rows - (mu - mu_x.to(mu.dtype)) @ scaled
    dx.addmm_(x - mu_x, scaled.to(x.dtype))
    dx.add_(const.to(x.dtype))


def _running_update(running: torch.Tensor, new: torch.Tensor, factor) -> torch.Tensor:
    return (1.0 - factor) * running + factor * new


def batchnorm_tower_reference(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                              eps: float, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, *,
                              training: bool, running_mean: None | torch.Tensor = None,
                              running_var: None | torch.Tensor = None, momentum: None | float = 0.1,
                              num_batches_tracked: int = 0, dout: None | torch.Tensor = None) -> dict:
    """The torch expression of what the BatchNorm tower route computes, in any dtype on any device, without autograd:
    the yardstick of the tests. ``out`` [B, n_out]; in training mode ``num_batches_tracked`` plus one and the moved
    ``running_mean`` / ``running_var`` (new tensors; ``momentum`` ``None`` is the cumulative average, as in
    ``nn.BatchNorm1d``); with ``dout`` the hand-written gradients ``dx, dw1, db1, dgamma, dbeta, dw2, db2, dw3, db3``."""
    rows = x.shape[0]
    got: dict[str, torch.Tensor] = {}
    if training:
        mu = x.mean(0)
        xc = x - mu
        cov = xc.t() @ xc / rows
        a, c, r, m_z, v = _fold_training(mu, cov, w1, b1, gamma, beta, eps)
        if running_mean is not None and running_var is not None:
            got["num_batches_tracked"] = num_batches_tracked + 1
            factor = 1.0 / (num_batches_tracked + 1) if momentum is None else momentum
            got["running_mean"] = _running_update(running_mean, m_z, factor)
            got["running_var"] = _running_update(running_var, v * (rows / (rows - 1)), factor)
    else:
        a, c, r = _fold_eval(w1, b1, gamma, beta, running_mean, running_var, eps)
    z1 = x @ a.t() + c
    h1 = torch.relu(z1)
    z2 = h1 @ w2.t() + b2
    h2 = torch.relu(z2)
    got["out"] = h2 @ w3.t() + b3
    if dout is None:
        return got
    dz2 = (dout @ w3) * (z2 > 0)
    dz1 = (dz2 @ w2) * (z1 > 0)
    got.update(dw3=dout.t() @ h2, db3=dout.sum(0), dw2=dz2.t() @ h1, db2=dz2.sum(0))
    ga, gc, dx = dz1.t() @ x, dz1.sum(0), dz1 @ a
    if training:
        dw1, dgamma, dbeta, dmu, dcov = _fold_training_backward(ga, gc, w1, gamma, mu, cov, r)
        db1 = torch.zeros_like(b1)
        _dx_statistics_term(dx, x, mu, dmu, dcov)
    else:
        dw1, db1, dgamma, dbeta = _fold_eval_backward(ga, gc, w1, b1 - running_mean, gamma, r)
    got.update(dx=dx, dw1=dw1, db1=db1, dgamma=dgamma, dbeta=dbeta)
    return got


def batchnorm_towers_on() -> bool:
    """``RL8_AMD_BATCHNORM_TOWERS=1`` (read on every call) turns the BatchNorm tower route on; unset or anything else
    keeps every BatchNorm tower on the torch modules (DESIGN.md section 8 says why it is not the default)."""
    return os.environ.get("RL8_AMD_BATCHNORM_TOWERS", "0") == "1"


class _NarrowBatchNormTower(torch.autograd.Function):
    """A narrow tower with a BatchNorm1d behind layer 1. Training: the moments of x (``rl8_tower_moments_f64``), the
    fold (``rl8_batchnorm_fold_f32``, which also moves the running statistics), then the plain narrow forward on the
    folded layer. The backward runs the narrow backward on the SAVED folded layer -- never folded again, so forward and
    backward agree on every gate bit -- and takes the fold's own backward in float64 on the ``[H, d_in]`` / ``[d_in,
    d_in]`` tensors with torch ops (no host synchronisation). Eval: the fold from the running statistics."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, w3, b3, norm):  # type: ignore[override]
        training = norm.training
        if training:
            mu, cov = hip.tower_moments(x)
            norm.num_batches_tracked.add_(1)
            cumulative = norm.momentum is None
            a, c, r, _, _ = hip.batchnorm_fold(w1, b1, gamma, beta, norm.eps, moments=(mu, cov, x.shape[0]),
                                               running_mean=norm.running_mean, running_var=norm.running_var,
                                               factor=0.0 if cumulative else norm.momentum,
                                               tracked=norm.num_batches_tracked if cumulative else None)
            ctx.save_for_backward(x, a, c, w2, b2, w3, w1, gamma, mu, cov, r)
        else:
            a, c = hip.batchnorm_fold(w1, b1, gamma, beta, norm.eps, running_mean=norm.running_mean,
                                      running_var=norm.running_var)
            r = torch.rsqrt(norm.running_var.double() + norm.eps)
            ctx.save_for_backward(x, a, c, w2, b2, w3, w1, gamma, b1.detach().double() - norm.running_mean.double(), r)
        ctx.training = training
        return hip.mlp_narrow_forward(x, a, c, w2, b2, w3, b3)

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        x, a, c, w2, b2, w3, w1, gamma, *stats = ctx.saved_tensors
        g = hip.mlp_narrow_backward(x, dout.contiguous().float(), a, c, w2, b2, w3, want_dx=ctx.needs_input_grad[0])
        ga, gc, w1d, gammad = (t.double() for t in (g["w1"], g["b1"], w1, gamma))
        dx = g.get("x")
        if ctx.training:
            mu, cov, r = stats
            dw1, dgamma, dbeta, dmu, dcov = _fold_training_backward(ga, gc, w1d, gammad, mu, cov, r)
            db1 = torch.zeros_like(c)
            if dx is not None:
                _dx_statistics_term(dx, x, mu, dmu, dcov)
        else:
            shift, r = stats
            dw1, db1, dgamma, dbeta = _fold_eval_backward(ga, gc, w1d, shift, gammad, r)
        return (dx, dw1.float(), db1.float(), dgamma.float(), dbeta.float(), g["w2"], g["b2"], g["w3"], g["b3"], None)


def _batchnorm_tower_forward(l1: nn.Linear, norm: nn.BatchNorm1d, l2: nn.Linear, w3: torch.Tensor, b3: torch.Tensor,
                             x: torch.Tensor) -> None | torch.Tensor:
    """The "narrow_bn" route, or ``None`` when this call is not its: the switch off, autocast, an ``x`` that is not
    dense or is empty, parameters that are not float32 on the device, one row in training mode (the module then raises
    torch's own ``ValueError``)."""
    if not batchnorm_towers_on() or torch.is_autocast_enabled() or not x.is_contiguous() or x.numel() == 0:
        return None
    if norm.training and x.shape[0] == 1:
        return None
    params = (l1.weight, l1.bias, norm.weight, norm.bias, l2.weight, l2.bias, w3, b3)
    if not all(p.is_cuda and p.dtype == torch.float32 for p in (*params, norm.running_mean, norm.running_var)):
        return None
    return _NarrowBatchNormTower.apply(x, *params, norm)


# --------------------------------------------------------------------------- #
# Wide-input towers: width 256 behind 17 to 128 inputs (mlp_wide_in_kernels.hip), fp32 MFMA throughout.  Never
# recorded or replayed for the rollout (no planes), and no input gradient: a call whose x asks for one is declined.
# --------------------------------------------------------------------------- #
#: Rows per segment of the wide-input backward: dZ1 and dZ2 ([rows, 256] fp32 each) are scratch of one segment, so
#: the two together never exceed 2 GiB however long the minibatch is.  Read on every call.
WIDE_INPUT_SEGMENT_ROWS = 1 << 20
#: dW2 = dZ2^T h1 of the wide-input backward on three exact bf16 planes per operand (``rl8_mlp_wgrad_split_strided_f32``:
#: 0.67 against 1.03 ms per 2^20 rows at the same fp64 bars); False: ``rl8_mlp_wgrad_f32``.  Read on
#: every call.
WIDE_INPUT_DW2_PLANES = True


def wide_input_towers_on() -> bool:
    """``RL8_AMD_WIDE_INPUT_TOWERS=0`` (read on every call) sends the wide-input towers to the torch modules: the
    tests' yardstick.  On by default."""
    return os.environ.get("RL8_AMD_WIDE_INPUT_TOWERS", "1") != "0"


@functools.lru_cache(maxsize=None)
def _wide_input_supported(d_in: int, n_out: int) -> bool:
    """Compiled for this width: fixed by the build, asked once per width."""
    return hip.mlp_wide_in_supports(d_in, n_out)


def _wide_input_family(trunk: nn.Module, heads: Sequence[nn.Linear]) -> None | tuple[nn.Linear, nn.Linear]:
    """(layer1, layer2) if ``trunk`` is the structure ``_family`` calls "wide" -- ``Sequential(MLP(Linear, ReLU,
    Linear), ReLU)`` at width 256 with biased layers and biased heads (one at least) that read it -- whose first layer
    reads MORE than ``hip.MLP_MAX_IN`` floats, up to what ``hip.mlp_wide_in_supports`` takes; else ``None``."""
    if not isinstance(trunk, nn.Sequential) or len(trunk) < 2:
        return None
    mlp, act = trunk[0], trunk[1]
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 3 or not isinstance(act, nn.ReLU):
        return None
    l1, a1, l2 = mlp[0], mlp[1], mlp[2]
    if not (isinstance(l1, nn.Linear) and isinstance(a1, nn.ReLU) and isinstance(l2, nn.Linear)):
        return None
    width = hip.MLP_HIDDEN
    if l1.out_features != width or l2.in_features != width or l2.out_features != width:
        return None
    if l1.in_features <= hip.MLP_MAX_IN or l1.bias is None or l2.bias is None:
        return None
    if not heads or any(h.bias is None or h.in_features != width for h in heads):
        return None
    n_out = sum(h.out_features for h in heads)
    if n_out > hip.MLP_MAX_OUT or not _wide_input_supported(l1.in_features, n_out):
        return None
    return l1, l2


def _packed_w1(layer: nn.Linear, family: str = "in") -> torch.Tensor:
    """``hip.mlp_wide_in_pack_w1(layer.weight)`` (``family`` "out": ``hip.mlp_wide_out_pack_w1``, which takes any
    1 <= d_in <= 128), cached on the layer as ``_packed`` caches W2: re-made when the optimizer has changed the weight
    (version counter) or the weight tensor has been replaced / moved."""
    w1 = layer.weight
    key = "_rl8_w1_pack" if family == "in" else "_rl8_w1_pack_out"
    hit = layer.__dict__.get(key)
    if hit is not None and hit[0] == w1._version and hit[1] == w1.data_ptr():
        return hit[2]
    packed = hip.mlp_wide_in_pack_w1(w1) if family == "in" else hip.mlp_wide_out_pack_w1(w1)
    layer.__dict__[key] = (w1._version, w1.data_ptr(), packed)
    return packed


class _WideInputTower(torch.autograd.Function):
    """A wide-input tower: one forward kernel (which stores h1 and h2 when a backward can follow); the backward walks
    the rows in segments of ``WIDE_INPUT_SEGMENT_ROWS`` -- per segment the data gradient (dZ1, dZ2 into scratch, one
    row of small-gradient partials per workgroup), dW1 += dZ1^T x and dW2 += dZ2^T h1 (``WIDE_INPUT_DW2_PLANES``) -- in
    order, so the sums are the same bits from run to run."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, layer1, layer2, grad_mode):  # type: ignore[override]
        # (grad_mode: the caller's; inside forward() grad mode is always off -- see _FusedTower)
        need_grad = grad_mode and any(ctx.needs_input_grad[1:7])
        if w3.shape[0] > hip.MLP_MAX_OUT:  # the wide-head family (mlp_wide_out_kernels.hip): the head on the matrix cores
            # (W3 is packed per call: two heads arrive concatenated, a fresh tensor every time)
            out, h1, h2 = hip.mlp_wide_out_forward(x, _packed_w1(layer1, "out"), b1, _packed(layer2, False, False), b2,
                                                   hip.mlp_wide_out_pack_w3(w3), b3, save=need_grad)
        else:
            out, h1, h2 = hip.mlp_wide_in_forward(x, _packed_w1(layer1), b1, _packed(layer2, False, False), b2, w3, b3,
                                                  save=need_grad)
        if need_grad:
            ctx.layer2 = layer2
            # (w1 and w2 are saved although the kernels read packed copies: autograd's version check then refuses a
            # backward after an in-place change of a weight, as it would for the eager modules)
            ctx.save_for_backward(x, h1, h2, w3, w1, w2)
        return out

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        x, h1, h2, w3, w1, w2 = ctx.saved_tensors
        dout = dout.contiguous().float()
        m, n_out, hidden = x.shape[0], w3.shape[0], hip.MLP_HIDDEN
        segment, planes = max(int(WIDE_INPUT_SEGMENT_ROWS), 1), bool(WIDE_INPUT_DW2_PLANES)
        w2t = _packed(ctx.layer2, True, False)
        dz1 = torch.empty(min(m, segment), hidden, dtype=torch.float32, device=x.device)
        dz2 = torch.empty_like(dz1)
        wide_head = n_out > hip.MLP_MAX_OUT  # (the family of the forward: its partial rows carry no dW3)
        partials = torch.empty(hip.load().rl8_mlp_wide_in_max_rows(),
                               2 * hidden + n_out if wide_head else 2 * hidden + n_out * hidden + n_out,
                               dtype=torch.float32, device=x.device)
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        w3t, dw3 = (hip.mlp_wide_out_pack_w3(w3, transposed=True), torch.empty_like(w3)) if wide_head else (None, None)
        small = None
        for at in range(0, m, segment):
            rows = slice(at, min(at + segment, m))
            z1, z2 = dz1[: rows.stop - at], dz2[: rows.stop - at]
            if wide_head:
                written = hip.mlp_wide_out_backward(h1[rows], h2[rows], dout[rows], w2t, w3t, z1, z2, partials)
            else:
                written = hip.mlp_wide_in_backward(h1[rows], h2[rows], dout[rows], w2t, w3, z1, z2, partials)
            part = partials[:written].sum(0)
            small = part if small is None else small + part
            if wide_head:
                hip.mlp_wide_out_wgrad(z1, x[rows], dw1, accumulate=at > 0)
                hip.mlp_wide_out_wgrad(h2[rows], dout[rows], dw3, accumulate=at > 0, transpose=True)
            else:
                hip.mlp_wide_in_wgrad(z1, x[rows], dw1, accumulate=at > 0)
            hip.mlp_wgrad(z2, h1[rows], out=dw2, accumulate=at > 0, planes=planes)
        if wide_head:
            db1, db2, db3 = torch.split(small, (hidden, hidden, n_out))
            return None, dw1, db1, dw2, db2, dw3, db3, None, None, None
        db1, db2, dw3, db3 = torch.split(small, (hidden, hidden, n_out * hidden, n_out))
        return None, dw1, db1, dw2, db2, dw3.view(n_out, hidden), db3, None, None, None


def _wide_input_tower_forward(l1: nn.Linear, l2: nn.Linear, heads: Sequence[nn.Linear], x: torch.Tensor, *,
                              switch=wide_input_towers_on) -> None | torch.Tensor:
    """The wide-input route (``switch``: ``wide_head_towers_on`` for the wide-head family, which runs through the same
    node), or ``None`` when this call is not its: the switch off, autocast, an ``x`` that is not dense or is empty or
    asks for its gradient (the family forms none, and must not drop one silently), parameters that are not float32 on
    the device."""
    if not switch() or torch.is_autocast_enabled() or not x.is_contiguous() or x.shape[0] < 1:
        return None
    if x.shape[1] != l1.in_features or (x.requires_grad and torch.is_grad_enabled()):
        return None
    w3 = heads[0].weight if len(heads) == 1 else torch.cat([h.weight for h in heads], 0)
    b3 = heads[0].bias if len(heads) == 1 else torch.cat([h.bias for h in heads], 0)
    params = (l1.weight, l1.bias, l2.weight, l2.bias, w3, b3)
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in params):
        return None
    return _WideInputTower.apply(x, *params, l1, l2, torch.is_grad_enabled())


# --------------------------------------------------------------------------- #
# Wide-head towers: width 256 with heads of 9 to 128 outputs in all, behind 1 to 128 inputs (mlp_wide_out_kernels.hip),
# fp32 MFMA throughout, the head and its gradients included.  They run through ``_WideInputTower``, which takes its
# entries from ``w3.shape[0]``.  Never recorded or replayed for the rollout (no planes: ``_Plan.recordable`` is not
# even asked, the family has no plan), and no input gradient: a call whose x asks for one is declined.
# --------------------------------------------------------------------------- #
def wide_head_towers_on() -> bool:
    """``RL8_AMD_WIDE_HEAD_TOWERS=0`` (read on every call) sends the wide-head towers to the torch modules: the
    tests' yardstick.  On by default."""
    return os.environ.get("RL8_AMD_WIDE_HEAD_TOWERS", "1") != "0"


@functools.lru_cache(maxsize=None)
def _wide_head_supported(d_in: int, n_out: int) -> bool:
    """Compiled for these widths: fixed by the build, asked once per pair."""
    return hip.mlp_wide_out_supports(d_in, n_out)


def _wide_head_family(trunk: nn.Module, heads: Sequence[nn.Linear]) -> None | tuple[nn.Linear, nn.Linear]:
    """(layer1, layer2) if ``trunk`` is the structure ``_family`` calls "wide" -- ``Sequential(MLP(Linear, ReLU,
    Linear), ReLU)`` at width 256 with biased layers and biased heads (one at least) that read it -- whose heads have
    MORE than ``hip.MLP_MAX_OUT`` outputs in all, up to what ``hip.mlp_wide_out_supports`` takes, behind any input
    width it takes; else ``None``.  Asked after ``_family`` and ``_wide_input_family`` have both said ``None``."""
    if not isinstance(trunk, nn.Sequential) or len(trunk) < 2:
        return None
    mlp, act = trunk[0], trunk[1]
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 3 or not isinstance(act, nn.ReLU):
        return None
    l1, a1, l2 = mlp[0], mlp[1], mlp[2]
    if not (isinstance(l1, nn.Linear) and isinstance(a1, nn.ReLU) and isinstance(l2, nn.Linear)):
        return None
    width = hip.MLP_HIDDEN
    if l1.out_features != width or l2.in_features != width or l2.out_features != width:
        return None
    if l1.bias is None or l2.bias is None:
        return None
    if not heads or any(h.bias is None or h.in_features != width for h in heads):
        return None
    n_out = sum(h.out_features for h in heads)
    if n_out <= hip.MLP_MAX_OUT or l1.in_features < 1 or not _wide_head_supported(l1.in_features, n_out):
        return None
    return l1, l2


def tower_forward(trunk: nn.Sequential, heads: Sequence[nn.Linear], x: torch.Tensor, *,
                  pair_gradients: None | bool = None) -> None | torch.Tensor:
    """``cat([head(trunk(x)) for head in heads], -1)`` through the fused kernels,
    or ``None`` when this tower / input is not eligible (caller then runs the
    modules eagerly).

    ``pair_gradients`` (two-output towers only): ``True`` -- the caller expects the two outputs' gradients to be
    exact negatives (a two-way categorical under the fused loss), so the forward keeps the gate bits of h2 alone;
    ``False`` -- h2 is stored; ``None`` -- whatever this tower's previous backward found (a tower used outside
    ``Algorithm``). Checked on the device in the backward either way.

    The gradient of ``x``: the narrow families (64 / 128, with or without the BatchNorm) form it where ``x`` requires
    one, from the same backward launch.  The 256-wide families -- the default kernels, the rollout replay, the
    piecewise tables, the wide-input and wide-head kernels -- form none and DECLINE such a call under grad mode (``None``: the caller
    runs the modules, which form it); under ``torch.no_grad()`` no gradient can follow and the kernels run."""
    if not ENABLED or not x.is_cuda or x.dtype != torch.float32 or x.ndim != 2:
        return None
    found = _family(trunk, heads)
    if found is None:  # (only then: the wide-input family begins where _family's input limit ends)
        wide = _wide_input_family(trunk, heads)
        if wide is not None:
            return _wide_input_tower_forward(*wide, heads, x)
        wide = _wide_head_family(trunk, heads)  # (more than MLP_MAX_OUT outputs, behind any input width)
        return None if wide is None else _wide_input_tower_forward(*wide, heads, x, switch=wide_head_towers_on)
    if x.shape[1] != found[1].in_features:
        return None
    family, l1, l2 = found
    if family == "wide" and x.requires_grad and torch.is_grad_enabled():
        return None  # (no 256-wide route forms dL/dx, and none may drop it silently: one attribute read for buffer data)
    if family == "narrow_bn" and not batchnorm_towers_on():  # (opt-in: nothing else is done for it while it is off)
        return None
    # opt-in prototype: scalar observations from an exact piecewise-linear table
    if family == "wide" and piecewise_mlp.ENABLED and x.shape[1] == 1:
        out = piecewise_mlp.tower_forward(l1, l2, heads, x)
        if out is not None:
            return out
    w3 = heads[0].weight if len(heads) == 1 else torch.cat([h.weight for h in heads], 0)
    b3 = heads[0].bias if len(heads) == 1 else torch.cat([h.bias for h in heads], 0)
    if family == "narrow_bn":
        return _batchnorm_tower_forward(l1, trunk[0][1], l2, w3, b3, x)
    if family == "narrow":  # (never recorded or replayed: everything below assumes width 256)
        return _NarrowTower.apply(x.contiguous(), l1.weight, l1.bias, l2.weight, l2.bias, w3, b3)
    if pair_gradients is None:
        pair_gradients = bool(l2.__dict__.get("_rl8_rank_one", False))
    w3_key = _param_key(h.weight for h in heads)
    n_out = w3.shape[0]
    plan = _plan(x.shape[1], n_out, bool(pair_gradients))
    if _RECORDING is not None and not torch.is_grad_enabled():
        # (``None``: refused a slab, or a second evaluation at this timestep.  Falling through is the plain launch
        # below: the replay branch needs grad mode on, and recording needs it off.)
        out = _RECORDING.record(l1, l2, heads, w3, b3, plan, x)
        if out is not None:
            return out
    if _REPLAY is not None and torch.is_grad_enabled() and plan.recordable:
        got = _REPLAY.hit(l1, l2, heads, x, n_out, plan)
        if got is not None:
            replay_stats["replayed_towers"] += 1
            replay_stats["replayed_rows"] += x.shape[0]
            return _ReplayedTower.apply(x, l1.weight, l1.bias, l2.weight, l2.bias, w3, b3, l2, plan, w3_key,
                                        got.out, got.gate, got.h2)
    return _FusedTower.apply(x.contiguous(), l1.weight, l1.bias, l2.weight, l2.bias, w3, b3, l2,
                             torch.is_grad_enabled(), plan, w3_key)
