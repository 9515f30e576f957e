"""Every row of ``tests/test_autograd_contract_host.py::CONTRACT`` held to fp64 on the device.

Each float tensor input of each fused autograd node is driven through the node's PUBLIC entry while it requires a
gradient -- as a leaf, and behind a small learned encoder (the realistic case: an ``nn.Linear`` or an ``nn.Embedding``
in front of a tower or an LSTM) -- and the caller-level result (the entry, and the torch modules where the entry
declines, exactly as the models fall back) is compared with fp64 autograd of the plain torch expression: the input's
gradient, the encoder's, and every parameter's.  A "formed" row must have run its family's kernels, a "declined" row
none of them, a "refused" row must raise before any launch.  Toggling the input's ``requires_grad`` must leave the
node's parameter gradients alone: bit for bit where the same launches ran, within the bars otherwise.

Bars (none is new).  Towers: ``tests/test_wide_input_tower_gpu.py::_check_gradients`` -- error against fp64 at most
``max(3 x eager fp32's error, 5e-6)``, relative to the largest wanted entry.  LSTMs: ``_check_grads`` of
``tests/test_lstm_narrow_gpu.py`` / ``tests/test_lstm_stack_gpu.py``.  Attention, feedforward and the masked functions:
the "three times torch's own error" bar of ``tests/test_attention_kernels_gpu.py`` /
``tests/test_feedforward_kernels_gpu.py``.  The PPO loss: ``tests/test_ppo_loss_edges_gpu.py::assert_grad``, plus three
times torch's own fp32 error for the sums an encoder's gradient is.  Always against the fp64 reference and torch's
fp32, never against the kernels.

ReLU kinks: ``dout`` is zeroed on the rows whose fp64 pre-activations (computed on the CPU) come within 1e-5, relative,
of a kink, as ``_away_from_kinks`` of the wide-input tests does; every case asserts that this removes at most 5 % of
its rows (seeds are chosen so; a case that exceeds the cap is reseeded, not loosened).

Inputs and parameters are drawn on the CPU from seeded generators, so the same numbers are tested on every machine.
"""

from __future__ import annotations

import contextlib
import copy
import dataclasses
import itertools
import os
from typing import Any, Callable

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402
from rl8_amd import models as models_module  # noqa: E402
from rl8_amd import models_recurrent  # noqa: E402
from rl8_amd.data import DataKeys  # noqa: E402
from rl8_amd.distributions import Categorical, Normal  # noqa: E402
from rl8_amd.models import DefaultContinuousModel  # noqa: E402
from rl8_amd.nn import functional as RF  # noqa: E402
from rl8_amd.nn import fused_attention, fused_feedforward, fused_lstm, fused_mlp, piecewise_mlp  # noqa: E402
from rl8_amd.specs import Unbounded  # noqa: E402
from rl8_amd.tensordict import TensorDict  # noqa: E402

from .test_autograd_contract_host import CONTRACT  # noqa: E402

DEV = "cuda:0"
TOWER_KERNELS = ("mlp_", "pw_", "batchnorm_fold", "tower_moments")
LSTM_KERNELS = ("lstm_",)
HEADS_KERNELS = ("linear_heads",)
ATTENTION_KERNELS = ("attention",)
FEEDFORWARD_KERNELS = ("feedforward",)
MASKED_KERNELS = ("masked_",)
PPO_KERNELS = ("ppo_loss",)


# --------------------------------------------------------------------------------------------------------------------
# The harness: a case builds modules and inputs on the CPU, ``run`` takes them through the public entry (or, as the
# reference, through the plain torch expression), ``_grads`` differentiates a fixed linear functional of the outputs.
# --------------------------------------------------------------------------------------------------------------------
class _Encoder(nn.Module):
    """What stands in front of a node in a real model: ``Linear(3, d)`` on raw features, or -- as ``LSTMTrader``
    does -- ``Embedding(2, 2)`` whose two columns replace the first two of the input."""

    def __init__(self, kind: str, d_out: int) -> None:
        super().__init__()
        self.kind = kind
        self.layer = nn.Linear(3, d_out) if kind == "encoder" else nn.Embedding(2, 2)

    def forward(self, raw: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
        if self.kind == "encoder":
            return self.layer(raw.to(self.layer.weight.dtype))
        return torch.cat([self.layer(raw), like[..., 2:]], dim=-1)


@dataclasses.dataclass
class Case:
    name: str
    #: input name -> the (node, forward parameter) rows of CONTRACT it reaches
    rows: dict[str, list[tuple[str, str]]]
    kernels: tuple[str, ...]
    #: (generator, which, drive) -> (modules, tensors, douts), all on the CPU in fp32
    build: Callable[..., tuple[nn.ModuleDict, dict[str, torch.Tensor], list[torch.Tensor]]]
    #: (modules, tensors, reference) -> (outputs, declined)
    run: Callable[..., tuple[list[torch.Tensor], bool]]
    bar: Callable[..., None]
    seed: int = 0
    env: dict[str, str] = dataclasses.field(default_factory=dict)
    patches: list[tuple[Any, str, Any]] = dataclasses.field(default_factory=list)
    drives: tuple[str, ...] = ("leaf", "encoder")

    def kind(self, which: str) -> str:
        kinds = {_row_kind(node, name) for node, name in self.rows[which]}
        assert len(kinds) == 1, (self.name, which, kinds)
        return kinds.pop()

    def apply(self, monkeypatch) -> None:
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        for obj, attr, value in self.patches:
            monkeypatch.setattr(obj, attr, value)


def _row_kind(node: str, name: str) -> str:
    (key,) = [k for k in CONTRACT if k.endswith("." + node)]
    kind = CONTRACT[key]["inputs"][name]
    if isinstance(kind, dict):
        kinds = set(kind.values()) - {"kernel output"}
        assert len(kinds) == 1
        return kinds.pop()
    return kind


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _init(module: nn.Module, g: torch.Generator, scale: float = 1.0) -> nn.Module:
    """The module's parameters redrawn from ``g`` in the ranges of torch's own default initialisation."""
    with torch.no_grad():
        for p in module.parameters():
            fan_in = p.shape[-1] if p.dim() > 1 else p.shape[0]
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale / fan_in ** 0.5)
    return module


def _timed(fn):
    """``fn()`` and ``{kernel: launches}`` of what it ran."""
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        out = fn()
        names = {k: int(v["launches"]) for k, v in hip.timer.summary().items()}
    finally:
        hip.timer.enabled = False
        hip.timer.reset()
    return out, names


def _of(names: dict[str, int], prefixes: tuple[str, ...]) -> dict[str, int]:
    return {k: v for k, v in sorted(names.items()) if k.startswith(prefixes)}


def _cast(mods: nn.Module, tensors: dict, dtype: None | torch.dtype):
    """Copies of the CPU modules and tensors on the device, in ``dtype`` (``None``: as they are, fp32)."""
    device = DEV
    mods = copy.deepcopy(mods).to(device)
    if dtype is not None:
        mods = mods.double() if dtype == torch.float64 else mods.float()
    tensors = {k: (v.to(device, dtype) if v.is_floating_point() and dtype is not None else v.to(device))
               for k, v in tensors.items()}
    return mods, tensors


def _prepare(mods: nn.Module, tensors: dict, which: None | str, drive: str, toggle: bool):
    """The inputs of one run, detached, with ``which`` made to require its gradient (``toggle``) as a leaf or behind
    the encoder.  Returns them and the leaf whose ``.grad`` is the input's gradient (``None`` behind an encoder)."""
    t = {k: v.detach() for k, v in tensors.items()}
    leaf = None
    if which is not None:
        if drive == "leaf":
            t[which] = t[which].clone().requires_grad_(toggle)
            leaf = t[which] if toggle else None
        else:
            x = mods["enc"](t[which + "_raw"], t[which])
            t[which] = x if toggle else x.detach()
    return t, leaf


def _loss(outs: list[torch.Tensor], douts: list[torch.Tensor]) -> torch.Tensor:
    assert len(outs) == len(douts)
    return sum((o.reshape(d.shape) * d.to(o.device, o.dtype)).sum() for o, d in zip(outs, douts))


def _grads(case: Case, mods: nn.Module, tensors: dict, douts: list, which: None | str, drive: str, *,
           reference: bool = False, toggle: bool = True) -> tuple[dict[str, None | torch.Tensor], bool]:
    for p in mods.parameters():
        p.grad = None
    t, leaf = _prepare(mods, tensors, which, drive, toggle)
    outs, declined = case.run(mods, t, reference)
    loss = _loss(outs, douts)
    if loss.requires_grad:  # (buffer data into a node without parameters: nothing to differentiate)
        loss.backward()
    g = {n: p.grad for n, p in mods.named_parameters()}
    if leaf is not None:
        g["input:" + which] = leaf.grad
    return g, declined


def _references(case: Case, mods, tensors, douts, which, drive):
    """fp64 and fp32 autograd of the plain torch expression on the same inputs."""
    out = []
    for dtype in (torch.float64, torch.float32):
        m, t = _cast(mods, tensors, dtype)
        out.append(_grads(case, m, t, douts, which, drive, reference=True)[0])
    return out


def _hold(case: Case, got: dict, want: dict, t32: dict, what: str, skip: tuple[str, ...] = ()) -> None:
    for k, w in want.items():
        if w is None or k.startswith(skip):
            continue
        assert got.get(k) is not None, f"{what}: the gradient of {k} is None -- dropped silently"
        assert got[k].shape == w.shape and torch.isfinite(got[k]).all(), (what, k)
        case.bar(got[k], w, t32[k], f"{what} {k}")


def _own(mods: nn.Module) -> list[str]:
    """The node's own parameters: everything but the encoder's."""
    return [n for n, _ in mods.named_parameters() if not n.startswith("enc.")]


def _check_row(case: Case, which: str, drive: str, monkeypatch) -> None:
    case.apply(monkeypatch)
    kind = case.kind(which)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed), which, drive)
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    want, t32 = _references(case, mods_cpu, tensors_cpu, douts, which, drive)
    what = f"{case.name} {which} {drive} ({kind})"
    (got, declined), names = _timed(lambda: _grads(case, mods, tensors, douts, which, drive))
    ran = _of(names, case.kernels)
    print(f"{what}: declined={declined} launches={ran}")
    if kind == "formed":
        assert not declined and ran, (what, names)
    else:
        assert kind == "declined", kind
        assert declined and not ran, (what, names)
    _hold(case, got, want, t32, what)
    # the same call on buffer data: the kernels, and the node's parameter gradients unmoved
    (off, declined_off), names_off = _timed(lambda: _grads(case, mods, tensors, douts, which, drive, toggle=False))
    assert not declined_off and _of(names_off, case.kernels), (what, names_off)
    own = _own(mods)
    if names == names_off:
        for k in own:
            assert torch.equal(off[k], got[k]), f"{what}: {k} moved with the input's requires_grad"
    _hold(case, {k: off[k] for k in own}, {k: want[k] for k in own}, t32, what + " requires_grad off")


# --------------------------------------------------------------------------------------------------------------------
# Bars.
# --------------------------------------------------------------------------------------------------------------------
def _tower_bar(got, want, t32, what):
    scale = float(want.abs().max()) + 1e-30
    rel, rel32 = (float((t.double() - want).abs().max()) / scale for t in (got, t32))
    print(f"gradient {what}: rel {rel:.3e} torch-fp32 {rel32:.3e} ratio {rel / rel32 if rel32 else float('nan'):.2f}")
    assert rel <= max(3 * rel32, 5e-6), (what, rel, rel32)


def _lstm_bar(got, want, t32, what):
    """``_check_grads`` of the LSTM tests; the heads' own parameters and input at the elementwise bars of their tests
    (``tests/test_lstm_gpu.py::test_linear_heads_match_torch``, ``tests/test_lstm_narrow_heads_gpu.py``), whose
    ``dout`` is scaled by one over the rows as it is here."""
    name = what.rsplit(" ", 1)[-1]
    if name.startswith("heads.") or name == "input:h":
        rtol, atol = (1e-4, 1e-7) if name.startswith("heads.") else (1e-5, 1e-9)
        err = (got.double() - want).abs()
        print(f"gradient {what}: err {float(err.max()):.3e} torch-fp32 {float((t32.double() - want).abs().max()):.3e} "
              f"largest {float(want.abs().max()):.3e}")
        torch.testing.assert_close(got.double(), want, rtol=rtol, atol=atol)
        return
    scale = float(want.abs().max())
    err, err32 = (float((t.double() - want).abs().max()) for t in (got, t32))
    print(f"gradient {what}: err {err:.3e} torch-fp32 {err32:.3e} scale {scale:.3e} "
          f"ratio {err / err32 if err32 else float('nan'):.2f}")
    assert err / scale < 2e-5, (what, err, scale)
    assert err <= max(3 * err32, 1e-6 * scale), (what, err, err32, scale)


def _three_times_bar(got, want, t32, what):
    torch_err, err = float((t32.double() - want).abs().max()), float((got.double() - want).abs().max())
    print(f"gradient {what}: err {err:.2e} / torch-fp32 {torch_err:.2e} = {err / torch_err if torch_err else float('nan'):.2f}")
    bar = 3 * torch_err + 2e-5 * float(want.abs().max()) + 1e-9
    assert err <= bar, (what, err, bar)


def _ppo_bar(got, want, t32, what):
    torch_err = float((t32.double() - want).abs().max())
    err = (got.double() - want).abs()
    print(f"gradient {what}: err {float(err.max()):.2e} torch-fp32 {torch_err:.2e}")
    bar = 2e-5 * want.abs() + 1e-6 * float(want.abs().max()) + 3 * torch_err
    assert bool((err <= bar).all()), (what, float((err - bar).max()))


def _near_kinks(*pre: torch.Tensor) -> torch.Tensor:
    """Rows (first dimension) with a pre-activation within 1e-5, relative to the largest, of a ReLU kink."""
    near = torch.zeros(pre[0].shape[0], dtype=torch.bool)
    for z in pre:
        z = z.detach().reshape(z.shape[0], -1)
        near |= (z.abs() < 1e-5 * float(z.abs().max())).any(1)
    assert int(near.sum()) * 20 <= near.numel(), f"{int(near.sum())} of {near.numel()} rows sit on a kink: reseed"
    return near


# --------------------------------------------------------------------------------------------------------------------
# Towers.
# --------------------------------------------------------------------------------------------------------------------
def _tower_modules(g, d_in: int, width: int, n_outs: tuple[int, ...], norm: bool) -> nn.ModuleDict:
    layers = [nn.Linear(d_in, width), *([nn.BatchNorm1d(width)] if norm else []), nn.ReLU(), nn.Linear(width, width)]
    trunk = nn.Sequential(nn.Sequential(*layers), nn.ReLU())
    mods = nn.ModuleDict({"trunk": trunk, "heads": nn.ModuleList([nn.Linear(width, n) for n in n_outs])})
    _init(mods, g)
    if norm:
        with torch.no_grad():
            bn = trunk[0][1]
            bn.weight.copy_(1.0 + 0.2 * torch.randn(width, generator=g))
            bn.bias.copy_(0.1 * torch.randn(width, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(width, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(width, generator=g))
    return mods


def _tower_build(d_in: int, width: int, n_outs: tuple[int, ...], m: int, *, norm: bool = False, training: bool = True):
    def build(g, which, drive):
        mods = _tower_modules(g, d_in, width, n_outs, norm)
        mods.train(training)
        tensors = {"x": torch.randn(m, d_in, generator=g)}
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, d_in), g)
            tensors["x_raw"] = torch.randn(m, 3, generator=g)
        ref = copy.deepcopy(mods).double()
        with torch.no_grad():
            x = tensors["x"].double() if drive == "leaf" else ref["enc"](tensors["x_raw"].double(), None)
            inner = ref["trunk"][0]
            z1, z2 = inner[:-2](x), inner(x)
        dout = torch.randn(m, sum(n_outs), generator=g).masked_fill(_near_kinks(z1, z2)[:, None], 0.0)
        return mods, tensors, [dout]
    return build


def _modules_tower(mods, x):
    return torch.cat([h(mods["trunk"](x)) for h in mods["heads"]], dim=-1)


def _tower_run(pair_gradients=None):
    def run(mods, t, reference):
        x = t["x"]
        out = None if reference else fused_mlp.tower_forward(mods["trunk"], list(mods["heads"]), x,
                                                             pair_gradients=pair_gradients)
        return [_modules_tower(mods, x) if out is None else out], out is None
    return run


def _replay_run(mods, t, reference):
    """The tower as ``Algorithm`` evaluates it in its first SGD pass: recorded during a one-step rollout on the very
    rows, then asked for inside the ``replay`` context."""
    x = t["x"]
    if reference:
        return [_modules_tower(mods, x)], True
    trunk, heads = mods["trunk"], list(mods["heads"])
    record = fused_mlp.RolloutRecord(1, x.shape[0], keep_general=True)
    record.begin()
    timing, hip.timer.enabled = hip.timer.enabled, False  # (the rollout's launch is not part of the call under test)
    try:
        with torch.no_grad(), record.at(0):
            assert fused_mlp.tower_forward(trunk, heads, x) is not None
    finally:
        hip.timer.enabled = timing
    record.seal(x)
    rows = record.rows_for(x, slice(0, x.shape[0]))
    assert rows, "nothing was recorded"
    before = fused_mlp.replay_stats["replayed_towers"]
    with fused_mlp.replay(rows, x):
        out = fused_mlp.tower_forward(trunk, heads, x)
    if out is not None:
        assert fused_mlp.replay_stats["replayed_towers"] == before + 1, "the record was not replayed"
    return [_modules_tower(mods, x) if out is None else out], out is None


def _tower_case(name, node, d_in, width, n_outs, m=65, *, run=None, seed=0, **kw) -> Case:
    build_kw = {k: kw.pop(k) for k in ("norm", "training") if k in kw}
    return Case(name, {"x": [(node, "x")]}, TOWER_KERNELS, _tower_build(d_in, width, n_outs, m, **build_kw),
                run or _tower_run(), _tower_bar, seed=seed, **kw)


_BN = {"RL8_AMD_BATCHNORM_TOWERS": "1"}
TOWERS = [
    _tower_case("tower256-n1", "_FusedTower", 5, 256, (1,), seed=101),
    _tower_case("tower256-n2", "_FusedTower", 5, 256, (2,), seed=2),
    _tower_case("tower256-n3", "_FusedTower", 5, 256, (3,), seed=3),
    _tower_case("tower256-two-heads", "_FusedTower", 5, 256, (2, 1), seed=4),
    _tower_case("wide-input", "_WideInputTower", 17, 256, (3,), seed=5),
    _tower_case("tower64", "_NarrowTower", 5, 64, (3,), seed=6),
    _tower_case("tower128", "_NarrowTower", 5, 128, (3,), seed=7),
    _tower_case("batchnorm64-training", "_NarrowBatchNormTower", 7, 64, (3,), 67, seed=8, norm=True, env=_BN),
    _tower_case("batchnorm64-eval", "_NarrowBatchNormTower", 7, 64, (3,), 67, seed=9, norm=True, training=False, env=_BN),
    _tower_case("piecewise", "_PiecewiseTower", 1, 256, (2,), seed=111, patches=[(piecewise_mlp, "ENABLED", True)]),
    _tower_case("replay", "_ReplayedTower", 5, 256, (1,), seed=11, run=_replay_run),
]


# --------------------------------------------------------------------------------------------------------------------
# LSTMs, through the default recurrent models' own callers (``_run_lstm_heads`` / ``_run_lstm``: every entry of
# ``fused_lstm`` and the models' fallback to the module).
# --------------------------------------------------------------------------------------------------------------------
B, L, D_IN = 33, 3, 4


def _lstm_build(hidden: int, layers: int, head_outs: tuple[int, ...]):
    def build(g, which, drive):
        mods = nn.ModuleDict({"lstm": nn.LSTM(D_IN, hidden, num_layers=layers, batch_first=True),
                              "heads": nn.ModuleList([nn.Linear(hidden, n) for n in head_outs])})
        _init(mods, g)
        tensors = {"x": torch.randn(B, L, D_IN, generator=g),
                   "h0": 0.5 * torch.randn(B, layers, hidden, generator=g),
                   "c0": 0.5 * torch.randn(B, layers, hidden, generator=g)}
        if drive == "encoder":
            mods["enc"] = _init(_Encoder(drive, tensors[which].shape[-1]), g)
            tensors[which + "_raw"] = torch.randn(*tensors[which].shape[:-1], 3, generator=g)
        elif drive == "embedding":
            mods["enc"] = _Encoder(drive, D_IN)
            with torch.no_grad():
                mods["enc"].layer.weight.copy_(torch.randn(2, 2, generator=g))
            tensors["x_raw"] = torch.randint(0, 2, (B, L), generator=g)
        # (the heads' gradients as their own tests scale them: dout over the rows)
        douts = ([torch.randn(B * L, n, generator=g) / (B * L) for n in head_outs] if head_outs
                 else [torch.randn(B, L, hidden, generator=g)])
        return mods, tensors, douts
    return build


def _lstm_run(mods, t, reference):
    lstm, heads = mods["lstm"], list(mods["heads"])
    x, h0, c0 = t["x"], t["h0"], t["c0"]
    if reference:
        with torch.backends.cudnn.flags(enabled=False):
            latents, _ = lstm(x, (h0.transpose(0, 1).contiguous(), c0.transpose(0, 1).contiguous()))
        return ([h(latents) for h in heads] if heads else [latents]), True
    states = TensorDict({DataKeys.HIDDEN_STATES: h0[:, None].expand(-1, L, -1, -1),
                         DataKeys.CELL_STATES: c0[:, None].expand(-1, L, -1, -1)}, batch_size=[B, L])
    calls: list[int] = []
    real = lstm.forward
    lstm.forward = lambda *a, **k: calls.append(1) or real(*a, **k)  # (the models' fallback is the module itself)
    try:
        if heads:
            outs, _ = models_recurrent._run_lstm_heads(lstm, heads, x, states)
        else:
            outs = [models_recurrent._run_lstm(lstm, x, states)[0]]
    finally:
        del lstm.forward
    return list(outs), bool(calls)


def _lstm_case(name, hidden, layers, head_outs, nodes, seed, patches=(), drives=("leaf", "encoder")) -> Case:
    rows = {which: [(node, which) for node in nodes] for which in ("x", "h0", "c0")}
    return Case(name, rows, LSTM_KERNELS, _lstm_build(hidden, layers, head_outs), _lstm_run, _lstm_bar, seed=seed,
                patches=[(fused_lstm, k, v) for k, v in patches], drives=drives)


def _plan_patches(gemm, rows, fuse):
    return (("FORWARD_GEMM", gemm), ("BACKWARD_ROWS", rows), ("FUSE_HEADS", fuse))


LSTMS = [
    _lstm_case(f"lstm256-{gemm}-rows{int(rows)}-fuse{int(fuse)}", 256, 1, (3, 1),
               ["_FusedLSTMHeads" if gemm == "split" and rows and fuse else "_FusedLSTM"], 20 + i,
               _plan_patches(gemm, rows, fuse), drives=("leaf", "encoder", "embedding") if i == 0 else ("leaf", "encoder"))
    for i, (gemm, rows, fuse) in enumerate(itertools.product(("split", "f32"), (True, False), (True, False)))
] + [
    _lstm_case("lstm256-no-heads", 256, 1, (), ["_FusedLSTM"], 30),
    _lstm_case("lstm64-fuse1", 64, 1, (3, 1), ["_NarrowLSTMHeads"], 31, (("FUSE_HEADS", True),),
               drives=("leaf", "encoder", "embedding")),
    _lstm_case("lstm64-fuse0", 64, 1, (3, 1), ["_NarrowLSTM"], 32, (("FUSE_HEADS", False),)),
    _lstm_case("lstm128-fuse1", 128, 1, (3, 1), ["_NarrowLSTMHeads"], 33, (("FUSE_HEADS", True),)),
    _lstm_case("lstm128-fuse0", 128, 1, (3, 1), ["_NarrowLSTM"], 34, (("FUSE_HEADS", False),)),
    _lstm_case("lstm64-no-heads", 64, 1, (), ["_NarrowLSTM"], 35),
    _lstm_case("stack64x2", 64, 2, (3, 1), ["_StackLSTM"], 36),
    _lstm_case("stack128x2-no-heads", 128, 2, (), ["_StackLSTM"], 37),
]


def _heads_build(hidden: int, head_outs: tuple[int, ...], m: int = 67):
    def build(g, which, drive):
        mods = nn.ModuleDict({"heads": _init(nn.ModuleList([nn.Linear(hidden, n) for n in head_outs]), g)})
        tensors = {"h": torch.randn(m, hidden, generator=g)}
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, hidden), g)
            tensors["h_raw"] = torch.randn(m, 3, generator=g)
        return mods, tensors, [torch.randn(m, n, generator=g) / m for n in head_outs]
    return build


def _heads_run(mods, t, reference):
    heads, h = list(mods["heads"]), t["h"]
    outs = None if reference else fused_lstm.heads_forward(heads, h)
    return ([head(h) for head in heads] if outs is None else outs), outs is None


HEADS = [Case(f"heads{hidden}", {"h": [("_Heads", "h")]}, HEADS_KERNELS, _heads_build(hidden, (3, 1)), _heads_run,
              _lstm_bar, seed=40 + i) for i, hidden in enumerate((256, 64, 128))]


# --------------------------------------------------------------------------------------------------------------------
# Attention, feedforward, the masked functions, the PPO loss.
# --------------------------------------------------------------------------------------------------------------------
E, HEADS_N = 8, 2


def _attention_build(tq: int, tk: None | int, padded: bool):
    def build(g, which, drive):
        mods = nn.ModuleDict({"mha": nn.MultiheadAttention(E, HEADS_N, batch_first=True)})
        _init(mods, g, scale=2.0)
        tensors = {"q": torch.randn(3, tq, E, generator=g)}
        if tk is not None:
            tensors["kv"] = torch.randn(3, tk, E, generator=g)
        if padded:
            mask = torch.rand(3, tk or tq, generator=g) < 0.4
            mask[:, 0] = False  # (every query keeps a key)
            tensors["padding"] = mask
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, E), g)
            tensors[which + "_raw"] = torch.randn(*tensors[which].shape[:-1], 3, generator=g)
        return mods, tensors, [torch.randn(3, tq, E, generator=g)]
    return build


def _attention_run(mods, t, reference):
    mha, q = mods["mha"], t["q"]
    kv = t.get("kv", q)  # (self-attention: the very tensor)
    out = None if reference else fused_attention.multihead_attention(mha, q, kv, t.get("padding"), t.get("bias"))
    if out is None:
        return [mha(q, kv, kv, key_padding_mask=t.get("padding"), attn_mask=t.get("bias"), need_weights=False)[0]], True
    return [out], False


ATTENTION = [
    Case("self-attention", {"q": [("_SelfAttentionCore", "qkv")]}, ATTENTION_KERNELS, _attention_build(5, None, False),
         _attention_run, _three_times_bar, seed=50),
    Case("cross-attention", {"q": [("_CrossAttentionCore", "q")], "kv": [("_CrossAttentionCore", "kv")]},
         ATTENTION_KERNELS, _attention_build(4, 5, True), _attention_run, _three_times_bar, seed=51),
]


def _feedforward_build(f: int, hidden: int, rows: int = 67):
    def build(g, which, drive):
        block = nn.Sequential(nn.LayerNorm(f), nn.Linear(f, hidden), nn.ReLU(), nn.Dropout(0.0), nn.Linear(hidden, f))
        _init(block, g)
        with torch.no_grad():
            block[0].weight.copy_(1.0 + 0.2 * torch.randn(f, generator=g))
            block[0].bias.copy_(0.3 * torch.randn(f, generator=g))
        mods = nn.ModuleDict({"block": block})
        tensors = {"y": torch.randn(rows, f, generator=g)}
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, f), g)
            tensors["y_raw"] = torch.randn(rows, 3, generator=g)
        ref = copy.deepcopy(mods).double()
        with torch.no_grad():
            y = tensors["y"].double() if drive == "leaf" else ref["enc"](tensors["y_raw"].double(), None)
            z = ref["block"][:2](y)
        return mods, tensors, [z, torch.randn(rows, f, generator=g)]  # (the pre-activations: see _feedforward_case)
    return build


def _feedforward_case(f, hidden, kind, seed) -> Case:
    inner = _feedforward_build(f, hidden)

    def build(g, which, drive):
        mods, tensors, (z, dy) = inner(g, which, drive)
        near = _near_kinks(z)[:, None]
        dout = torch.cat([torch.randn(dy.shape, generator=g), dy], dim=-1) if kind == "cat" else dy
        return mods, tensors, [dout.masked_fill(near, 0.0)]

    def run(mods, t, reference):
        y = t["y"]
        out = None if reference else fused_feedforward.skip_feedforward(mods["block"], y, kind)
        return [RF.skip_connection(y, mods["block"](y), kind=kind) if out is None else out], out is None

    return Case(f"feedforward-{f}x{hidden}-{kind}", {"y": [("_FeedforwardBlock", "x")]}, FEEDFORWARD_KERNELS, build, run,
                _three_times_bar, seed=seed, env={"RL8_AMD_FEEDFORWARD_KERNELS": "1"})


FEEDFORWARD = [_feedforward_case(f, hidden, kind, 60 + i)
               for i, ((f, hidden), kind) in enumerate(itertools.product(((1, 1), (5, 3)), ("residual", "cat", None)))]


@contextlib.contextmanager
def _environment(name: str, value: str):
    before = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = before


def _masked_case(name, node, fn, shape, mask_shape, seed) -> Case:
    def build(g, which, drive):
        mods = nn.ModuleDict()
        tensors = {"x": torch.randn(*shape, generator=g)}
        mask = torch.rand(*mask_shape, generator=g) < 0.6
        mask[:, 0] = True  # (a row without a valid cell is 0 / 0, in torch as in the kernel)
        tensors["mask"] = mask
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, shape[-1]), g)
            tensors["x_raw"] = torch.randn(*shape[:-1], 3, generator=g)
        out_shape = {"avg": (shape[0], *shape[2:]), "max": (shape[0], 1, *shape[2:]), "log_softmax": shape}[name]
        return mods, tensors, [torch.randn(*out_shape, generator=g)]

    def run(mods, t, reference):
        # (the reference is the function's own torch expression, which every input the kernels do not take runs)
        with _environment("RL8_AMD_MASKED_KERNELS", "0" if reference else "1"):
            out = fn(t["x"], mask=t["mask"])
        return [out[0] if isinstance(out, tuple) else out], reference

    return Case("masked-" + name, {"x": [(node, "x")]}, MASKED_KERNELS, build, run, _three_times_bar, seed=seed)


MASKED = [
    _masked_case("avg", "_MaskedAvg", RF.masked_avg, (65, 5, 3), (65, 5), 70),
    _masked_case("max", "_MaskedMax", RF.masked_max, (65, 5, 3), (65, 5), 71),
    _masked_case("log_softmax", "_MaskedLogSoftmax", RF.masked_log_softmax, (65, 3), (65, 3), 72),
]

PPO = dict(clip_param=0.2, dual_clip_param=5.0, entropy_coeff=0.01, vf_clip_param=1.0, vf_coeff=0.7)
M_PPO = 67


class _ComposedCategorical(Categorical):
    """The same maths under another ``logp``: ``ppo_losses`` then composes the loss from torch operations."""

    def logp(self, samples):
        return super().logp(samples)


class _ComposedNormal(Normal):
    def logp(self, samples):
        return super().logp(samples)


def _ppo_case(name, seed) -> Case:
    features = ("logits",) if name == "categorical" else ("mean", "log_std")

    def build(g, which, drive):
        m = M_PPO
        tensors = {"values": torch.randn(m, 1, generator=g), "returns": torch.randn(m, 1, generator=g),
                   "advantages": torch.randn(m, 1, generator=g)}
        if name == "categorical":
            tensors["logits"] = torch.randn(m, 1, 3, generator=g)
            tensors["actions"] = torch.randint(0, 3, (m, 1), generator=g)
            ref = Categorical(TensorDict({"logits": tensors["logits"].double()}, batch_size=[m]), None)
        else:
            tensors["mean"] = torch.randn(m, 2, generator=g)
            tensors["log_std"] = 0.3 * torch.randn(m, 2, generator=g)
            tensors["actions"] = tensors["mean"] + torch.randn(m, 2, generator=g)
            ref = Normal(TensorDict({k: tensors[k].double() for k in features}, batch_size=[m]), None)
        # the old log-probabilities a ratio of 0.85 to 1.15 away, and no sample on a clip boundary or the Huber clamp
        log_ratio = torch.log(0.85 + 0.3 * torch.rand(m, 1, generator=g, dtype=torch.float64))
        tensors["logp"] = (ref.logp(tensors["actions"].double() if name != "categorical" else tensors["actions"])
                           - log_ratio).float()
        mods = nn.ModuleDict()
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, tensors[which].shape[-1]), g, scale=0.1)
            tensors[which + "_raw"] = torch.randn(*tensors[which].shape[:-1], 3, generator=g)
        return mods, tensors, [torch.ones(())]

    def run(mods, t, reference):
        m = t["values"].shape[0]
        composed, fused = (_ComposedCategorical, Categorical) if name == "categorical" else (_ComposedNormal, Normal)
        dist = (composed if reference else fused)(TensorDict({k: t[k] for k in features}, batch_size=[m]), None)
        buffer = TensorDict({DataKeys.ACTIONS: t["actions"], DataKeys.LOGP: t["logp"],
                             DataKeys.ADVANTAGES: t["advantages"], DataKeys.RETURNS: t["returns"]}, batch_size=[m])
        sample = TensorDict({DataKeys.VALUES: t["values"]}, batch_size=[m])
        return [RF.ppo_losses(buffer, sample, dist, **PPO)["total"]], reference

    rows = {k: [("_AttachPrecomputedGrads", "tensors")] for k in (*features, "values")}
    return Case("ppo-" + name, rows, PPO_KERNELS, build, run, _ppo_bar, seed=seed)


PPO_CASES = [_ppo_case("categorical", 80), _ppo_case("normal", 81)]

ALL = TOWERS + LSTMS + HEADS + ATTENTION + FEEDFORWARD + MASKED + PPO_CASES


def _drives(case: Case, which: str) -> tuple[str, ...]:
    """An initial state behind an encoder at one case per width; everywhere else as a leaf."""
    if which in ("h0", "c0"):
        return ("leaf", "encoder") if case.name in ("lstm256-split-rows1-fuse1", "lstm64-fuse1") else ("leaf",)
    return case.drives


ROWS = [pytest.param(case, which, drive, id=f"{case.name}-{which}-{drive}")
        for case in ALL for which in case.rows for drive in _drives(case, which)]


@pytest.mark.parametrize("case,which,drive", ROWS)
def test_an_input_that_requires_a_gradient_gets_it_or_the_entry_declines(case, which, drive, monkeypatch):
    _check_row(case, which, drive, monkeypatch)


def test_every_float_input_of_every_node_is_driven():
    """Each (node, float input) of the table is reached by a case above, or by one of the tests below that names it."""
    driven = {(node, name) for case in ALL for rows in case.rows.values() for node, name in rows}
    driven |= {("_MeanAndLogStd", "out"), ("_SelfAttentionCore", "bias"), ("_CrossAttentionCore", "bias"),
               ("_MaskedSample", "x"), ("_MaskedSample", "noise")}
    params = {"w1", "b1", "w2", "b2", "w3", "b3", "gamma", "beta", "w_ih", "w_hh", "b_ih", "b_hh", "w_heads", "b_heads",
              "w", "b", "weights"}
    for key, row in CONTRACT.items():
        node = key.rsplit(".", 1)[1]
        for name, kind in row["inputs"].items():
            leaves = set(kind.values()) if isinstance(kind, dict) else {kind}
            if leaves & {"formed", "declined", "refused"} and name not in params:
                assert (node, name) in driven, (node, name)


# --------------------------------------------------------------------------------------------------------------------
# Direct pins of the declining and refusing entries.
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in LSTMS if c.name in ("lstm256-split-rows1-fuse1", "lstm64-fuse1", "stack64x2")],
                         ids=lambda c: c.name)
def test_the_lstm_entries_decline_what_they_do_not_differentiate(case, monkeypatch):
    case.apply(monkeypatch)
    mods, t = _cast(*case.build(_gen(case.seed), "x", "leaf")[:2], None)
    lstm, heads = mods["lstm"], list(mods["heads"])
    stack = lstm.num_layers > 1

    def entries(x, h0, c0):
        if stack:
            return [fused_lstm.lstm_stack_forward(lstm, x, h0, c0)]
        return [fused_lstm.lstm_forward(lstm, x, h0[:, 0], c0[:, 0]),
                fused_lstm.lstm_heads_forward(lstm, heads, x, h0[:, 0], c0[:, 0])]

    x, h0, c0 = t["x"], t["h0"], t["c0"]
    assert all(out is not None for out in entries(x, h0, c0))
    want_x = lstm.hidden_size != 256
    for which in ("x", "h0", "c0"):
        args = {"x": x, "h0": h0, "c0": c0}
        args[which] = args[which].clone().requires_grad_(True)
        (outs, names) = _timed(lambda: entries(**args))
        if which == "x" and want_x:
            assert all(out is not None for out in outs)
        else:
            assert all(out is None for out in outs) and not _of(names, LSTM_KERNELS), (which, names)
        with torch.no_grad():  # (a rollout: nothing can follow, the kernels run)
            outs = [fused_lstm.lstm_forward(lstm, args["x"], args["h0"][:, 0], args["c0"][:, 0])] if not stack else \
                entries(**args)
            assert all(out is not None for out in outs), which


def test_a_float_attention_mask_that_requires_a_gradient_is_declined():
    for case in ATTENTION:
        mods, t = _cast(*case.build(_gen(case.seed), "q", "leaf")[:2], None)
        q, kv = t["q"], t.get("kv", t["q"])
        bias = torch.randn(q.shape[1], kv.shape[1], device=DEV)
        assert fused_attention.multihead_attention(mods["mha"], q, kv, t.get("padding"), bias) is not None
        out, names = _timed(lambda: fused_attention.multihead_attention(mods["mha"], q, kv, t.get("padding"),
                                                                        bias.clone().requires_grad_(True)))
        assert out is None and not _of(names, ATTENTION_KERNELS), names


def test_a_noise_that_requires_a_gradient_takes_the_torch_route_of_the_sampler():
    g = _gen(90)
    x, noise = torch.randn(65, 3, generator=g).to(DEV), (torch.rand(65, 3, generator=g) + 0.1).to(DEV)
    (value, index), names = _timed(lambda: RF.masked_categorical_sample(x.clone().requires_grad_(True), noise=noise))
    assert "masked_categorical_sample" in names and value.requires_grad and not index.requires_grad
    leaf = noise.clone().requires_grad_(True)
    (value, index), names = _timed(lambda: RF.masked_categorical_sample(x, noise=leaf))
    assert not _of(names, MASKED_KERNELS), names
    with torch.no_grad():
        _, names = _timed(lambda: RF.masked_categorical_sample(x, noise=leaf))
    assert "masked_categorical_sample" in names


@pytest.mark.parametrize("case", PPO_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("column", ["logp", "advantages", "returns"])
def test_ppo_losses_refuses_a_buffer_column_that_requires_a_gradient(case, column):
    mods, t = _cast(*case.build(_gen(case.seed), "values", "leaf")[:2], None)
    t = {k: v.detach() for k, v in t.items()}
    t["values"].requires_grad_(True)
    case.run(mods, t, False)[0][0].backward()  # (buffer data: the fused loss)
    assert t["values"].grad is not None
    t[column] = t[column].clone().requires_grad_(True)

    def refused():
        with pytest.raises((ValueError, TypeError), match=column):
            case.run(mods, t, False)

    _, names = _timed(refused)
    assert not names, f"launched before refusing: {names}"
    with torch.no_grad():  # (no gradient can follow: the kernel)
        _, names = _timed(lambda: case.run(mods, t, False))
    assert _of(names, PPO_KERNELS)


# --------------------------------------------------------------------------------------------------------------------
# _MeanAndLogStd, through the default continuous model.
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,which,drive", [(256, None, "leaf"), (64, None, "leaf"), (64, "x", "leaf"),
                                               (64, "x", "encoder")])
def test_the_continuous_models_mean_and_log_std_node(width, which, drive):
    """``_MeanAndLogStd`` stands between the policy tower and the loss: its ``out`` is the tower's output, whose gradient
    it forms.  On buffer observations at both widths; at width 64, where the tower forms dL/dx, also on observations
    that require a gradient (at 256 the tower declines them, and the model's fallback never reaches the node)."""
    m, d_in = 65, 5

    def build(g, which, drive):
        torch.manual_seed(int(g.initial_seed()))
        model = DefaultContinuousModel(Unbounded(d_in, device="cpu"), Unbounded(shape=torch.Size([2]), device="cpu"),
                                       hiddens=(width, width))
        mods = nn.ModuleDict({"model": _init(model, g)})
        tensors = {"x": torch.randn(m, d_in, generator=g)}
        if drive != "leaf":
            mods["enc"] = _init(_Encoder(drive, d_in), g)
            tensors["x_raw"] = torch.randn(m, 3, generator=g)
        ref = copy.deepcopy(mods).double()
        with torch.no_grad():
            x = tensors["x"].double() if drive == "leaf" or which is None else ref["enc"](tensors["x_raw"].double(), None)
            towers = (ref["model"].latent_model, ref["model"].vf_model)
            pre = [z for tower in towers for z in (tower[0][0](x), tower[0](x))]
        near = _near_kinks(*pre)[:, None]
        return mods, tensors, [torch.randn(m, n, generator=g).masked_fill(near, 0.0) for n in (2, 2, 1)]

    def run(mods, t, reference):
        model = mods["model"]
        before = fused_mlp.ENABLED
        fused_mlp.ENABLED = not reference
        try:
            features = model(TensorDict({DataKeys.OBS: t["x"]}, batch_size=[m]))
            return [features["mean"], features["log_std"], model.value_function()], reference
        finally:
            fused_mlp.ENABLED = before

    case = Case(f"continuous-model-{width}", {"x": [("_NarrowTower", "x")]}, TOWER_KERNELS, build, run, _tower_bar, seed=95)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed + width), which, drive)
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    want, t32 = _references(case, mods_cpu, tensors_cpu, douts, which, drive)
    calls: list[int] = []
    apply = models_module._MeanAndLogStd.apply
    models_module._MeanAndLogStd.apply = staticmethod(lambda *a: calls.append(1) or apply(*a))
    try:
        (got, _), names = _timed(lambda: _grads(case, mods, tensors, douts, which, drive))
    finally:
        del models_module._MeanAndLogStd.apply
    assert calls and _of(names, TOWER_KERNELS), "the node under test did not run"
    _hold(case, got, want, t32, f"{case.name} {which} {drive}")


# --------------------------------------------------------------------------------------------------------------------
# Further cases on the same harness.
# --------------------------------------------------------------------------------------------------------------------
FURTHER = [c for c in TOWERS + LSTMS + HEADS if c.name in (
    "tower256-n1", "tower256-n2", "tower256-n3", "wide-input", "tower64", "batchnorm64-training", "piecewise", "replay",
    "lstm256-split-rows1-fuse1", "lstm256-f32-rows0-fuse0", "lstm64-fuse1", "lstm64-fuse0", "stack64x2", "heads256")]


def _first_input(case: Case) -> str:
    return next(iter(case.rows))


@pytest.mark.parametrize("case", FURTHER, ids=lambda c: c.name)
def test_only_the_input_requires_a_gradient(case, monkeypatch):
    """Every module parameter frozen: the input's gradient is right, or the route has declined (a backward that reads
    ``ctx.saved_tensors`` after a forward that saved nothing raises here)."""
    case.apply(monkeypatch)
    which = _first_input(case)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed), which, "leaf")
    mods_cpu.requires_grad_(False)
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    want, t32 = _references(case, mods_cpu, tensors_cpu, douts, which, "leaf")
    (got, declined), names = _timed(lambda: _grads(case, mods, tensors, douts, which, "leaf"))
    print(f"{case.name}: declined={declined} launches={_of(names, case.kernels)}")
    assert declined or _of(names, case.kernels)
    _hold(case, got, want, t32, f"{case.name} frozen parameters")
    assert got["input:" + which] is not None


def _frozen(case: Case, mods: nn.Module) -> list[str]:
    if "lstm" in dict(mods.named_children()):
        return ["lstm.weight_ih_l0"]
    if "trunk" in dict(mods.named_children()):
        return ["trunk.0.0.weight", "trunk.0.0.bias"]  # layer 1
    return ["heads.0.bias"]


@pytest.mark.parametrize("case", FURTHER, ids=lambda c: c.name)
def test_a_frozen_subset_gets_no_gradient_and_moves_no_other(case, monkeypatch):
    case.apply(monkeypatch)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed), None, "leaf")
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    whole, declined = _grads(case, mods, tensors, douts, None, "leaf")
    assert not declined
    whole = {k: v.clone() for k, v in whole.items()}
    names = _frozen(case, mods)
    for n, p in mods.named_parameters():
        p.requires_grad_(n not in names)
    (part, declined), launched = _timed(lambda: _grads(case, mods, tensors, douts, None, "leaf"))
    assert not declined and _of(launched, case.kernels)
    for k, v in whole.items():
        if k in names:
            assert part[k] is None, k
        else:
            assert torch.equal(part[k], v), k


@pytest.mark.parametrize("case", FURTHER, ids=lambda c: c.name)
def test_the_same_module_twice_in_one_graph(case, monkeypatch):
    """Two calls on two inputs under one ``backward()``: the parameter gradients are fp64's sum."""
    case.apply(monkeypatch)
    which = _first_input(case)
    mods_cpu, ta, da = case.build(_gen(case.seed), None, "leaf")
    _, tb, db = case.build(_gen(case.seed + 1000), None, "leaf")

    def both(mods, first, second, reference):
        for p in mods.parameters():
            p.grad = None
        loss = 0.0
        declined = False
        for t, douts in ((first, da), (second, db)):
            outs, d = case.run(mods, {k: v.detach() for k, v in t.items()}, reference)
            loss = loss + _loss(outs, douts)
            declined |= d
        loss.backward()
        return {n: p.grad for n, p in mods.named_parameters()}, declined

    refs = []
    for dtype in (torch.float64, torch.float32):
        m, a = _cast(mods_cpu, ta, dtype)
        refs.append(both(m, a, _cast(mods_cpu, tb, dtype)[1], True)[0])
    mods, a = _cast(mods_cpu, ta, None)
    b = _cast(mods_cpu, tb, None)[1]
    (got, declined), names = _timed(lambda: both(mods, a, b, False))
    assert not declined and _of(names, case.kernels), (which, names)
    _hold(case, got, refs[0], refs[1], f"{case.name} twice")


@pytest.mark.parametrize("order", ["pair-then-general", "general-then-pair"])
@pytest.mark.parametrize("hint", [None, False])
def test_a_pair_call_and_a_general_call_of_one_two_output_tower_in_one_graph(order, hint):
    """The 256-wide tower with two outputs: one call under ``pair_gradients=True`` whose ``dout`` columns are exact
    negatives (gate bits only, no h2 saved), one general call, one ``backward()``, in both orders of the two nodes.  What
    one call's backward finds (the ``_rl8_rank_one`` memo on layer 2) must not be applied to the other's saved tensors."""
    case = next(c for c in TOWERS if c.name == "tower256-n2")
    mods_cpu, ta, (da,) = case.build(_gen(case.seed), None, "leaf")
    _, tb, (db,) = case.build(_gen(case.seed + 1000), None, "leaf")
    da = torch.cat([da[:, :1], -da[:, :1]], dim=1)
    calls = [("pair", ta, da), ("general", tb, db)]
    if order == "general-then-pair":
        calls.reverse()

    def both(mods, calls, reference):
        for p in mods.parameters():
            p.grad = None
        loss = 0.0
        for kind, t, dout in calls:
            run = _tower_run(pair_gradients=True if kind == "pair" else hint)
            outs, declined = run(mods, {k: v.detach() for k, v in t.items()}, reference)
            assert reference or not declined
            loss = loss + _loss(outs, [dout])
        loss.backward()
        return {n: p.grad for n, p in mods.named_parameters()}

    refs = [both(_cast(mods_cpu, {}, dtype)[0], [(k, _cast(mods_cpu, t, dtype)[1], d) for k, t, d in calls], True)
            for dtype in (torch.float64, torch.float32)]
    mods = _cast(mods_cpu, {}, None)[0]
    on_device = [(k, _cast(mods_cpu, t, None)[1], d) for k, t, d in calls]
    for attempt in ("first", "second"):  # (the second with the memo the first has left)
        got, names = _timed(lambda: both(mods, on_device, False))
        print(f"{order} hint={hint} {attempt}: {_of(names, TOWER_KERNELS)}")
        assert names.get("mlp_wgrad_gate") == 1 and names.get("mlp_wgrad") == 1, names
        _hold(case, got, refs[0], refs[1], f"{order} {attempt}")


@pytest.mark.parametrize("case", FURTHER, ids=lambda c: c.name)
def test_a_second_backward_over_a_retained_graph_repeats_the_first(case, monkeypatch):
    case.apply(monkeypatch)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed), None, "leaf")
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    outs, declined = case.run(mods, {k: v.detach() for k, v in tensors.items()}, False)
    assert not declined
    loss = _loss(outs, douts)
    loss.backward(retain_graph=True)
    first = {n: p.grad.clone() for n, p in mods.named_parameters()}
    loss.backward()
    for n, p in mods.named_parameters():
        # (.grad = first + second, one rounding of a sum of two equal numbers: exact)
        assert torch.equal(p.grad, 2 * first[n]), n
        assert torch.equal(p.grad - first[n], first[n]), n


@pytest.mark.parametrize("case", [c for c in ALL if c.name != "replay"], ids=lambda c: c.name)
def test_under_no_grad_an_input_that_requires_a_gradient_still_takes_the_kernels(case, monkeypatch):
    """The rollout: no gradient can follow, so nothing is declined."""
    case.apply(monkeypatch)
    which = _first_input(case)
    mods, tensors = _cast(*case.build(_gen(case.seed), which, "leaf")[:2], None)
    t, _ = _prepare(mods, tensors, which, "leaf", True)
    assert t[which].requires_grad
    with torch.no_grad():
        (outs, declined), names = _timed(lambda: case.run(mods, t, False))
    assert not declined and _of(names, case.kernels), names
    assert not any(o.requires_grad for o in outs)


#: ``{kernel: launches}`` of one forward and backward of each entry on buffer data (``requires_grad=False``), as the
#: commit before the entries learned to decline launched them: the default path still launches exactly these.
LAUNCHES_BEFORE: dict[str, dict[str, int]] = {
    "tower256-n1": {"mlp_tower_backward_gate": 1, "mlp_tower_forward_save": 1, "mlp_wgrad_gate": 1},
    "tower256-n2": {"mlp_tower_backward": 1, "mlp_tower_forward_save": 1, "mlp_wgrad": 1},
    "tower256-n3": {"mlp_tower_backward": 1, "mlp_tower_forward_save": 1, "mlp_wgrad": 1},
    "tower256-two-heads": {"mlp_tower_backward": 1, "mlp_tower_forward_save": 1, "mlp_wgrad": 1},
    "wide-input": {"mlp_wgrad": 1, "mlp_wide_in_backward": 1, "mlp_wide_in_forward_save": 1, "mlp_wide_in_wgrad": 1},
    "tower64": {"mlp_narrow_backward": 1, "mlp_narrow_forward": 1, "mlp_narrow_reduce": 1},
    "tower128": {"mlp_narrow_backward": 1, "mlp_narrow_forward": 1, "mlp_narrow_reduce": 1},
    "batchnorm64-training": (
        {"batchnorm_fold": 1, "mlp_narrow_backward": 1, "mlp_narrow_forward": 1, "mlp_narrow_reduce": 1,
        "tower_moments": 1}),
    "batchnorm64-eval": (
        {"batchnorm_fold": 1, "mlp_narrow_backward": 1, "mlp_narrow_forward": 1, "mlp_narrow_reduce": 1}),
    "piecewise": {"pw_segment_sums": 1, "pw_tower_forward": 1},
    "replay": {"mlp_tower_backward_gate": 1, "mlp_wgrad_gate": 1},
    "lstm256-split-rows1-fuse1": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_rows_backward": 1, "lstm_step_save": 3,
        "lstm_wgrad": 1}),
    "lstm256-split-rows1-fuse0": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_rows_backward": 1, "lstm_step_save": 3,
        "lstm_wgrad": 1}),
    "lstm256-split-rows0-fuse1": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_step_save": 3, "lstm_wgrad":
        1}),
    "lstm256-split-rows0-fuse0": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_step_save": 3, "lstm_wgrad":
        1}),
    "lstm256-f32-rows1-fuse1": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_forward_save": 1,
        "lstm_wgrad": 1}),
    "lstm256-f32-rows1-fuse0": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_forward_save": 1,
        "lstm_wgrad": 1}),
    "lstm256-f32-rows0-fuse1": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_forward_save": 1,
        "lstm_wgrad": 1}),
    "lstm256-f32-rows0-fuse0": (
        {"linear_heads_backward": 1, "linear_heads_forward": 1, "lstm_backward": 1, "lstm_forward_save": 1,
        "lstm_wgrad": 1}),
    "lstm256-no-heads": {"lstm_rows_backward": 1, "lstm_step_save": 3, "lstm_wgrad": 1},
    "lstm64-fuse1": (
        {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1, "lstm_narrow_backward": 1,
        "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1}),
    "lstm64-fuse0": (
        {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1, "lstm_narrow_backward": 1,
        "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1}),
    "lstm128-fuse1": (
        {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1, "lstm_narrow_backward": 1,
        "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1}),
    "lstm128-fuse0": (
        {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1, "lstm_narrow_backward": 1,
        "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1}),
    "lstm64-no-heads": {"lstm_narrow_backward": 1, "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1},
    "stack64x2": (
        {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1, "lstm_narrow_backward": 1,
        "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1, "lstm_stack_backward": 1, "lstm_stack_forward": 1,
        "lstm_stack_reduce": 1}),
    "stack128x2-no-heads": (
        {"lstm_narrow_backward": 1, "lstm_narrow_forward": 1, "lstm_narrow_reduce": 1, "lstm_stack_backward": 1,
        "lstm_stack_forward": 1, "lstm_stack_reduce": 1}),
    "heads256": {"linear_heads_backward": 1, "linear_heads_forward": 1},
    "heads64": {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1},
    "heads128": {"linear_heads_narrow_backward": 1, "linear_heads_narrow_forward": 1},
    "self-attention": {"attention": 1, "attention_backward": 1},
    "cross-attention": {"attention": 1, "attention_backward": 1},
    "feedforward-1x1-residual": {"feedforward": 1, "feedforward_backward": 1},
    "feedforward-1x1-cat": {"feedforward": 1, "feedforward_backward": 1},
    "feedforward-1x1-None": {"feedforward": 1, "feedforward_backward": 1},
    "feedforward-5x3-residual": {"feedforward": 1, "feedforward_backward": 1},
    "feedforward-5x3-cat": {"feedforward": 1, "feedforward_backward": 1},
    "feedforward-5x3-None": {"feedforward": 1, "feedforward_backward": 1},
    "masked-avg": {"masked_pool": 1},
    "masked-max": {"masked_pool": 1},
    "masked-log_softmax": {"masked_log_softmax": 1},
    "ppo-categorical": {"ppo_loss_categorical": 1},
    "ppo-normal": {"ppo_loss_normal": 1},
}


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_launches_on_buffer_data_are_those_of_before(case, monkeypatch):
    case.apply(monkeypatch)
    mods_cpu, tensors_cpu, douts = case.build(_gen(case.seed), None, "leaf")
    mods, tensors = _cast(mods_cpu, tensors_cpu, None)
    (_, declined), names = _timed(lambda: _grads(case, mods, tensors, douts, None, "leaf"))
    print(f'    "{case.name}": {dict(sorted(names.items()))},')
    assert not declined
    assert names == LAUNCHES_BEFORE[case.name]
