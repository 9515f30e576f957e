"""The LSTM's route table (``fused_lstm._plan``) on the CPU: the plane-support query is stubbed with the envelope
``include/rl8_amd.h`` documents, and every plan is checked against the rules each call site applied before the decision
was made in one place."""

from __future__ import annotations

import itertools
import types

import pytest
import torch

from rl8_amd import hip
from rl8_amd.data import DataKeys
from rl8_amd.nn import fused_lstm

ENV_SWITCHES = ("RL8_AMD_LSTM_WGRAD_PLANES", "RL8_AMD_LSTM_WGRAD_GATES")


def _split_envelope(d_in: int) -> bool:
    """rl8_lstm_split_supports: every observation width up to seven."""
    return 1 <= d_in <= 7


@pytest.fixture
def envelope(monkeypatch):
    calls = []

    def supports(d_in):
        calls.append(d_in)
        return _split_envelope(d_in)

    fused_lstm._planes_supported.cache_clear()
    monkeypatch.setattr(hip, "lstm_split_supports", supports)
    yield calls
    fused_lstm._planes_supported.cache_clear()  # (before the stub goes: nothing may keep its answers)


def _switches(monkeypatch, gemm="split", rows=True, fuse=True, planes=None, gates=None):
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", gemm)
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", rows)
    monkeypatch.setattr(fused_lstm, "FUSE_HEADS", fuse)
    for name, value in zip(ENV_SWITCHES, (planes, gates)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _routes_by_call_site(gemm, rows, fuse, planes, gates, d_in, b) -> dict:
    """The routes as ``use_split``, ``_FusedLSTM.backward``, ``lstm_heads_forward`` and ``hip.lstm_backward`` each
    worked them out."""
    use_split = gemm == "split" and _split_envelope(d_in)
    rows_backward = use_split and rows                      # _FusedLSTM.backward: split=True, rows_packed
    split = True if rows_backward else use_split            # ... else split=use_split, the transposed pack
    fused_colsums = split and _split_envelope(d_in)         # hip.lstm_backward from here on
    f16 = rows_backward and (planes or "f16") != "bf16"    # (dg_bound comes from the rows kernel only)
    if not fused_colsums:
        wgrad = "f32"
    elif f16 and b >= 128 and (gates or "fused") != "separate":
        wgrad = "f16-gates"
    else:
        wgrad = "f16" if f16 else "bf16"
    return {"forward_planes": use_split, "backward_rows": rows_backward, "wgrad": wgrad,
            "fuse_heads": fuse and use_split and rows}


def _as_dict(plan) -> dict:
    return {k: getattr(plan, k) for k in ("forward_planes", "backward_rows", "wgrad", "fuse_heads")}


def test_plan_matches_the_call_sites_rules(envelope, monkeypatch):
    for switches in itertools.product(("split", "f32"), (True, False), (True, False), (None, "f16", "bf16"),
                                      (None, "fused", "separate")):
        _switches(monkeypatch, *switches)
        for d_in, b in itertools.product(range(1, 9), (1, 127, 128, 4096)):
            want = _routes_by_call_site(*switches, d_in, b)
            assert _as_dict(fused_lstm._plan(d_in, b)) == want, (switches, d_in, b)


def test_plan_reads_the_switches_per_call_and_the_build_once(envelope, monkeypatch):
    _switches(monkeypatch)
    assert [fused_lstm._plan(d, 4096).wgrad for d in range(1, 9)] == ["f16-gates"] * 7 + ["f32"]
    monkeypatch.setenv("RL8_AMD_LSTM_WGRAD_GATES", "separate")
    assert fused_lstm._plan(3, 4096).wgrad == "f16"
    monkeypatch.setenv("RL8_AMD_LSTM_WGRAD_PLANES", "bf16")
    assert fused_lstm._plan(3, 4096).wgrad == "bf16"
    monkeypatch.setattr(fused_lstm, "FUSE_HEADS", False)
    assert not fused_lstm._plan(3, 4096).fuse_heads
    monkeypatch.setattr(fused_lstm, "BACKWARD_ROWS", False)
    assert not fused_lstm._plan(3, 4096).backward_rows
    monkeypatch.setattr(fused_lstm, "FORWARD_GEMM", "f32")
    assert [fused_lstm._plan(d, 4096).wgrad for d in range(1, 9)] == ["f32"] * 8
    assert envelope == list(range(1, 9))  # one query per width, then the memo


class _Ctx:
    pass


def _ctx(plan, b=4, l=2):
    z = torch.zeros
    ctx = _Ctx()
    ctx.saved_tensors = (z(b, l, 1), z(b, 256), z(b, 256), z(b, l, 256), z(b, l, 4, 256), z(b, l, 256), z(3, 256))
    ctx.lstm, ctx.plan, ctx.h0_bound = torch.nn.LSTM(1, 256, batch_first=True), plan, z(1)
    return ctx


@pytest.mark.parametrize("made_under", [{}, {"planes": "bf16"}, {"gates": "separate"}, {"rows": False},
                                        {"gemm": "f32"}])
def test_backwards_run_the_forwards_plan(envelope, monkeypatch, made_under):
    """Switches flipped between forward and backward do not reach either backward: both follow ``ctx.plan``."""
    _switches(monkeypatch, **made_under)
    plan = fused_lstm._plan(1, 4096)
    if plan.forward_planes:  # every switch the other way
        _switches(monkeypatch, gemm="f32", rows=False, fuse=False, planes="bf16", gates="separate")
    else:
        _switches(monkeypatch)

    packs, seen = [], []
    monkeypatch.setattr(fused_lstm, "_packs", lambda lstm, kind: packs.append(kind) or kind)

    def backward(x, h0, c0, hs, gates, cs, dhs, whht_packed, *, wgrad, rows_packed=None, **kw):
        seen.append((wgrad, whht_packed, rows_packed))
        return {"w_ih": None, "w_hh": None, "b": None}

    monkeypatch.setattr(hip, "lstm_backward", backward)
    monkeypatch.setattr(hip, "linear_heads_backward",
                        lambda h, dout, w, need_dh=True: (torch.zeros_like(h) if need_dh else None, None, None))
    b, l = 4, 2
    ctx = _ctx(plan, b, l)
    ctx.saved_tensors = ctx.saved_tensors[:6]
    fused_lstm._FusedLSTM.backward(ctx, torch.zeros(b, l, 256), None)
    want_packs = ["rows"] if plan.backward_rows else ["transposed"]
    assert packs == want_packs
    assert seen == [(plan.wgrad, None, "rows") if plan.backward_rows else (plan.wgrad, "transposed", None)]
    if plan.fuse_heads:  # the heads node exists only where its plan runs the rows kernel
        packs.clear()
        seen.clear()
        for dhs in (None, torch.zeros(b, l, 256)):
            fused_lstm._FusedLSTMHeads.backward(_ctx(plan, b, l), torch.zeros(b * l, 3), dhs, None)
        assert packs == ["rows", "rows"] and seen == [(plan.wgrad, None, "rows")] * 2


def _lean_rollout(monkeypatch, d_in: int, n: int = 64, horizon: int = 4):
    """``_LeanRollout`` set up on CPU stand-ins for the algorithm and the library: (rollout, pack kinds asked for)."""
    from rl8_amd.algorithms._recurrent import _LeanRollout

    packs = []

    def stub_packs(lstm, kind):
        packs.append(kind)
        return (torch.zeros(1), torch.zeros(1)) if kind == "split" else torch.zeros(1)

    monkeypatch.setattr(hip, "load", lambda: None)
    monkeypatch.setattr(hip, "lstm_state_planes", lambda rows, device, copies=1: torch.zeros(copies * 64, dtype=torch.uint8))
    monkeypatch.setattr(fused_lstm, "_packs", stub_packs)
    ns = types.SimpleNamespace
    model = ns(lstm=torch.nn.LSTM(d_in, 256, batch_first=True), feature_head=torch.nn.Linear(256, 2),
               vf_head=torch.nn.Linear(256, 1))
    tm = {k: torch.zeros(horizon + 1, n, w) for k, w in ((DataKeys.OBS, d_in), (DataKeys.ACTIONS, 1), (DataKeys.LOGP, 1),
                                                          (DataKeys.VALUES, 1), (DataKeys.REWARDS, 1))}
    stm = {k: torch.zeros(horizon + 1, n, 256) for k in (DataKeys.HIDDEN_STATES, DataKeys.CELL_STATES)}
    algo = ns(policy=ns(model=model), _tm=tm, _tm_states=stm, local_num_envs=n, env=ns(state=torch.zeros(n), env_offset=0),
              hparams=ns(gamma=0.99), noise=ns(seed=0))
    return _LeanRollout(algo, False), packs


@pytest.mark.parametrize("gemm, d_in", [("split", 1), ("split", 7), ("split", 8), ("f32", 1), ("f32", 5)])
def test_lean_rollout_takes_its_step_kernel_from_the_plan(envelope, monkeypatch, gemm, d_in):
    _switches(monkeypatch, gemm=gemm)
    for fuse in ("1", "0"):
        monkeypatch.setenv("RL8_AMD_ROLLOUT_FUSE_HEADS", fuse)
        lean, packs = _lean_rollout(monkeypatch, d_in)
        planes = fused_lstm._plan(d_in, lean.n).forward_planes
        assert lean.split == planes and packs == ["split" if planes else "step"]
        assert lean.fuse_heads == (fuse == "1")  # (read when the rollout is set up)


# --- which family of kernels an nn.LSTM gets (``fused_lstm._family`` / ``_input_ok``) -----------------------------------
@pytest.fixture
def families(monkeypatch):
    """The build's three envelope queries stubbed with what ``include/rl8_amd.h`` documents."""
    monkeypatch.setattr(hip, "lstm_supports", lambda d_in: 1 <= d_in <= 7)
    monkeypatch.setattr(hip, "lstm_narrow_supports", lambda hidden, d_in: hidden in (64, 128) and 1 <= d_in <= 16)
    monkeypatch.setattr(hip, "lstm_stack_supports", lambda hidden: hidden in (64, 128))
    fused_lstm._narrow_supported.cache_clear()
    yield
    fused_lstm._narrow_supported.cache_clear()  # (before the stubs go: nothing may keep their answers)


def _families_by_predicate(enabled, lstm, x) -> tuple[bool, bool, bool]:
    """``_eligible``, ``_narrow_eligible`` and ``_stack_eligible`` as they stood while each family had its own
    predicate, clause for clause, on the stubbed envelopes."""
    wide = bool(
        enabled and x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and lstm.num_layers == 1
        and lstm.hidden_size == 256 and lstm.batch_first and lstm.bias and not lstm.bidirectional
        and lstm.proj_size == 0 and x.shape[2] == lstm.input_size and 1 <= lstm.input_size <= 7
    )
    narrow = bool(
        enabled and x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and lstm.num_layers == 1
        and lstm.hidden_size in (64, 128) and lstm.batch_first and lstm.bias and not lstm.bidirectional
        and lstm.proj_size == 0 and x.shape[2] == lstm.input_size
        and (lstm.hidden_size in (64, 128) and 1 <= lstm.input_size <= 16)
    )
    stack = bool(
        enabled and x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and lstm.num_layers >= 2
        and lstm.dropout == 0 and lstm.hidden_size in (64, 128) and lstm.batch_first and lstm.bias
        and not lstm.bidirectional and lstm.proj_size == 0 and x.shape[2] == lstm.input_size
        and (lstm.hidden_size in (64, 128) and 1 <= lstm.input_size <= 16) and lstm.hidden_size in (64, 128)
    )
    return wide, narrow, stack


def test_family_matches_the_three_predicates_it_replaced(families, monkeypatch):
    """Every clause of the old predicates flipped, every answer reached, ``ENABLED`` off as well; and the lean rollout's
    ``available`` says yes exactly for the one-layer families. The classifier reads a module's attributes, never its
    weights, so ONE module (inside one default model, for ``available``) has its attributes set row by row."""
    from rl8_amd import models_recurrent
    from rl8_amd.algorithms._recurrent import _LeanRollout
    from rl8_amd.distributions import Categorical
    from rl8_amd.env import DiscreteDummyEnv
    from rl8_amd.specs import Categorical as CategoricalSpec, Unbounded

    ns = types.SimpleNamespace
    model = models_recurrent.DefaultDiscreteRecurrentModel(
        Unbounded(shape=torch.Size([1]), device="cpu"), CategoricalSpec(2, shape=torch.Size([1]), device="cpu"), hidden_size=8)
    lstm = model.lstm
    algo = ns(policy=ns(model=model, distribution_cls=Categorical), _tm={DataKeys.OBS: torch.zeros(2, 1, 1)},
              env=object.__new__(DiscreteDummyEnv))  # (a DummyEnv, which `available` type-checks; nothing of it is run)
    # x as the input check sees it: device, dtype, rank, and a last extent that is input_size or one more
    inputs = list(itertools.product((True, False), (torch.float32, torch.float16), (3, 2), (0, 1)))
    seen, rows = set(), 0
    for enabled, hidden, layers, d_in, bias, batch_first, bidirectional, proj, dropout in itertools.product(
            (True, False), (32, 64, 96, 128, 256), (1, 2, 3), range(1, 18), (True, False), (True, False), (False, True),
            (0, 16), (0.0, 0.5)):
        monkeypatch.setattr(fused_lstm, "ENABLED", enabled)
        lstm.hidden_size, lstm.num_layers, lstm.input_size, lstm.bias = hidden, layers, d_in, bias
        lstm.batch_first, lstm.bidirectional, lstm.proj_size, lstm.dropout = batch_first, bidirectional, proj, dropout
        family = fused_lstm._family(lstm)
        assert _LeanRollout.available(algo) == (family in ("256", "narrow")), vars(lstm)
        for is_cuda, dtype, ndim, wider in inputs:
            x = ns(is_cuda=is_cuda, dtype=dtype, ndim=ndim, shape=(4, 3, d_in + wider)[:ndim] + (0,) * (3 - ndim))
            wide, narrow, stack = old = _families_by_predicate(enabled, lstm, x)
            assert sum(old) <= 1  # (so the order the old call sites asked them in carried no behaviour)
            want = "256" if wide else "narrow" if narrow else "stack" if stack else None
            got = family if fused_lstm._input_ok(lstm, x) else None
            assert got == want == fused_lstm._family_for(lstm, x), (enabled, vars(lstm), vars(x))
            seen.add(got)
            rows += 1
    assert seen == {None, "256", "narrow", "stack"} and rows >= 40320
