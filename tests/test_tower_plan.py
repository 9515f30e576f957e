"""The towers' route table (``fused_mlp._plan``) on the CPU: the support predicates are stubbed with the envelopes
``include/rl8_amd.h`` documents, and every plan is checked against the rules each call site applied before the
decision was made in one place."""

from __future__ import annotations

import functools
import itertools

import pytest
import torch

from rl8_amd import hip
from rl8_amd.nn import fused_mlp


def _forward_envelope(d_in: int, n_out: int) -> bool:
    """rl8_mlp_forward_f16_supports: any d_in <= 8 with n_out <= 8, and d_in 9..16 with n_out <= 4."""
    return 1 <= d_in <= 16 and 1 <= n_out <= 8 and not (d_in > 8 and n_out > 4)


def _backward_envelope(d_in: int, n_out: int) -> bool:
    """rl8_mlp_backward_f16_supports: d_in <= 7, n_out <= 4, 7 x 4 excepted."""
    return 1 <= d_in <= 7 and 1 <= n_out <= 4 and (d_in, n_out) != (7, 4)


@pytest.fixture
def envelopes(monkeypatch):
    calls = []

    def stub(envelope):
        def supports(d_in, n_out):
            calls.append((d_in, n_out))
            return envelope(d_in, n_out)
        return supports

    fused_mlp._planes_supported.cache_clear()
    monkeypatch.setattr(hip, "mlp_forward_f16_supports", stub(_forward_envelope))
    monkeypatch.setattr(hip, "mlp_backward_f16_supports", stub(_backward_envelope))
    yield calls
    fused_mlp._planes_supported.cache_clear()  # (before the stubs go: nothing may keep their answers)


def _routes_by_call_site(fwd: str, bwd: str, d_in: int, n_out: int, pair: bool, gates_on: bool) -> dict:
    """The routes as ``_FusedTower.forward``, ``_tower_backward`` and ``tower_forward`` each worked them out."""
    fwd_ok, bwd_ok = _forward_envelope(d_in, n_out), _backward_envelope(d_in, n_out)
    forward_planes = fwd == "f16" and fwd_ok
    keep_h1 = not (bwd == "f16" and bwd_ok) if forward_planes else True  # (the fp32 forward always stores h1)
    gate_only = (forward_planes and not keep_h1 and bwd == "f16" and bwd_ok and gates_on
                 and (n_out == 1 or (n_out == 2 and pair)))
    # (the backward's gate bits exist only after the plane forward)
    backward_planes = bwd == "f16" and forward_planes and bwd_ok
    recordable = fwd == "f16" and bwd == "f16" and fwd_ok and bwd_ok
    if recordable:  # the record's own rule
        assert gate_only == (gates_on and (n_out == 1 or (n_out == 2 and pair)))
    return {"forward_planes": forward_planes, "backward_planes": backward_planes, "wgrad_planes": bwd == "f16",
            "keep_h1": keep_h1, "gate_only": gate_only, "recordable": recordable, "gates": gates_on,
            "rank_one": gates_on and (n_out == 1 or (n_out == 2 and pair))}


def _as_dict(plan) -> dict:
    return {k: getattr(plan, k) for k in ("forward_planes", "backward_planes", "wgrad_planes", "keep_h1", "gate_only",
                                          "recordable", "gates", "rank_one")}


def test_plan_matches_the_call_sites_rules(envelopes, monkeypatch):
    for fwd, bwd, gates_on in itertools.product(("f16", "f32"), ("f16", "f32"), (True, False)):
        monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", fwd)
        monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", bwd)
        if gates_on:
            monkeypatch.delenv("RL8_WGRAD_GATE_OFF", raising=False)
        else:
            monkeypatch.setenv("RL8_WGRAD_GATE_OFF", "1")
        for d_in, n_out, pair in itertools.product((1, 5, 7, 8, 12, 16), (1, 2, 3, 4, 5, 6), (False, True)):
            want = _routes_by_call_site(fwd, bwd, d_in, n_out, pair, gates_on)
            assert _as_dict(fused_mlp._plan(d_in, n_out, pair)) == want, (fwd, bwd, gates_on, d_in, n_out, pair)


@pytest.mark.parametrize("d_in, n_out", [(8, 5), (12, 2), (7, 4), (16, 4)])
def test_mixed_route(envelopes, monkeypatch, d_in, n_out):
    """Plane forward, fp32 data gradient (h1 kept for it), dW2 on planes; never recorded."""
    monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", "f16")
    monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", "f16")
    plan = fused_mlp._plan(d_in, n_out, True)
    assert plan.forward_planes and not plan.backward_planes and plan.wgrad_planes
    assert plan.keep_h1 and not plan.gate_only and not plan.recordable


def test_plan_reads_the_switches_per_call_and_the_build_once(envelopes, monkeypatch):
    monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", "f16")
    monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", "f16")
    monkeypatch.delenv("RL8_WGRAD_GATE_OFF", raising=False)
    assert fused_mlp._plan(3, 1, False).gate_only
    monkeypatch.setenv("RL8_WGRAD_GATE_OFF", "1")
    assert not fused_mlp._plan(3, 1, False).gate_only
    monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", "f32")
    assert not fused_mlp._plan(3, 1, False).backward_planes
    monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", "f32")
    assert not fused_mlp._plan(3, 1, False).forward_planes
    assert envelopes == [(3, 1), (3, 1)]  # one forward and one backward query for the width, then the memo


def test_backward_runs_the_forwards_plan(envelopes, monkeypatch):
    """Switches flipped between forward and backward do not reach the backward: it follows ``ctx.plan``."""
    monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", "f16")
    monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", "f16")
    monkeypatch.delenv("RL8_WGRAD_GATE_OFF", raising=False)
    plan = fused_mlp._plan(3, 1, False)
    monkeypatch.setattr(fused_mlp, "FORWARD_GEMM", "f32")
    monkeypatch.setattr(fused_mlp, "BACKWARD_GEMM", "f32")
    monkeypatch.setenv("RL8_WGRAD_GATE_OFF", "1")

    packs, seen = [], {}
    monkeypatch.setattr(fused_mlp, "_packed", lambda layer, transposed, planes: packs.append((transposed, planes)))

    def backward(x, h1, h2, dout, w2t_packed, w3, w1, b1, **kw):
        seen.update(kw)
        return {k: None for k in ("w1", "b1", "w2", "b2", "w3", "b3")}

    monkeypatch.setattr(hip, "mlp_tower_backward", backward)

    class Ctx:
        pass

    ctx = Ctx()
    m, z = 4, torch.zeros
    gate = z(m, 8, dtype=torch.int32)
    ctx.saved_tensors = (z(m, 3), None, None, z(1, 256), z(256, 3), z(256), gate, z(256), z(1), z(256, 256))
    ctx.plan, ctx.layer2, ctx.w3_key = plan, torch.nn.Linear(256, 256), ()
    fused_mlp._tower_backward(ctx, z(m, 1))
    assert packs == [(True, True)]
    assert seen["gates_on"] is True and seen["wgrad_split"] is True and seen["gate2"] is gate
    assert seen["gate_pack"] is not None


# --------------------------------------------------------------------------- #
# ``fused_mlp._family`` against the two predicates it replaced.
# --------------------------------------------------------------------------- #
def _match(trunk, heads):
    """``fused_mlp._match`` as it stood while each family had its own predicate."""
    nn = torch.nn
    if not isinstance(trunk, nn.Sequential) or len(trunk) < 2:
        return None
    mlp, act = trunk[0], trunk[1]
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 3 or not isinstance(act, nn.ReLU):
        return None
    l1, a1, l2 = mlp[0], mlp[1], mlp[2]
    if not (isinstance(l1, nn.Linear) and isinstance(a1, nn.ReLU) and isinstance(l2, nn.Linear)):
        return None
    if l1.out_features != hip.MLP_HIDDEN or l2.out_features != hip.MLP_HIDDEN or l2.in_features != hip.MLP_HIDDEN:
        return None
    if l1.in_features > hip.MLP_MAX_IN or l1.bias is None or l2.bias is None:
        return None
    if sum(h.out_features for h in heads) > hip.MLP_MAX_OUT or any(h.bias is None for h in heads):
        return None
    if any(h.in_features != hip.MLP_HIDDEN for h in heads):
        return None
    return l1, l2


def _match_narrow(trunk, heads):
    """``fused_mlp._match_narrow`` as it stood, likewise."""
    nn = torch.nn
    if not isinstance(trunk, nn.Sequential) or len(trunk) < 2:
        return None
    mlp, act = trunk[0], trunk[1]
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 3 or not isinstance(act, nn.ReLU):
        return None
    l1, a1, l2 = mlp[0], mlp[1], mlp[2]
    if not (isinstance(l1, nn.Linear) and isinstance(a1, nn.ReLU) and isinstance(l2, nn.Linear)):
        return None
    width = l1.out_features
    if width not in hip.MLP_NARROW_HIDDEN or l2.in_features != width or l2.out_features != width:
        return None
    if l1.in_features > hip.MLP_MAX_IN or l1.bias is None or l2.bias is None:
        return None
    if not heads or sum(h.out_features for h in heads) > hip.MLP_MAX_OUT or any(h.bias is None for h in heads):
        return None
    if any(h.in_features != width for h in heads):
        return None
    return l1, l2


@functools.lru_cache(maxsize=None)
def _linear(d_in: int, d_out: int, bias: bool = True) -> torch.nn.Linear:
    """(the classifier reads a layer's attributes, never its weights: one module per shape serves every row)"""
    return torch.nn.Linear(d_in, d_out, bias=bias)


#: head lists as (input width relative to the trunk's: 0 = right, 1 = one more; outputs), by what they flip
_HEADS = {"none": [], "one": [(0, 1)], "one_of_8": [(0, 8)], "one_of_9": [(0, 9)], "two_sum_8": [(0, 4), (0, 4)],
          "two_sum_9": [(0, 4), (0, 5)], "one_wrong_width": [(1, 2)], "second_wrong_width": [(0, 1), (1, 1)]}


def _tower(width=256, d_in=4, *, l2="ok", no_bias=None, heads="one", act1="relu", act2="relu", shape="ok"):
    nn = torch.nn
    acts = {"relu": nn.ReLU, "tanh": nn.Tanh}
    l2_in, l2_out = {"ok": (width, width), "in": (width + 1, width), "out": (width, width + 1)}[l2]
    mlp = nn.Sequential(_linear(d_in, width, no_bias != "l1"), acts[act1](), _linear(l2_in, l2_out, no_bias != "l2"))
    hs = [_linear(width + off, n, not (no_bias == "head" and i == len(_HEADS[heads]) - 1))
          for i, (off, n) in enumerate(_HEADS[heads])]
    trunk = {"ok": lambda: nn.Sequential(mlp, acts[act2]()),
             "three": lambda: nn.Sequential(mlp, acts[act2](), nn.Identity()),  # (trunk[:2] is all either predicate read)
             "one": lambda: nn.Sequential(mlp),
             "not_sequential": lambda: nn.ModuleList([mlp, acts[act2]()]),
             "mlp_not_sequential": lambda: nn.Sequential(nn.ModuleList(list(mlp)), acts[act2]()),
             "mlp_of_four": lambda: nn.Sequential(nn.Sequential(*mlp, nn.Identity()), acts[act2]()),
             "l1_not_linear": lambda: nn.Sequential(nn.Sequential(nn.Identity(), mlp[1], mlp[2]), acts[act2]()),
             "l2_not_linear": lambda: nn.Sequential(nn.Sequential(mlp[0], mlp[1], nn.Identity()), acts[act2]())}[shape]()
    return trunk, hs


def _old_answer(trunk, heads):
    """What ``tower_forward`` did with the two predicates: narrow asked first, then wide."""
    narrow, wide = _match_narrow(trunk, heads), _match(trunk, heads)
    assert narrow is None or wide is None  # (so "narrow before wide" carried no behaviour)
    return ("narrow", *narrow) if narrow is not None else ("wide", *wide) if wide is not None else None


def _same(got, want) -> bool:
    return (got is None and want is None) or (got is not None and want is not None and got[0] == want[0]
                                               and got[1] is want[1] and got[2] is want[2])


#: one change to an accepted tower per clause of the old predicates; each must turn every family's answer to ``None``
_CLAUSE_FLIPS = {
    "trunk is a Sequential": dict(shape="not_sequential"),
    "trunk has two elements": dict(shape="one"),
    "trunk[0] is a Sequential": dict(shape="mlp_not_sequential"),
    "trunk[0] has three elements": dict(shape="mlp_of_four"),
    "trunk[1] is a ReLU": dict(act2="tanh"),
    "layer 1 is a Linear": dict(shape="l1_not_linear"),
    "the inner activation is a ReLU": dict(act1="tanh"),
    "layer 2 is a Linear": dict(shape="l2_not_linear"),
    "layer 2 reads the width": dict(l2="in"),
    "layer 2 writes the width": dict(l2="out"),
    "d_in <= 16": dict(d_in=17),
    "layer 1 has a bias": dict(no_bias="l1"),
    "layer 2 has a bias": dict(no_bias="l2"),
    "one head: outputs <= 8": dict(heads="one_of_9"),
    "two heads: outputs <= 8": dict(heads="two_sum_9"),
    "every head has a bias": dict(no_bias="head"),
    "the head reads the width": dict(heads="one_wrong_width"),
    "every head reads the width": dict(heads="second_wrong_width"),
}


def test_family_matches_the_two_predicates_it_replaced():
    """Every clause of ``_match`` / ``_match_narrow`` flipped on its own and in combination, every answer reached.
    The one intended difference: an empty ``heads`` list at width 256, which ``_match`` let through to a
    ``torch.cat([])`` that raised, is declined as it always was at 64 / 128."""
    families = {64: "narrow", 128: "narrow", 256: "wide"}
    for width, family in families.items():
        for d_in, heads in itertools.product((1, 16), ("one", "one_of_8", "two_sum_8")):
            trunk, hs = _tower(width, d_in, heads=heads)
            got = fused_mlp._family(trunk, hs)
            assert got is not None and got[0] == family and _same(got, _old_answer(trunk, hs))
            assert got[1] is trunk[0][0] and got[2] is trunk[0][2]
        for clause, change in _CLAUSE_FLIPS.items():  # each clause alone
            trunk, hs = _tower(width, **change)
            assert _old_answer(trunk, hs) is None and fused_mlp._family(trunk, hs) is None, (width, clause)
        trunk, hs = _tower(width, shape="three")  # (a longer trunk: only its first two elements are looked at)
        assert fused_mlp._family(trunk, hs)[0] == family and _same(fused_mlp._family(trunk, hs), _old_answer(trunk, hs))
    for width in (32, 512):
        trunk, hs = _tower(width)
        assert _old_answer(trunk, hs) is None and fused_mlp._family(trunk, hs) is None
    assert len(_CLAUSE_FLIPS) == 18  # (a thinned-out table fails here)

    seen, rows, empty_at_256 = set(), 0, []
    for width, d_in, l2, no_bias, heads, act1, act2, shape in itertools.product(
            (32, 64, 128, 256, 512), (1, 16, 17), ("ok", "in", "out"), (None, "l1", "l2", "head"), list(_HEADS),
            ("relu", "tanh"), ("relu", "tanh"), ("ok", "three", "one", "not_sequential")):
        trunk, hs = _tower(width, d_in, l2=l2, no_bias=no_bias, heads=heads, act1=act1, act2=act2, shape=shape)
        got, want = fused_mlp._family(trunk, hs), _old_answer(trunk, hs)
        rows += 1
        if not hs and want is not None:  # the rows that differ, by name: no heads at width 256
            assert want[0] == "wide" and width == 256 and got is None
            empty_at_256.append((d_in, act1, act2, shape))
            continue
        assert _same(got, want), (width, d_in, l2, no_bias, heads, act1, act2, shape)
        seen.add(None if got is None else got[0])
    assert seen == {None, "wide", "narrow"} and rows == 5 * 3 * 3 * 4 * 8 * 2 * 2 * 4
    # d_in 1 and 16, both activations right, the trunk of two or three elements, with or without the (absent) head's bias
    assert len(empty_at_256) == 2 * 2 * 2 and {r[0] for r in empty_at_256} == {1, 16}
