"""The towers' route table (``fused_mlp._plan``) on the CPU: the support predicates are stubbed with the envelopes
``include/rl8_amd.h`` documents, and every plan is checked against the rules each call site applied before the
decision was made in one place."""

from __future__ import annotations

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
