"""The rollout record's decisions (``fused_mlp.RolloutRecord``: what is recorded, what may be replayed) on the CPU:
the forward launch, the weight pack and the strided gather are stubbed, the tensors are host tensors, and no device
runtime is started.  ``tests/test_rollout_reuse_gpu.py`` checks the same policy end to end on the device."""

from __future__ import annotations

import dataclasses

import pytest
import torch

from rl8_amd import hip
from rl8_amd.nn import fused_mlp

H, N, D_IN = 4, 8, 3


def _plan(*, rank_one: bool = True, recordable: bool = True) -> fused_mlp._TowerPlan:
    return fused_mlp._TowerPlan(forward_planes=True, backward_planes=recordable, wgrad_planes=True, gates=True,
                                rank_one=rank_one)


class Tower:
    def __init__(self, n_out: int = 1) -> None:
        self.l1, self.l2 = torch.nn.Linear(D_IN, 256), torch.nn.Linear(256, 256)
        self.heads = [torch.nn.Linear(256, n_out)]
        self.w3, self.b3 = self.heads[0].weight, self.heads[0].bias

    def record(self, rec: fused_mlp.RolloutRecord, x: torch.Tensor, plan=None):
        return rec.record(self.l1, self.l2, self.heads, self.w3, self.b3, plan or _plan(), x)

    def bump(self) -> None:
        with torch.no_grad():
            self.l1.weight.mul_(1.0)  # values unchanged, version counter bumped


@pytest.fixture
def launches(monkeypatch):
    """Every forward the record launches, as the keyword arguments it was given; the stub returns the ``out`` slab."""
    calls = []

    def forward_split(x, w1, b1, w2_split, b2, w3, b3, **kw):
        assert w2_split == "pack"
        calls.append(kw)
        kw["out"].fill_(float(len(calls)))
        return kw["out"], None, kw["h2_out"], kw["gate_out"]

    def gather(index, h, leaves):  # leaves are [N, H, ...] views, sample ids env * H + t
        return [leaf.reshape(leaf.shape[0] * h, *leaf.shape[2:])[index] for leaf in leaves]

    def no_device(*a, **k):
        raise AssertionError("the record asked the device runtime for something")

    monkeypatch.setattr(hip, "mlp_tower_forward_split", forward_split)
    monkeypatch.setattr(hip, "gather_minibatch", gather)
    monkeypatch.setattr(fused_mlp, "_packed", lambda layer, transposed, planes: "pack")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(fused_mlp, "replay_stats", dict.fromkeys(fused_mlp.replay_stats, 0))
    yield calls
    assert not torch.cuda.is_initialized()


def _rollout(rec, tower, obs, *, plan=None, twice_at=None, bump_at=None):
    rec.begin()
    outs = []
    for t in range(H):
        if t == bump_at:
            tower.bump()
        with rec.at(t) as inside:
            assert inside is rec and fused_mlp._RECORDING is rec
            outs.append(tower.record(rec, obs[t], plan))
            if t == twice_at:
                outs.append(tower.record(rec, obs[t] + 1.0, plan))
        assert fused_mlp._RECORDING is None
    return outs


def test_every_timestep_once_is_a_valid_record_and_rows_for_hands_it_out(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    outs = _rollout(rec, tower, obs)
    (tr,) = rec.towers.values()
    assert list(rec.towers) == [id(tower.l2)] and tr.h2 is None and not tr.spoiled and not rec.refused
    for t, (out, kw) in enumerate(zip(outs, launches)):
        assert out.data_ptr() == tr.out[t * N:].data_ptr() and out.shape == (N, 1)
        assert kw["gate_out"].data_ptr() == tr.gate[t * N:].data_ptr() and kw["gate_out"].shape == (N, 8)
        assert kw["h2_out"] is None and kw["timer_name"] == "mlp_tower_forward_record"
        assert (kw["save"], kw["save_h1"], kw["save_gate"], kw["save_h2"]) == (True, False, True, False)
    assert len(launches) == H and fused_mlp.replay_stats["recorded_rows"] == H * N
    assert rec.valid()
    assert rec.rows_for(obs, slice(0, H * N)) is None  # not sealed: the rollout has not ended
    rec.seal(obs)
    rows = rec.rows_for(obs, slice(0, H * N))
    assert list(rows) == [id(tower.l2)]
    got = rows[id(tower.l2)]
    assert got.key == tr.current_key() and got.h2 is None
    assert got.out.data_ptr() == tr.out.data_ptr() and got.out.shape == (H * N, 1) and got.gate.shape == (H * N, 8)
    # sample ids env * H + t against the [H][N] slabs
    index = torch.tensor([0 * H + 1, 5 * H + 3, 7 * H + 0])
    gathered = rec.rows_for(obs, index)[id(tower.l2)]
    assert gathered.key == got.key and gathered.h2 is None
    assert torch.equal(gathered.out, tr.out[[1 * N + 0, 3 * N + 5, 0 * N + 7]])
    # the replay check: the very tensor the context was made for, and the recorded parameters
    x = obs[:H].reshape(H * N, D_IN)
    args = (tower.l1, tower.l2, tower.heads)
    ctx = fused_mlp.replay(rows, x)
    assert ctx.hit(*args, x, 1, _plan()) is got
    assert ctx.hit(*args, x.clone(), 1, _plan()) is None and ctx.hit(*args, x[:N], 1, _plan()) is None
    assert ctx.hit(*args, x, 2, _plan()) is None
    assert ctx.hit(*args, x, 1, _plan(rank_one=False)) is None  # a record without h2 serves only gate-only plans
    assert ctx.hit(tower.l1, torch.nn.Linear(256, 256), tower.heads, x, 1, _plan()) is None
    tower.bump()
    assert ctx.hit(*args, x, 1, _plan()) is None
    assert not rec.valid() and rec.rows_for(obs, slice(0, H * N)) is None


def test_recorded_rows_slice():
    out, gate, h2 = torch.arange(10.0).view(10, 1), torch.arange(80, dtype=torch.int32).view(10, 8), torch.randn(10, 256)
    for with_h2 in (h2, None):
        rows = fused_mlp._RecordedRows(("key",), out, gate, with_h2)
        part = rows.slice(3, 7)
        assert part.key == ("key",) and torch.equal(part.out, out[3:7]) and torch.equal(part.gate, gate[3:7])
        assert part.out.data_ptr() == out[3:].data_ptr() and part.gate.data_ptr() == gate[3:].data_ptr()  # views
        if with_h2 is None:
            assert part.h2 is None
        else:
            assert part.h2.data_ptr() == h2[3:].data_ptr() and part.h2.shape == (4, 256)
    with pytest.raises(dataclasses.FrozenInstanceError):
        rows.key = ()


def test_a_second_evaluation_at_one_timestep_spoils_the_tower(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    outs = _rollout(rec, tower, obs, twice_at=2)
    assert outs[3] is None and all(o is not None for o in outs[:3] + outs[4:])
    assert len(launches) == H  # the second evaluation launched nothing here: the caller runs the tower normally
    (tr,) = rec.towers.values()
    assert tr.spoiled and not rec.valid()
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N)) is None and rec.rows(0, H * N) == {}
    _rollout(rec, tower, obs)  # the next rollout starts clean
    assert not tr.spoiled and rec.valid()


def test_parameters_changed_half_way_or_a_new_rollout_invalidate(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    outs = _rollout(rec, tower, obs, bump_at=2)
    assert all(o is not None for o in outs)  # recorded, under the new key, from t = 2 on
    (tr,) = rec.towers.values()
    assert tr.seen == {2, 3} and set(tr.inputs) == {2, 3} and not rec.valid()
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N)) is None
    _rollout(rec, tower, obs)
    rec.seal(obs)
    assert rec.valid() and rec.rows_for(obs, slice(0, H * N))
    rec.begin()
    assert not rec.valid() and tr.key is None and not tr.seen and not tr.inputs
    assert rec.rows_for(obs, slice(0, H * N)) is None


def test_other_row_counts_and_unrecordable_plans_are_not_recorded(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    rec.begin()
    with rec.at(0):
        assert tower.record(rec, obs[0, :N - 1]) is None
        assert tower.record(rec, torch.randn(2 * N, D_IN)) is None
        assert tower.record(rec, obs[0], _plan(recordable=False)) is None
    assert not launches and not rec.towers and not rec.refused


def test_inputs_that_are_not_the_callers_rows_are_never_replayed(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    _rollout(rec, tower, obs)
    rec.require_inputs(obs.data_ptr(), N * D_IN * 4)
    assert rec.valid()
    rec.require_inputs(obs.data_ptr() + 16, N * D_IN * 4)
    assert not rec.valid()
    # through rows_for: a tower recorded on a copy of the observations
    _rollout(rec, tower, obs.clone())
    rec.seal(obs)
    assert rec.valid() and rec.rows_for(obs, slice(0, H * N)) is None and not rec.valid()


def test_a_write_to_the_observations_or_an_unsealed_record_is_not_replayed(launches):
    rec, tower, obs = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(), torch.randn(H + 1, N, D_IN)
    _rollout(rec, tower, obs)
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N))
    obs[1, 3] += 1.0  # an in-place write after the rollout ended
    assert rec.valid() and rec.rows_for(obs, slice(0, H * N)) is None
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N))
    # a later rollout that records nothing (not fused, or reuse switched off): the towers stand, the record does not
    rec.unseal()
    assert rec.valid() and rec.rows_for(obs, slice(0, H * N)) is None
    assert rec.rows_for(obs, torch.tensor([0, 1])) is None
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N))
    rec.begin()  # a later rollout that records
    assert rec.rows_for(obs, slice(0, H * N)) is None


def test_a_general_head_over_the_byte_budget_is_refused(launches, monkeypatch):
    obs = torch.randn(H + 1, N, D_IN)
    general = _plan(rank_one=False)
    assert general.recordable and not general.gate_only
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device: (1 << 40, 1 << 40))
    need = H * N * (256 * 4 + 32 + 4 * 2)

    rec, tower = fused_mlp.RolloutRecord(H, N, keep_general=True), Tower(2)
    monkeypatch.setattr(fused_mlp, "RECORD_H2_BUDGET_BYTES", need - 1)
    assert all(o is None for o in _rollout(rec, tower, obs, plan=general))
    assert rec.refused == {id(tower.l2)} and not rec.towers and not launches and not rec.valid()

    monkeypatch.setattr(fused_mlp, "RECORD_H2_BUDGET_BYTES", need)
    assert all(o is None for o in _rollout(rec, tower, obs, plan=general))  # once refused, not asked again
    rec, tower = fused_mlp.RolloutRecord(H, N, keep_general=True), Tower(2)
    assert all(o is not None for o in _rollout(rec, tower, obs, plan=general))
    (tr,) = rec.towers.values()
    assert tr.h2.shape == (H * N, 256) and launches[-1]["h2_out"].data_ptr() == tr.h2[(H - 1) * N:].data_ptr()
    assert launches[-1]["save_h2"] is True
    rec.seal(obs)
    assert rec.rows_for(obs, slice(0, H * N))[id(tower.l2)].h2.data_ptr() == tr.h2.data_ptr()
    # a second general tower would take the held slabs over the budget; a third of free memory; keep_general off
    other = Tower(2)
    assert all(o is None for o in _rollout(rec, other, obs, plan=general)) and id(other.l2) in rec.refused
    monkeypatch.setattr(fused_mlp, "RECORD_H2_BUDGET_BYTES", 1 << 40)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device: (3 * need - 1, 1 << 40))
    rec, tower = fused_mlp.RolloutRecord(H, N, keep_general=True), Tower(2)
    assert all(o is None for o in _rollout(rec, tower, obs, plan=general)) and rec.refused
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device: (1 << 40, 1 << 40))
    rec, tower = fused_mlp.RolloutRecord(H, N, keep_general=False), Tower(2)
    assert all(o is None for o in _rollout(rec, tower, obs, plan=general)) and rec.refused
