"""``views.window_plan``: which models get their observation views from the window kernels, and that the views the
plan lays out have the keys ``Model.apply_view_requirements`` gives; ``MLPTrader`` on CPU specs; the two entries in the
built library.  No GPU."""

from __future__ import annotations

import pytest
import torch

from rl8_amd import hip
from rl8_amd.data import DataKeys
from rl8_amd.envs import AlgoTrading, MLPTrader
from rl8_amd.models import Model
from rl8_amd.specs import Categorical, Composite, Unbounded
from rl8_amd.tensordict import TensorDict
from rl8_amd.views import MAX_WINDOW_FIELDS, ViewRequirement, WindowLeaf, window_plan

ACTIONS = Categorical(2, shape=torch.Size([1]))
LC, LCP = "LOG_CHANGE(price)", "LOG_CHANGE(price, position)"


def model_with(spec, requirements) -> Model:
    """A bare ``Model`` whose view requirements are ``requirements`` (``None``: the default identity view)."""
    model = Model(spec, ACTIONS)
    if requirements is not None:
        model.view_requirements = requirements
    return model


def dict_spec(**extra) -> Composite:
    return Composite({"x": Unbounded(2), "count": Unbounded(1, dtype=torch.int64),
                      "flags": Categorical(2, shape=torch.Size([3]), dtype=torch.bool), **extra})


def key_structure(item):
    """``None`` for a tensor, a dict of the same for a tensordict."""
    if torch.is_tensor(item):
        return None
    return {k: key_structure(v) for k, v in item.items()}


def buffer_for(spec, b: int = 3, t: int = 6) -> TensorDict:
    def leaf(s):
        return torch.zeros(b, t, *s.shape, dtype=s.dtype)

    obs = TensorDict({k: leaf(spec[k]) for k in spec.keys()}, batch_size=[b, t]) if isinstance(spec, Composite) else leaf(spec)
    return TensorDict({DataKeys.OBS: obs}, batch_size=[b, t])


WINDOW = {DataKeys.INPUTS: None, DataKeys.PADDING_MASK: None}


def test_identity_views_plan_every_leaf_at_size_one():
    plan = window_plan(model_with(Unbounded(4), None), Unbounded(4))
    assert plan.leaves == (WindowLeaf(None, 1),) and plan.layout() == {DataKeys.OBS: None}
    spec = dict_spec()
    plan = window_plan(model_with(spec, None), spec)
    assert plan.leaves == tuple(WindowLeaf(name, 1) for name in ("x", "count", "flags"))
    assert plan.sizes == [1, 1, 1]


def test_tensor_obs_with_a_padded_shift():
    spec = Unbounded(4)
    plan = window_plan(model_with(spec, {DataKeys.OBS: ViewRequirement(shift=3)}), spec)
    assert plan.leaves == (WindowLeaf(None, 4),) and plan.layout() == {DataKeys.OBS: WINDOW}
    for dtype in (torch.int64, torch.bool):
        assert window_plan(model_with(spec, {DataKeys.OBS: ViewRequirement(shift=1)}), Unbounded(2, dtype=dtype)) is not None


def test_tuple_key_leaf_overwrites_the_leaf_inside_obs():
    spec = dict_spec()
    model = model_with(spec, None)
    model.view_requirements[(DataKeys.OBS, "x")] = ViewRequirement(shift=3)
    plan = window_plan(model, spec)
    assert plan.leaves == (WindowLeaf("x", 4), WindowLeaf("count", 1), WindowLeaf("flags", 1))
    assert plan.layout() == {DataKeys.OBS: {"x": WINDOW, "count": None, "flags": None}}
    # in the order of the requirements: "obs" after the tuple key takes the whole of "obs" back
    plan = window_plan(model_with(spec, {(DataKeys.OBS, "x"): ViewRequirement(shift=3),
                                         DataKeys.OBS: ViewRequirement(shift=0)}), spec)
    assert plan.sizes == [1, 1, 1]
    # a tuple key alone: the views hold that leaf only; "obs" with a shift windows every leaf
    plan = window_plan(model_with(spec, {(DataKeys.OBS, "flags"): ViewRequirement(shift=2)}), spec)
    assert plan.leaves == (WindowLeaf("flags", 3),)
    plan = window_plan(model_with(spec, {DataKeys.OBS: ViewRequirement(shift=2)}), spec)
    assert plan.sizes == [3, 3, 3]


def test_what_stays_on_the_torch_route():
    spec = dict_spec()
    tensor = Unbounded(4)
    rolling = ViewRequirement(shift=2, method="rolling_window")
    assert window_plan(model_with(tensor, {DataKeys.OBS: rolling}), tensor) is None
    assert window_plan(model_with(spec, {DataKeys.OBS: ViewRequirement(), (DataKeys.OBS, "x"): rolling}), spec) is None
    # (rolling_window without a shift is the identity: nothing is dropped)
    assert window_plan(model_with(tensor, {DataKeys.OBS: ViewRequirement(shift=0, method="rolling_window")}), tensor) is not None
    # keys outside obs, leaves that are not there, a tuple key on a tensor observation
    assert window_plan(model_with(tensor, {DataKeys.OBS: ViewRequirement(), DataKeys.ACTIONS: ViewRequirement(shift=1)}),
                       tensor) is None
    assert window_plan(model_with(spec, {(DataKeys.OBS, "missing"): ViewRequirement(shift=1)}), spec) is None
    assert window_plan(model_with(spec, {(DataKeys.OBS, "x", "y"): ViewRequirement(shift=1)}), spec) is None
    assert window_plan(model_with(tensor, {(DataKeys.OBS, "x"): ViewRequirement(shift=1)}), tensor) is None
    # nested specs, other dtypes
    nested = Composite({"outer": Composite({"x": Unbounded(2)})})
    assert window_plan(model_with(nested, None), nested) is None
    half = Unbounded(2, dtype=torch.float16)
    assert window_plan(model_with(half, {DataKeys.OBS: ViewRequirement(shift=1)}), half) is None
    # models without view requirements (the recurrent ones)
    assert window_plan(object(), tensor) is None


def test_nine_fields_stay_on_the_torch_route():
    assert MAX_WINDOW_FIELDS == hip.MAX_GATHER_FIELDS == 8
    eight = Composite({f"leaf{i}": Unbounded(1) for i in range(8)})
    nine = Composite({f"leaf{i}": Unbounded(1) for i in range(9)})
    requirement = {DataKeys.OBS: ViewRequirement(), (DataKeys.OBS, "leaf0"): ViewRequirement(shift=2)}
    assert len(window_plan(model_with(eight, dict(requirement)), eight).leaves) == 8
    assert window_plan(model_with(nine, dict(requirement)), nine) is None
    # (nine leaves in the spec, one read by the model: one field)
    assert window_plan(model_with(nine, {(DataKeys.OBS, "leaf0"): ViewRequirement(shift=2)}), nine).sizes == [3]


def test_the_env_switch_is_read_per_call(monkeypatch):
    spec = Unbounded(4)
    model = model_with(spec, {DataKeys.OBS: ViewRequirement(shift=3)})
    assert window_plan(model, spec) is not None
    monkeypatch.setenv("RL8_AMD_WINDOW_KERNELS", "0")
    assert window_plan(model, spec) is None
    monkeypatch.setenv("RL8_AMD_WINDOW_KERNELS", "1")
    assert window_plan(model, spec) is not None


@pytest.mark.parametrize("kind", ["last", "all"])
def test_plan_layout_is_the_key_structure_of_apply_view_requirements(kind):
    spec = dict_spec()
    tensor = Unbounded(4)
    cases = [
        (tensor, None),
        (tensor, {DataKeys.OBS: ViewRequirement(shift=3)}),
        (spec, None),
        (spec, {DataKeys.OBS: ViewRequirement(), (DataKeys.OBS, "x"): ViewRequirement(shift=3)}),
        (spec, {DataKeys.OBS: ViewRequirement(), (DataKeys.OBS, "x"): ViewRequirement(shift=7),
                (DataKeys.OBS, "flags"): ViewRequirement(shift=1)}),
        (spec, {(DataKeys.OBS, "x"): ViewRequirement(shift=3), DataKeys.OBS: ViewRequirement()}),
        (spec, {(DataKeys.OBS, "count"): ViewRequirement(shift=2)}),
        (spec, {DataKeys.OBS: ViewRequirement(shift=2)}),
    ]
    for obs_spec, requirements in cases:
        model = model_with(obs_spec, requirements)
        views = model.apply_view_requirements(buffer_for(obs_spec), kind=kind)
        plan = window_plan(model, obs_spec)
        assert plan.layout() == key_structure(views), requirements
        # and the views the plan builds from a launch's outputs: the same keys, shapes and dtypes
        rows = views.batch_size[0]
        outs = []
        for leaf in plan.leaves:
            s = obs_spec if leaf.name is None else obs_spec[leaf.name]
            if leaf.size == 1:
                outs.append((torch.zeros(rows, *s.shape, dtype=s.dtype), None))
            else:
                outs.append((torch.zeros(rows, leaf.size, *s.shape, dtype=s.dtype), torch.zeros(rows, leaf.size, dtype=torch.bool)))
        built = plan.views(outs)
        assert key_structure(built) == key_structure(views) and built.batch_size == views.batch_size

        def compare(a, b, path):
            if torch.is_tensor(a):
                assert a.shape == b.shape and a.dtype == b.dtype, (requirements, path)
                return
            for k in a.keys():
                compare(a[k], b[k], path + (k,))

        compare(views, built, ())


def test_mlp_trader_builds_on_cpu_specs_with_the_documented_parameters():
    env = AlgoTrading(4, device="cpu")
    model = MLPTrader(env.observation_spec, env.action_spec)
    assert model.seq_len == 4 and model.view_requirements[(DataKeys.OBS, LC)].shift == 4
    assert model.view_requirements[DataKeys.OBS].is_identity
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {"invested_embedding.weight": (2, 2)}
    for tower, outputs in (("feature_model", 3), ("vf_model", 1)):
        want.update({
            f"{tower}.0.0.weight": (128, 7), f"{tower}.0.0.bias": (128,),
            f"{tower}.0.1.weight": (128,), f"{tower}.0.1.bias": (128,), f"{tower}.0.1.running_mean": (128,),
            f"{tower}.0.1.running_var": (128,), f"{tower}.0.1.num_batches_tracked": (),
            f"{tower}.0.3.weight": (128, 128), f"{tower}.0.3.bias": (128,),
            f"{tower}.2.weight": (outputs, 128), f"{tower}.2.bias": (outputs,),
        })
    assert shapes == want
    head = model.feature_model[2]
    assert float(head.weight.detach().abs().max()) <= 1e-3 and not head.bias.any()
    plan = window_plan(model, env.observation_spec)
    assert plan.leaves == (WindowLeaf("action_mask", 1), WindowLeaf("invested", 1), WindowLeaf(LC, 5), WindowLeaf(LCP, 1))

    wide = MLPTrader(env.observation_spec, env.action_spec, invested_embed_dim=3, seq_len=8, hiddens=(32, 16, 8))
    assert wide.view_requirements[(DataKeys.OBS, LC)].shift == 8
    assert tuple(wide.feature_model[0][0].weight.shape) == (32, 8) and tuple(wide.vf_model[2].weight.shape) == (1, 8)
    with pytest.raises(AssertionError, match="factor of 4"):
        MLPTrader(env.observation_spec, env.action_spec, seq_len=6)

    # a forward pass on the views of a CPU buffer: masked logits and a value per sample
    b, t = 3, 7
    obs = buffer_for(env.observation_spec, b, t)
    obs[DataKeys.OBS]["action_mask"][..., 0] = True
    obs[DataKeys.OBS][LC].normal_()
    model.eval()
    out = model(model.apply_view_requirements(obs, kind="all"))
    assert out["logits"].shape == (b * t, 1, 3) and model.value_function().shape == (b * t, 1)
    finfo = torch.finfo(torch.float32)
    assert bool((out["logits"][:, 0, 1:] <= finfo.min / 2).all()) and bool(torch.isfinite(out["logits"]).all())


def test_both_symbols_are_exported_by_the_built_library():
    lib = hip.load()
    for name in ("rl8_gather_windows", "rl8_window_last"):
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert lib.rl8_gather_windows(None, 1, 1, None, 1, None) == -1
    assert lib.rl8_window_last(0, 1, None, 1, None) == -1
