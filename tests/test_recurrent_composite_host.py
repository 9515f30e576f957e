"""Without a GPU: the two entries behind the recurrent algorithm's dict observations (``rl8_gather_sequences``,
``rl8_lstm_narrow_input_grad_f32``) are declared, exported, bound and refuse bad arguments before any launch; the
input-gradient kernel compiles for gfx950 within the resources its launch bounds promise; and the leaf rules of
``RecurrentAlgorithm``."""

from __future__ import annotations

import os
import re
import shutil
import subprocess
import types
from typing import Any

import pytest
import torch

from rl8_amd import RecurrentAlgorithmConfig, hip
from rl8_amd.algorithms._recurrent import RecurrentAlgorithm, _LeanRollout
from rl8_amd.data import DataKeys
from rl8_amd.env import Env
from rl8_amd.specs import Categorical, Composite, Unbounded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_gather_sequences", "rl8_lstm_narrow_input_grad_f32")
FAKE = 4096  # (never dereferenced: every call below fails its checks first)


def test_entries_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        header = f.read()
    lib = hip.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        params = re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1))
        assert len(params.split(",")) == len(hip.SIGNATURES[name]), name
    assert hip.abi_version()[0] == hip.ABI_VERSION == 107  # (compatible additions: no bump)


def test_input_grad_refuses_bad_arguments_before_launching():
    fn = hip.load().rl8_lstm_narrow_input_grad_f32

    def call(ws=FAKE, b=10, l=2, d_in=4, w_ih=FAKE, hidden=64, dx=FAKE):
        return fn(ws, b, l, d_in, w_ih, hidden, dx, None)

    for missing in ("ws", "w_ih", "dx"):
        assert call(**{missing: None}) == -1, missing
    for kw in ({"b": 0}, {"l": 0}, {"d_in": 0}, {"d_in": 17}, {"hidden": 96}, {"hidden": 256}, {"l": 1 << 20}):
        assert call(**kw) == -2, kw
    assert call(ws=FAKE + 4) == -3 and call(w_ih=FAKE + 2) == -3 and call(dx=FAKE + 1) == -3


def test_gather_sequences_refuses_bad_arguments_before_launching():
    fn = hip.load().rl8_gather_sequences

    def fields(*rows):
        arr = (hip.GatherField * len(rows))()
        for i, row in enumerate(rows):
            arr[i] = hip.GatherField(*row)
        return arr

    one = fields((FAKE, FAKE, 1, 8, 3, 1))

    def call(index=FAKE, seqs=4, seq_len=2, h=8, f=one, n=1):
        return fn(index, seqs, seq_len, h, f, n, None)

    assert call(f=None) == -1
    assert call(f=fields((None, FAKE, 1, 8, 3, 1))) == -1 and call(f=fields((FAKE, None, 1, 8, 3, 1))) == -1
    for kw in ({"seqs": 0}, {"seq_len": 0}, {"h": 0}, {"h": 7}, {"n": 0}, {"n": hip.MAX_GATHER_FIELDS + 1}):
        assert call(**kw) == -2, kw
    assert call(f=fields((FAKE, FAKE, 1, 8, 0, 4))) == -2
    for width in (2, 3, 16, 0):
        assert call(f=fields((FAKE, FAKE, 1, 8, 1, width))) == -4, width
    assert call(f=fields((FAKE + 2, FAKE, 1, 8, 1, 4))) == -3 and call(f=fields((FAKE, FAKE + 4, 1, 8, 1, 8))) == -3
    # (byte-wide leaves need no alignment; a second, bad field stops the call before the launch)
    assert call(f=fields((FAKE + 3, FAKE + 1, 1, 8, 3, 1), (FAKE, FAKE, 1, 8, 1, 2)), n=2) == -4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_input_grad_kernels_compile_within_their_launch_bounds(tmp_path):
    """Every instantiation (H = 64 / 128 x KIN = 4 / 16) present, no scratch, and LDS and VGPRs within what
    ``Geo<H>::kWgPerCU`` workgroups of H / 16 waves per CU leave each (160 KiB of LDS, 512 VGPRs per SIMD lane)."""
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "lstm_narrow.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "lstm_narrow_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    mine = {name: body for name, body in kernels.items() if "lstm_narrow_input_grad_kernel" in name}
    assert len(mine) == 4, sorted(mine)
    wg_per_cu = {64: 2, 128: 1}
    for hidden in (64, 128):
        for kin in (4, 16):
            (name, body), = [(n, b) for n, b in mine.items() if f"ILi{hidden}ELi{kin}EE" in n]

            def field(key: str) -> int:
                return int(re.search(rf"\.amdhsa_{key} (\d+)", body).group(1))

            assert field("private_segment_fixed_size") == 0, name
            assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
            assert "enable_private_segment 1" not in body, name
            waves_per_simd = (hidden // 16) * wg_per_cu[hidden] // 4
            assert field("group_segment_fixed_size") == (hidden // 16) * 32 * (kin + 4) * 4, name
            assert field("group_segment_fixed_size") * wg_per_cu[hidden] <= 160 * 1024, name
            assert field("next_free_vgpr") <= 512 // waves_per_simd, (name, field("next_free_vgpr"))


# --------------------------------------------------------------------------- #
# Leaf rules (no device: the rules run before anything is built on the specs).
# --------------------------------------------------------------------------- #
class DictEnv(Env):
    def __init__(self, num_envs: int, /, horizon: None | int = None, *, device: Any = "cpu") -> None:
        super().__init__(num_envs, horizon, device=device)
        self.observation_spec = Composite({
            "x": Unbounded(2, device=device),
            "flags": Categorical(2, shape=torch.Size([3]), device=device, dtype=torch.bool),
        })
        self.action_spec = Categorical(2, shape=torch.Size([1]), device=device)

    def reset(self, *, config=None):
        raise NotImplementedError

    def step(self, action):
        raise NotImplementedError


def _leaves(config: RecurrentAlgorithmConfig, observation_spec=None, action_spec=None):
    """``RecurrentAlgorithm``'s leaf rules for ``config`` on a ``DictEnv`` with the given specs: what ``build()``
    runs first, on an algorithm that has nothing but its env and its config yet."""
    algo = object.__new__(RecurrentAlgorithm)
    algo.env = DictEnv(4, 4)
    if observation_spec is not None:
        algo.env.observation_spec = observation_spec
    if action_spec is not None:
        algo.env.action_spec = action_spec
    algo._recurrent_config = config
    return algo._composite_obs_leaves()


def _model_cls(*args, **kwargs):
    raise AssertionError("the rules run before any model is made")


def test_leaf_rules_of_the_recurrent_algorithm():
    assert RecurrentAlgorithm.composite_observations is True
    with_model = RecurrentAlgorithmConfig(num_envs=4, horizon=4, model_cls=_model_cls)
    assert _leaves(with_model) == ["x", "flags"]
    assert _leaves(with_model, observation_spec=Unbounded(3)) is None
    assert _leaves(RecurrentAlgorithmConfig(num_envs=4, horizon=4), observation_spec=Unbounded(3)) is None
    outside = "composite specs are outside the accelerated path"
    # no model: there is no default recurrent model for a dict
    with pytest.raises(NotImplementedError, match=outside):
        _leaves(RecurrentAlgorithmConfig(num_envs=4, horizon=4))
    with pytest.raises(NotImplementedError, match=outside):  # nested
        _leaves(with_model, observation_spec=Composite({"outer": Composite({"x": Unbounded(2)})}))
    with pytest.raises(NotImplementedError, match=outside):  # composite actions
        _leaves(with_model, action_spec=Composite({"a": Categorical(2, shape=torch.Size([1]))}))
    with pytest.raises(NotImplementedError, match=outside):
        _leaves(with_model, observation_spec=Unbounded(3), action_spec=Composite({"a": Categorical(2, shape=torch.Size([1]))}))
    with pytest.raises(NotImplementedError, match=outside):  # a leaf dtype the buffer does not hold
        _leaves(with_model, observation_spec=Composite({"x": Unbounded(2, dtype=torch.float64)}))
    nine = Composite({f"leaf{i}": Unbounded(1) for i in range(hip.MAX_GATHER_FIELDS + 1)})
    with pytest.raises(NotImplementedError, match="at most 8 leaves"):
        _leaves(with_model, observation_spec=nine)
    assert len(_leaves(with_model, observation_spec=Composite({f"leaf{i}": Unbounded(1) for i in range(8)}))) == 8


def test_lean_rollout_is_not_available_for_dict_observations():
    """The lean launches read one float32 observation slab; a dict-observation algorithm holds its leaves in
    ``_tm_obs`` and has no ``_tm["obs"]``, whatever its model and env."""
    from rl8_amd import models_recurrent
    from rl8_amd.distributions import Categorical as CategoricalDistribution
    from rl8_amd.env import DiscreteDummyEnv

    ns = types.SimpleNamespace
    model = models_recurrent.DefaultDiscreteRecurrentModel(
        Unbounded(shape=torch.Size([1]), device="cpu"), Categorical(2, shape=torch.Size([1]), device="cpu"), hidden_size=64)
    tm = {k: torch.zeros(5, 4, 1) for k in (DataKeys.ACTIONS, DataKeys.LOGP, DataKeys.VALUES, DataKeys.REWARDS)}
    algo = ns(policy=ns(model=model, distribution_cls=CategoricalDistribution), _tm=tm,
              _tm_obs={"x": torch.zeros(5, 4, 1)}, env=object.__new__(DiscreteDummyEnv))
    assert _LeanRollout.available(algo) is False


def test_the_envs_package_exports_the_trader():
    from rl8_amd import envs
    from rl8_amd.envs.algotrading_models import LSTMTrader
    from rl8_amd.models_recurrent import RecurrentModel

    assert envs.LSTMTrader is LSTMTrader and "LSTMTrader" in envs.__all__ and issubclass(LSTMTrader, RecurrentModel)
    model = LSTMTrader(envs.AlgoTrading(2).observation_spec, envs.AlgoTrading(2).action_spec)
    assert (model.lstm.input_size, model.lstm.hidden_size, model.lstm.num_layers) == (4, 64, 1)
    assert tuple(model.invested_embedding.weight.shape) == (2, 2)
    assert list(model.state_spec.keys()) == [DataKeys.HIDDEN_STATES, DataKeys.CELL_STATES]
    assert float(model.feature_head.weight.detach().abs().max()) <= 1e-3 and model.vf_head.out_features == 1
