"""The binding's checks of a rollout timestep's tensors, without a GPU: every ``rollout_step_*`` wrapper and the two
scatter functions refuse a wrong dtype (TypeError), a wrong element count and a non-contiguous column (ValueError)
before the library is loaded or a pointer taken -- the tensors here live on the CPU, which ``_ptr`` would refuse."""

import pytest
import torch

from rl8_amd import hip
from rl8_amd.envs import CartPoleConfig, MountainCarConfig, PendulumConfig

N = 6


def f32(*shape):
    return torch.zeros(*shape)


def columns(action_dtype):
    return dict(action_col=torch.zeros(N, 1, dtype=action_dtype), logp_col=f32(N, 1), value_col=f32(N, 1),
                reward_col=f32(N, 1), rdr_t=f32(N, 1), rdr_t1=f32(N, 1))


TAIL = dict(gamma=0.95, seed=1, step=2, env_offset=3, deterministic=False)


def _dummy(**bad):
    kw = dict(discrete=True, squashed=False, features=f32(N, 1, 2), features2=None, value=f32(N, 1), noise=f32(N, 1, 2),
              state=f32(N, 1), obs_col_next=f32(N, 1), **columns(torch.int64), **TAIL)
    hip.rollout_step_dummy(**{**kw, **bad})


def _cartpole(**bad):
    kw = dict(logits=f32(N, 1, 3), value=f32(N, 1), noise=None, state=f32(4, N), cfg=CartPoleConfig().to_abi(),
              obs_col_next=f32(N, 5), **columns(torch.int64), **TAIL)
    hip.rollout_step_cartpole(**{**kw, **bad})


def _mountain_car(**bad):
    kw = dict(logits=f32(N, 1, 3), value=f32(N, 1), noise=None, state=f32(2, N), cfg=MountainCarConfig().to_abi(),
              obs_col_next=f32(N, 2), **columns(torch.int64), **TAIL)
    hip.rollout_step_mountain_car(**{**kw, **bad})


def _pendulum(**bad):
    kw = dict(squashed=True, mean=f32(N, 1), log_std=f32(N, 1), value=f32(N, 1), noise=f32(N, 1), state=f32(2, N),
              cfg=PendulumConfig().to_abi(), obs_col_next=f32(N, 3), **columns(torch.float32), **TAIL)
    hip.rollout_step_pendulum(**{**kw, **bad})


def _algotrading(**bad):
    obs = {key: torch.zeros(N, d, dtype=dtype) for key, dtype, d in hip.ALGOTRADING_LEAVES}
    kw = dict(logits=f32(N, 1, 3), value=f32(N, 1), noise=None, state=f32(9, N), obs_col_next=obs,
              **columns(torch.int64), **TAIL)
    hip.rollout_step_algotrading(**{**kw, **bad})


def _heads_narrow(**bad):
    kw = dict(h=f32(N, 64), w_pol=f32(2, 64), b_pol=f32(2), w_vf=f32(1, 64), b_vf=f32(1), noise=None, state=f32(N, 1),
              obs_col_next=f32(N, 1), **columns(torch.int64), **TAIL)
    hip.rollout_step_dummy_heads_narrow(**{**kw, **bad})


def _scatter(**bad):
    kw = dict(action=torch.zeros(N, 1, dtype=torch.int64), logp=f32(N, 1), value=f32(N, 1), reward=f32(N, 1),
              obs=f32(N, 3), obs_col_next=f32(N, 3), **columns(torch.int64), gamma=0.95)
    hip.rollout_scatter(**{**kw, **bad})


def _scatter_leaves(**bad):
    kw = dict(action=torch.zeros(N, 1, dtype=torch.int64), logp=f32(N, 1), value=f32(N, 1), reward=f32(N, 1),
              obs=[f32(N, 3), torch.zeros(N, 1, dtype=torch.bool)],
              obs_cols_next=[f32(N, 3), torch.zeros(N, 1, dtype=torch.bool)], **columns(torch.int64), gamma=0.95)
    hip.rollout_scatter_leaves(**{**kw, **bad})


CALLS = [_dummy, _cartpole, _mountain_car, _pendulum, _algotrading, _heads_narrow, _scatter, _scatter_leaves]
IDS = [call.__name__.lstrip("_") for call in CALLS]


@pytest.fixture(autouse=True)
def library_stays_unloaded(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the tensors were checked")

    monkeypatch.setattr(hip, "load", refuse)


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_a_wrong_dtype_is_a_type_error(call):
    with pytest.raises(TypeError):
        call(value_col=torch.zeros(N, 1, dtype=torch.float64))  # would be read as 2 N floats of garbage
    with pytest.raises(TypeError):
        call(rdr_t=torch.zeros(N, 1, dtype=torch.float16))
    if call not in (_scatter, _scatter_leaves):  # (those take the action's dtype from the sampled action)
        wrong = torch.int32 if call is not _pendulum else torch.int64
        with pytest.raises(TypeError):
            call(action_col=torch.zeros(N, 1, dtype=wrong))


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_a_wrong_element_count_is_a_value_error(call):
    with pytest.raises(ValueError):
        call(reward_col=f32(N + 1, 1))
    with pytest.raises(ValueError):
        call(rdr_t1=f32(N - 1, 1))
    with pytest.raises(ValueError):
        call(value_col=f32(N, 2))


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_a_column_that_is_not_contiguous_is_a_value_error(call):
    with pytest.raises(ValueError):
        call(logp_col=f32(N, 2)[:, :1])
    with pytest.raises(ValueError):
        call(rdr_t=f32(2 * N, 1)[::2])


def test_the_calls_above_pass_their_checks():
    """(so that each refusal above is the one changed tensor's: unchanged, every call gets as far as loading the
    library or taking the pointers, where the CPU tensors are turned away)"""
    for call in CALLS:
        with pytest.raises((hip.HipExtensionError, AssertionError), match="HIP device tensors only|library was loaded"):
            call()
