"""Records what every fused rollout-timestep entry writes, so that a later change to those kernels can be held to
"unchanged, bit for bit" (tests/test_rollout_step_parity_gpu.py replays the cases and compares with np.array_equal).

``rollout_step_parity.npz`` was produced by this script on an MI355X at commit 6103783 ("Add the rl8.nn surface, masked
sequence kernels and TransformerTrader"), the parent of the change that gave the rollout timestep one owner.  Regenerate
it only from a commit whose kernels are known good:

    python tests/golden/generate_rollout_step_fixtures.py [output.npz]

It uses only the public ``hip.rollout_step_*`` wrappers and, for ``rl8_rollout_step_dummy_heads_f32`` (which has no
wrapper), a direct call through ``hip.load()``.  No input is stored: all are closed-form integer arithmetic
(:func:`wave`), shared with the test through this module.  Every categorical entry has a row whose logits tie.

Cases: the eleven entry variants x n in {1, 65, 321} x noise {Philox, injected, deterministic} x rdr {present, absent},
with nonzero seed, step and env_offset.  The grid-stride branch (more than 2048 blocks) is tests/test_full_size_gpu.py's.
"""

from __future__ import annotations

import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rollout_step_parity.npz")

ENTRIES = ("dummy_discrete", "dummy_normal", "dummy_squashed", "dummy_heads_256", "dummy_heads_narrow_64",
           "dummy_heads_narrow_128", "cartpole", "mountain_car", "pendulum_normal", "pendulum_squashed", "algotrading")
SIZES = (1, 65, 321)  # a lone lane; one wave plus one; a 256-lane block plus a ragged one (heads: five blocks plus one env)
MODES = ("philox", "injected", "deterministic")
SEED, STEP, ENV_OFFSET, GAMMA = 1234, 7, 5, float(np.float32(0.95))
SENTINEL = 7  # what every output buffer holds before the launch: an element the kernel skips shows up

CASES = tuple(itertools.product(ENTRIES, SIZES, MODES, (True, False)))


def case_id(entry: str, n: int, mode: str, rdr: bool) -> str:
    return f"{entry}/n{n}/{mode}/{'rdr' if rdr else 'nordr'}"


def wave(shape, salt: int) -> np.ndarray:
    """float32 values in [-2, 2] on a grid of 1/500, a fixed function of the element's index and ``salt``."""
    count = int(np.prod(shape))
    i = np.arange(count, dtype=np.int64) + 7919 * salt
    return (((i * 2654435761) % 2001 - 1000).astype(np.float32) / np.float32(500)).reshape(shape)


def exponentials(shape, salt: int) -> np.ndarray:
    """Stand-ins for Exp(1) draws: positive, in [0.01, 4.01]."""
    return wave(shape, salt) + np.float32(2.01)


def tie_row(n: int) -> int:
    return n // 2


def inputs(entry: str, n: int) -> dict[str, np.ndarray]:
    """Host arrays of one entry at ``n`` envs (noise included; the mode decides whether it is passed)."""
    x: dict[str, np.ndarray] = {"value": wave((n, 1), 3), "rdr_t": wave((n, 1), 5)}
    k = tie_row(n)
    if entry.startswith("dummy"):
        x["state"] = wave((n, 1), 4) * np.float32(50)
    if entry == "dummy_discrete":
        x["features"] = wave((n, 1, 2), 1)
        x["features"][k] = 0.5
        x["noise"] = exponentials((n, 1, 2), 2)
    elif entry in ("dummy_normal", "dummy_squashed", "pendulum_normal", "pendulum_squashed"):
        x["mean"] = wave((n, 1), 1)
        x["log_std"] = wave((n, 1), 6) / np.float32(2)
        x["noise"] = wave((n, 1), 2)
    elif entry.startswith("dummy_heads"):
        hidden = int(entry.rsplit("_", 1)[1])
        x["h"] = wave((n, hidden), 1) / np.float32(2)
        x["h"][k] = 0.0  # with equal policy biases: a tie
        x["w_pol"], x["b_pol"] = wave((2, hidden), 7) / np.float32(16), np.full(2, 0.25, np.float32)
        x["w_vf"], x["b_vf"] = wave((1, hidden), 8) / np.float32(16), np.full(1, -0.125, np.float32)
        x["noise"] = exponentials((n, 2), 2)
        del x["value"]
    else:
        x["logits"] = wave((n, 1, 3), 1)
        x["logits"][k] = 0.25
        if n > 2:
            x["logits"][k + 1, 0, :2] = 1.5  # the two leading classes tie above the third
        x["noise"] = exponentials((n, 1, 3), 2)
    if entry == "cartpole":
        x["state"] = np.stack([wave(n, 10), wave(n, 11), wave(n, 12) / np.float32(10), wave(n, 13)])
    elif entry == "mountain_car":
        x["state"] = np.stack([wave(n, 10) * np.float32(0.4) - np.float32(0.3), wave(n, 11) * np.float32(0.03)])
    elif entry.startswith("pendulum"):
        x["state"] = np.stack([wave(n, 10) * np.float32(3), wave(n, 11) * np.float32(4)])
    elif entry == "algotrading":
        i = np.arange(n)
        invested = (i % 2).astype(np.float32)
        x["state"] = np.stack([
            invested, np.float32(700) + wave(n, 10) * np.float32(100), (wave(n, 11) + np.float32(2)) / np.float32(10),
            wave(n, 12) / np.float32(10), wave(n, 13) / np.float32(400), (i % 10).astype(np.float32),
            np.float32(2000) + wave(n, 14) * np.float32(500), wave(n, 15) / np.float32(100), wave(n, 16) / np.float32(100)])
        # the logits as the policy hands them over: the class the action mask forbids is -inf (buy when invested, else sell)
        x["logits"][i, 0, np.where(invested == 1, 1, 2)] = -np.inf
    return {name: np.ascontiguousarray(a, dtype=np.float32) for name, a in x.items()}


def run_case(entry: str, n: int, mode: str, rdr: bool, device: str = "cuda:0") -> dict[str, np.ndarray]:
    """Launch one case; every buffer the entry writes, as host arrays."""
    import torch

    from rl8_amd import hip
    from rl8_amd.envs import CartPoleConfig, MountainCarConfig, PendulumConfig

    x = {name: torch.from_numpy(a).to(device) for name, a in inputs(entry, n).items()}
    noise = x.pop("noise") if mode == "injected" else None
    if noise is None:
        x.pop("noise", None)
    state = x["state"]

    def out(*shape, dtype=torch.float32):
        return torch.full(shape, SENTINEL, dtype=dtype, device=device)

    discrete = not entry.endswith(("normal", "squashed"))
    got = {"state": state, "action": out(n, 1, dtype=torch.int64 if discrete else torch.float32), "logp": out(n, 1),
           "value": out(n, 1), "reward": out(n, 1)}
    if rdr:
        got["rdr_t1"] = out(n, 1)
    cols = dict(action_col=got["action"], logp_col=got["logp"], value_col=got["value"], reward_col=got["reward"],
                rdr_t=x["rdr_t"] if rdr else None, rdr_t1=got.get("rdr_t1"), gamma=GAMMA, seed=SEED, step=STEP,
                env_offset=ENV_OFFSET, deterministic=mode == "deterministic")
    if entry == "algotrading":
        obs = {key: out(n, d, dtype=torch.uint8).view(torch.bool) if dtype == torch.bool else out(n, d, dtype=dtype)
               for key, dtype, d in hip.ALGOTRADING_LEAVES}
        got.update({f"obs[{key}]": t for key, t in obs.items()})
        hip.rollout_step_algotrading(logits=x["logits"], value=x["value"], noise=noise, state=state, obs_col_next=obs, **cols)
    else:
        obs_dim = {"cartpole": 5, "mountain_car": 2, "pendulum_normal": 3, "pendulum_squashed": 3}.get(entry, 1)
        got["obs"] = cols["obs_col_next"] = out(n, obs_dim)
    if entry in ("dummy_discrete", "dummy_normal", "dummy_squashed"):
        hip.rollout_step_dummy(discrete=discrete, squashed=entry == "dummy_squashed",
                               features=x["features"] if discrete else x["mean"],
                               features2=None if discrete else x["log_std"], value=x["value"], noise=noise, state=state,
                               **cols)
    elif entry == "dummy_heads_256":
        tail = [cols[name] for name in ("action_col", "logp_col", "value_col", "reward_col", "obs_col_next", "rdr_t", "rdr_t1")]
        hip._check(hip.load().rl8_rollout_step_dummy_heads_f32(
            *(hip._ptr(t) for t in (x["h"], x["w_pol"], x["b_pol"], x["w_vf"], x["b_vf"], noise, state, *tail)), GAMMA, n,
            SEED, STEP, ENV_OFFSET, int(mode == "deterministic"), hip._stream()), "rl8_rollout_step_dummy_heads_f32")
    elif entry.startswith("dummy_heads_narrow"):
        hip.rollout_step_dummy_heads_narrow(x["h"], x["w_pol"], x["b_pol"], x["w_vf"], x["b_vf"], noise, state, **cols)
    elif entry == "cartpole":
        hip.rollout_step_cartpole(logits=x["logits"], value=x["value"], noise=noise, state=state,
                                  cfg=CartPoleConfig().to_abi(), **cols)
    elif entry == "mountain_car":
        hip.rollout_step_mountain_car(logits=x["logits"], value=x["value"], noise=noise, state=state,
                                      cfg=MountainCarConfig().to_abi(), **cols)
    elif entry.startswith("pendulum"):
        hip.rollout_step_pendulum(squashed=entry == "pendulum_squashed", mean=x["mean"], log_std=x["log_std"],
                                  value=x["value"], noise=noise, state=state, cfg=PendulumConfig().to_abi(), **cols)
    torch.cuda.synchronize()
    return {name: (t.view(torch.uint8) if t.dtype == torch.bool else t).cpu().numpy() for name, t in got.items()}


def main() -> None:
    sys.path.insert(0, ROOT)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    arrays = {}
    for case in CASES:
        for name, a in run_case(*case).items():
            arrays[f"{case_id(*case)}/{name}"] = a
    np.savez_compressed(path, **arrays)
    print(f"{len(CASES)} cases, {len(arrays)} arrays, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
