#!/usr/bin/env python
"""A/B of the narrow LSTM kernels behind wide inputs (``RL8_AMD_NARROW_WIDE_INPUT_LSTM=1``) against ``torch.nn.LSTM``
(the switch unset: what a recurrent model of hidden width 64 / 128 runs on an observation of more than 16 floats).

``collect()`` + ``step()`` of ``RecurrentAlgorithmConfig(num_envs, horizon, model_config={"hidden_size": H})`` with the
default discrete recurrent model on an environment of ``--widths`` floats defined here (the arithmetic of
``tests/_envs.py::walk_env``), for H in ``--hidden``.  One process: per (H, width) two algorithms built from the same
seed, one per route; after ``--warmup`` iterations of each, ``--rounds`` rounds alternate the routes -- the switch is
read on every call -- and time one iteration of each between device synchronisations.  The report gives the median
[min - max] over the rounds.  The route earns its place where its median beats the module route's by more than the
module route's own min - max spread.  A last iteration per route runs with the per-kernel HIP event timers on (never
mixed with the end-to-end numbers: the events cost host time).

    python tools/narrow_wide_input_lstm_ab.py --out profiles/narrow_wide_input_lstm_ab.txt
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "RL8_AMD_NARROW_WIDE_INPUT_LSTM"
ROUTES = {"kernels": "1", "torch's LSTM": None}  # route -> the switch's value (None: unset)


def _env(d: int, a: int):
    import torch

    from rl8_amd.data import DataKeys
    from rl8_amd.env import Env
    from rl8_amd.specs import Categorical, Unbounded
    from rl8_amd.tensordict import TensorDict

    class Walk(Env):
        def __init__(self, num_envs, /, horizon=None, *, device="cpu"):
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Unbounded(d, device=device)
            self.action_spec = Categorical(a, shape=torch.Size([1]), device=device)

        def reset(self, *, config=None):
            self.state = torch.empty(self.num_envs, d, device=self.device).uniform_(-1.0, 1.0)
            return self.state

        def step(self, action):
            push = torch.zeros_like(self.state)
            push.scatter_(1, action.reshape(-1, 1) % d, 1.0)
            self.state = 0.75 * self.state + push - 0.25
            rewards = -self.state.abs().sum(-1, keepdim=True)
            return TensorDict({DataKeys.OBS: self.state, DataKeys.REWARDS: rewards}, batch_size=self.num_envs,
                              device=self.device)

    return Walk


def _set(switch: None | str) -> None:
    os.environ.pop(SWITCH, None)
    if switch is not None:
        os.environ[SWITCH] = switch


def _iteration(algo, switch: None | str) -> tuple[float, float]:
    """(collect, step) of one iteration in ms, each ending in a device synchronise."""
    import torch

    _set(switch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    algo.collect()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    algo.step()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def _fmt(values: list[float]) -> str:
    return f"{statistics.median(values):8.2f} ms [{min(values):.2f} - {max(values):.2f}]"


def measure(args, hidden: int, obs: int) -> list[str]:
    import torch

    from rl8_amd import RecurrentAlgorithmConfig, hip

    algos = {}
    for route, switch in ROUTES.items():
        _set(switch)
        torch.manual_seed(1)
        algos[route] = RecurrentAlgorithmConfig(num_envs=args.num_envs, horizon=args.horizon,
                                                model_config={"hidden_size": hidden}).build(_env(obs, 3))
        for _ in range(args.warmup):
            _iteration(algos[route], switch)
    times: dict[str, list[tuple[float, float]]] = {route: [] for route in ROUTES}
    for _ in range(args.rounds):
        for route, switch in ROUTES.items():
            times[route].append(_iteration(algos[route], switch))
    lines = [f"\nhidden {hidden}, observation of {obs} floats"]
    total = {}
    for route in ROUTES:
        total[route] = [c + s for c, s in times[route]]
        lines.append(f"  {route:12s}: collect {_fmt([c for c, _ in times[route]])}   step {_fmt([s for _, s in times[route]])}"
                     f"   collect+step {_fmt(total[route])}")
    ours, module = statistics.median(total["kernels"]), statistics.median(total["torch's LSTM"])
    spread = max(total["torch's LSTM"]) - min(total["torch's LSTM"])
    lines.append(f"  kernels ahead of torch's LSTM by {module - ours:.2f} ms per iteration ({module / ours:.2f}x); the"
                 f" module route's own min - max spread is {spread:.2f} ms: {'a win' if module - ours > spread else 'NOT a win'}")
    for route, switch in ROUTES.items():
        hip.timer.reset()
        hip.timer.enabled = True
        _iteration(algos[route], switch)
        hip.timer.enabled = False
        lines.append(f"  per-kernel HIP-event times, {route} (an iteration of its own; ms, launches):")
        for name, v in sorted(hip.timer.summary().items(), key=lambda kv: -kv[1]["total_ms"]):
            lines.append(f"    {name:32s} {v['total_ms']:9.3f} ms  {v['launches']:5d}")
        hip.timer.reset()
    _set(None)
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--widths", type=int, nargs="+", default=[24, 128])
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = [f"narrow-wide-input LSTM A/B: RecurrentAlgorithmConfig(num_envs={args.num_envs}, horizon={args.horizon},"
             f" model_config={{'hidden_size': H}}), default discrete recurrent model (LSTM(obs, H), heads 3 + 1); one"
             f" process, {args.warmup} warm-up iterations per route, then {args.rounds} rounds alternating the routes;"
             " median [min - max] over the rounds"]
    for hidden in args.hidden:
        for obs in args.widths:
            lines += measure(args, hidden, obs)
            if args.out:  # (kept as it grows: a run that is cut short leaves the shapes it finished)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
