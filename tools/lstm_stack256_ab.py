#!/usr/bin/env python
"""A/B of the width-256 stack kernels against ``torch.nn.LSTM`` (``RL8_AMD_LSTM_STACK_256=0``: what the default
recurrent models ran with ``num_layers >= 2`` before the family existed).

``collect()`` and ``step()`` of ``RecurrentAlgorithmConfig(num_envs, horizon, model_config={"num_layers": n})`` with the
default discrete recurrent model on an environment of ``obs`` floats defined here (the arithmetic of
``tests/_envs.py::walk_env``), for every ``obs:layers`` of ``--variants``.  Without ``--child`` this starts fresh
processes, alternating the routes -- the kernels (the switch at 1) and torch's LSTM (the switch at 0) --, ``--repeats`` of
each per variant; each process warms up, times ``--steps`` iterations between device synchronisations and reports its
medians and its peak memory.  The report gives the median over the processes and their spread (max - min), then one more
process per route with the per-kernel HIP event timers on (never mixed with the end-to-end numbers: the events cost host
time).  A tree without the family ignores the switch, so the same command there measures torch's LSTM twice: the
baseline's own spread.

    python tools/lstm_stack256_ab.py --out profiles/lstm_stack256_ab.txt
    python tools/lstm_stack256_ab.py --num-envs 512 --out profiles/lstm_stack256_ab_512.txt
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "RL8_AMD_LSTM_STACK_256"


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


def child(args) -> None:
    import torch

    from rl8_amd import RecurrentAlgorithmConfig, hip

    torch.manual_seed(1)
    algo = RecurrentAlgorithmConfig(num_envs=args.num_envs, horizon=args.horizon,
                                    model_config={"num_layers": args.layers}).build(_env(args.obs, 3))
    for _ in range(args.warmup):
        algo.collect()
        algo.step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    if args.kernels:
        hip.timer.reset()
        hip.timer.enabled = True
    collect_s, step_s = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        algo.collect()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        algo.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        collect_s.append(t1 - t0)
        step_s.append(t2 - t1)
    result = {
        "obs": args.obs, "layers": args.layers,
        "collect_ms": statistics.median(collect_s) * 1e3, "step_ms": statistics.median(step_s) * 1e3,
        "peak_GB": torch.cuda.max_memory_allocated() / 1e9,
    }
    if args.kernels:
        hip.timer.enabled = False
        result["kernels"] = {k: {"launches": v["launches"] // args.steps, "ms_per_iteration": v["total_ms"] / args.steps}
                             for k, v in hip.timer.summary().items()}
    print("RESULT " + json.dumps(result), flush=True)


#: route -> (what the report calls it, the switch's value: None = unset)
ROUTES = {
    "kernels": ("kernels     ", "1"),
    "torch": ("torch's LSTM", "0"),
}


def _run_child(args, obs: int, layers: int, route: str, kernels: bool) -> dict:
    _, switch = ROUTES[route]
    env = dict(os.environ)
    env.pop(SWITCH, None)
    if switch is not None:
        env[SWITCH] = switch
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--obs", str(obs), "--layers", str(layers), "--num-envs", str(args.num_envs),
           "--horizon", str(args.horizon), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if kernels:
        cmd.append("--kernels")
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout, check=True)
    line = next(ln for ln in done.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def _stats(values: list[float]) -> tuple[float, float]:
    return statistics.median(values), max(values) - min(values)


def parent(args) -> int:
    lines = [f"width-256 LSTM stack A/B: RecurrentAlgorithmConfig(num_envs={args.num_envs}, horizon={args.horizon}), default"
             f" discrete recurrent model (LSTM(obs, 256, num_layers), heads 3 + 1); {args.repeats} alternating processes per route,"
             f" {args.warmup} warm-up + {args.steps} timed iterations each; median over processes of the per-process median"
             " [spread = max - min]"]
    for obs, layers in (map(int, v.split(":")) for v in args.variants):
        runs: dict[str, list[dict]] = {route: [] for route in ROUTES}
        for _ in range(args.repeats):
            for route in ROUTES:
                runs[route].append(_run_child(args, obs, layers, route, False))
        lines.append(f"\nobservation of {obs} floats, {layers} layers")
        total = {}
        for route, (name, _) in ROUTES.items():
            c, cs = _stats([r["collect_ms"] for r in runs[route]])
            s, ss = _stats([r["step_ms"] for r in runs[route]])
            total[route] = _stats([r["collect_ms"] + r["step_ms"] for r in runs[route]])
            peak = max(r["peak_GB"] for r in runs[route])
            lines.append(f"  {name}: collect {c:9.2f} ms [{cs:.2f}]   step {s:9.2f} ms [{ss:.2f}]   collect+step"
                         f" {total[route][0]:9.2f} ms [{total[route][1]:.2f}]   peak memory {peak:.2f} GB")
        gain, bar = total["torch"][0] - total["kernels"][0], 2 * total["torch"][1]
        lines.append(f"  kernels ahead of torch's LSTM by {gain:.2f} ms per iteration"
                     f" ({total['torch'][0] / total['kernels'][0]:.2f}x); twice the latter's own spread is {bar:.2f} ms:"
                     f" {'a win' if gain > bar else 'NOT a win'}")
        for route in ROUTES:
            k = _run_child(args, obs, layers, route, True)
            lines.append(f"  per-kernel HIP-event times, {ROUTES[route][0].strip()} (a run of its own; ms per iteration,"
                         " launches per iteration):")
            for name, v in sorted(k["kernels"].items(), key=lambda kv: -kv[1]["ms_per_iteration"]):
                lines.append(f"    {name:32s} {v['ms_per_iteration']:9.3f} ms  {v['launches']:5d}")
        if args.out:  # (kept as it grows: a long run that is cut short leaves the variants it finished)
            _write(args.out, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        _write(args.out, lines)
    return 0


def _write(path: str, lines: list[str]) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variants", nargs="+", default=["1:2", "1:3", "24:2", "24:3"], metavar="OBS:LAYERS")
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--obs", type=int, default=24, help=argparse.SUPPRESS)
    ap.add_argument("--layers", type=int, default=2, help=argparse.SUPPRESS)
    ap.add_argument("--kernels", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
