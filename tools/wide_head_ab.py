#!/usr/bin/env python
"""A/B of the wide-head tower kernels against the torch modules (``RL8_AMD_WIDE_HEAD_TOWERS=0``: what the default
models ran for heads of more than 8 outputs before the family existed).

``collect()`` and ``step()`` of ``AlgorithmConfig(num_envs, horizon)`` with the default models on environments defined
here: the default discrete model with 18 and with 100 actions on a 4-float observation (the arithmetic of
``tests/_envs.py::walk_env``), and the default continuous model with 8 action dimensions on a 24-float observation.
Without ``--child`` this starts fresh processes, alternating the routes -- the kernels and the torch modules --,
``--repeats`` of each per workload; each process warms up, times ``--steps`` iterations between device
synchronisations and reports its medians and its peak memory.  The report gives the median over the processes and
their spread (max - min), then one more process with the per-kernel HIP event timers on (never mixed with the
end-to-end numbers: the events cost host time).

    python tools/wide_head_ab.py --out profiles/wide_head_ab.txt
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
SWITCH = "RL8_AMD_WIDE_HEAD_TOWERS"
#: workload -> (what the report calls it, observation floats, actions, continuous)
WORKLOADS = {
    "discrete18": ("default discrete model, 18 actions on a 4-float observation (policy tower 4 -> 256 -> 256 -> 18)", 4, 18, False),
    "discrete100": ("default discrete model, 100 actions on a 4-float observation (policy tower 4 -> 256 -> 256 -> 100)", 4, 100, False),
    "continuous8": ("default continuous model, 8 action dimensions on a 24-float observation (policy tower 24 -> 256 -> 256 -> [8 | 8])", 24, 8, True),
}


def _env(d: int, a: int, continuous: bool):
    import torch

    from rl8_amd.data import DataKeys
    from rl8_amd.env import Env
    from rl8_amd.specs import Categorical, Unbounded
    from rl8_amd.tensordict import TensorDict

    class Walk(Env):
        def __init__(self, num_envs, /, horizon=None, *, device="cpu"):
            super().__init__(num_envs, horizon, device=device)
            self.observation_spec = Unbounded(d, device=device)
            self.action_spec = (Unbounded(shape=torch.Size([a]), device=device) if continuous
                                else Categorical(a, shape=torch.Size([1]), device=device))

        def reset(self, *, config=None):
            self.state = torch.empty(self.num_envs, d, device=self.device).uniform_(-1.0, 1.0)
            return self.state

        def step(self, action):
            push = torch.zeros_like(self.state)
            if continuous:
                push[:, :a] = action.reshape(-1, a).clamp(-1.0, 1.0)
            else:
                push.scatter_(1, action.reshape(-1, 1) % d, 1.0)
            self.state = 0.75 * self.state + push - 0.25
            rewards = -self.state.abs().sum(-1, keepdim=True)
            return TensorDict({DataKeys.OBS: self.state, DataKeys.REWARDS: rewards}, batch_size=self.num_envs,
                              device=self.device)

    return Walk


def child(args) -> None:
    import torch

    from rl8_amd import AlgorithmConfig, hip

    torch.manual_seed(1)
    _, obs, actions, continuous = WORKLOADS[args.workload]
    algo = AlgorithmConfig(num_envs=args.num_envs, horizon=args.horizon).build(_env(obs, actions, continuous))
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
        "workload": args.workload,
        "collect_ms": statistics.median(collect_s) * 1e3, "step_ms": statistics.median(step_s) * 1e3,
        "peak_GB": torch.cuda.max_memory_allocated() / 1e9,
    }
    if args.kernels:
        hip.timer.enabled = False
        result["kernels"] = {k: {"launches": v["launches"] // args.steps, "ms_per_iteration": v["total_ms"] / args.steps}
                             for k, v in hip.timer.summary().items()}
    print("RESULT " + json.dumps(result), flush=True)


#: route -> (what the report calls it, the switch's value, extra child arguments)
ROUTES = {
    "kernels": ("kernels           ", "1", []),
    "torch": ("torch modules     ", "0", []),
}


def _run_child(args, workload: str, route: str, kernels: bool) -> dict:
    _, switch, extra = ROUTES[route]
    env = dict(os.environ, **{SWITCH: switch})
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", workload, "--num-envs", str(args.num_envs),
           "--horizon", str(args.horizon), "--steps", str(args.steps), "--warmup", str(args.warmup), *extra]
    if kernels:
        cmd.append("--kernels")
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout, check=True)
    line = next(ln for ln in done.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def _stats(values: list[float]) -> tuple[float, float]:
    return statistics.median(values), max(values) - min(values)


def parent(args) -> int:
    lines = [f"wide-head towers A/B: AlgorithmConfig(num_envs={args.num_envs}, horizon={args.horizon}), default models"
             f" (256, 256); {args.repeats} alternating processes per route, {args.warmup} warm-up +"
             f" {args.steps} timed iterations each; median over processes of the per-process median [spread = max - min]"]
    for obs in args.workloads:
        runs: dict[str, list[dict]] = {route: [] for route in ROUTES}
        for _ in range(args.repeats):
            for route in ROUTES:
                runs[route].append(_run_child(args, obs, route, False))
                print(f"{obs} {route}: {runs[route][-1]['collect_ms'] + runs[route][-1]['step_ms']:.2f} ms", file=sys.stderr,
                      flush=True)
        lines.append(f"\n{WORKLOADS[obs][0]}")
        total = {}
        for route, (name, _, _) in ROUTES.items():
            c, cs = _stats([r["collect_ms"] for r in runs[route]])
            s, ss = _stats([r["step_ms"] for r in runs[route]])
            total[route] = _stats([r["collect_ms"] + r["step_ms"] for r in runs[route]])
            peak = max(r["peak_GB"] for r in runs[route])
            lines.append(f"  {name}: collect {c:9.2f} ms [{cs:.2f}]   step {s:9.2f} ms [{ss:.2f}]   collect+step"
                         f" {total[route][0]:9.2f} ms [{total[route][1]:.2f}]   peak memory {peak:.2f} GB")
        for ahead, behind in (("kernels", "torch"),):
            gain, bar = total[behind][0] - total[ahead][0], 2 * total[behind][1]
            lines.append(f"  {ROUTES[ahead][0].strip()} ahead of {ROUTES[behind][0].strip()} by {gain:.2f} ms per iteration"
                         f" ({total[behind][0] / total[ahead][0]:.2f}x); twice the latter's own spread is {bar:.2f} ms:"
                         f" {'a win' if gain > bar else 'NOT a win'}")
        for route in ("kernels",):
            k = _run_child(args, obs, route, True)
            lines.append(f"  per-kernel HIP-event times, {ROUTES[route][0].strip()} (a run of its own; ms per iteration,"
                         " launches per iteration):")
            for name, v in sorted(k["kernels"].items(), key=lambda kv: -kv[1]["ms_per_iteration"]):
                lines.append(f"    {name:32s} {v['ms_per_iteration']:9.3f} ms  {v['launches']:5d}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", choices=sorted(WORKLOADS), default=list(WORKLOADS))
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="discrete18", help=argparse.SUPPRESS)
    ap.add_argument("--kernels", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
