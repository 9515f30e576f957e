#!/usr/bin/env python
"""A/B of the narrow-wide tower kernels (``RL8_AMD_NARROW_WIDE_TOWERS=1``) against the torch modules (the switch off:
what the default models of width 64 / 128 run behind more than 16 inputs or with more than 8 outputs).

``collect()`` and ``step()`` of ``AlgorithmConfig(num_envs, horizon, model_config={"hiddens": (H, H)})`` with the
default discrete model on ``tests/_envs.py::walk_env(d, a)`` for (d, a) in (24, 4), (24, 12), (128, 34) and H in 64,
128.  Without ``--child`` this starts fresh processes, alternating the routes, ``--repeats`` of each per workload; each
process warms up, times ``--steps`` iterations between device synchronisations and reports its medians.  The report
gives the median over the processes and their spread (max - min), then one more process per workload with the
per-kernel HIP event timers on (never mixed with the end-to-end numbers: the events cost host time).

    python tools/narrow_wide_ab.py --out profiles/narrow_wide_ab.txt
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
SWITCH = "RL8_AMD_NARROW_WIDE_TOWERS"
SHAPES = ((24, 4), (24, 12), (128, 34))
WORKLOADS = {f"h{h}_d{d}_a{a}": (h, d, a) for h in (64, 128) for d, a in SHAPES}
ROUTES = {"kernels": "1", "torch": "0"}


def child(args) -> None:
    import torch

    from rl8_amd import AlgorithmConfig, hip
    from tests._envs import walk_env

    torch.manual_seed(1)
    h, d, a = WORKLOADS[args.workload]
    algo = AlgorithmConfig(num_envs=args.num_envs, horizon=args.horizon, model_config={"hiddens": (h, h)}).build(walk_env(d, a))
    for _ in range(args.warmup):
        algo.collect()
        algo.step()
    torch.cuda.synchronize()
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
    result = {"collect_ms": statistics.median(collect_s) * 1e3, "step_ms": statistics.median(step_s) * 1e3}
    if args.kernels:
        hip.timer.enabled = False
        result["kernels"] = {k: {"launches": v["launches"] // args.steps, "ms_per_iteration": v["total_ms"] / args.steps}
                             for k, v in hip.timer.summary().items()}
    print("RESULT " + json.dumps(result), flush=True)


def _run_child(args, workload: str, route: str, kernels: bool) -> dict:
    env = dict(os.environ, **{SWITCH: ROUTES[route]})
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", workload, "--num-envs", str(args.num_envs),
           "--horizon", str(args.horizon), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if kernels:
        cmd.append("--kernels")
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout, check=True)
    line = next(ln for ln in done.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def _stats(values: list[float]) -> tuple[float, float]:
    return statistics.median(values), max(values) - min(values)


def parent(args) -> int:
    lines = [f"narrow-wide towers A/B: AlgorithmConfig(num_envs={args.num_envs}, horizon={args.horizon}), default discrete"
             f" model on walk_env(d, a); {args.repeats} alternating processes per route, {args.warmup} warm-up +"
             f" {args.steps} timed iterations each; median over processes of the per-process median [spread = max - min]"]
    for name in args.workloads:
        h, d, a = WORKLOADS[name]
        runs: dict[str, list[dict]] = {route: [] for route in ROUTES}
        for _ in range(args.repeats):
            for route in ROUTES:
                runs[route].append(_run_child(args, name, route, False))
                print(f"{name} {route}: {runs[route][-1]['collect_ms'] + runs[route][-1]['step_ms']:.2f} ms", file=sys.stderr,
                      flush=True)
        lines.append(f"\nhiddens=({h}, {h}), walk_env({d}, {a}): policy tower {d} -> {h} -> {h} -> {a}, value tower {d} -> {h} -> {h} -> 1")
        total = {}
        for route in ROUTES:
            c, cs = _stats([r["collect_ms"] for r in runs[route]])
            s, ss = _stats([r["step_ms"] for r in runs[route]])
            total[route] = _stats([r["collect_ms"] + r["step_ms"] for r in runs[route]])
            lines.append(f"  {route:8s}: collect {c:9.2f} ms [{cs:.2f}]   step {s:9.2f} ms [{ss:.2f}]   collect+step"
                         f" {total[route][0]:9.2f} ms [{total[route][1]:.2f}]")
        gain, spread = total["torch"][0] - total["kernels"][0], total["torch"][1]
        verdict = "a win" if gain > 2 * spread else "a LOSS" if -gain > spread else "no difference beyond the spread"
        lines.append(f"  kernels ahead of torch by {gain:.2f} ms per iteration ({total['torch'][0] / total['kernels'][0]:.2f}x);"
                     f" the torch route's own spread is {spread:.2f} ms: {verdict}")
        k = _run_child(args, name, "kernels", True)
        lines.append("  per-kernel HIP-event times, kernels (a run of its own; ms per iteration, launches per iteration):")
        for kernel, v in sorted(k["kernels"].items(), key=lambda kv: -kv[1]["ms_per_iteration"])[:6]:
            lines.append(f"    {kernel:32s} {v['ms_per_iteration']:9.3f} ms  {v['launches']:5d}")
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
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=180.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="h64_d24_a12", help=argparse.SUPPRESS)
    ap.add_argument("--kernels", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
