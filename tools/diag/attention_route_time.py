"""The attention blocks on the short-sequence attention kernels and with ``RL8_AMD_ATTENTION_KERNELS=0`` (DESIGN.md §6
rules: wall time around a synchronise, median [min-max] of the repeats, after two warm-up calls).

    python tools/diag/attention_route_time.py [--repeats 5] [--skip-core] [--skip-algorithm] [--routes on,off]
                                              [--label this-commit] [--num-envs 65536] [--horizon 128] [--minibatches 1]

One JSON line per measurement:

* the core under ``nn.MultiheadAttention(8, 4)`` on ``[2^20, 5, 8]`` under a window mask (row i pads ``i % 5`` leading
  cells), the module's projections on both routes: forward, and forward + backward; the per-launch time of the two
  entries from HIP events, and their achieved GB/s against the algorithmic bytes (forward: the packed projection and
  the mask read, ``out`` and ``lse`` written; backward: the projection, the mask, ``out``, ``lse`` and ``dout`` read, the
  packed gradient written);
* ``AlgorithmConfig(num_envs, horizon, model_cls=TransformerTrader)`` on AlgoTrading: ``collect()``, ``step()`` and
  ``torch.cuda.max_memory_allocated()`` over a step, per route.

The second part uses the public API only: the same file run from a checkout of an earlier commit (``--skip-core
--routes on --label parent``) gives that commit's figures, the switch meaning nothing there.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.envs import AlgoTrading, TransformerTrader  # noqa: E402

DEV = "cuda"
SWITCH = "RL8_AMD_ATTENTION_KERNELS"
ROUTES = {"on": "1", "off": "0"}


def spread(ms: list[float]) -> dict[str, float]:
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(fn) -> float:
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def measure(fn, repeats: int) -> dict[str, float]:
    for _ in range(2):  # warm-up: allocator, code objects, rocBLAS
        fn()
    return spread([timed(fn) for _ in range(repeats)])


def kernel_times(fn) -> dict[str, float]:
    """Per-launch microseconds of the attention entries in one call of ``fn`` (HIP events around each launch)."""
    fn()
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        fn()
        summary = hip.timer.summary()
    finally:
        hip.timer.enabled = False
    return {name: round(s["avg_ms"] * 1e3, 2) for name, s in summary.items() if name.startswith("attention")}


def core_lines(routes: list[str], repeats: int) -> None:
    from rl8_amd.nn.modules.attention import _attend

    rows, t, e, heads = 2**20, 5, 8, 4
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(e, heads, batch_first=True).to(DEV)
    x = torch.randn(rows, t, e, device=DEV, requires_grad=True)
    padding = torch.arange(t, device=DEV).expand(rows, t) < (torch.arange(rows, device=DEV) % t).unsqueeze(1)
    dout = torch.randn(rows, t, e, device=DEV)

    def forward():
        with torch.no_grad():
            _attend(mha, x, x, padding, None)

    def both():
        x.grad = None
        mha.zero_grad()
        _attend(mha, x, x, padding, None).backward(dout)

    line: dict = {"module": "MultiheadAttention", "shape": [rows, t, e], "heads": heads, "repeats": repeats}
    for route in routes:
        os.environ[SWITCH] = ROUTES[route]
        line[f"forward_ms_{route}"] = measure(forward, repeats)
        line[f"forward_backward_ms_{route}"] = measure(both, repeats)
    if "on" in routes:
        os.environ[SWITCH] = "1"
        line["kernel_us"] = kernel_times(both)
        projection, mask, out, lse = rows * t * 3 * e * 4, rows * t, rows * t * e * 4, rows * heads * t * 4
        forward_bytes = projection + mask + out + lse
        backward_bytes = projection + mask + out + lse + out + projection
        line["GB_per_s"] = {
            "forward": round(forward_bytes / (line["kernel_us"]["attention"] * 1e-6) / 1e9, 1),
            "backward": round(backward_bytes / (line["kernel_us"]["attention_backward"] * 1e-6) / 1e9, 1),
            "forward_bytes": forward_bytes, "backward_bytes": backward_bytes}
    print(json.dumps(line), flush=True)


def algorithm_lines(routes: list[str], label: str, n: int, h: int, minibatches: int, repeats: int) -> None:
    for route in routes:
        os.environ[SWITCH] = ROUTES[route]
        torch.manual_seed(0)
        algo = AlgorithmConfig(num_envs=n, horizon=h, sgd_minibatch_size=n * h // minibatches,
                               model_cls=TransformerTrader).build(AlgoTrading)
        for _ in range(2):  # warm-up: allocator, rocBLAS
            algo.collect()
            algo.step()
        collect_ms, step_ms, peaks = [], [], []
        for _ in range(repeats):
            collect_ms.append(timed(algo.collect))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step_ms.append(timed(algo.step))
            peaks.append(torch.cuda.max_memory_allocated())
        print(json.dumps({"model": "TransformerTrader", "commit": label, "route": route, "num_envs": n, "horizon": h,
                          "num_minibatches": minibatches, "repeats": repeats, "collect_ms": spread(collect_ms),
                          "step_ms": spread(step_ms), "step_peak_MiB": round(max(peaks) / 2**20, 1)}), flush=True)
        del algo
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-core", action="store_true")
    ap.add_argument("--skip-algorithm", action="store_true")
    ap.add_argument("--routes", default="on,off")
    ap.add_argument("--label", default="this-commit")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--minibatches", type=int, default=1)
    args = ap.parse_args()
    routes = [r for r in args.routes.split(",") if r]
    assert all(r in ROUTES for r in routes), routes
    if not args.skip_core:
        core_lines(routes, args.repeats)
    if not args.skip_algorithm:
        algorithm_lines(routes, args.label, args.num_envs, args.horizon, args.minibatches, args.repeats)


if __name__ == "__main__":
    main()
