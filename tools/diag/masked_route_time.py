"""The masked sequence functions on their kernels and with ``RL8_AMD_MASKED_KERNELS=0`` (DESIGN.md §6 rules: wall time
around a synchronise, median [min-max] of the repeats).

    python tools/diag/masked_route_time.py [--repeats 5] [--skip-algorithm] [--num-envs 65536] [--horizon 128]
                                           [--minibatches 1]

One JSON line per measurement:

* ``masked_avg`` forward and forward + backward at ``[2^20, 5, 8]`` under a window mask (row i pads ``i % 5`` leading
  cells), with the pool kernel's achieved GB/s against its algorithmic bytes (x read once, the mask read once, the
  output written once; backward: dout and the mask read, dx written);
* ``masked_log_softmax`` forward and forward + backward at ``[2^20, 3]`` (one lane per row) and ``[2^16, 1000]`` (one
  wave per row);
* ``AlgorithmConfig(num_envs, horizon, model_cls=TransformerTrader)`` on AlgoTrading: ``collect()``, ``step()`` and
  ``torch.cuda.max_memory_allocated()`` over a step.
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
from rl8_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
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
    for _ in range(2):  # warm-up: allocator, code objects
        fn()
    return spread([timed(fn) for _ in range(repeats)])


def kernel_times(fn) -> dict[str, float]:
    """Per-launch microseconds of the masked kernels in one call of ``fn`` (HIP events around each launch)."""
    fn()
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        fn()
        summary = hip.timer.summary()
    finally:
        hip.timer.enabled = False
    return {name: round(s["avg_ms"] * 1e3, 2) for name, s in summary.items() if name.startswith("masked_")}


def function_lines(repeats: int) -> None:
    rows, t, e = 2**20, 5, 8
    x = torch.randn(rows, t, e, device=DEV, requires_grad=True)
    mask = torch.arange(t, device=DEV).expand(rows, t) >= (torch.arange(rows, device=DEV) % t).unsqueeze(1)
    dout = torch.randn(rows, e, device=DEV)

    def avg_forward():
        with torch.no_grad():
            F.masked_avg(x, mask=mask)

    def avg_both():
        x.grad = None
        F.masked_avg(x, mask=mask).backward(dout)

    cases = [("masked_avg", [rows, t, e], avg_forward, avg_both)]
    for shape in ([2**20, 3], [2**16, 1000]):
        logits = torch.randn(*shape, device=DEV, requires_grad=True)
        valid = torch.rand(*shape, device=DEV) > 0.25
        grad = torch.randn(*shape, device=DEV)

        def forward(logits=logits, valid=valid):
            with torch.no_grad():
                F.masked_log_softmax(logits, mask=valid)

        def both(logits=logits, valid=valid, grad=grad):
            logits.grad = None
            F.masked_log_softmax(logits, mask=valid).backward(grad)

        cases.append(("masked_log_softmax", shape, forward, both))
    for name, shape, forward, both in cases:
        line: dict = {"function": name, "shape": shape, "repeats": repeats}
        for route, switch in ROUTES.items():
            os.environ["RL8_AMD_MASKED_KERNELS"] = switch
            line[f"forward_ms_{route}"] = measure(forward, repeats)
            line[f"forward_backward_ms_{route}"] = measure(both, repeats)
        os.environ["RL8_AMD_MASKED_KERNELS"] = "1"
        line["kernel_us"] = kernel_times(both)
        if name == "masked_avg":
            forward_bytes = rows * t * e * 4 + rows * t + rows * e * 4
            backward_bytes = rows * e * 4 + rows * t + rows * t * e * 4
            line["pool_GB_per_s"] = {
                "forward": round(forward_bytes / (line["kernel_us"]["masked_pool"] * 1e-6) / 1e9, 1),
                "backward": round(backward_bytes / (line["kernel_us"]["masked_pool_backward"] * 1e-6) / 1e9, 1),
                "forward_bytes": forward_bytes, "backward_bytes": backward_bytes}
        print(json.dumps(line), flush=True)


def algorithm_lines(n: int, h: int, minibatches: int, repeats: int) -> None:
    for route, switch in ROUTES.items():
        os.environ["RL8_AMD_MASKED_KERNELS"] = switch
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
        print(json.dumps({"model": "TransformerTrader", "route": route, "num_envs": n, "horizon": h,
                          "num_minibatches": minibatches, "repeats": repeats, "collect_ms": spread(collect_ms),
                          "step_ms": spread(step_ms), "step_peak_MiB": round(max(peaks) / 2**20, 1)}), flush=True)
        del algo
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-functions", action="store_true")
    ap.add_argument("--skip-algorithm", action="store_true")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--minibatches", type=int, default=1)
    args = ap.parse_args()
    if not args.skip_functions:
        function_lines(args.repeats)
    if not args.skip_algorithm:
        algorithm_lines(args.num_envs, args.horizon, args.minibatches, args.repeats)


if __name__ == "__main__":
    main()
