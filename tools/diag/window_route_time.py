"""collect() and step() of a windowed feed-forward model on AlgoTrading, on the window kernels and with
``RL8_AMD_WINDOW_KERNELS=0`` (DESIGN.md §6 rules: wall time around a synchronise, median [min-max] of the repeats).

    python tools/diag/window_route_time.py [--model mlp|masked] [--num-envs 65536] [--horizon 128] [--repeats 5]
                                           [--minibatches 1 8] [--routes on off]

``--model mlp``: ``rl8_amd.envs.MLPTrader`` (seq_len 4).  ``--model masked``: the windowed ``MaskedTrader`` of
tests/test_algotrading_gpu.py, which exists on commits before the window kernels too: the same command on both commits
shows that the switch-off route is the earlier code (``--routes off`` there; the switch is not read before them).

Per (route, num_minibatches) one JSON line: collect / step wall times in ms, ``torch.cuda.max_memory_allocated()``
over a step, and -- route on -- the per-launch time of ``rl8_window_last`` and ``rl8_gather_windows`` from
``hip.KernelTimer`` (a separate, timed collect + step) against their algorithmic bytes.
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
from rl8_amd.envs import AlgoTrading  # noqa: E402


def spread(ms: list[float]) -> dict[str, float]:
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def timed(fn) -> float:
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def window_bytes(model: str, n: int, h: int, minibatches: int) -> dict[str, float]:
    """Algorithmic bytes per launch: every source cell read once and every output byte written once.  Leaves of
    AlgoTrading: mask 3 B, invested 8 B, two f32; the window of ``size`` f32 cells carries a ``size``-byte mask."""
    size = 5 if model == "mlp" else 4
    row = (3 + 8 + 4) * 2 + size * 4 * 2 + size  # (unwindowed leaves in and out, the window in and out, its mask)
    return {"window_last": float(n * row), "gather_windows": float(n * h // minibatches * (row + 8 * (minibatches > 1)))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("mlp", "masked"), default="mlp")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--minibatches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--routes", nargs="+", default=["on", "off"])
    args = ap.parse_args()
    if args.model == "mlp":
        from rl8_amd.envs import MLPTrader

        model = {"model_cls": MLPTrader, "model_config": {"seq_len": 4}}
    else:
        from tests.test_algotrading_gpu import MaskedTrader

        model = {"model_cls": MaskedTrader, "model_config": {"window": 3}}
    n, h = args.num_envs, args.horizon
    for minibatches in args.minibatches:
        for route in args.routes:
            os.environ["RL8_AMD_WINDOW_KERNELS"] = "1" if route == "on" else "0"
            torch.manual_seed(0)
            algo = AlgorithmConfig(num_envs=n, horizon=h, sgd_minibatch_size=n * h // minibatches, **model).build(AlgoTrading)
            for _ in range(2):  # warm-up: allocator, rocBLAS
                algo.collect()
                algo.step()
            collect_ms, step_ms, peaks = [], [], []
            for _ in range(args.repeats):
                collect_ms.append(timed(algo.collect))
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                step_ms.append(timed(algo.step))
                peaks.append(torch.cuda.max_memory_allocated())
            line = {"model": args.model, "route": route, "num_envs": n, "horizon": h, "num_minibatches": minibatches,
                    "repeats": args.repeats, "collect_ms": spread(collect_ms), "step_ms": spread(step_ms),
                    "step_peak_MiB": round(max(peaks) / 2**20, 1)}
            if route == "on" and hasattr(hip, "gather_windows"):
                hip.timer.reset()
                hip.timer.enabled = True
                try:
                    algo.collect()
                    algo.step()
                    summary = hip.timer.summary()
                finally:
                    hip.timer.enabled = False
                nbytes = window_bytes(args.model, n, h, minibatches)
                line["kernels"] = {
                    name: {"launches": s["launches"], "avg_us": round(s["avg_ms"] * 1e3, 2),
                           "GB_per_s": round(nbytes[name] / (s["avg_ms"] * 1e-3) / 1e9, 1)}
                    for name, s in summary.items() if name in nbytes}
            print(json.dumps(line), flush=True)
            del algo
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
