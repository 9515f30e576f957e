"""The traders' BatchNorm towers on the narrow tower kernels (``RL8_AMD_BATCHNORM_TOWERS=1``) and on the torch modules
(DESIGN.md §6 rules: wall time around a synchronise, median [min-max] of the repeats, after two warm-up calls).

    python tools/diag/batchnorm_tower_time.py [--repeats 5] [--skip-tower] [--skip-algorithm] [--routes on,off]
                                              [--label this-commit] [--num-envs 65536] [--horizon 128]
                                              [--models MLPTrader,TransformerTrader]

One JSON line per measurement:

* ``AlgorithmConfig(num_envs, horizon, model_cls=...)`` on AlgoTrading for ``MLPTrader`` and ``TransformerTrader``:
  ``collect()``, ``step()`` and ``torch.cuda.max_memory_allocated()`` over a step, per route;
* one tower, ``Sequential(MLP(d_in, (W, W), norm_layer=BatchNorm1d), ReLU, Linear(W, n))`` in training mode, at
  ``2^20 x 7`` (W 128, n 3) and ``2^20 x 11`` (W 64, n 1) with an input that asks for its gradient: forward, and forward +
  backward, per route;
* from HIP events around the raw entries: the moments launches, the fold launch and the narrow backward with and
  without dx, with each one's algorithmic bytes (the rows it must read and write) and its share of the 8 TB/s HBM peak.

The first part uses the public API only: the same file run from a checkout of an earlier commit (``--skip-tower
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
import torch.nn as nn  # noqa: E402

import rl8_amd.envs as envs  # noqa: E402
from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.nn import MLP  # noqa: E402

DEV = "cuda"
SWITCH = "RL8_AMD_BATCHNORM_TOWERS"
ROUTES = {"on": "1", "off": "0"}
HBM_BYTES_PER_S = 8.0e12


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


def event_us(fn, repeats: int) -> float:
    """Median microseconds of ``fn``'s launches between two HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    us = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        us.append(start.elapsed_time(end) * 1e3)
    return round(statistics.median(us), 2)


def traffic(us: float, nbytes: int) -> dict:
    return {"us": us, "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1),
            "share_of_hbm_peak": round(nbytes / HBM_BYTES_PER_S * 1e6 / us, 4)}


def algorithm_lines(models: list[str], routes: list[str], label: str, n: int, h: int, repeats: int) -> None:
    for name in models:
        for route in routes:
            os.environ[SWITCH] = ROUTES[route]
            torch.manual_seed(0)
            algo = AlgorithmConfig(num_envs=n, horizon=h, model_cls=getattr(envs, name)).build(envs.AlgoTrading)
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
            print(json.dumps({"model": name, "commit": label, "route": route, "num_envs": n, "horizon": h,
                              "repeats": repeats, "collect_ms": spread(collect_ms), "step_ms": spread(step_ms),
                              "step_peak_MiB": round(max(peaks) / 2**20, 1)}), flush=True)
            del algo
            torch.cuda.empty_cache()


def tower_lines(routes: list[str], repeats: int) -> None:
    from rl8_amd.envs import algotrading_models

    rows = 2**20
    for d_in, width, n in ((7, 128, 3), (11, 64, 1)):
        torch.manual_seed(0)
        net = nn.Sequential(MLP(d_in, (width, width), norm_layer=nn.BatchNorm1d), nn.ReLU(), nn.Linear(width, n)).to(DEV)
        x = torch.randn(rows, d_in, device=DEV, requires_grad=True)
        dout = torch.randn(rows, n, device=DEV)

        def forward():
            with torch.no_grad():
                algotrading_models._tower(net, x)

        def both():
            x.grad = None
            net.zero_grad()
            algotrading_models._tower(net, x).backward(dout)

        line: dict = {"tower": f"Linear({d_in}, {width}) BatchNorm1d ReLU Linear({width}, {width}) ReLU Linear({width}, {n})",
                      "rows": rows, "repeats": repeats}
        for route in routes:
            os.environ[SWITCH] = ROUTES[route]
            line[f"forward_ms_{route}"] = measure(forward, repeats)
            line[f"forward_backward_ms_{route}"] = measure(both, repeats)
        print(json.dumps(line), flush=True)
        if "on" not in routes:
            continue
        l1, norm, l2, head = net[0][0], net[0][1], net[0][3], net[2]
        xd = x.detach()
        mu, cov = hip.tower_moments(xd)
        rm, rv = norm.running_mean.clone(), norm.running_var.clone()

        def fold():
            return hip.batchnorm_fold(l1.weight, l1.bias, norm.weight, norm.bias, norm.eps, moments=(mu, cov, rows),
                                      running_mean=rm, running_var=rv, factor=0.1)

        a, c = fold()[:2]
        weights = (a, c, l2.weight.detach(), l2.bias.detach(), head.weight.detach())
        x_bytes, dout_bytes = rows * d_in * 4, rows * n * 4
        kernels = {
            "moments": traffic(event_us(lambda: hip.tower_moments(xd), repeats), x_bytes),
            "fold": {"us": event_us(fold, repeats)},
            "forward": traffic(event_us(lambda: hip.mlp_narrow_forward(xd, *weights, head.bias.detach()), repeats),
                               x_bytes + dout_bytes),
            "backward_and_reduce": traffic(event_us(lambda: hip.mlp_narrow_backward(xd, dout, *weights), repeats),
                                           x_bytes + dout_bytes),
            "backward_dx_and_reduce": traffic(event_us(lambda: hip.mlp_narrow_backward(xd, dout, *weights, want_dx=True),
                                                       repeats), 2 * x_bytes + dout_bytes),
        }
        print(json.dumps({"kernels": kernels, "rows": rows, "d_in": d_in, "width": width, "n_out": n}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-tower", action="store_true")
    ap.add_argument("--skip-algorithm", action="store_true")
    ap.add_argument("--routes", default="on,off")
    ap.add_argument("--label", default="this-commit")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--models", default="MLPTrader,TransformerTrader")
    args = ap.parse_args()
    routes = [r for r in args.routes.split(",") if r]
    assert all(r in ROUTES for r in routes), routes
    if not args.skip_algorithm:
        algorithm_lines([m for m in args.models.split(",") if m], routes, args.label, args.num_envs, args.horizon,
                        args.repeats)
    if not args.skip_tower:
        tower_lines(routes, args.repeats)


if __name__ == "__main__":
    main()
