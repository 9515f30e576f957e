"""The attention blocks' feedforward block on the fused feedforward kernels and with ``RL8_AMD_FEEDFORWARD_KERNELS=0``
(DESIGN.md §6 rules: wall time around a synchronise, median [min-max] of the repeats, after two warm-up calls).

    python tools/diag/feedforward_route_time.py [--repeats 5] [--skip-block] [--skip-algorithm] [--routes on,off]
                                                [--label this-commit] [--num-envs 65536] [--horizon 128] [--minibatches 1]

One JSON line per measurement:

* the block alone, ``skip(y, Linear(64, 8)(relu(Linear(8, 64)(LayerNorm(8)(y)))))`` with a residual skip connection on
  ``[2^20, 5, 8]`` through ``SequentialSkipConnection``'s route: forward, and forward + backward, per route; then, from
  HIP events around the raw entries, the time of the forward kernel, of the dx kernel, of the weight-gradient kernel
  with the final sum, and of the whole backward entry; each kernel's algorithmic bytes (the rows it must read and
  write; the parameters and partial sums are left out) and multiply-adds (2 F H, 3 F H and 4 F H per row), its rates,
  their shares of the 8 TB/s HBM peak and of the fp32 vector peak (157.3 TFLOP/s = 78.65e12 multiply-adds per second),
  and which of the two bounds it -- the one whose least time is the larger;
* ``AlgorithmConfig(num_envs, horizon, model_cls=TransformerTrader)`` on AlgoTrading: ``collect()``, ``step()`` and
  ``torch.cuda.max_memory_allocated()`` over a step, per route.

The second part uses the public API only: the same file run from a checkout of an earlier commit (``--skip-block
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
SWITCH = "RL8_AMD_FEEDFORWARD_KERNELS"
ROUTES = {"on": "1", "off": "0"}
HBM_BYTES_PER_S = 8.0e12
FP32_FMA_PER_S = 157.3e12 / 2


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


def roofline(us: float, nbytes: int, fma: int) -> dict:
    least_bytes_us, least_fma_us = nbytes / HBM_BYTES_PER_S * 1e6, fma / FP32_FMA_PER_S * 1e6
    return {"us": us, "bytes": nbytes, "multiply_adds": fma, "GB_per_s": round(nbytes / us / 1e3, 1),
            "share_of_hbm_peak": round(least_bytes_us / us, 3), "Gfma_per_s": round(fma / us / 1e3, 1),
            "share_of_fp32_vector_peak": round(least_fma_us / us, 3),
            "bound_by": "HBM" if least_bytes_us > least_fma_us else "fp32 vector"}


def block_lines(routes: list[str], repeats: int) -> None:
    from rl8_amd.nn.modules.attention import _feedforward
    from rl8_amd.nn.modules.skip import SequentialSkipConnection

    rows, t, f, hidden = 2**20, 5, 8, 64
    torch.manual_seed(0)
    skip = SequentialSkipConnection(f, kind="residual")
    skip.append(_feedforward(skip, hidden, "relu", 0.0))
    skip = skip.to(DEV)
    x = torch.randn(rows, t, f, device=DEV)
    y = torch.randn(rows, t, f, device=DEV, requires_grad=True)
    dout = torch.randn(rows, t, f, device=DEV)

    def forward():
        with torch.no_grad():
            skip(x, y)

    def both():
        y.grad = None
        skip.zero_grad()
        skip(x, y).backward(dout)

    line: dict = {"module": "SequentialSkipConnection(8, 'residual') + feedforward(64)", "shape": [rows, t, f],
                  "hidden": hidden, "repeats": repeats}
    for route in routes:
        os.environ[SWITCH] = ROUTES[route]
        line[f"forward_ms_{route}"] = measure(forward, repeats)
        line[f"forward_backward_ms_{route}"] = measure(both, repeats)
    print(json.dumps(line), flush=True)
    if "on" not in routes:
        return
    norm, up, _, _, down = skip._layers[1]
    p = [q.detach() for q in (norm.weight, norm.bias, up.weight, up.bias, down.weight, down.bias)]
    lib, n = hip.load(), rows * t
    xd, stream = y.detach(), torch.cuda.current_stream().cuda_stream
    out, dx = torch.empty_like(xd), torch.empty_like(xd)
    grads = [torch.empty_like(q) for q in p]
    workspace = torch.empty(hip.feedforward_workspace_floats(n, f, hidden), device=DEV)
    ptr = lambda q: None if q is None else q.data_ptr()  # noqa: E731

    def backward(dx, grads, workspace):
        status = lib.rl8_feedforward_backward_f32(ptr(xd), ptr(dout), ptr(p[0]), ptr(p[1]), norm.eps, ptr(p[2]), ptr(p[3]),
                                                  ptr(p[4]), n, f, hidden, 1, ptr(dx), *(ptr(g) for g in grads),
                                                  ptr(workspace), stream)
        assert status == 0, status

    def forward_kernel():
        status = lib.rl8_feedforward_f32(ptr(xd), ptr(p[0]), ptr(p[1]), norm.eps, ptr(p[2]), ptr(p[3]), ptr(p[4]),
                                         ptr(p[5]), n, f, hidden, 1, ptr(out), stream)
        assert status == 0, status

    row_bytes = n * f * 4
    kernels = {
        "forward": roofline(event_us(forward_kernel, repeats), 2 * row_bytes, n * 2 * f * hidden),
        "dx": roofline(event_us(lambda: backward(dx, [None] * 6, None), repeats), 3 * row_bytes, n * 3 * f * hidden),
        "weight_gradients_and_sum": roofline(event_us(lambda: backward(None, [None, None] + grads[2:], workspace),
                                                      repeats), 2 * row_bytes, n * 4 * f * hidden),
    }
    whole = event_us(lambda: backward(dx, grads, workspace), repeats)
    print(json.dumps({"kernels": kernels, "backward_entry_us": whole, "rows": n, "f": f, "hidden": hidden,
                      "workspace_MiB": round(workspace.numel() * 4 / 2**20, 2)}), flush=True)


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
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--skip-algorithm", action="store_true")
    ap.add_argument("--routes", default="on,off")
    ap.add_argument("--label", default="this-commit")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--minibatches", type=int, default=1)
    args = ap.parse_args()
    routes = [r for r in args.routes.split(",") if r]
    assert all(r in ROUTES for r in routes), routes
    if not args.skip_block:
        block_lines(routes, args.repeats)
    if not args.skip_algorithm:
        algorithm_lines(routes, args.label, args.num_envs, args.horizon, args.minibatches, args.repeats)


if __name__ == "__main__":
    main()
