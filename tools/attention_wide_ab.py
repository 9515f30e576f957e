"""``SelfAttention`` on the MFMA attention kernels (``RL8_AMD_WIDE_ATTENTION=1``) against the module route (unset), after
``tools/diag/attention_route_time.py`` (DESIGN.md §6 rules: wall time around a synchronise, median [min-max] of the
repeats after two warm-up calls, one process).

    python tools/attention_wide_ab.py [--repeats 5] > profiles/attention_wide_ab.txt

One JSON line per shape -- ``SelfAttention(64, num_heads=2)`` on ``[16384, 33, 64]`` and ``SelfAttention(128,
num_heads=2)`` on ``[4096, 128, 128]``, both under a window mask: forward and forward + backward per route, the peak of
``torch.cuda.max_memory_allocated()`` over a forward + backward per route, the per-launch microseconds of the wide
entries from ``hip.timer`` (the backward entry is its two kernels together), and the fraction of the fp32-MFMA rate of
``mfma_tile.hip.h`` (155 TFLOP/s) that the issued matrix instructions reach: tiles are 16 rows and 16-feature
columns, so the count is over the padded sizes.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl8_amd import hip  # noqa: E402
from rl8_amd.nn import SelfAttention  # noqa: E402

DEV = "cuda"
SWITCH = "RL8_AMD_WIDE_ATTENTION"
MFMA_FP32_FLOPS = 155e12
#: (embed, heads, B, T)
SHAPES = ((64, 2, 16384, 33), (128, 2, 4096, 128))


def set_route(on: bool) -> None:
    os.environ.pop(SWITCH, None)
    if on:
        os.environ[SWITCH] = "1"


def timed(fn) -> float:
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def measure(fn, repeats: int) -> dict[str, float]:
    for _ in range(2):  # warm-up: allocator, code objects, rocBLAS
        fn()
    ms = [timed(fn) for _ in range(repeats)]
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def mfma_flops(b: int, heads: int, t: int, d: int) -> dict[str, float]:
    """Flops of the matrix instructions one launch issues: products of [tp x dp] by [dp x tp] over the padded sizes, two
    in the forward, three in the dQ kernel, four in the dK/dV kernel."""
    tp, dp = -(-t // 16) * 16, -(-d // 16) * 16
    product = 2.0 * b * heads * tp * tp * dp
    return {"attention_wide": 2 * product, "attention_wide_backward": 7 * product}


def shape_line(embed: int, heads: int, b: int, t: int, repeats: int) -> dict:
    torch.manual_seed(0)
    layer = SelfAttention(embed, num_heads=heads).to(DEV)
    x = torch.randn(b, t, embed, device=DEV, requires_grad=True)
    padding = torch.arange(t, device=DEV).expand(b, t) < (torch.arange(b, device=DEV) % t).unsqueeze(1)
    dout = torch.randn(b, t, embed, device=DEV)

    def forward():
        with torch.no_grad():
            layer(x, key_padding_mask=padding)

    def both():
        x.grad = None
        layer.zero_grad()
        layer(x, key_padding_mask=padding).backward(dout)

    line: dict = {"module": f"SelfAttention({embed}, num_heads={heads})", "shape": [b, t, embed], "repeats": repeats}
    for route, on in (("wide", True), ("module", False)):
        set_route(on)
        line[f"forward_ms_{route}"] = measure(forward, repeats)
        line[f"forward_backward_ms_{route}"] = measure(both, repeats)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        both()
        torch.cuda.synchronize()
        line[f"peak_MiB_{route}"] = round(torch.cuda.max_memory_allocated() / 2**20, 1)
    set_route(True)
    hip.timer.reset()
    hip.timer.enabled = True
    try:
        both()
        summary = hip.timer.summary()
    finally:
        hip.timer.enabled = False
        set_route(False)
    line["kernel_us"] = {n: round(s["avg_ms"] * 1e3, 2) for n, s in summary.items() if n.startswith("attention")}
    line["mfma_rate_fraction"] = {n: round(f / (line["kernel_us"][n] * 1e-6) / MFMA_FP32_FLOPS, 4)
                                  for n, f in mfma_flops(b, heads, t, embed // heads).items() if n in line["kernel_us"]}
    for what in ("forward", "forward_backward"):
        line[f"{what}_wide_median_below_module_min"] = (line[f"{what}_ms_wide"]["median"]
                                                         < line[f"{what}_ms_module"]["min"])
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert os.environ.get("RL8_AMD_ATTENTION_KERNELS", "1") != "0"
    for embed, heads, b, t in SHAPES:
        print(json.dumps(shape_line(embed, heads, b, t, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
