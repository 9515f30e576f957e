"""``CrossAttention`` and ``SelfAttention`` on the streaming attention kernels (``RL8_AMD_LONG_ATTENTION=1``) against the
module route (unset), after ``tools/attention_wide_ab.py`` (DESIGN.md §6 rules: wall time around a synchronise, median
[min-max] of the repeats after two warm-up calls per route, one process, the routes alternating call by call).

    python tools/attention_long_ab.py [--repeats 5] > profiles/attention_long_ab.txt

One JSON line per shape -- ``CrossAttention(64, num_heads=2)`` with q ``[4096, 16, 64]`` over kv ``[4096, 512, 64]`` (a
Perceiver's shape: one strip of queries, four lanes over the keys) and ``SelfAttention(64, num_heads=2)`` on
``[2048, 256, 64]``, both under a window mask: forward and forward + backward per route, the peak of
``torch.cuda.max_memory_allocated()`` over a forward + backward per route, and the per-launch microseconds of the long
entries from ``hip.timer`` (the backward entry is its two kernels together).
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
from rl8_amd.nn import CrossAttention, SelfAttention  # noqa: E402

DEV = "cuda"
SWITCH = "RL8_AMD_LONG_ATTENTION"
ROUTES = (("long", True), ("module", False))
#: (module, embed, heads, B, Tq, Tk)
SHAPES = (("CrossAttention", 64, 2, 4096, 16, 512), ("SelfAttention", 64, 2, 2048, 256, 256))


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


def measure(fn, repeats: int) -> dict[str, dict[str, float]]:
    """Per route: two warm-up calls, then ``repeats`` timed calls, one of each route in turn."""
    for _, on in ROUTES:
        set_route(on)
        for _ in range(2):  # warm-up: allocator, code objects, rocBLAS
            fn()
    ms: dict[str, list[float]] = {route: [] for route, _ in ROUTES}
    for _ in range(repeats):
        for route, on in ROUTES:
            set_route(on)
            ms[route].append(timed(fn))
    return {route: {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}
            for route, x in ms.items()}


def shape_line(kind: str, embed: int, heads: int, b: int, tq: int, tk: int, repeats: int) -> dict:
    torch.manual_seed(0)
    layer = (CrossAttention if kind == "CrossAttention" else SelfAttention)(embed, num_heads=heads).to(DEV)
    xs = [torch.randn(b, t, embed, device=DEV, requires_grad=True) for t in ((tq, tk) if kind == "CrossAttention" else (tq,))]
    padding = torch.arange(tk, device=DEV).expand(b, tk) < (torch.arange(b, device=DEV) % tk).unsqueeze(1)
    dout = torch.randn(b, tq, embed, device=DEV)

    def forward():
        with torch.no_grad():
            layer(*xs, key_padding_mask=padding)

    def both():
        for x in xs:
            x.grad = None
        layer.zero_grad()
        layer(*xs, key_padding_mask=padding).backward(dout)

    line: dict = {"module": f"{kind}({embed}, num_heads={heads})", "q": [b, tq, embed], "kv": [b, tk, embed],
                  "repeats": repeats}
    for what, fn in (("forward", forward), ("forward_backward", both)):
        for route, figures in measure(fn, repeats).items():
            line[f"{what}_ms_{route}"] = figures
    for route, on in ROUTES:
        set_route(on)
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
    assert set(line["kernel_us"]) == {"attention_long", "attention_long_backward"}, line["kernel_us"]
    for what in ("forward", "forward_backward"):
        line[f"{what}_long_median_below_module_min"] = (line[f"{what}_ms_long"]["median"]
                                                         < line[f"{what}_ms_module"]["min"])
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert os.environ.get("RL8_AMD_ATTENTION_KERNELS", "1") != "0"
    for shape in SHAPES:
        print(json.dumps(shape_line(*shape, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
