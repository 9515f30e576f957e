"""The feedforward block of wide attention layers on the MFMA feedforward kernels (``RL8_AMD_WIDE_FEEDFORWARD=1``)
against the torch modules (unset: what runs without the switch), after ``tools/attention_wide_ab.py`` (DESIGN.md §6
rules: wall time around a synchronise, one process, two warm-up calls per route, then the routes ALTERNATE, one timed
call each per repeat; median [min-max] of the repeats).

    python tools/feedforward_wide_ab.py [--repeats 7] > profiles/feedforward_wide_ab.txt

One JSON line per shape -- ``SelfAttention(64, num_heads=2, skip_kind="residual")`` on ``[16384, 33, 64]`` (a block of
64 features through 128 hidden units), ``SelfAttention(128, num_heads=2, skip_kind="residual")`` and
``SelfAttention(128, num_heads=2)`` (the default "cat" skip, whose ``Linear`` brings the block's input back to 128
features) on ``[4096, 128, 128]``, all under a window mask: forward and forward + backward per
route, the peak of ``torch.cuda.max_memory_allocated()`` over a forward + backward per route, the per-launch
microseconds of the wide entries from ``hip.timer`` (the backward entry is its kernels together), and the fraction of
the fp32-MFMA rate of ``mfma_tile.hip.h`` (155 TFLOP/s) that the issued matrix instructions reach, counted over the
padded sizes.  The attention core runs on whatever the environment selects, the same on both routes.
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
SWITCH = "RL8_AMD_WIDE_FEEDFORWARD"
MFMA_FP32_FLOPS = 155e12
#: (embed, heads, skip_kind, B, T)
SHAPES = ((64, 2, "residual", 16384, 33), (128, 2, "residual", 4096, 128), (128, 2, "cat", 4096, 128))


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
    """``fn`` on both routes, alternating: ``{"wide": {...}, "module": {...}}``."""
    routes = (("module", False), ("wide", True))
    for _, on in routes:  # warm-up: allocator, code objects, rocBLAS
        set_route(on)
        fn()
        fn()
    ms: dict[str, list[float]] = {name: [] for name, _ in routes}
    for _ in range(repeats):
        for name, on in routes:
            set_route(on)
            ms[name].append(timed(fn))
    set_route(False)
    return {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for name, v in ms.items()}


def mfma_flops(rows: int, f: int, hidden: int) -> dict[str, float]:
    """Flops of the matrix instructions one launch issues: products of [rows x fp] by [fp x hp] over the padded sizes,
    two in the forward, three in the dx kernel and four in the weight-gradient kernel."""
    lim = hip.feedforward_wide_limits()
    product = 2.0 * (-(-rows // lim.tile_rows) * lim.tile_rows) * (-(-f // 16) * 16) * (-(-hidden // lim.chunk) * lim.chunk)
    return {"feedforward_wide": 2 * product, "feedforward_wide_backward": 7 * product}


def shape_line(embed: int, heads: int, kind: str, b: int, t: int, repeats: int) -> dict:
    torch.manual_seed(0)
    layer = SelfAttention(embed, num_heads=heads, skip_kind=kind).to(DEV)
    up = layer.skip_connection._layers[1][1]
    f, hidden = up.in_features, up.out_features
    x = torch.randn(b, t, embed, device=DEV, requires_grad=True)
    padding = torch.arange(t, device=DEV).expand(b, t) < (torch.arange(b, device=DEV) % t).unsqueeze(1)
    with torch.no_grad():
        dout = torch.randn_like(layer(x, key_padding_mask=padding))

    def forward():
        with torch.no_grad():
            layer(x, key_padding_mask=padding)

    def both():
        x.grad = None
        layer.zero_grad()
        layer(x, key_padding_mask=padding).backward(dout)

    line: dict = {"module": f"SelfAttention({embed}, num_heads={heads}, skip_kind={kind!r})", "shape": [b, t, embed],
                  "block": {"f": f, "hidden": hidden, "inside": hip.feedforward_wide_supports(f, hidden)},
                  "repeats": repeats}
    for what, fn in (("forward", forward), ("forward_backward", both)):
        for route, figures in measure(fn, repeats).items():
            line[f"{what}_ms_{route}"] = figures
    for route, on in (("wide", True), ("module", False)):
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
    line["kernel_us"] = {n: round(s["avg_ms"] * 1e3, 2) for n, s in summary.items() if n.startswith("feedforward_wide")}
    line["mfma_rate_fraction"] = {n: round(flops / (line["kernel_us"][n] * 1e-6) / MFMA_FP32_FLOPS, 4)
                                  for n, flops in mfma_flops(b * t, f, hidden).items() if n in line["kernel_us"]}
    for what in ("forward", "forward_backward"):
        line[f"{what}_wide_median_below_module_min"] = (line[f"{what}_ms_wide"]["median"]
                                                         < line[f"{what}_ms_module"]["min"])
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    for embed, heads, kind, b, t in SHAPES:
        print(json.dumps(shape_line(embed, heads, kind, b, t, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
