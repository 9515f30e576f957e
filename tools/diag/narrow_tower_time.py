"""Time the narrow towers (hidden width 64 / 128, mlp_narrow_kernels.hip) against the same towers on the eager modules.

    python tools/diag/narrow_tower_time.py [--rows 1048576,33554432] [--reps 5]

For each (H, d_in, n_out) and row count: the fused forward, the fused forward + backward (through autograd, as a
model runs it), and both again with ``fused_mlp.ENABLED = False``, in microseconds (torch events on the launch stream,
median of the repetitions), plus the layer-2 rate of the fused runs as a fraction of the 157 TFLOP/s fp32 matrix peak
(forward: one H x H product per row; forward + backward: four -- the forward, its recomputation, dh1 and dW2).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch
import torch.nn as nn

from rl8_amd.nn import fused_mlp

PEAK = 157e12
p = argparse.ArgumentParser()
p.add_argument("--rows", default=f"{1 << 20},{1 << 25}")
p.add_argument("--reps", type=int, default=5)
p.add_argument("--shapes", default="64x1x2,64x4x1,64x16x8,128x1x2,128x4x1,128x16x8")
args = p.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def measure(trunk, head, x, enabled):
    fused_mlp.ENABLED = enabled

    def forward():
        with torch.no_grad():
            out = fused_mlp.tower_forward(trunk, [head], x)
            return head(trunk(x)) if out is None else out

    def train():
        out = fused_mlp.tower_forward(trunk, [head], x)
        out = head(trunk(x)) if out is None else out
        out.sum().backward()

    try:
        return timed(forward), timed(train)
    finally:
        fused_mlp.ENABLED = True


print(f"{'H':>4} {'d_in':>4} {'n_out':>5} {'rows':>9} | {'fwd us':>10} {'eager':>10} {'x':>5} {'peak':>5} | "
      f"{'fwd+bwd us':>10} {'eager':>10} {'x':>5} {'peak':>5}")
for rows in (int(r) for r in args.rows.split(",")):
    for shape in args.shapes.split(","):
        h, d_in, n_out = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        trunk = nn.Sequential(nn.Sequential(nn.Linear(d_in, h), nn.ReLU(), nn.Linear(h, h)), nn.ReLU()).to(dev)
        head = nn.Linear(h, n_out).to(dev)
        x = torch.randn(rows, d_in, device=dev)
        f_fwd, f_train = measure(trunk, head, x, True)
        e_fwd, e_train = measure(trunk, head, x, False)
        flop = 2.0 * rows * h * h
        print(f"{h:>4} {d_in:>4} {n_out:>5} {rows:>9} | {f_fwd:>10.1f} {e_fwd:>10.1f} {e_fwd / f_fwd:>5.2f} "
              f"{flop / (f_fwd * 1e-6) / PEAK:>5.2f} | {f_train:>10.1f} {e_train:>10.1f} {e_train / f_train:>5.2f} "
              f"{4 * flop / (f_train * 1e-6) / PEAK:>5.2f}", flush=True)
        del x
        torch.cuda.empty_cache()
