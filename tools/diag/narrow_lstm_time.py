"""Time the narrow LSTMs (hidden width 64 / 128, lstm_narrow_kernels.hip) against the same LSTMs on the eager module.

    python tools/diag/narrow_lstm_time.py [--reps 5] [--no-algo]

For each (H, d_in) at a rollout step (65536 sequences x L = 1) and a training pass (2^19 sequences x L = 4): the fused
forward, the fused forward + backward (through autograd, as a model runs it), and both again with
``fused_lstm.ENABLED = False``, in microseconds (torch events on the launch stream, median of the repetitions), with
the fused runs' achieved bytes/s against the algorithmic bytes per row-step (computed from the shapes below).  Then one
collect() + step() of RecurrentAlgorithmConfig(num_envs=65536, horizon=256, hidden_size=64) on DiscreteDummyEnv, fused
against eager.

Algorithmic bytes per row-step (fp32): forward x_t, h_t written (d_in + H floats; the states once per sequence are
left out); a training forward also writes the gates and the cell state (+ 5H); the backward reads dL/dh_t, the gates,
c_t and c_{t-1} (7H), writes dz (4H) and reads dz back with h_{t-1} and x_t for the weight gradient (5H + d_in).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch
import torch.nn as nn

from rl8_amd.nn import fused_lstm

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=5)
p.add_argument("--no-algo", action="store_true")
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


def run_lstm(lstm, x, h0, c0):
    out = fused_lstm.lstm_forward(lstm, x, h0, c0)
    if out is not None:
        return out[0]
    with torch.backends.cudnn.flags(enabled=False):
        return lstm(x, (h0[None], c0[None]))[0]


def measure(lstm, x, h0, c0, enabled):
    fused_lstm.ENABLED = enabled

    def forward():
        with torch.no_grad():
            run_lstm(lstm, x, h0, c0)

    def train():
        run_lstm(lstm, x, h0, c0).sum().backward()

    try:
        return timed(forward), timed(train)
    finally:
        fused_lstm.ENABLED = True


print("| H | d_in | B x L | fused fwd us | eager fwd us | fused fwd+bwd us | eager fwd+bwd us | fwd GB/s | fwd+bwd GB/s |")
print("|---|---|---|---|---|---|---|---|---|")
for hidden in (64, 128):
    for d_in in (1, 4, 16):
        torch.manual_seed(0)
        lstm = nn.LSTM(d_in, hidden, batch_first=True).to(dev)
        for b, l in ((65536, 1), (1 << 19, 4)):
            x = torch.randn(b, l, d_in, device=dev)
            h0 = torch.randn(b, hidden, device=dev) * 0.5
            c0 = torch.randn(b, hidden, device=dev)
            ff, ft = measure(lstm, x, h0, c0, True)
            ef, et = measure(lstm, x, h0, c0, False)
            rows = b * l
            fwd_bytes = 4 * rows * (d_in + hidden)
            train_bytes = 4 * rows * (d_in + hidden + 5 * hidden + 7 * hidden + 4 * hidden + 5 * hidden + d_in)
            print(f"| {hidden} | {d_in} | {b} x {l} | {ff:.0f} | {ef:.0f} | {ft:.0f} | {et:.0f} | "
                  f"{fwd_bytes / ff / 1e3:.0f} | {train_bytes / ft / 1e3:.0f} |", flush=True)
            del x, h0, c0

if not args.no_algo:
    from rl8_amd import RecurrentAlgorithmConfig
    from rl8_amd.env import DiscreteDummyEnv

    for enabled in (True, False):
        fused_lstm.ENABLED = enabled
        try:
            torch.manual_seed(0)
            algo = RecurrentAlgorithmConfig(num_envs=65536, horizon=256,
                                            model_config={"hidden_size": 64}).build(DiscreteDummyEnv)
            algo.collect()
            algo.step()  # (warm-up)
            ts = []
            for _ in range(max(1, args.reps // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                algo.collect()
                algo.step()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            print(f"collect()+step() hidden 64, 65536 envs x 256: {'fused' if enabled else 'eager'} "
                  f"{sorted(ts)[len(ts) // 2] * 1e3:.1f} ms", flush=True)
            del algo
        finally:
            fused_lstm.ENABLED = True
