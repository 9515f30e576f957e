"""Time the narrow LSTMs' input-gradient kernel (rl8_lstm_narrow_input_grad_f32) and the recurrent trading model.

    python tools/diag/lstm_input_grad_time.py [--reps 9] [--no-algo]

1. The kernel alone at B x L = 2^20 row-steps, H = 64 / 128, d_in = 4 / 16, on gate gradients a backward through
   time left in its workspace layout (random values: the kernel's time does not depend on them): microseconds
   (torch events on the launch stream, median [min-max] of the repetitions after a warm-up) and achieved bytes/s
   against the algorithmic bytes per row-step, 4 (4H + d_in): dz read once, dx written once. Beside it, in the same
   run, a device-to-device copy of the same dz (torch ``copy_``: 2 x the bytes), as the streaming rate this machine
   gives a plain kernel at that footprint. dz is 1 / 2 GiB, several times the last-level cache.
2. One ``step()`` of ``RecurrentAlgorithmConfig(num_envs=65536, horizon=128, model_cls=LSTMTrader)`` on AlgoTrading,
   fused (one node: LSTM + heads + dx) against ``fused_lstm.ENABLED = False`` (the ``nn.LSTM`` module), wall time
   around a device synchronise, median [min-max]; and the ``hip.timer`` share of the input-gradient launch.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from rl8_amd import hip
from rl8_amd.nn import fused_lstm

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=9)
p.add_argument("--no-algo", action="store_true")
args = p.parse_args()
dev = torch.device("cuda:0")


def times(fn):
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
    return sorted(ts)


def spread(ts, unit=""):
    return f"{ts[len(ts) // 2]:.0f} [{ts[0]:.0f}-{ts[-1]:.0f}]{unit}"


rows = 1 << 20
lib = hip.load()
print(f"input gradient at {rows} row-steps; us: median [min-max] of {args.reps}")
print("| H | d_in | kernel us | GB/s (4 (4H + d_in) B per row-step) | copy of dz us | copy GB/s (2 x dz) |")
print("|---|---|---|---|---|---|")
for hidden in (64, 128):
    dz = torch.randn(rows, 4 * hidden, device=dev)
    other = torch.empty_like(dz)
    copy = times(lambda: other.copy_(dz))
    del other
    for d_in in (4, 16):
        w_ih = torch.randn(4 * hidden, d_in, device=dev) * 0.1
        dx = torch.empty(rows, 1, d_in, device=dev)

        def launch():
            hip._check(lib.rl8_lstm_narrow_input_grad_f32(dz.data_ptr(), rows, 1, d_in, w_ih.data_ptr(), hidden,
                                                          dx.data_ptr(), hip._stream()), "rl8_lstm_narrow_input_grad_f32")

        ts = times(launch)
        want = dz[:4096].double() @ w_ih.double()
        assert float((dx[:4096, 0].double() - want).abs().max()) < 1e-4 * float(want.abs().max())
        nbytes = 4 * rows * (4 * hidden + d_in)
        print(f"| {hidden} | {d_in} | {spread(ts)} | {nbytes / ts[len(ts) // 2] / 1e3:.0f} | {spread(copy)} | "
              f"{2 * dz.numel() * 4 / copy[len(copy) // 2] / 1e3:.0f} |", flush=True)
    del dz

if not args.no_algo:
    from rl8_amd import RecurrentAlgorithmConfig
    from rl8_amd.envs import AlgoTrading, LSTMTrader

    for enabled in (True, False):
        torch.manual_seed(0)
        algo = RecurrentAlgorithmConfig(num_envs=1 << 16, horizon=128, model_cls=LSTMTrader).build(AlgoTrading)
        algo.collect()
        fused_lstm.ENABLED = enabled
        try:
            algo.step()  # (warm-up)
            ts = []
            for _ in range(max(3, args.reps // 3)):
                algo.collect()  # (step() clears the buffer; only step() is timed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                algo.step()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            label = "fused" if enabled else "eager"
            print(f"LSTMTrader step() on AlgoTrading, 65536 envs x 128: {label} {spread(sorted(ts), ' ms')}", flush=True)
            if enabled:
                algo.collect()
                hip.timer.reset()
                hip.timer.enabled = True
                algo.step()
                summary = hip.timer.summary()
                hip.timer.enabled = False
                for name in ("lstm_narrow_forward", "lstm_narrow_backward", "lstm_narrow_reduce", "lstm_narrow_input_grad",
                             "gather_sequences", "gather_minibatch"):
                    if name in summary:
                        s = summary[name]
                        print(f"  {name}: {s['launches']} launches, {s['total_ms']:.2f} ms in all", flush=True)
        finally:
            fused_lstm.ENABLED = True
        del algo
