"""Time the narrow LSTMs (hidden width 64 / 128, lstm_narrow_kernels.hip) against the same LSTMs on the eager module.

    python tools/diag/narrow_lstm_time.py [--reps 5] [--no-algo] [--layers N] [--fused-only] [--only train|rollout]
                                          [--heads]

For each (H, d_in) at a rollout step (65536 sequences x L = 1) and a training pass (2^19 sequences x L = 4): the fused
forward, the fused forward + backward (through autograd, as a model runs it), and both again with
``fused_lstm.ENABLED = False``, in microseconds (torch events on the launch stream, median of the repetitions), with
the fused runs' achieved bytes/s against the algorithmic bytes per row-step (computed from the shapes below).  Then one
collect() + step() of RecurrentAlgorithmConfig(num_envs=65536, horizon=256, hidden_size=64) on DiscreteDummyEnv, fused
against eager.

Algorithmic bytes per row-step (fp32): forward x_t, h_t written (d_in + H floats; the states once per sequence are
left out); a training forward also writes the gates and the cell state (+ 5H); the backward reads dL/dh_t, the gates,
c_t and c_{t-1} (7H), writes dz (4H) and reads dz back with h_{t-1} and x_t for the weight gradient (5H + d_in).

``--layers N`` (N >= 2) times the stacked LSTM (``fused_lstm.lstm_stack_forward``, lstm_narrow_stack_* kernels) in the
same way, printing median [min-max] of the repetitions, and the collect() + step() with ``num_layers=N``.  An upper
layer's algorithmic bytes per row-step: forward 2H (the lower layer's h_t read, its own written), training + 5H, the
backward as above with an H-wide x (7H + 4H + 6H) plus dx (dz read, dx written: 5H).  ``--fused-only`` leaves the
eager runs and the algorithm out and ``--only`` keeps one of the two shapes: for a kernel trace
(``rocprofv3 --kernel-trace --stats -- python tools/diag/narrow_lstm_time.py --layers 2 --fused-only --only train``).

``--heads`` times the default discrete and continuous recurrent MODELS instead of the bare LSTM -- LSTM (``--layers``)
plus output heads, through ``model(batch, states)`` alone, so the same file runs on any commit that has the models:
forward (no grad) and forward + backward at the two shapes, median [min-max]; then collect() + step() for hidden 64 and
128 at 65536 and 8192 environments x 256 steps on DiscreteDummyEnv, median [min-max] of wall time.
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
p.add_argument("--layers", type=int, default=1)
p.add_argument("--fused-only", action="store_true")
p.add_argument("--only", choices=("train", "rollout"))
p.add_argument("--heads", action="store_true")
args = p.parse_args()
dev = torch.device("cuda:0")
SHAPES = [s for name, s in (("rollout", (65536, 1)), ("train", (1 << 19, 4))) if args.only in (None, name)]


def timed(fn):
    """Median of the repetitions; for a stack (median, min, max)."""
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
    ts.sort()
    return ts[len(ts) // 2] if args.layers == 1 else (ts[len(ts) // 2], ts[0], ts[-1])


def run_lstm(lstm, x, h0, c0):
    if lstm.num_layers > 1:  # h0 / c0 [B, layers, H]
        out = fused_lstm.lstm_stack_forward(lstm, x, h0, c0)
        if out is not None:
            return out[0]
        with torch.backends.cudnn.flags(enabled=False):
            return lstm(x, (h0.permute(1, 0, 2).contiguous(), c0.permute(1, 0, 2).contiguous()))[0]
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


def cell(t):
    return f"{t[0]:.0f} [{t[1]:.0f}-{t[2]:.0f}]" if t else "-"


def spread(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:.0f} [{ts[0]:.0f}-{ts[-1]:.0f}]"


def times(fn):
    """Every repetition's time in us (after one warm-up call)."""
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
    return ts


def heads_mode():
    from rl8_amd import RecurrentAlgorithmConfig
    from rl8_amd.data import DataKeys
    from rl8_amd.env import ContinuousDummyEnv, DiscreteDummyEnv
    from rl8_amd.models_recurrent import DefaultContinuousRecurrentModel, DefaultDiscreteRecurrentModel
    from rl8_amd.tensordict import TensorDict

    n = args.layers
    print(f"default recurrent models, layers = {n}; times in us: median [min-max] of {args.reps} repetitions")
    print("| model | H | B x L | forward | forward + backward |")
    print("|---|---|---|---|---|")
    for name, model_cls, env_cls in (("discrete", DefaultDiscreteRecurrentModel, DiscreteDummyEnv),
                                     ("continuous", DefaultContinuousRecurrentModel, ContinuousDummyEnv)):
        env = env_cls(4, 8, device=str(dev))
        for hidden in (64, 128):
            torch.manual_seed(0)
            model = model_cls(env.observation_spec, env.action_spec, hidden_size=hidden, num_layers=n).to(dev)
            for b, l in SHAPES:
                batch = TensorDict({DataKeys.OBS: torch.randn(b, l, 1, device=dev)}, batch_size=[b, l])
                # (only [:, 0] of the states is read: one step's worth, expanded over l)
                states = TensorDict(
                    {DataKeys.HIDDEN_STATES: (torch.randn(b, 1, n, hidden, device=dev) * 0.5).expand(b, l, n, hidden),
                     DataKeys.CELL_STATES: torch.randn(b, 1, n, hidden, device=dev).expand(b, l, n, hidden)},
                    batch_size=[b, l])

                def forward():
                    with torch.no_grad():
                        model(batch, states)

                def train():
                    model.zero_grad(set_to_none=True)
                    feats, _ = model(batch, states)
                    (sum(v.sum() for v in feats.values()) + model.value_function().sum()).backward()

                print(f"| {name} | {hidden} | {b} x {l} | {spread(times(forward))} | {spread(times(train))} |", flush=True)
                del batch, states
            del model
    if args.no_algo:
        return
    for hidden in (64, 128):
        for envs in (65536, 8192):
            torch.manual_seed(0)
            algo = RecurrentAlgorithmConfig(num_envs=envs, horizon=256,
                                            model_config={"hidden_size": hidden, "num_layers": n}).build(DiscreteDummyEnv)
            algo.collect()
            algo.step()  # (warm-up)
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                algo.collect()
                algo.step()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            print(f"collect()+step() hidden {hidden}, {n} layer(s), {envs} envs x 256: "
                  f"{ts[len(ts) // 2]:.1f} ms [{ts[0]:.1f}-{ts[-1]:.1f}]", flush=True)
            del algo


if args.heads:
    heads_mode()
    sys.exit(0)

if args.layers == 1:
    print("| H | d_in | B x L | fused fwd us | eager fwd us | fused fwd+bwd us | eager fwd+bwd us | fwd GB/s | fwd+bwd GB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for hidden in (64, 128):
        for d_in in (1, 4, 16):
            torch.manual_seed(0)
            lstm = nn.LSTM(d_in, hidden, batch_first=True).to(dev)
            for b, l in SHAPES:
                x = torch.randn(b, l, d_in, device=dev)
                h0 = torch.randn(b, hidden, device=dev) * 0.5
                c0 = torch.randn(b, hidden, device=dev)
                ff, ft = measure(lstm, x, h0, c0, True)
                ef, et = (float("nan"),) * 2 if args.fused_only else measure(lstm, x, h0, c0, False)
                rows = b * l
                fwd_bytes = 4 * rows * (d_in + hidden)
                train_bytes = 4 * rows * (d_in + hidden + 5 * hidden + 7 * hidden + 4 * hidden + 5 * hidden + d_in)
                print(f"| {hidden} | {d_in} | {b} x {l} | {ff:.0f} | {ef:.0f} | {ft:.0f} | {et:.0f} | "
                      f"{fwd_bytes / ff / 1e3:.0f} | {train_bytes / ft / 1e3:.0f} |", flush=True)
                del x, h0, c0
else:
    n = args.layers
    print(f"layers = {n}; times in us: median [min-max] of {args.reps} repetitions")
    print("| H | d_in | B x L | fused fwd | eager fwd | fused fwd+bwd | eager fwd+bwd | fwd GB/s | fwd+bwd GB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for hidden in (64, 128):
        for d_in in (1, 16):
            torch.manual_seed(0)
            lstm = nn.LSTM(d_in, hidden, num_layers=n, batch_first=True).to(dev)
            for b, l in SHAPES:
                x = torch.randn(b, l, d_in, device=dev)
                h0 = torch.randn(b, n, hidden, device=dev) * 0.5
                c0 = torch.randn(b, n, hidden, device=dev)
                ff, ft = measure(lstm, x, h0, c0, True)
                ef, et = (None, None) if args.fused_only else measure(lstm, x, h0, c0, False)
                rows = b * l
                fwd_bytes = 4 * rows * (d_in + hidden + (n - 1) * 2 * hidden)
                train_bytes = 4 * rows * (22 * hidden + 2 * d_in + (n - 1) * 29 * hidden)
                print(f"| {hidden} | {d_in} | {b} x {l} | {cell(ff)} | {cell(ef)} | {cell(ft)} | {cell(et)} | "
                      f"{fwd_bytes / ff[0] / 1e3:.0f} | {train_bytes / ft[0] / 1e3:.0f} |", flush=True)
                del x, h0, c0

if not args.no_algo and not args.fused_only:
    from rl8_amd import RecurrentAlgorithmConfig
    from rl8_amd.env import DiscreteDummyEnv

    for enabled in (True, False):
        fused_lstm.ENABLED = enabled
        try:
            torch.manual_seed(0)
            model_config = {"hidden_size": 64} if args.layers == 1 else {"hidden_size": 64, "num_layers": args.layers}
            algo = RecurrentAlgorithmConfig(num_envs=65536, horizon=256,
                                            model_config=model_config).build(DiscreteDummyEnv)
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
            spread = "" if args.layers == 1 else f" [{min(ts) * 1e3:.1f}-{max(ts) * 1e3:.1f}], {args.layers} layers"
            print(f"collect()+step() hidden 64, 65536 envs x 256: {'fused' if enabled else 'eager'} "
                  f"{sorted(ts)[len(ts) // 2] * 1e3:.1f} ms{spread}", flush=True)
            del algo
        finally:
            fused_lstm.ENABLED = True
