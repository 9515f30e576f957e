"""Per-call time of the sixteen-wave weight-gradient kernels at the bench's shapes -- rl8_mlp_wgrad_gate_bits_f32 (d_in 1,
one output and exact pair) and rl8_mlp_wgrad_fused_split_f32 (5 x 3) at 2^23 rows, rl8_lstm_wgrad_f16_f32 at 2^21
row-steps -- for A/B runs of what is read once per process: one library (RL8_AMD_LIBRARY) and one RL8_WGRAD_PHASES
value per process, both from the environment; the caller alternates them (profiles/wgrad_phases_ab.txt).  Prints one
line, "AB " + JSON: ms per call, HIP events around 10 calls, median of 5 such groups.

    python tools/diag/wgrad_phases_microbench.py TAG [--only=gate_n1 --only=gate_pair --only=fused_5x3 --only=lstm] [--small]

--small: 2^20 rows and a few calls, the target of tools/diag/pmc_sq_counters.sh's counter passes."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from rl8_amd import hip

tag = sys.argv[1]
small = "--small" in sys.argv
only = [a.split("=")[1] for a in sys.argv if a.startswith("--only=")]
lib, dev = hip.load(), torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
M = 1 << 20 if small else 1 << 23
ML = 1 << 20 if small else 1 << 21
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = torch.cuda.current_stream().cuda_stream
H = 256


def rn(*shape, scale=1.0):
    return torch.randn(*shape, device=dev, generator=g) * scale


ws = torch.empty(int(lib.rl8_mlp_wgrad_workspace_bytes()) // 4, device=dev)
ws[-64:].zero_()
dw = torch.empty(4 * H * H, device=dev)
max_rows = int(lib.rl8_mlp_backward_max_rows())
w2, b2 = rn(H, H, scale=1 / 16), rn(H, scale=0.1)
calls = {}


def gate(n_out):
    x, w1, b1, w3 = rn(M, 1, scale=3.0), rn(H, 1, scale=0.5), rn(H, scale=0.5), rn(n_out, H, scale=1 / 16)
    g0 = rn(M) / M
    dout = g0[:, None].contiguous() if n_out == 1 else torch.stack([g0, -g0], dim=1).contiguous()
    gate2 = torch.randint(-(1 << 31), (1 << 31) - 1, (M, 8), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    small_ = torch.empty(max_rows * int(lib.rl8_mlp_backward_partial_floats(1, n_out)), device=dev)
    keep = (x, w1, b1, w3, dout, gate2, small_)

    def call():
        s = lib.rl8_mlp_wgrad_gate_bits_f32(p(gate2), p(dout), p(x), p(w1), p(b1), p(w2), p(b2), p(w3), M, 1, n_out, p(ws), p(dw),
                                            p(small_), stream)
        assert s == 0, s
    call.keep = keep
    return call


def fused(d_in, n_out):
    x, w1, b1, w3 = rn(M, d_in, scale=3.0), rn(H, d_in, scale=0.5), rn(H, scale=0.5), rn(n_out, H, scale=1 / 16)
    dout = rn(M, n_out) / M
    h2 = torch.relu(rn(M, H))
    small_ = torch.empty(max_rows * int(lib.rl8_mlp_backward_partial_floats(d_in, n_out)), device=dev)

    def call():
        s = lib.rl8_mlp_wgrad_fused_split_f32(p(h2), p(dout), p(x), p(w1), p(b1), p(w3), M, d_in, n_out, p(ws), p(dw), p(small_),
                                              stream)
        assert s == 0, s
    call.keep = (x, w1, b1, w3, dout, h2, small_)
    return call


def lstm():
    m, d_in = ML, 1
    dz = rn(m, 4 * H) / m
    h = torch.tanh(rn(m, H))
    x = rn(m, d_in, scale=3.0)
    dzb = dz.abs().max().reshape(1)
    hb = torch.ones(1, device=dev)
    sums = torch.empty(4 * 256 * H * (d_in + 1), device=dev)
    rows = C.c_int(0)

    def call():
        s = lib.rl8_lstm_wgrad_f16_f32(p(dz), 4 * H, p(dzb), p(h), H, p(hb), m, p(ws), p(dw), 0, p(x), d_in, p(sums), C.byref(rows),
                                       stream)
        assert s == 0, s
    call.keep = (dz, h, x, dzb, hb, sums)
    return call


builders = {"gate_n1": lambda: gate(1), "gate_pair": lambda: gate(2), "fused_5x3": lambda: fused(5, 3), "lstm": lstm}
out = {"tag": tag, "phases": os.environ.get("RL8_WGRAD_PHASES", ""), "lib": os.path.basename(os.environ.get("RL8_AMD_LIBRARY", "tree"))}
reps = 3 if small else 10
for name, build in builders.items():
    if only and name not in only:
        continue
    call = build()
    for _ in range(2 if small else 5):
        call()
    torch.cuda.synchronize()
    if not small:  # clocks up
        t_end = time.time() + 0.5
        while time.time() < t_end:
            call()
            torch.cuda.synchronize()
    rounds = []
    for _ in range(1 if small else 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) / reps)
    out[name] = round(sorted(rounds)[len(rounds) // 2], 4)
    del call
    torch.cuda.empty_cache()
print("AB " + json.dumps(out), flush=True)
