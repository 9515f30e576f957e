"""Cases, inputs and runner of tests/test_wgrad_gate_bitwise_gpu.py, and the recorder of its fixture.

    python tests/golden/record_wgrad_gate_bitwise.py          (on a GPU, with the library whose bits are the reference)

writes tests/golden/wgrad_gate_bitwise.npz: per case the SHA-256 of the inputs, of dW2 and of the whole buffer of
partial rows (as the kernels left it: untouched words keep their fill), and dW2 itself for the cases named in
FULL_CASES.  A dW2 is 256 KiB and a buffer of partial rows up to 7 MiB; fifty cases of them do not fit a
committed file, so all but two cases are held to their digests -- which are equal exactly when every bit is.

The inputs come from numpy's frozen RandomState streams; their digest is in the fixture so that a change of the
stream shows as what it is.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "wgrad_gate_bitwise.npz")
HIDDEN = 256
FILL = 12345.0   # what partial rows and dW2 hold before a call
GUARD = 4096     # sentinel floats on either side of every buffer a kernel writes
SENTINEL = -7.75


def _gate_cases():
    out = []
    for d_in in (1, 5):
        for n_out in (1, 2):
            for m in (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097):
                out.append({"id": f"gate-d{d_in}-n{n_out}-m{m}", "kind": "gate", "m": m, "d_in": d_in, "n_out": n_out,
                            "planes": ""})
    # two segments of 2^23 rows: the second one adds to dW2 and to the partial rows
    out.append({"id": "gate-d1-n1-two-segments", "kind": "gate", "m": (1 << 23) + 17, "d_in": 1, "n_out": 1, "planes": ""})
    # the exact bf16 planes by request (unset above: the guard looks at dOut and lets the fp16 planes run)
    for n_out in (1, 2):
        out.append({"id": f"gate-d1-n{n_out}-m65-bf16", "kind": "gate", "m": 65, "d_in": 1, "n_out": n_out, "planes": "bf16"})
    # the widest inputs ask for their scalar operands at the wait, not a step ahead: a request path of its own
    out.append({"id": "gate-d6-n2-m65", "kind": "gate", "m": 65, "d_in": 6, "n_out": 2, "planes": ""})
    out.append({"id": "gate-d7-n1-m4097", "kind": "gate", "m": 4097, "d_in": 7, "n_out": 1, "planes": ""})
    out.append({"id": "fused-d1-n3-m17", "kind": "fused", "m": 17, "d_in": 1, "n_out": 3, "planes": ""})
    out.append({"id": "fused-d5-n2-m65", "kind": "fused", "m": 65, "d_in": 5, "n_out": 2, "planes": ""})
    out.append({"id": "loadh-d1-m17", "kind": "loadh", "m": 17, "d_in": 1, "n_out": 0, "planes": ""})
    out.append({"id": "loadh-d3-m65", "kind": "loadh", "m": 65, "d_in": 3, "n_out": 0, "planes": ""})
    return out


CASES = _gate_cases()
FULL_CASES = ("gate-d1-n1-m65", "gate-d5-n2-m4097")


def inputs(case: dict) -> dict[str, np.ndarray]:
    """The case's arrays (host), from a seed that depends on nothing but its id."""
    seed = int.from_bytes(hashlib.sha256(case["id"].encode()).digest()[:4], "little")
    rng = np.random.RandomState(seed)
    m, d_in, n_out = case["m"], case["d_in"], case["n_out"]
    f32 = np.float32
    a = {"x": (rng.standard_normal((m, d_in)) * 3.0).astype(f32)}
    if case["kind"] == "loadh":
        a["dz"] = (rng.standard_normal((m, 4 * HIDDEN)) / m).astype(f32)       # gate 1 of [m][4][256] rows is the operand
        a["h"] = np.tanh(rng.standard_normal((m, HIDDEN))).astype(f32)
        a["dz_bound"] = np.array([np.abs(a["dz"]).max()], dtype=f32)
        a["h_bound"] = np.array([1.0], dtype=f32)
        return a
    g0 = (rng.standard_normal(m) / m).astype(f32)
    if case["kind"] == "gate":
        a["dout"] = g0[:, None].copy() if n_out == 1 else np.stack([g0, -g0], axis=1).copy()
        a["gate2"] = rng.randint(0, 1 << 32, size=(m, 8), dtype=np.uint64).astype(np.uint32)
    else:
        a["dout"] = (rng.standard_normal((m, n_out)) / m).astype(f32)
        a["h2"] = np.maximum(rng.standard_normal((m, HIDDEN)), 0.0).astype(f32)
    a["w1"] = (rng.standard_normal((HIDDEN, d_in)) * 0.5).astype(f32)
    a["b1"] = (rng.standard_normal(HIDDEN) * 0.5).astype(f32)
    a["w2"] = (rng.standard_normal((HIDDEN, HIDDEN)) / 16.0).astype(f32)
    a["b2"] = (rng.standard_normal(HIDDEN) * 0.1).astype(f32)
    a["w3"] = (rng.standard_normal((n_out, HIDDEN)) / 16.0).astype(f32)
    return a


def digest(array: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def inputs_digest(arrays: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode())
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    return h.hexdigest()


class Fenced:
    """A device buffer with GUARD sentinel floats in front of and behind the part a kernel is given."""

    def __init__(self, torch, floats: int, fill: float | None, device):
        self.whole = torch.full((floats + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
        self.inner = self.whole[GUARD:GUARD + floats]
        if fill is not None:
            self.inner.fill_(fill)

    def intact(self) -> bool:
        front, back = self.whole[:GUARD], self.whole[GUARD + self.inner.numel():]
        return bool((front == SENTINEL).all().item()) and bool((back == SENTINEL).all().item())


def run(case: dict, arrays: dict[str, np.ndarray], workspace=None) -> dict[str, np.ndarray]:
    """One call of the case's entry point on cuda:0; dW2 and the partial rows (or column sums) as host arrays.
    `workspace`: a Fenced of rl8_mlp_wgrad_workspace_bytes() to reuse (its slabs are scratch; the last 64 words
    hold the guard's lifetime counters and must start zeroed)."""
    import torch

    from rl8_amd import hip

    lib, dev = hip.load(), torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in arrays.items()}
    m, d_in, n_out = case["m"], case["d_in"], case["n_out"]
    if workspace is None:
        workspace = new_workspace()
    dw = Fenced(torch, HIDDEN * HIDDEN, FILL, dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    before = os.environ.get("RL8_WGRAD_GATE_PLANES")
    try:
        if case["planes"]:
            os.environ["RL8_WGRAD_GATE_PLANES"] = case["planes"]
        else:
            os.environ.pop("RL8_WGRAD_GATE_PLANES", None)
        if case["kind"] == "loadh":
            rows = C.c_int(0)
            sums = Fenced(torch, 256 * HIDDEN * (d_in + 1), FILL, dev)
            status = lib.rl8_mlp_wgrad_f16_strided_f32(
                C.c_void_p(t["dz"].data_ptr() + 4 * HIDDEN), 4 * HIDDEN, p(t["dz_bound"]), p(t["h"]), HIDDEN, p(t["h_bound"]),
                m, p(workspace.inner), p(dw.inner), 0, p(t["x"]), d_in, p(sums.inner), C.byref(rows), stream)
            small = sums
        else:
            width = int(lib.rl8_mlp_backward_partial_floats(d_in, n_out))
            small = Fenced(torch, int(lib.rl8_mlp_backward_max_rows()) * width, FILL, dev)
            if case["kind"] == "gate":
                status = lib.rl8_mlp_wgrad_gate_bits_f32(
                    p(t["gate2"]), p(t["dout"]), p(t["x"]), p(t["w1"]), p(t["b1"]), p(t["w2"]), p(t["b2"]), p(t["w3"]),
                    m, d_in, n_out, p(workspace.inner), p(dw.inner), p(small.inner), stream)
            else:
                status = lib.rl8_mlp_wgrad_fused_split_f32(
                    p(t["h2"]), p(t["dout"]), p(t["x"]), p(t["w1"]), p(t["b1"]), p(t["w3"]), m, d_in, n_out,
                    p(workspace.inner), p(dw.inner), p(small.inner), stream)
        torch.cuda.synchronize()
    finally:
        if before is None:
            os.environ.pop("RL8_WGRAD_GATE_PLANES", None)
        else:
            os.environ["RL8_WGRAD_GATE_PLANES"] = before
    assert status == 0, (case["id"], status)
    assert workspace.intact() and dw.intact() and small.intact(), (case["id"], "a sentinel was overwritten")
    return {"dw2": dw.inner.cpu().numpy().reshape(HIDDEN, HIDDEN), "small": small.inner.cpu().numpy()}


def new_workspace():
    import torch

    from rl8_amd import hip

    floats = int(hip.load().rl8_mlp_wgrad_workspace_bytes()) // 4
    ws = Fenced(torch, floats, None, torch.device("cuda:0"))
    ws.inner[-64:].zero_()
    return ws


def main() -> None:
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out: dict[str, np.ndarray] = {}
    ws = new_workspace()
    for case in CASES:
        arrays = inputs(case)
        got = run(case, arrays, ws)
        again = run(case, arrays, ws)
        assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got), case["id"]
        out[case["id"] + "/inputs"] = np.array(inputs_digest(arrays))
        out[case["id"] + "/dw2"] = np.array(digest(got["dw2"]))
        out[case["id"] + "/small"] = np.array(digest(got["small"]))
        if case["id"] in FULL_CASES:
            out[case["id"] + "/dw2_full"] = got["dw2"]
        print(case["id"], out[case["id"] + "/dw2"][()][:12], out[case["id"] + "/small"][()][:12], flush=True)
    np.savez(os.environ.get("RL8_WGRAD_FIXTURE_OUT", FIXTURE), **out)


if __name__ == "__main__":
    main()
