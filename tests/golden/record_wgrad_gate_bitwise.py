"""Cases, inputs and runner of tests/test_wgrad_gate_bitwise_gpu.py, and the recorder of its fixture.

    python tests/golden/record_wgrad_gate_bitwise.py          (on a GPU, with the library whose bits are the reference)

writes tests/golden/wgrad_gate_bitwise.npz: per case the SHA-256 of the inputs, of dW2 and of the whole buffer of
partial rows (as the kernels left it: untouched words keep their fill), and dW2 itself for the cases named in
FULL_CASES.  A dW2 is 256 KiB and a buffer of partial rows up to 7 MiB; fifty cases of them do not fit a
committed file, so all but two cases are held to their digests -- which are equal exactly when every bit is.

The cases of _launch_layer_cases() hold every tower entry point's host launch code -- width dispatch, grids, grid cap,
segment offsets -- the same way: per case the digests of every buffer the entry was given (fenced), and of the row count
it returned.  They were recorded with the library as it stood before that code moved into tower_launch.hip.h.

A new record keeps the old one: main() loads the fixture that is there and refuses to write unless every key in it
comes out with the value it has.  RL8_WGRAD_GATE_OFF must be unset (the library reads it once per process).

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


def _case(cid, kind, m, d_in, n_out, planes="", **more):
    return {"id": cid, "kind": kind, "m": m, "d_in": d_in, "n_out": n_out, "planes": planes, **more}


def _backward_supports(d_in, n_out):
    return 1 <= d_in <= 7 and 1 <= n_out <= 4 and not (d_in == 7 and n_out == 4)


def _launch_layer_cases():
    """Every width variant, grid rule and offset of the tower entries' host launch code, at the smallest sizes that
    tell a wrong variant, grid or offset: m = 17 for the weight gradients (one 16-sample chunk and a ragged row),
    m = 129 for the forward and data-gradient kernels (one 128-row tile and a row)."""
    out = []
    # rl8_mlp_wgrad_gate_bits_f32: the widths not held above, and the exact planes at every width
    for d_in in (2, 3, 4):
        for n_out in (1, 2):
            out.append(_case(f"gate-d{d_in}-n{n_out}-m17", "gate", 17, d_in, n_out))
    for d_in in range(1, 8):
        for n_out in (1, 2):
            out.append(_case(f"gate-d{d_in}-n{n_out}-m17-bf16", "gate", 17, d_in, n_out, "bf16"))
    # rl8_mlp_wgrad_fused_split_f32: every supported width on both planes; one output (the gate-plane kernel on h2)
    for d_in in range(1, 8):
        for n_out in (2, 3, 4):
            if not _backward_supports(d_in, n_out):
                continue
            if (d_in, n_out) != (1, 3):  # (held above)
                out.append(_case(f"fused-d{d_in}-n{n_out}-m17", "fused", 17, d_in, n_out))
            out.append(_case(f"fused-d{d_in}-n{n_out}-m17-bf16", "fused", 17, d_in, n_out, "bf16"))
    for d_in in range(1, 8):
        out.append(_case(f"fused-d{d_in}-n1-m17", "fused", 17, d_in, 1))
    out.append(_case("fused-d7-n4-esize", "fused", 17, 7, 4, status=-2))
    for d_in in range(1, 8):
        out.append(_case(f"pair-d{d_in}-m17", "pair", 17, d_in, 2))
    # the guard fires (row 0 of dOut 2^20 above the others): fp16 planes dropped, the exact ones kept
    out.append(_case("gate-d1-n1-m65-guard", "gate", 65, 1, 1, spike=True))
    out.append(_case("gate-d5-n2-m65-guard", "gate", 65, 5, 2, spike=True))
    out.append(_case("fused-d1-n3-m65-guard", "fused", 65, 1, 3, spike=True))
    out.append(_case("fused-d5-n2-m65-guard", "fused", 65, 5, 2, spike=True))
    # rl8_mlp_wgrad_split_f32: the compiled widths, the run-time width, accumulate
    for d_in in (1, 2, 3, 5, 4, 8, 16):
        out.append(_case(f"split-d{d_in}-m17", "split", 17, d_in, 0))
    out.append(_case("split-d3-m17-acc", "split", 17, 3, 0, accumulate=1))
    # rl8_mlp_wgrad_split_strided_f32 (exact planes, no bounds), rl8_mlp_wgrad_f16_strided_f32, rl8_lstm_wgrad_f16_f32
    out.append(_case("sstrided-nosums-m17", "sstrided", 17, 0, 0))
    for d_in in range(1, 8):
        out.append(_case(f"sstrided-d{d_in}-m17", "sstrided", 17, d_in, 0))
    for d_in in (2, 4, 5, 6, 7):
        out.append(_case(f"loadh-d{d_in}-m17", "loadh", 17, d_in, 0))
    for d_in in (1, 5):
        for m in (128, 129, 2049):
            out.append(_case(f"lstm-d{d_in}-m{m}", "lstm", m, d_in, 0))
    out.append(_case("wgrad32-m17", "wgrad32", 17, 0, 0, pitches=None))
    out.append(_case("wgrad32-strided-m17", "wgrad32", 17, 0, 0, pitches=(1024, 512)))
    # rl8_mlp_tower_forward_f16_f32: one width per class pair, three save modes
    for d_in in (1, 2, 3, 4, 8, 9, 16):
        for n_out in (1, 2, 3, 4, 5, 8):
            if d_in > 8 and n_out > 4:  # (input class 16 has no variant with output class 8: rl8_mlp_forward_f16_supports)
                out.append(_case(f"fwd16-d{d_in}-n{n_out}-esize", "fwd16", 129, d_in, n_out, save="none", status=-2))
                continue
            for save in ("none", "h2", "bits"):
                out.append(_case(f"fwd16-d{d_in}-n{n_out}-{save}", "fwd16", 129, d_in, n_out, save=save))
    for d_in in range(1, 8):
        for n_out in range(1, 5):
            if _backward_supports(d_in, n_out):
                out.append(_case(f"bwd16-d{d_in}-n{n_out}", "bwd16", 129, d_in, n_out))
    for d_in in range(1, 6):
        for n_out in range(1, 5):
            out.append(_case(f"bwd16-d{d_in}-n{n_out}-tile", "bwd16", 129, d_in, n_out, tile=True))
    for d_in in range(1, 8):
        for n_out in (1, 2):
            out.append(_case(f"bwdgate-d{d_in}-n{n_out}", "bwdgate", 129, d_in, n_out))
    for d_in in (1, 2, 3, 4, 5, 16):
        for n_out in (1, 2, 3, 4, 8):
            out.append(_case(f"fwd32-d{d_in}-n{n_out}-none", "fwd32", 129, d_in, n_out, save="none"))
            out.append(_case(f"fwd32-d{d_in}-n{n_out}-save", "fwd32", 129, d_in, n_out, save="h2"))
            out.append(_case(f"bwd32-d{d_in}-n{n_out}", "bwd32", 129, d_in, n_out))
    # the grid cap: 512 and 513 tiles of 128 rows against the default cap of 512 workgroups
    for m in (65536, 65537):
        out.append(_case(f"fwd16-d1-n2-bits-m{m}", "fwd16", m, 1, 2, save="bits"))
        out.append(_case(f"bwdgate-d1-n2-m{m}", "bwdgate", m, 1, 2))
    return out


CASES = _gate_cases() + _launch_layer_cases()
FULL_CASES = ("gate-d1-n1-m65", "gate-d5-n2-m4097")


def inputs(case: dict) -> dict[str, np.ndarray]:
    """The case's arrays (host), from a seed that depends on nothing but its id."""
    seed = int.from_bytes(hashlib.sha256(case["id"].encode()).digest()[:4], "little")
    rng = np.random.RandomState(seed)
    m, d_in, n_out = case["m"], case["d_in"], case["n_out"]
    f32 = np.float32
    kind = case["kind"]
    if kind not in ("gate", "fused", "loadh"):
        return _launch_layer_inputs(case, rng)
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
    if case.get("spike"):
        # The guard fires when the entries BELOW the call's largest lie 2^12 under it on average.  A rank-one row
        # (g, -g) is scaled whole -- both entries are then the largest, and a pair stays a pair.  Of a general row only
        # entry 0 is: its neighbours in the row, scaled too, would sit within a few binades of the largest and their
        # fractions alone would outweigh every other row's (run() asserts that the guard did fire).
        if case["kind"] == "gate":
            a["dout"][0] *= f32(2.0 ** 20)
        else:
            a["dout"][0, 0] *= f32(2.0 ** 20)
    return a


def _launch_layer_inputs(case: dict, rng) -> dict[str, np.ndarray]:
    m, d_in, n_out, kind = case["m"], case["d_in"], case["n_out"], case["kind"]
    f32 = np.float32
    normal = lambda *shape: rng.standard_normal(shape)  # noqa: E731
    a = {}
    if kind in ("sstrided", "lstm"):
        if d_in:
            a["x"] = (normal(m, d_in) * 3.0).astype(f32)
        a["dz"] = (normal(m, 4 * HIDDEN) / m).astype(f32)
        a["h"] = np.tanh(normal(m, HIDDEN)).astype(f32)
        a["dz_bound"] = np.array([np.abs(a["dz"]).max()], dtype=f32)
        a["h_bound"] = np.array([1.0], dtype=f32)
        return a
    if kind == "wgrad32":
        dz_pitch, h_pitch = case["pitches"] or (HIDDEN, HIDDEN)
        a["dz"] = (normal(m, dz_pitch) / m).astype(f32)
        a["h"] = np.maximum(normal(m, h_pitch), 0.0).astype(f32)
        return a
    a["x"] = (normal(m, d_in) * 3.0).astype(f32)
    a["w1"] = (normal(HIDDEN, d_in) * 0.5).astype(f32)
    a["b1"] = (normal(HIDDEN) * 0.5).astype(f32)
    if kind == "split":
        a["dz"] = (normal(m, HIDDEN) / m).astype(f32)
        return a
    a["w2"] = (normal(HIDDEN, HIDDEN) / 16.0).astype(f32)
    a["b2"] = (normal(HIDDEN) * 0.1).astype(f32)
    a["w3"] = (normal(n_out, HIDDEN) / 16.0).astype(f32)
    a["b3"] = (normal(n_out) * 0.1).astype(f32)
    if kind in ("fwd16", "fwd32"):
        return a
    g0 = (normal(m) / m).astype(f32)
    if kind in ("pair", "bwdgate"):
        a["dout"] = g0[:, None].copy() if n_out == 1 else np.stack([g0, -g0], axis=1).copy()
    else:
        a["dout"] = (normal(m, n_out) / m).astype(f32)
    if kind in ("bwd16", "bwdgate"):
        a["gate2"] = rng.randint(0, 1 << 32, size=(m, 8), dtype=np.uint64).astype(np.uint32)
    else:  # pair, bwd32
        a["h2"] = np.maximum(normal(m, HIDDEN), 0.0).astype(f32)
    if kind == "bwd32":
        a["h1"] = np.maximum(normal(m, HIDDEN), 0.0).astype(f32)
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
    # RL8_WGRAD_GATE_OFF is read once per process by the library: one value for the record and for every test
    assert "RL8_WGRAD_GATE_OFF" not in os.environ, "RL8_WGRAD_GATE_OFF must be unset for this record"
    # the plane variable of the case's own entry, and the tile switch of the data gradient: set here, restored below
    env = {"RL8_WGRAD_PLANES": case["planes"] if case["kind"] == "fused" else "",
           "RL8_WGRAD_GATE_PLANES": case["planes"] if case["kind"] == "gate" else "",
           "RL8_MLP_DGRAD_TILE": "1" if case.get("tile") else ""}
    before = {k: os.environ.get(k) for k in env}
    fires = int(workspace.inner[-64:].view(torch.int32)[33].item())
    try:
        for k, v in env.items():
            if v:
                os.environ[k] = v
            else:
                os.environ.pop(k, None)
        if case["kind"] not in ("gate", "fused", "loadh"):
            status, fenced, got = _run_launch_layer(lib, torch, case, t, workspace, dw, stream)
            torch.cuda.synchronize()
        elif case["kind"] == "loadh":
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
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert status == case.get("status", 0), (case["id"], status)
    if case["kind"] in ("gate", "fused", "loadh"):
        fenced = [small]
        got = {"dw2": dw.inner.cpu().numpy().reshape(HIDDEN, HIDDEN), "small": small.inner.cpu().numpy()}
    assert workspace.intact() and dw.intact() and all(f.intact() for f in fenced), (case["id"], "a sentinel was overwritten")
    if case.get("spike"):  # (else the case would hold the fp16 planes, which the other cases hold already)
        assert int(workspace.inner[-64:].view(torch.int32)[33].item()) == fires + 1, (case["id"], "the guard did not fire")
    if status != 0:
        return {"status": np.array([status], dtype=np.int32)}
    return got


def _run_launch_layer(lib, torch, case, t, workspace, dw, stream):
    """The entry points beside the three above.  Returns the status, the fenced buffers and the outputs by name."""
    dev = dw.whole.device
    m, d_in, n_out, kind = case["m"], case["d_in"], case["n_out"], case["kind"]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    host = lambda f: f.inner.cpu().numpy()  # noqa: E731
    rows = C.c_int(-1)
    ws = p(workspace.inner)
    max_rows = int(lib.rl8_mlp_backward_max_rows())

    def packed_f16(name, *args):
        buf = torch.zeros(int(lib.rl8_mlp_f16_packed_bytes()), dtype=torch.uint8, device=dev)
        assert getattr(lib, name)(*args, p(buf), stream) == 0, name
        return buf

    def packed_f32(transposed):
        buf = torch.zeros(HIDDEN * HIDDEN, dtype=torch.float32, device=dev)
        assert lib.rl8_mlp_pack_w2_f32(p(t["w2"]), p(buf), transposed, stream) == 0
        return buf

    if kind == "pair":
        small = Fenced(torch, max_rows * int(lib.rl8_mlp_backward_partial_floats(d_in, 2)), FILL, dev)
        status = lib.rl8_mlp_wgrad_fused_pair_f32(p(t["h2"]), p(t["dout"]), p(t["x"]), p(t["w1"]), p(t["b1"]), p(t["w3"]), m,
                                                  d_in, ws, p(dw.inner), p(small.inner), stream)
        return status, [small], {"dw2": host(dw), "small": host(small)}
    if kind == "split":
        status = lib.rl8_mlp_wgrad_split_f32(p(t["dz"]), p(t["x"]), p(t["w1"]), p(t["b1"]), m, d_in, ws, p(dw.inner),
                                             case.get("accumulate", 0), stream)
        return status, [], {"dw2": host(dw)}
    if kind == "wgrad32":
        if case["pitches"] is None:
            status = lib.rl8_mlp_wgrad_f32(p(t["dz"]), p(t["h"]), m, ws, p(dw.inner), 0, stream)
        else:
            status = lib.rl8_mlp_wgrad_strided_f32(p(t["dz"]), case["pitches"][0], p(t["h"]), case["pitches"][1], m, ws,
                                                   p(dw.inner), 0, stream)
        return status, [], {"dw2": host(dw)}
    if kind == "sstrided":
        sums = Fenced(torch, 256 * HIDDEN * (d_in + 1), FILL, dev)
        with_sums = d_in > 0
        status = lib.rl8_mlp_wgrad_split_strided_f32(
            C.c_void_p(t["dz"].data_ptr() + 4 * HIDDEN), 4 * HIDDEN, p(t["h"]), HIDDEN, m, ws, p(dw.inner), 0,
            p(t["x"]) if with_sums else None, d_in, p(sums.inner) if with_sums else None,
            C.byref(rows) if with_sums else None, stream)
        return status, [sums], {"dw2": host(dw), "small": host(sums), "rows": np.array([rows.value], dtype=np.int32)}
    if kind == "lstm":
        dw4 = Fenced(torch, 4 * HIDDEN * HIDDEN, FILL, dev)
        sums = Fenced(torch, 4 * 64 * HIDDEN * (d_in + 1), FILL, dev)
        status = lib.rl8_lstm_wgrad_f16_f32(p(t["dz"]), 4 * HIDDEN, p(t["dz_bound"]), p(t["h"]), HIDDEN, p(t["h_bound"]), m, ws,
                                            p(dw4.inner), 0, p(t["x"]), d_in, p(sums.inner), C.byref(rows), stream)
        return status, [dw4, sums], {"dw2": host(dw4), "small": host(sums), "rows": np.array([rows.value], dtype=np.int32)}
    if kind in ("fwd16", "fwd32"):
        out = Fenced(torch, m * n_out, FILL, dev)
        save = case["save"]
        h1 = h2 = Fenced(torch, m * HIDDEN, FILL, dev) if save == "h2" else None
        if save == "h2":
            h2 = Fenced(torch, m * HIDDEN, FILL, dev)
        bits = Fenced(torch, m * 8, FILL, dev) if save != "none" and kind == "fwd16" else None
        given = lambda f: p(f.inner) if f is not None else None  # noqa: E731
        if kind == "fwd16":
            w2s = packed_f16("rl8_mlp_pack_w2_f16", p(t["w2"]), 0)
            status = lib.rl8_mlp_tower_forward_f16_f32(
                p(t["x"]), m, d_in, p(t["w1"]), p(t["b1"]), p(w2s), p(t["b2"]), p(t["w3"]), p(t["b3"]), n_out, p(out.inner),
                given(h1), given(h2), given(bits), stream)
        else:
            w2p = packed_f32(0)
            status = lib.rl8_mlp_tower_forward_f32(
                p(t["x"]), m, d_in, p(t["w1"]), p(t["b1"]), p(w2p), p(t["b2"]), p(t["w3"]), p(t["b3"]), n_out, p(out.inner),
                given(h1), given(h2), stream)
        buffers = {k: f for k, f in (("out", out), ("h1", h1), ("h2", h2), ("bits", bits)) if f is not None}
        return status, list(buffers.values()), {k: host(f) for k, f in buffers.items()}
    small = Fenced(torch, max_rows * int(lib.rl8_mlp_backward_partial_floats(d_in, n_out)), FILL, dev)
    fenced, got = [small], {}
    if kind == "bwd16":
        w2t = packed_f16("rl8_mlp_pack_w2_f16", p(t["w2"]), 1)
        status = lib.rl8_mlp_tower_backward_f16_f32(p(t["x"]), p(t["w1"]), p(t["b1"]), p(t["dout"]), m, d_in, p(w2t), p(t["w3"]),
                                                    n_out, p(small.inner), C.byref(rows), p(t["gate2"]), stream)
    elif kind == "bwdgate":
        w2t = packed_f16("rl8_mlp_pack_w2_f16_gate", p(t["w2"]), p(t["w3"]), n_out)
        status = lib.rl8_mlp_tower_backward_gate_f16_f32(p(t["x"]), p(t["w1"]), p(t["b1"]), p(t["dout"]), m, d_in, p(w2t), n_out,
                                                         p(small.inner), C.byref(rows), p(t["gate2"]), stream)
    else:
        assert kind == "bwd32", kind
        dz2 = Fenced(torch, m * HIDDEN, FILL, dev)
        w2tp = packed_f32(1)
        status = lib.rl8_mlp_tower_backward_f32(p(t["x"]), p(t["h1"]), p(t["h2"]), p(t["dout"]), m, d_in, p(w2tp), p(t["w3"]),
                                                n_out, p(dz2.inner), p(small.inner), C.byref(rows), stream)
        fenced.append(dz2)
        got["dz2"] = host(dz2)
    got["small"] = host(small)
    got["rows"] = np.array([rows.value], dtype=np.int32)
    return status, fenced, got


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
        for k in got:
            out[case["id"] + "/" + k] = np.array(digest(got[k]))
        if case["id"] in FULL_CASES:
            out[case["id"] + "/dw2_full"] = got["dw2"]
        print(case["id"], *(k + "=" + str(out[case["id"] + "/" + k])[:12] for k in got), flush=True)
    # what an earlier record holds is kept, not re-made: every key it has must come out as it stands there
    if os.path.exists(FIXTURE):
        with np.load(FIXTURE) as held:
            for k in held.files:
                assert k in out and np.array_equal(held[k], out[k]), (k, "differs from the committed record")
    np.savez_compressed(os.environ.get("RL8_WGRAD_FIXTURE_OUT", FIXTURE), **out)


if __name__ == "__main__":
    main()
