"""The sixteen-wave weight-gradient kernels give the same bits whichever phase order their waves run.

By default half of the waves of mlp_wgrad_gate16_kernel (d_in <= 2) run each interval between two barriers "late" --
produce, then consume -- so that a SIMD's four waves do not all queue on the matrix pipe at once
(rl8_amd/csrc/mlp_split_kernels.hip, RL8_WGRAD_PHASES).  ``RL8_WGRAD_PHASES=inphase`` gives every wave the one order
the kernel had before.  Both must leave the same dW2 and the same buffer of partial rows (LSTM form: column sums), word
for word.  The general and the LSTM kernel keep one order; their cases hold the switch to changing
nothing there either.

The switch is read once per process, so every case runs in two fresh child interpreters (this file as a script), one
per value, side by side; each writes dW2 and the whole small buffer, as the kernels left them in sentinel-fenced
allocations, to a file the test compares as int32.  The runner, the inputs and the fences are those of
tests/golden/record_wgrad_gate_bitwise.py, whose ``run`` fails the child when a sentinel was overwritten.
tests/test_wgrad_gate_bitwise_gpu.py holds the default order to recorded bits; this file adds the sizes and widths it
does not hold: m = 1, 17, 65 (ragged step; one loop trip, and one more), 4097 (one chunk more than workgroups) for
rl8_mlp_wgrad_gate_bits_f32 at d_in 1 (one output, exact pair) and d_in 6 (scalars requested at the wait), the general
fused entry at 1 x 2 and 5 x 3 and the LSTM form; 2^23 + 17 rows (two segments, the accumulate path) at d_in 1.

The loop's issue budget (tests/test_wgrad_gate_issue_count.py looks at the shorter of the two loop copies) is held
here for EVERY copy of the loop, without a GPU.
"""

import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


rec = _load("record_wgrad_gate_bitwise", os.path.join(HERE, "golden", "record_wgrad_gate_bitwise.py"))


def _cases():
    forms = [("gate", 1, 1), ("gate", 1, 2), ("gate", 6, 1), ("fused", 1, 2), ("fused", 5, 3), ("loadh", 3, 0)]
    out = [{"id": f"phases-{kind}-d{d_in}-n{n_out}-m{m}", "kind": kind, "m": m, "d_in": d_in, "n_out": n_out, "planes": ""}
           for kind, d_in, n_out in forms for m in (1, 17, 65, 4097)]
    out.append({"id": "phases-gate-d1-n1-two-segments", "kind": "gate", "m": (1 << 23) + 17, "d_in": 1, "n_out": 1,
                "planes": ""})
    return out


CASES = _cases()


def _child(case_json: str, out_path: str) -> None:
    sys.path.insert(0, ROOT)
    case = json.loads(case_json)
    got = rec.run(case, rec.inputs(case))  # (asserts status 0 and every sentinel)
    np.savez(out_path, dw2=got["dw2"].view(np.int32), small=got["small"].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_late_waves_leave_the_bits_of_the_one_order(case, tmp_path):
    children = {}
    for value in ("inphase", ""):
        env = dict(os.environ)
        env.pop("RL8_WGRAD_PHASES", None)
        env.pop("RL8_WGRAD_GATE_PLANES", None)
        if value:
            env["RL8_WGRAD_PHASES"] = value
        out = tmp_path / f"{value or 'default'}.npz"
        children[value] = (out, subprocess.Popen([sys.executable, os.path.abspath(__file__), json.dumps(case), str(out)],
                                                 env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    results = {}
    for value, (out, proc) in children.items():
        log, _ = proc.communicate(timeout=300)
        assert proc.returncode == 0, (value or "default", log[-2000:])  # (status, sentinels: rec.run's asserts)
        with np.load(out) as f:
            results[value] = {k: f[k] for k in f.files}
    for k in ("dw2", "small"):
        a, b = results["inphase"][k], results[""][k]
        assert a.dtype == np.int32 and a.shape == b.shape
        assert np.array_equal(a, b), (k, int((a != b).sum()), "words differ")


def test_every_copy_of_the_gate16_loop_keeps_the_issue_budget(tmp_path):
    """Two phase orders are two copies of the steady-state loop: each holds 32 MFMAs and stays within the budget of
    tests/test_wgrad_gate_issue_count.py (whose counter and limits these are)."""
    ic = _load("wgrad_gate_issue_count", os.path.join(HERE, "test_wgrad_gate_issue_count.py"))
    if not os.path.exists(ic.HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "split.s"
    subprocess.run(
        [ic.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "mlp_split_kernels.hip")],
        check=True, capture_output=True, timeout=900,
    )
    seen = 0
    for name, body in ic.inflight.kernels_of(asm.read_text()):
        if not re.search(r"mlp_wgrad_gate16_kernelILi1ELb[01]E", name):
            continue
        loops = _loops_of(body)
        assert len(loops) == 2, (name, len(loops))
        for block in loops:
            got = ic.count(block)
            print(name, got)
            assert got["mfma"] == 32
            assert got["valu"] <= ic.VALU_MAX and got["salu"] <= ic.SALU_MAX, (name, got)
            assert got["cmp64"] == 0 and got["scratch"] == 0, (name, got)
        seen += 1
    assert seen == 2


def _loops_of(body: str) -> list[list[str]]:
    """Every block that branches back to its own label and holds 32 MFMAs (test_wgrad_gate_issue_count.loop_of
    returns the shortest of them)."""
    lines = body.split("\n")
    labels = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"\.LBB\d+_\d+:", ln)}
    found = []
    for i, ln in enumerate(lines):
        b = re.match(r"\s+s_cbranch_\w+ (\.LBB\d+_\d+)", ln)
        if not b or labels.get(b.group(1), i) >= i:
            continue
        block = [x.split(";")[0].strip() for x in lines[labels[b.group(1)] + 1:i + 1]]
        block = [x for x in block if x and not x.startswith(".")]
        if sum(x.startswith("v_mfma") for x in block) == 32:
            found.append(block)
    return found


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
