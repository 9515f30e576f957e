"""The sixteen-wave weight-gradient kernels give the bits they gave before their operand requests were reworked.

tests/golden/wgrad_gate_bitwise.npz was recorded (tests/golden/record_wgrad_gate_bitwise.py, which also holds the
cases, the inputs and the runner used here) with the library as it stood before mlp_wgrad_gate16_kernel took its
rows through one descriptor per operand.  Every case runs twice into fresh, sentinel-fenced outputs: the two runs
must agree with each other and with the record -- dW2 and the whole buffer of partial rows [dW1 | db1 | db2 | dW3 |
db3] (for the LSTM form: the column sums).  The fixture keeps SHA-256 digests, equal exactly when every bit is, and
the full dW2 of two cases, compared with torch.equal: fifty outputs of 256 KiB and more do not fit a committed file.

Cases: rl8_mlp_wgrad_gate_bits_f32 at d_in 1 and 5, one output and an exact pair, m = 1, 15, 16, 17, 63, 64, 65 (the
16-sample step and the four-step loop trip), 4095, 4096, 4097 (as many chunks as workgroups), 2^23 + 17 (two
segments: the accumulate path); d_in 6 and 7 once each (scalar operands requested at the wait); the exact bf16
planes by request at m = 65; the general mlp_wgrad_fused16_kernel
and the LSTM's mlp_wgrad_loadh16_kernel at m = 17 and 65.

The host launch code of the tower entries (grids, grid cap, segments, run-time width -> compiled variant) is held the
same way, by a record made before it moved into rl8_amd/csrc/tower_launch.hip.h: every weight-gradient entry at every
compiled width (m = 17: one chunk and a ragged row; the four-gate LSTM entry at 128, 129 and 2049 rows), both plane
modes, the guard firing (the workspace's fires counter must rise by one), and the forward and data-gradient entries
of both precisions at one width per class pair (m = 129: a tile and a row; 65536 and 65537 rows: 512 and 513 tiles
against the grid cap of 512), with the digest of every buffer given and of the returned row count.  Widths that have
no variant are asserted to return RL8_ESIZE.  The two-segment case of the bits entry speaks for the segment walk all
weight-gradient entries share.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("record_wgrad_gate_bitwise",
                                               os.path.join(HERE, "golden", "record_wgrad_gate_bitwise.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

@pytest.fixture(scope="module")
def record():
    with np.load(rec.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def workspace():
    return rec.new_workspace()


def test_the_fixture_covers_every_case(record):
    assert {k.split("/")[0] for k in record} == {c["id"] for c in rec.CASES}
    assert {k.split("/")[0] for k in record if k.endswith("/dw2_full")} == set(rec.FULL_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=[c["id"] for c in rec.CASES])
def test_bits_are_those_of_the_record(case, record, workspace):
    arrays = rec.inputs(case)
    assert rec.inputs_digest(arrays) == str(record[case["id"] + "/inputs"]), "the inputs are not the recorded ones"
    got = rec.run(case, arrays, workspace)
    again = rec.run(case, arrays, workspace)
    for k in got:
        assert torch.equal(torch.from_numpy(got[k]).view(torch.int32), torch.from_numpy(again[k]).view(torch.int32)), k
    assert {case["id"] + "/" + k for k in got} | {case["id"] + "/inputs"} == \
        {k for k in record if k.split("/")[0] == case["id"] and not k.endswith("/dw2_full")}, "the outputs are not the recorded ones"
    for k in got:  # (dw2: dW2; small: the partial rows or column sums; the tower entries: every buffer they were given)
        assert rec.digest(got[k]) == str(record[case["id"] + "/" + k]), k
    if case["id"] in rec.FULL_CASES:
        want = torch.from_numpy(record[case["id"] + "/dw2_full"])
        assert torch.equal(torch.from_numpy(got["dw2"]).view(torch.int32), want.view(torch.int32))
