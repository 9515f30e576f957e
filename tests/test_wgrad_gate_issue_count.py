"""What the steady-state loop of mlp_wgrad_gate16_kernel issues ("Rank-one weight gradient: what the
loop issues"): compiled to gfx950 assembly with the flags of tests/test_kernel_resources.py, the block that branches
to itself and holds 32 MFMAs -- one trip: four 16-sample steps, 16 elements per thread -- is counted.

Before the operand requests were reworked the loop held 201 vector and 135 scalar instructions per 32 MFMAs, nine of
the vector ones 64-bit row-bound compares.  Now: no 64-bit compare, the scalar side under 80, and the vector side at
what the levers that were kept reach (VALU_MAX below; DESIGN says which were dropped and why).
"""

import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_inflight_regs as inflight  # noqa: E402

VALU_MAX = 180   # 201 before; 165 was the aim with a gate plane of its own in LDS, which measured slower (DESIGN)
SALU_MAX = 80    # 135 before
VGPR_MAX = 128   # as before: four waves per SIMD
SGPR_MAX = 95    # as before


def loop_of(body: str) -> list[str]:
    """The instructions of the block that branches back to its own label and holds 32 MFMAs."""
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
    assert found, "no loop of 32 MFMAs"
    return min(found, key=len)  # (the innermost, should an outer loop hold nothing else)


def count(block: list[str]) -> dict[str, int]:
    ops = collections.Counter(x.split()[0] for x in block)
    return {
        "mfma": sum(v for k, v in ops.items() if k.startswith("v_mfma")),
        "valu": sum(v for k, v in ops.items() if k.startswith("v_") and not k.startswith("v_mfma")),
        # every scalar instruction but the waits, the no-ops and the loop's branch
        "salu": sum(v for k, v in ops.items() if k.startswith("s_") and k not in ("s_waitcnt", "s_nop")
                    and not k.startswith("s_cbranch")),
        "cmp64": sum(v for k, v in ops.items() if re.match(r"v_cmpx?_\w+_[iu]64", k)),
        "scratch": sum(v for k, v in ops.items() if k.startswith("scratch_")),
    }


def test_counter_counts_what_it_should():
    block = ["v_mfma_f32_32x32x16_f16 v[0:15], v[16:19], v[20:23], v[0:15]", "v_and_b32_e32 v1, v2, v3",
             "v_cmp_lt_i64_e64 s[0:1], s[2:3], v[4:5]", "s_add_i32 s0, s1, s2", "s_waitcnt lgkmcnt(0)", "s_barrier",
             "s_buffer_load_dwordx8 s[8:15], s[4:7], s3", "s_nop 1", "ds_read_b128 v[4:7], v1", "s_cbranch_scc0 .LBB0_1"]
    assert count(block) == {"mfma": 1, "valu": 2, "salu": 3, "cmp64": 1, "scratch": 0}
    body = "\n".join(["\ts_mov_b32 s0, 0", ".LBB0_1:"] + ["\t" + x for x in block[:1] * 32 + block[1:]] + ["\ts_endpgm"])
    assert len(loop_of(body)) == 32 + 9


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_gate16_loop_issue_count(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "split.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "mlp_split_kernels.hip")],
        check=True, capture_output=True, timeout=900,
    )
    text = asm.read_text()
    descriptors = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    seen = 0
    for name, body in inflight.kernels_of(text):
        if not re.search(r"mlp_wgrad_gate16_kernelILi1ELb[01]E", name):
            continue
        got = count(loop_of(body))
        print(name, got)
        assert got["mfma"] == 32
        assert got["valu"] <= VALU_MAX and got["salu"] <= SALU_MAX, (name, got)
        assert got["cmp64"] == 0 and got["scratch"] == 0, (name, got)
        d = descriptors[name]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", d).group(1)) <= VGPR_MAX, name
        assert int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", d).group(1)) <= SGPR_MAX, name
        violations, _ = inflight.check_kernel(name, body)
        assert not violations, (name, [(v.index, v.line, v.load) for v in violations[:3]])
        seen += 1
    assert seen == 2
