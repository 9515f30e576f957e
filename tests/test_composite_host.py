"""Dict-observation entries of the C ABI without a GPU: rl8_rollout_scatter_leaves_f32 and the three AlgoTrading
entries are declared, exported and bound, refuse bad arguments before any launch, and the AlgoTrading kernels
compile for gfx950 without scratch."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("rl8_rollout_scatter_leaves_f32", "rl8_algotrading_reset_f32", "rl8_algotrading_step_f32",
           "rl8_rollout_step_algotrading_f32")
FAKE = 4096  # (never dereferenced: every call below fails its checks first)


def test_entries_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        header = f.read()
    lib = hip.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
    assert "} rl8_scatter_leaf;" in header
    assert hip.abi_version()[0] == hip.ABI_VERSION == 107  # (compatible additions: no bump)


def test_the_binding_matches_the_header_argument_for_argument():
    """Each entry's ``SIGNATURES`` row has one ctypes type per declared parameter."""
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        header = f.read()
    for name in ENTRIES:
        params = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        params = re.sub(r"/\*.*?\*/", "", params)
        assert len(params.split(",")) == len(hip.SIGNATURES[name]), name


def _leaves(*rows):
    arr = (hip.ScatterLeaf * len(rows))()
    for i, (src, dst, row_bytes) in enumerate(rows):
        arr[i] = hip.ScatterLeaf(src, dst, row_bytes)
    return arr


def test_scatter_leaves_refuses_bad_arguments_before_launching():
    fn = hip.load().rl8_rollout_scatter_leaves_f32
    one = _leaves((FAKE, FAKE, 3))

    def call(action=FAKE, arb=8, logp=FAKE, value=FAKE, reward=FAKE, leaves=one, n_leaves=1, action_col=FAKE,
             logp_col=FAKE, value_col=FAKE, reward_col=FAKE, rdr_t=FAKE, rdr_t1=FAKE, n=10):
        return fn(action, arb, logp, value, reward, leaves, n_leaves, action_col, logp_col, value_col, reward_col,
                  rdr_t, rdr_t1, 0.5, n, None)

    for missing in ("action", "logp", "value", "reward", "leaves", "action_col", "logp_col", "value_col", "reward_col"):
        assert call(**{missing: None}) == -1, missing
    assert call(rdr_t=None) == -1 and call(rdr_t1=None) == -1  # (both or neither)
    assert call(leaves=_leaves((None, FAKE, 4))) == -1 and call(leaves=_leaves((FAKE, None, 4))) == -1
    assert call(n=0) == -2 and call(n=-1) == -2
    assert call(n_leaves=0) == -2 and call(n_leaves=hip.MAX_GATHER_FIELDS + 1) == -2
    assert call(arb=0) == -2 and call(arb=6) == -2
    assert call(leaves=_leaves((FAKE, FAKE, 0))) == -2 and call(leaves=_leaves((FAKE, FAKE, -4))) == -2
    for misaligned in ("action", "logp", "value", "reward", "action_col", "logp_col", "value_col", "reward_col",
                       "rdr_t", "rdr_t1"):
        assert call(**{misaligned: FAKE + 2}) == -3, misaligned


def test_algotrading_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    reset, step, fused = lib.rl8_algotrading_reset_f32, lib.rl8_algotrading_step_f32, lib.rl8_rollout_step_algotrading_f32

    def call_reset(state=FAKE, n=10, outs=(FAKE, FAKE, FAKE, FAKE)):
        return reset(state, n, 3.14, 0.05, 0.05, 1, 0, 0, *outs, None)

    assert call_reset(state=None) == -1
    assert call_reset(outs=(FAKE, None, FAKE, FAKE)) == -1  # (the four leaves together, or none)
    assert call_reset(n=0) == -2
    assert call_reset(state=FAKE + 2) == -3 and call_reset(outs=(FAKE, FAKE + 4, FAKE, FAKE)) == -3
    assert call_reset(outs=(FAKE, FAKE, FAKE + 1, FAKE)) == -3

    def call_step(n=10, **bad):
        args = dict(state=FAKE, action=FAKE, mask=FAKE, invested=FAKE, lc=FAKE, lcp=FAKE, reward=FAKE)
        args.update(bad)
        return step(*args.values(), n, None)

    for missing in ("state", "action", "mask", "invested", "lc", "lcp", "reward"):
        assert call_step(**{missing: None}) == -1, missing
    assert call_step(n=0) == -2
    assert call_step(action=FAKE + 4) == -3 and call_step(invested=FAKE + 4) == -3 and call_step(reward=FAKE + 2) == -3

    def call_fused(n=10, **bad):
        args = dict(logits=FAKE, value=FAKE, noise=FAKE, state=FAKE, action_col=FAKE, logp_col=FAKE, value_col=FAKE,
                    reward_col=FAKE, mask=FAKE, invested=FAKE, lc=FAKE, lcp=FAKE, rdr_t=FAKE, rdr_t1=FAKE)
        args.update(bad)
        return fused(*args.values(), 0.5, n, 1, 0, 0, 0, None)

    for missing in ("logits", "value", "state", "action_col", "logp_col", "value_col", "reward_col", "mask",
                    "invested", "lc", "lcp"):
        assert call_fused(**{missing: None}) == -1, missing
    assert call_fused(rdr_t=None) == -1 and call_fused(rdr_t1=None) == -1
    assert call_fused(n=0) == -2
    for misaligned, by in (("action_col", 4), ("invested", 4), ("logits", 2), ("noise", 2), ("lc", 1), ("rdr_t1", 2)):
        assert call_fused(**{misaligned: FAKE + by}) == -3, misaligned


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_algotrading_kernels_compile_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "algotrading.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "algotrading_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    for want in ("algotrading_reset_kernel", "algotrading_step_kernel", "rollout_step_algotrading_kernel"):
        assert any(want in name for name in kernels), (want, sorted(kernels))
    assert len(kernels) == 3, sorted(kernels)
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        assert "enable_private_segment 1" not in body, name


def test_the_envs_package_exports_algotrading():
    from rl8_amd import envs
    from rl8_amd.envs.algotrading import AlgoTrading

    assert envs.AlgoTrading is AlgoTrading and "AlgoTrading" in envs.__all__
    assert AlgoTrading.max_horizon == 128
