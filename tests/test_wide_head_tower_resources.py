"""The wide-head tower kernels (rl8_amd/csrc/mlp_wide_out_kernels.hip) compiled for gfx950, from the kernel
descriptors alone: every variant present, no private segment and no dynamic stack, registers within what the workgroups
per CU of its ``__launch_bounds__`` leave a wave, and LDS times workgroups per CU within the CU's 160 KiB."""

import os
import re
import shutil
import subprocess

import pytest

from rl8_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CU_LDS_BYTES = 160 * 1024
SIMD_VGPRS = 512  # per lane, arch + accumulation registers, shared by the waves resident on one SIMD


def _field(body: str, name: str) -> int:
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", body).group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_wide_head_kernels_fit_their_occupancy(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "wide_out.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "mlp_wide_out_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    # name pattern -> (threads per workgroup, workgroups per CU of its __launch_bounds__, kernel index of
    # rl8_mlp_wide_out_lds_bytes, the width the LDS is asked for)
    want = {}
    for kin in (32, 64, 128):
        for save in (0, 1):
            want[f"mlp_wide_out_forward_kernelILi{kin}ELb{save}E"] = (256, 2, 0, kin)
    for kout in (32, 64, 128):
        want[f"mlp_wide_out_backward_kernelILi{kout}E"] = (256, 2, 1, kout)
    for ct in (1, 2, 3, 4):
        want[f"mlp_wide_out_wgrad_kernelILi{ct}E"] = (512, 1, 2, 32 * ct)
    lib = hip.load()
    for pattern, (threads, per_cu, which, width) in want.items():
        found = [(name, body) for name, body in kernels.items() if pattern in name]
        assert len(found) == 1, pattern
        name, body = found[0]
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        waves_per_simd = threads // 64 * per_cu // 4
        assert _field(body, "next_free_vgpr") <= SIMD_VGPRS // waves_per_simd, (name, _field(body, "next_free_vgpr"))
        lds = _field(body, "group_segment_fixed_size") + int(lib.rl8_mlp_wide_out_lds_bytes(which, width))
        assert 0 < lds and lds * per_cu <= CU_LDS_BYTES, (name, lds, per_cu)
    for name, body in kernels.items():  # (the pack and the slab-reduction kernel too)
        assert "mlp_wide_out" in name and _field(body, "private_segment_fixed_size") == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
    assert len(kernels) == len(want) + 2
    # the same bits from run to run: no float atomics anywhere in the unit
    assert not re.search(r"\b(global|flat|buffer|ds)_(atomic|add_f|pk_add)\w*", text)
    assert "v_mfma_f32_32x32x2_f32" in text or "v_mfma_f32_32x32x2f32" in text
