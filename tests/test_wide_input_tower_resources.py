"""The wide-input tower kernels (rl8_amd/csrc/mlp_wide_in_kernels.hip) compiled for gfx950, from the kernel
descriptors alone: every variant present, no private segment, registers within what the workgroups per CU of its
``__launch_bounds__`` leave a wave, and LDS times workgroups per CU within the CU's 160 KiB."""

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
def test_wide_input_kernels_fit_their_occupancy(tmp_path):
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "wide_in.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "mlp_wide_in_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S))
    # name pattern -> (threads per workgroup, workgroups per CU of its __launch_bounds__, kernel index of
    # rl8_mlp_wide_in_lds_bytes, d_in the LDS is asked for)
    want = {}
    for kin in (32, 64, 128):
        for kout in (2, 4, 8):
            for save in (0, 1):
                want[f"mlp_wide_in_forward_kernelILi{kin}ELi{kout}ELb{save}E"] = (256, 2, 0, kin)
    for kout in (2, 4, 8):
        want[f"mlp_wide_in_backward_kernelILi{kout}E"] = (256, 2, 1, 24)
    for ct in (1, 2, 3, 4):
        want[f"mlp_wide_in_wgrad_kernelILi{ct}E"] = (512, 1, 2, 32 * ct)
    lib = hip.load()
    for pattern, (threads, per_cu, which, d_in) in want.items():
        found = [(name, body) for name, body in kernels.items() if pattern in name]
        assert len(found) == 1, pattern
        name, body = found[0]
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        waves_per_simd = threads // 64 * per_cu // 4
        assert _field(body, "next_free_vgpr") <= SIMD_VGPRS // waves_per_simd, (name, _field(body, "next_free_vgpr"))
        lds = _field(body, "group_segment_fixed_size") + int(lib.rl8_mlp_wide_in_lds_bytes(which, d_in))
        assert 0 < lds and lds * per_cu <= CU_LDS_BYTES, (name, lds, per_cu)
    for name, body in kernels.items():  # (the pack and the slab-reduction kernel too)
        assert "mlp_wide_in" in name and _field(body, "private_segment_fixed_size") == 0, name
    assert len(kernels) == len(want) + 2
