"""The wave-per-row categorical entries of the C ABI without a GPU: rl8_categorical_wide_sample_logp_f32 and
rl8_ppo_loss_categorical_wide_fwd_bwd_f32 are declared, exported and bound, refuse bad arguments before any launch,
and compile for gfx950 without scratch (hence with none in their class loops)."""

import ctypes as C
import os
import re
import subprocess

import pytest

from rl8_amd import hip

from .test_kernel_resources import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rl8_categorical_wide_sample_logp_f32", "rl8_ppo_loss_categorical_wide_fwd_bwd_f32")
FAKE = 4096  # (never dereferenced: every call below fails its checks first)


def _header():
    with open(os.path.join(ROOT, "include", "rl8_amd.h")) as f:
        return f.read()


def test_entries_are_declared_exported_and_bound():
    header = _header()
    lib = hip.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert hasattr(lib, name) and name in hip.SIGNATURES, name
        params = re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1))
        assert len(params.split(",")) == len(hip.SIGNATURES[name]), name
    # the wide entries take what the narrow ones take
    assert hip.SIGNATURES[ENTRIES[0]] == hip.SIGNATURES["rl8_categorical_sample_logp_f32"]
    assert hip.SIGNATURES[ENTRIES[1]] == hip.SIGNATURES["rl8_ppo_loss_categorical_fwd_bwd_f32"]
    assert re.search(r"#define RL8_MAX_WIDE_CLASSES 65536\b", header)
    assert hip.MAX_WIDE_CLASSES == 65536 and hip.MAX_CLASSES == 64
    assert callable(hip.categorical_sample_logp_wide) and callable(hip.ppo_loss_categorical_wide)


def test_abi_version_is_unchanged():
    assert hip.abi_version()[0] == hip.ABI_VERSION == 107  # (new entries only: no bump)
    assert re.search(r"#define RL8_ABI_VERSION 107\b", _header())


def _sample(logits=FAKE, noise=None, action=FAKE, logp=FAKE, m=8, a=1, k=100):
    return hip.load().rl8_categorical_wide_sample_logp_f32(logits, noise, action, logp, m, a, k, 1, 0, 0, 0, None)


def _hp(**kw):
    return hip.ppo_hparams(**{**dict(clip_param=0.2, dual_clip_param=None, entropy_coeff=0.0, vf_clip_param=1.0,
                                     vf_coeff=1.0, grad_scale=1.0), **kw})


def _loss(logits=FAKE, value=FAKE, action=FAKE, logp_old=FAKE, adv=FAKE, ret=FAKE, m=8, a=1, k=100, hp=None,
          g_logits=FAKE, g_value=FAKE, sums=FAKE, scratch=FAKE, null_hp=False):
    hp = None if null_hp else C.byref(hp or _hp())
    return hip.load().rl8_ppo_loss_categorical_wide_fwd_bwd_f32(logits, value, action, logp_old, adv, ret, m, a, k, hp,
                                                              g_logits, g_value, sums, scratch, None)


@pytest.mark.parametrize("call", [_sample, _loss], ids=["sampler", "loss"])
def test_sizes_are_refused_before_any_launch(call):
    assert call(k=1) == -2 and call(k=0) == -2 and call(k=-5) == -2
    assert call(k=hip.MAX_WIDE_CLASSES + 1) == -2
    assert call(a=1 << 15, k=1 << 16) == -2  # a k = 2^31: the Philox word index would not fit
    assert call(a=(1 << 15) + 1, k=1 << 16) == -2
    assert call(m=0) == -2 and call(m=-1) == -2
    assert call(a=0) == -2


def test_null_pointers_are_refused_before_any_launch():
    for missing in ("logits", "action", "logp"):
        assert _sample(**{missing: None}) == -1, missing
    for missing in ("logits", "value", "action", "logp_old", "adv", "ret", "sums", "scratch"):
        assert _loss(**{missing: None}) == -1, missing
    assert _loss(g_logits=None) == -1 and _loss(g_value=None) == -1  # (both gradients, or neither)
    assert _loss(null_hp=True) == -1
    assert _loss(hp=_hp(clip_param=0.0)) == -4 and _loss(hp=_hp(vf_clip_param=0.0)) == -4


def test_the_python_wrappers_name_the_limit():
    import torch

    too_wide = torch.zeros(1, 1, hip.MAX_WIDE_CLASSES + 1)
    with pytest.raises(ValueError, match=str(hip.MAX_WIDE_CLASSES)):
        hip.categorical_sample_logp_wide(too_wide, None)
    one = torch.zeros(1, 1)
    with pytest.raises(ValueError, match=str(hip.MAX_WIDE_CLASSES)):
        hip.ppo_loss_categorical_wide(too_wide, one, one.long(), one, one, one, _hp())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_compiled_wide_kernels_use_no_scratch(tmp_path):
    """Every compiled variant -- the sampler, and the loss at 1, 2, 4, 8 and 16 register-held chunks of 64 classes and
    with the row read again, each with and without gradients -- has a private segment of 0 bytes and no scratch
    instruction anywhere, so none in a class loop; the widest register-held row leaves two waves per SIMD."""
    csrc = os.path.join(ROOT, "rl8_amd", "csrc")
    asm = tmp_path / "wide.s"
    subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{csrc}",
         "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "categorical_wide_kernels.hip")],
        check=True, capture_output=True, timeout=600,
    )
    text = asm.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    loss = [name for name, _ in kernels if "ppo_loss_categorical_wide_kernel" in name]
    assert len(loss) == 12 and sum("categorical_wide_sample_kernel" in name for name, _ in kernels) == 1
    assert len(kernels) == 13
    for name, body in kernels:
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert scratch == 0 and vgprs <= 256, (name, scratch, vgprs)
        code = text[text.index("\n" + name + ":"):]
        code = code[:code.index(".Lfunc_end")]
        assert "scratch_" not in code, name
        assert "global_load_dword" in code, name  # (the walked code is the kernel's: it reads its rows)
