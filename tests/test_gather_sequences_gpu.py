"""``rl8_gather_sequences`` / ``hip.gather_sequences``: whole sequences out of time-major buffer leaves of 1-, 4- and
8-byte elements (a dict observation's bool mask beside its int64 and float32 leaves), byte-equal to torch indexing."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

from rl8_amd import hip  # noqa: E402

DEV = "cuda"
N, H = 7, 12


def _leaves(gen: torch.Generator) -> list[torch.Tensor]:
    """[N, H + 1, d] views of time-major [H + 1, N, d] storage, as the rollout buffer hands them out."""
    def rand(d: int, dtype: torch.dtype) -> torch.Tensor:
        if dtype == torch.bool:
            t = torch.rand(H + 1, N, d, device=DEV, generator=gen) < 0.5
        elif dtype == torch.int64:
            t = torch.randint(-2 ** 40, 2 ** 40, (H + 1, N, d), device=DEV, generator=gen)
        else:
            t = torch.randn(H + 1, N, d, device=DEV, generator=gen)
        return t.transpose(0, 1)

    return [rand(3, torch.bool), rand(1, torch.int64), rand(1, torch.float32), rand(5, torch.float32)]


def _index(kind: str, seqs: int, gen: torch.Generator) -> None | torch.Tensor:
    if kind == "none":
        return None
    if kind == "permutation":
        return torch.randperm(seqs, device=DEV, generator=gen)
    return torch.randint(0, seqs, (2 * seqs + 1,), device=DEV, generator=gen)[: max(1, seqs // 2 + 2)].contiguous()


def _expected(leaf: torch.Tensor, index: None | torch.Tensor, seq_len: int) -> torch.Tensor:
    per_env = H // seq_len
    q = torch.arange(N * per_env, device=DEV) if index is None else index
    env, s = q // per_env, q % per_env
    t = s[:, None] * seq_len + torch.arange(seq_len, device=DEV)[None, :]
    return leaf[env[:, None], t].reshape(-1, *leaf.shape[2:])


@pytest.mark.parametrize("kind", ["none", "permutation", "subset-with-repeats"])
@pytest.mark.parametrize("seq_len", [1, 4, 12])
def test_sequences_are_byte_equal_to_torch_indexing(seq_len, kind):
    gen = torch.Generator(device=DEV).manual_seed(10 * seq_len + len(kind))
    leaves = _leaves(gen)
    seqs = N * (H // seq_len)
    index = _index(kind, seqs, gen)
    if kind == "subset-with-repeats":
        index[-1] = index[0]  # (at least one repeat)
    got = hip.gather_sequences(index, seq_len, H, leaves)
    rows = (seqs if index is None else index.numel()) * seq_len
    for leaf, out in zip(leaves, got):
        assert out.dtype == leaf.dtype and out.shape == (rows, *leaf.shape[2:]) and out.is_contiguous()
        want = _expected(leaf, index, seq_len).contiguous()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), leaf.dtype


@pytest.mark.parametrize("seq_len", [1, 4, 12])
def test_nothing_is_written_around_the_destinations(seq_len):
    """The entry itself, each destination inside an allocation of 0xA5 bytes (the bool[3] leaf at an odd offset)."""
    gen = torch.Generator(device=DEV).manual_seed(seq_len)
    leaves = _leaves(gen)
    index = torch.randperm(N * (H // seq_len), device=DEV, generator=gen)[:5].contiguous()
    rows = index.numel() * seq_len
    fields = (hip.GatherField * len(leaves))()
    guards = []
    for i, leaf in enumerate(leaves):
        row = leaf.shape[2]
        nbytes = rows * row * leaf.element_size()
        off = 8 + (3 if leaf.element_size() == 1 else 0)
        raw = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        fields[i] = hip.GatherField(leaf.data_ptr(), raw.data_ptr() + off, leaf.stride(0), leaf.stride(1), row,
                                    leaf.element_size())
        guards.append((raw, off, nbytes, leaf))
    status = hip.load().rl8_gather_sequences(index.data_ptr(), index.numel(), seq_len, H, fields, len(leaves),
                                             hip._stream())
    assert status == 0
    torch.cuda.synchronize()
    for raw, off, nbytes, leaf in guards:
        assert bool((raw[:off] == 0xA5).all()) and bool((raw[off + nbytes:] == 0xA5).all()), leaf.dtype
        want = _expected(leaf, index, seq_len).contiguous().view(torch.uint8).reshape(-1)
        assert torch.equal(raw[off:off + nbytes], want), leaf.dtype


def test_field_count_and_element_width_are_checked():
    gen = torch.Generator(device=DEV).manual_seed(0)
    leaf = _leaves(gen)[2]
    outs = hip.gather_sequences(None, 4, H, [leaf] * hip.MAX_GATHER_FIELDS)
    assert len(outs) == 8 and all(torch.equal(o, outs[0]) for o in outs)
    with pytest.raises(ValueError, match="at most 8 leaves"):
        hip.gather_sequences(None, 4, H, [leaf] * 9)
    fields = (hip.GatherField * 9)(*[hip.GatherField(leaf.data_ptr(), outs[0].data_ptr(), leaf.stride(0), leaf.stride(1),
                                                     1, 4)] * 9)
    assert hip.load().rl8_gather_sequences(None, N * 3, 4, H, fields, 9, hip._stream()) == -2
    halves = torch.zeros(H + 1, N, 2, dtype=torch.int16, device=DEV).transpose(0, 1)
    with pytest.raises(ValueError, match="unsupported combination"):  # RL8_ECONFIG
        hip.gather_sequences(None, 4, H, [halves])
    with pytest.raises(ValueError, match="multiple of seq_len"):
        hip.gather_sequences(None, 5, H, [leaf])
