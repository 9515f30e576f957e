"""The MFMA feedforward entries without a GPU: their envelope, their refusals before any launch, and the route's switch
(``RL8_AMD_WIDE_FEEDFORWARD``), after ``tests/test_feedforward_host.py``."""

import pytest
import torch

from rl8_amd import hip
from rl8_amd.nn import fused_feedforward

from .test_feedforward_host import _skip_block


def test_wide_supports_at_the_envelope_s_edges():
    supports = hip.load().rl8_feedforward_wide_supports
    assert supports(32, 64) == 0 and supports(33, 1) == 1 and supports(128, 512) == 1
    assert supports(129, 64) == 0 and supports(64, 513) == 0
    for args in ((0, 1), (64, 0), (-1, 64), (64, -64)):
        assert supports(*args) == -2, args
    assert hip.feedforward_wide_supports(64, 128) and not hip.feedforward_wide_supports(32, 128)
    limits = hip.feedforward_wide_limits()
    assert limits.tile_rows % 16 == 0 and limits.chunk % 16 == 0 and limits.grid_cap >= limits.wgrad_grid_cap >= 16
    floats = hip.feedforward_wide_workspace_floats
    assert floats(1, 64, 128) >= (2 * 64 * 128 + 128 + 64) + 2 * 64
    assert floats(10 ** 9, 128, 512) == floats(10 ** 10, 128, 512) < 2 ** 26
    with pytest.raises(ValueError, match="out of range"):
        floats(0, 64, 128)
    with pytest.raises(ValueError, match="unsupported"):
        floats(5, 32, 128)
    assert hip.ABI_VERSION == 107  # (new entries only: no bump)


def test_wide_entries_refuse_bad_arguments_before_launching():
    lib = hip.load()
    p = [4096 * (i + 1) for i in range(20)]  # (never dereferenced: every call fails its checks first)

    def forward(x=p[0], gamma=p[1], beta=p[2], w1=p[3], b1=p[4], w2=p[5], b2=p[6], rows=8, f=64, hidden=128, out=p[7]):
        return lib.rl8_feedforward_wide_f32(x, gamma, beta, 1e-5, w1, b1, w2, b2, rows, f, hidden, 1, out, None)

    def backward(x=p[0], dout=p[8], gamma=p[1], beta=p[2], w1=p[3], b1=p[4], w2=p[5], rows=8, f=64, hidden=128, dx=p[9],
                 dgamma=p[10], dbeta=p[11], dw1=p[12], db1=p[13], dw2=p[14], db2=p[15], workspace=p[16]):
        return lib.rl8_feedforward_wide_backward_f32(x, dout, gamma, beta, 1e-5, w1, b1, w2, rows, f, hidden, 1, dx,
                                                     dgamma, dbeta, dw1, db1, dw2, db2, workspace, None)

    inputs = ("x", "gamma", "beta", "w1", "b1", "w2")
    outputs = ("dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")
    for name in inputs + ("b2", "out"):
        assert forward(**{name: None}) == -1 and forward(**{name: p[17] + 2}) == -3, name
    for name in inputs + ("dout", "workspace"):
        assert backward(**{name: None}) == -1, name
    for name in outputs[1:]:  # the workspace as soon as one parameter gradient is wanted
        assert backward(workspace=None, **{other: None for other in outputs if other != name}) == -1, name
    for name in inputs + ("dout", "workspace") + outputs:
        assert backward(**{name: p[17] + 1}) == -3, name
    for name in ("rows", "f", "hidden"):
        assert forward(**{name: 0}) == -2 and backward(**{name: -1}) == -2, name
    for shape in (dict(f=32), dict(f=129), dict(hidden=513)):
        assert forward(**shape) == -4 and backward(**shape) == -4, shape
    nothing = {name: None for name in outputs}
    assert backward(workspace=None, **nothing) == 0  # no output wanted: nothing to do
    assert backward(workspace=None, f=32, **nothing) == -4 and backward(workspace=None, x=None, **nothing) == -1


def test_skip_feedforward_takes_a_wide_block_only_with_its_own_switch(monkeypatch):
    reached = []

    class Reached:
        @staticmethod
        def apply(*args):
            reached.append(args)
            raise RuntimeError("reached the kernels")

    block = _skip_block("residual", 64, 128, torch.Generator().manual_seed(3))._layers[1]
    y = torch.zeros(3, 5, 64)

    def taken() -> bool:
        try:
            return fused_feedforward.skip_feedforward(block, y, "residual") is not None
        except RuntimeError as err:
            assert "reached the kernels" in str(err)
            return True

    monkeypatch.setattr(fused_feedforward, "_FeedforwardBlock", Reached)  # (one node for both families)
    monkeypatch.delenv("RL8_AMD_FEEDFORWARD_KERNELS", raising=False)
    monkeypatch.setenv("RL8_AMD_WIDE_FEEDFORWARD", "1")
    assert not taken()  # (a CPU tensor, whatever the switch says)
    monkeypatch.setattr(fused_feedforward, "_on_device", lambda t: True)  # (host tensors stand in for HIP ones)
    assert taken() and reached[0][0] is y and reached[0][7:] == (block[0].eps, True)
    monkeypatch.setenv("RL8_AMD_FEEDFORWARD_KERNELS", "1")  # (the narrow family's switch is not this family's)
    for value in ("0", "true"):
        monkeypatch.setenv("RL8_AMD_WIDE_FEEDFORWARD", value)
        assert not taken()
    monkeypatch.delenv("RL8_AMD_WIDE_FEEDFORWARD")
    assert not taken()
    assert len(reached) == 1
