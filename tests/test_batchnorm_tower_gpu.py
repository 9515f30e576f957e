"""The BatchNorm tower route on the GPU: ``rl8_tower_moments_f64``, ``rl8_batchnorm_fold_f32`` and
``rl8_mlp_narrow_backward_dx_f32`` as raw entries, ``fused_mlp.tower_forward`` on ``"narrow_bn"`` towers with
``RL8_AMD_BATCHNORM_TOWERS`` ``1`` against ``0``, plain narrow towers whose input asks for a gradient, and the two
traders.

Yardsticks.  ``ref64``: the torch modules in float64 under autograd (``tests/test_batchnorm_tower_host.py`` pins
``fused_mlp.batchnorm_tower_reference`` to them at 1e-12).  ``torch32``: the same modules, eager, in float32 on the
device -- what runs with the switch off.

Inputs are seeded on the CPU and drawn until the comparison is well-conditioned, checked in float64: every channel's
batch variance of z1 is at least 1e-2 (``1 / sqrt(v + eps)`` amplifies nothing) and no pre-activation behind the norm or
in layer 2 is nearer to 0 than 1e-4 (no ReLU gate differs between float32 and float64; a gate that does moves a gradient
by one whole sample's contribution, which says nothing about a kernel).  Offending rows are drawn again (plain towers)
or moved by 5e-3 (BatchNorm towers, where a new row would move every other row's pre-activations through the batch
statistics); a draw that fails the variance condition is replaced as a whole.

Bars (the "3x the yardstick's own error + floor" rule of DESIGN.md section 5 / 8):
* outputs and running statistics, elementwise: ``|got - ref64| <= 3 max|torch32 - ref64| + 1e-6 + 1e-5 |ref64|``;
* dx and each parameter gradient: ``|got - ref64| <= 3 max|torch32 - ref64| + 2e-5 max|ref64| + 1e-9``
  (``db1`` in training mode is 0 up to rounding in ``ref64``: the bar is the absolute floor);
* moments against torch in float64: ``C`` within ``m 2^-52 max|x - p|^2`` (fp64 summation of m terms of that size),
  ``mu`` within ``m 2^-52 max|x - p| + 2^-52 max|x|`` (the sum, and the final ``p + S1 / m``).
Each case prints ``max|got - ref64| / max|torch32 - ref64|`` per tensor before it asserts (measured on an MI355X: the
dx entry 0.45 .. 1.88 and up to 3.69 at m = 1; the route: out 0.66 .. 1.57, dx 0.58 .. 1.24, dw1 0.17 .. 1.60, dgamma
0.60 .. 1.32, dbeta 0.69 .. 1.80, dw2 0.11 .. 3.43, db2 0.79 .. 1.68, dw3 0.17 .. 2.18, db3 0.09 .. 1.00, the running statistics
0.23 .. 1.00, the ratios above 3 at one and three rows where the floor carries the bar; the traders 0.02 .. 1.52 and
``invested_embedding.weight`` of ``MLPTrader`` 7.90, under its floor).
"""

import copy
import functools
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rl8_amd import AlgorithmConfig, hip  # noqa: E402
from rl8_amd.envs import AlgoTrading, MLPTrader, TransformerTrader, algotrading_models  # noqa: E402
from rl8_amd.nn import MLP, fused_mlp  # noqa: E402

DEV = "cuda"
GUARD = 64
SWITCH = "RL8_AMD_BATCHNORM_TOWERS"
ROUTE_TIMERS = ("tower_moments", "batchnorm_fold", "mlp_narrow_forward", "mlp_narrow_backward",
                "mlp_narrow_backward_dx", "mlp_narrow_reduce")


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def guarded(numel: int, dtype=torch.float32, shift: int = 0):
    """A sentinel-filled buffer and the ``numel`` elements ``GUARD + shift`` into it that a kernel may write."""
    buf = torch.full((numel + shift + 2 * GUARD,), -77.0, dtype=dtype, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + numel]


def assert_guards(buf, inner, what: str) -> None:
    front = (inner.data_ptr() - buf.data_ptr()) // buf.element_size()
    assert bool((buf[:front] == -77).all()) and bool((buf[front + inner.numel():] == -77).all()), \
        f"{what}: wrote outside its output"
    assert not bool((inner == -77).any()), f"{what}: an element was not written"


def placed(t: torch.Tensor, shift: int = 0) -> torch.Tensor:
    """A device copy of ``t`` whose base pointer sits ``shift`` elements into its allocation."""
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=DEV)
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


def launches() -> dict[str, int]:
    return {name: int(s["launches"]) for name, s in hip.timer.summary().items() if name in ROUTE_TIMERS}


class counted:
    """Context in which ``hip.timer`` counts the route's launches; ``.ran`` afterwards."""

    def __enter__(self):
        hip.timer.reset()
        hip.timer.enabled = True
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ran = launches()
        finally:
            hip.timer.enabled = False
        return False


def grad_bar(want: torch.Tensor, torch_err: float) -> float:
    return 3 * torch_err + 2e-5 * float(want.abs().max()) + 1e-9


def value_bar(want: torch.Tensor, torch_err: float) -> torch.Tensor:
    return 3 * torch_err + 1e-6 + 1e-5 * want.abs()


def hold(name: str, got, want, t32, *, value: bool, figures: list) -> None:
    got, want, t32 = got.double().cpu(), want.double().cpu(), t32.double().cpu()
    assert got.shape == want.shape and not torch.isnan(got).any(), name
    err, torch_err = float((got - want).abs().max()), float((t32 - want).abs().max())
    figures.append(f"{name} {err:.2e} / {torch_err:.2e} = {err / torch_err if torch_err else math.nan:.2f}")
    bar = value_bar(want, torch_err) if value else torch.full_like(want, grad_bar(want, torch_err))
    assert bool(((got - want).abs() <= bar).all()), (name, err, torch_err, figures)


# --- the moments ----------------------------------------------------------------------------------------------------
def moments_rows() -> list[int]:
    limits = hip.tower_limits()
    return [1, 2, 63, 64, 65, 4099, limits.moments_grid_cap * limits.moments_rows + 77]


def run_moments(x: torch.Tensor, shift: int = 0):
    m, d_in = x.shape
    lib = hip.load()
    xd = placed(x, shift)
    mbuf, mu = guarded(d_in, torch.float64)
    cbuf, cov = guarded(d_in * d_in, torch.float64)
    wbuf, ws = guarded(int(lib.rl8_tower_moments_workspace_bytes(m, d_in)) // 8, torch.float64)
    assert lib.rl8_tower_moments_f64(ptr(xd), m, d_in, ptr(mu), ptr(cov), ptr(ws), stream()) == 0
    for buf, inner, what in ((mbuf, mu, "mu"), (cbuf, cov, "C"), (wbuf, ws, "workspace")):
        assert_guards(buf, inner, what)
    return mu.cpu(), cov.view(d_in, d_in).cpu()


def assert_moments(x: torch.Tensor, shift: int = 0):
    m, d_in = x.shape
    mu, cov = run_moments(x, shift)
    xd = x.double()
    want_mu = xd.mean(0)
    want_cov = (xd - want_mu).t() @ (xd - want_mu) / m
    d = float((xd - xd[0]).abs().max())
    mu_err, cov_err = float((mu - want_mu).abs().max()), float((cov - want_cov).abs().max())
    mu_bar, cov_bar = m * 2.0 ** -52 * d + 2.0 ** -52 * float(xd.abs().max()), m * 2.0 ** -52 * d * d
    print(f"m {m} d_in {d_in}: mu {mu_err:.2e} (bar {mu_bar:.2e})  C {cov_err:.2e} (bar {cov_bar:.2e})")
    assert mu_err <= mu_bar and cov_err <= cov_bar
    assert torch.equal(cov, cov.t())
    mu2, cov2 = run_moments(x, shift)
    assert torch.equal(mu, mu2) and torch.equal(cov, cov2), "two runs differ"
    return mu, cov


@pytest.mark.parametrize("d_in", [1, 7, 16])
@pytest.mark.parametrize("index", range(7))
def test_moments_against_torch_in_float64(index, d_in):
    m = moments_rows()[index]
    assert_moments(torch.randn(m, d_in, generator=gen(10 * index + d_in)))


def test_moments_of_rows_of_mean_30_a_constant_column_and_a_shifted_base_pointer():
    x = torch.randn(4099, 7, generator=gen(3)) + 30.0
    assert_moments(x)
    x[:, 2] = 4.25
    mu, cov = assert_moments(x, shift=1)
    assert float(mu[2]) == 4.25
    assert not bool(cov[2].any()) and not bool(cov[:, 2].any()), "a constant column has a variance that is not exactly 0"
    assert bool((cov.diagonal()[[0, 1, 3, 4, 5, 6]] > 0.5).all())


# --- the fold -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,d_in", [(64, 1), (64, 11), (128, 7), (128, 16)])
def test_fold_against_the_reference_expression_in_float64(hidden, d_in):
    g = gen(hidden + d_in)
    x = torch.randn(257, d_in, generator=g) + 1.5
    w1, b1 = torch.randn(hidden, d_in, generator=g) / d_in ** 0.5, torch.randn(hidden, generator=g)
    gamma, beta = torch.rand(hidden, generator=g) + 0.5, torch.randn(hidden, generator=g)
    rm, rv = torch.randn(hidden, generator=g), torch.rand(hidden, generator=g) + 0.5
    eps, factor = 1e-5, 0.1
    mu, cov = hip.tower_moments(x.to(DEV))
    d = [t.to(DEV) for t in (w1, b1, gamma, beta)]
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    a, c, r, m_z, v = hip.batchnorm_fold(*d, eps, moments=(mu, cov, 257), running_mean=rmd, running_var=rvd, factor=factor)
    w = [t.double() for t in (w1, b1, gamma, beta)]
    wa, wc, wr, wm, wv = fused_mlp._fold_training(mu.cpu(), cov.cpu(), *w, eps)
    for name, got, want, rel in (("A", a, wa, 2.0 ** -24), ("c", c, wc, 2.0 ** -24), ("r", r, wr, 2.0 ** -48),
                                 ("m_z", m_z, wm, 2.0 ** -48), ("v", v, wv, 2.0 ** -48)):
        # (fp32 outputs: formed in fp64 and rounded once, half an ulp; fp64 outputs: a few ulps of fp64 chains)
        err = (got.double().cpu() - want).abs()
        assert bool((err <= rel * want.abs() + 2.0 ** -48 * float(want.abs().max())).all()), (name, float(err.max()))
    want_rm = (1 - factor) * rm.double() + factor * wm
    want_rv = (1 - factor) * rv.double() + factor * wv * (257 / 256)
    assert bool(((rmd.double().cpu() - want_rm).abs() <= 2.0 ** -24 * want_rm.abs() + 1e-12).all())
    assert bool(((rvd.double().cpu() - want_rv).abs() <= 2.0 ** -24 * want_rv.abs() + 1e-12).all())
    # the cumulative factor from the device counter; eval mode from the running statistics, nothing else written
    tracked = torch.tensor(4, dtype=torch.int64, device=DEV)
    rm4 = rm.to(DEV)
    hip.batchnorm_fold(*d, eps, moments=(mu, cov, 257), running_mean=rm4, running_var=rv.to(DEV), tracked=tracked)
    want_rm4 = 0.75 * rm.double() + 0.25 * wm
    assert bool(((rm4.double().cpu() - want_rm4).abs() <= 2.0 ** -24 * want_rm4.abs() + 1e-12).all())
    before = (rmd.clone(), rvd.clone())
    ea, ec = hip.batchnorm_fold(*d, eps, running_mean=rmd, running_var=rvd)
    wea, wec, _ = fused_mlp._fold_eval(*w, rmd.double().cpu(), rvd.double().cpu(), eps)
    assert bool(((ea.double().cpu() - wea).abs() <= 2.0 ** -24 * wea.abs() + 1e-12).all())
    assert bool(((ec.double().cpu() - wec).abs() <= 2.0 ** -24 * wec.abs() + 1e-12).all())
    assert torch.equal(rmd, before[0]) and torch.equal(rvd, before[1])


# --- the plain narrow tower and its dx entry -----------------------------------------------------------------------
DX_SHAPES = [(64, 1, 1), (64, 7, 3), (128, 11, 1), (128, 16, 8)]


def dx_rows(hidden: int) -> list[int]:
    limits = hip.tower_limits()
    cap = limits.narrow_grid_cap_64 if hidden == 64 else limits.narrow_grid_cap_128
    return [1, 63, 64, 65, 257, cap * limits.narrow_rows + 77]


def plain_parameters(hidden: int, d_in: int, n: int, seed: int) -> dict[str, torch.Tensor]:
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        layers = nn.Linear(d_in, hidden), nn.Linear(hidden, hidden), nn.Linear(hidden, n)
    return {f"{k}{i + 1}": getattr(layer, attr).detach().clone()
            for i, layer in enumerate(layers) for k, attr in (("w", "weight"), ("b", "bias"))}


def plain_pre_activations(x, p):
    z1 = x @ p["w1"].t() + p["b1"]
    return z1, torch.relu(z1) @ p["w2"].t() + p["b2"]


def plain_with_grads(x, p, dout):
    """``(out, dx, dw1, db1, dw2, db2, dw3, db3)`` of the plain tower under autograd, in the dtype of the operands."""
    x = x.clone().requires_grad_(True)
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    _, z2 = plain_pre_activations(x, q)
    out = torch.relu(z2) @ q["w3"].t() + q["b3"]
    out.backward(dout)
    return (out.detach(), x.grad) + tuple(q[k].grad for k in ("w1", "b1", "w2", "b2", "w3", "b3"))


@functools.lru_cache(maxsize=None)
def plain_case(shape_index: int, row_index: int) -> dict:
    hidden, d_in, n = DX_SHAPES[shape_index]
    m = dx_rows(hidden)[row_index]
    seed = 100 * shape_index + row_index
    g = gen(seed)
    p = plain_parameters(hidden, d_in, n, seed + 1000)
    p64 = {k: v.double() for k, v in p.items()}
    x = torch.randn(m, d_in, generator=g)
    for _ in range(64):
        z1, z2 = plain_pre_activations(x.double(), p64)
        close = (z1.abs() < 1e-4).any(-1) | (z2.abs() < 1e-4).any(-1)
        if not bool(close.any()):
            break
        x[close] = torch.randn(int(close.sum()), d_in, generator=g)
    else:
        raise AssertionError("rows with a pre-activation at 0 after 64 rounds")
    dout = torch.randn(m, n, generator=g)
    ref64 = plain_with_grads(x.double(), p64, dout.double())
    torch32 = plain_with_grads(x.to(DEV), {k: v.to(DEV) for k, v in p.items()}, dout.to(DEV))
    return dict(x=x, dout=dout, p=p, ref64=ref64, torch32=tuple(t.cpu() for t in torch32))


def run_backward_entries(x, dout, p):
    """The workspace of ``rl8_mlp_narrow_backward_f32``, of the dx entry with ``dx == NULL`` and with ``dx`` set, and
    ``dx``; workspaces and ``dx`` between guard words."""
    m, d_in = x.shape
    hidden, n = p["w1"].shape[0], p["w3"].shape[0]
    lib = hip.load()
    xd, gd = x.to(DEV), dout.to(DEV)
    d = {k: v.to(DEV) for k, v in p.items()}
    weights = [ptr(d[k]) for k in ("w1", "b1", "w2", "b2", "w3")]
    floats = int(lib.rl8_mlp_narrow_workspace_bytes(m, hidden, d_in, n)) // 4
    spaces = [guarded(floats) for _ in range(3)]
    dbuf, dx = guarded(m * d_in)
    assert lib.rl8_mlp_narrow_backward_f32(ptr(xd), ptr(gd), m, d_in, *weights, n, hidden, ptr(spaces[0][1]), stream()) == 0
    assert lib.rl8_mlp_narrow_backward_dx_f32(ptr(xd), ptr(gd), m, d_in, *weights, n, hidden, ptr(spaces[1][1]), None,
                                              stream()) == 0
    assert lib.rl8_mlp_narrow_backward_dx_f32(ptr(xd), ptr(gd), m, d_in, *weights, n, hidden, ptr(spaces[2][1]), ptr(dx),
                                              stream()) == 0
    for i, (buf, inner) in enumerate(spaces):
        assert_guards(buf, inner, f"workspace {i}")
    assert_guards(dbuf, dx, "dx")
    return [inner for _, inner in spaces], dx.view(m, d_in)


@pytest.mark.parametrize("row_index", range(6))
@pytest.mark.parametrize("shape_index", range(len(DX_SHAPES)))
def test_dx_entry_against_float64_and_the_workspace_bit_for_bit(shape_index, row_index):
    c = plain_case(shape_index, row_index)
    spaces, dx = run_backward_entries(c["x"], c["dout"], c["p"])
    assert torch.equal(spaces[0], spaces[1]), "dx == NULL: the workspace differs from rl8_mlp_narrow_backward_f32's"
    assert torch.equal(spaces[0], spaces[2]), "dx set: the workspace differs from rl8_mlp_narrow_backward_f32's"
    figures: list = []
    try:
        hold("dx", dx, c["ref64"][1], c["torch32"][1], value=False, figures=figures)
    finally:
        print(f"{DX_SHAPES[shape_index]} m {c['x'].shape[0]}: " + "  ".join(figures))


def test_a_closed_gate_contributes_exactly_nothing_to_dx():
    hidden, d_in, n, m, j = 64, 7, 3, 257, 17
    g = gen(71)
    p = plain_parameters(hidden, d_in, n, 72)
    x, dout = torch.randn(m, d_in, generator=g), torch.randn(m, n, generator=g)
    x[:, 0] = 0.5
    p["w1"][j] = 0.0
    p["w1"][j, 0] = 2.0
    p["b1"][j] = -1.0  # z1_j = -1 + 2 * 0.5 = +0 exactly on every row: the gate is closed
    _, dx = run_backward_entries(x, dout, p)
    other = {k: v.clone() for k, v in p.items()}
    other["w2"][:, j] = 1000.0 * torch.randn(hidden, generator=g)  # what would come back through the unit changes ...
    _, dx2 = run_backward_entries(x, dout, other)
    assert torch.equal(dx, dx2)  # ... and its share of dx stays exactly 0
    open_gate = {k: v.clone() for k, v in other.items()}
    open_gate["b1"][j] = -0.5
    _, dx3 = run_backward_entries(x, dout, open_gate)
    assert not torch.equal(dx, dx3)


def plain_tower(hidden: int, d_in: int, n: int, p: dict) -> nn.Sequential:
    net = nn.Sequential(MLP(d_in, (hidden, hidden)), nn.ReLU(), nn.Linear(hidden, n))
    with torch.no_grad():
        for layer, i in ((net[0][0], 1), (net[0][2], 2), (net[2], 3)):
            layer.weight.copy_(p[f"w{i}"])
            layer.bias.copy_(p[f"b{i}"])
    return net.to(DEV)


@pytest.mark.parametrize("shape_index", [1, 3])
def test_plain_narrow_tower_gives_its_input_a_gradient(shape_index):
    c = plain_case(shape_index, 4)
    hidden, d_in, n = DX_SHAPES[shape_index]
    net = plain_tower(hidden, d_in, n, c["p"])
    assert fused_mlp._family(net[:2], [net[2]])[0] == "narrow"
    runs = []
    for wants in (True, False):
        net.zero_grad()
        x = c["x"].to(DEV).requires_grad_(wants)
        with counted() as count:
            out = fused_mlp.tower_forward(net[:2], [net[2]], x)
            out.backward(c["dout"].to(DEV))
        runs.append((out.detach(), x.grad, [q.grad.clone() for q in net.parameters()], count.ran))
    (out, dx, grads, ran), (out0, dx0, grads0, ran0) = runs
    assert ran == {"mlp_narrow_forward": 1, "mlp_narrow_backward_dx": 1, "mlp_narrow_reduce": 1}
    assert ran0 == {"mlp_narrow_forward": 1, "mlp_narrow_backward": 1, "mlp_narrow_reduce": 1} and dx0 is None
    assert torch.equal(out, out0) and all(torch.equal(a, b) for a, b in zip(grads, grads0))
    # the route without dx is the parent's: the old entries, called directly, give the same bits
    d = {k: v.to(DEV) for k, v in c["p"].items()}
    old = hip.mlp_narrow_backward(c["x"].to(DEV), c["dout"].to(DEV), d["w1"], d["b1"], d["w2"], d["b2"], d["w3"])
    for q, key in zip(grads0, ("w1", "b1", "w2", "b2", "w3", "b3")):
        assert torch.equal(q, old[key]), key
    figures: list = []
    try:
        hold("out", out, c["ref64"][0], c["torch32"][0], value=True, figures=figures)
        hold("dx", dx, c["ref64"][1], c["torch32"][1], value=False, figures=figures)
    finally:
        print("  ".join(figures))


# --- the whole route ------------------------------------------------------------------------------------------------
ROUTE_SHAPES = [(3, 7, 128, 3), (67, 11, 64, 3), (257, 16, 128, 8), (4099, 7, 128, 1)]
GRADS = ("dx", "dw1", "db1", "dgamma", "dbeta", "dw2", "db2", "dw3", "db3")


def bn_tower(d_in: int, width: int, n: int, momentum, seed: int) -> nn.Sequential:
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        net = nn.Sequential(MLP(d_in, (width, width), norm_layer=nn.BatchNorm1d), nn.ReLU(), nn.Linear(width, n))
        norm = net[0][1]
        norm.momentum = momentum
        with torch.no_grad():
            norm.weight.uniform_(0.5, 1.5)
            norm.bias.normal_()
            norm.running_mean.normal_(std=0.3)
            norm.running_var.uniform_(0.5, 2.0)
            norm.num_batches_tracked.fill_(3)
    return net


def conditions(net64: nn.Sequential, x64: torch.Tensor):
    """(every channel's batch variance of z1 >= 1e-2, rows with a |y| or |z2| below 1e-4), in float64 in the mode the
    tower is in."""
    with torch.no_grad():
        probe = copy.deepcopy(net64)
        z1 = probe[0][0](x64)
        y = probe[0][1](z1)
        z2 = probe[0][3](torch.relu(y))
    return bool((z1.var(0, unbiased=False) >= 1e-2).all()), (y.abs() < 1e-4).any(-1) | (z2.abs() < 1e-4).any(-1)


def run_tower(net: nn.Sequential, x: torch.Tensor, dout: torch.Tensor) -> dict:
    """Outputs, gradients and statistics of one forward + backward of a COPY of ``net`` through the traders' route
    (``algotrading_models._tower``: the kernels where they take the call, else the modules)."""
    net = copy.deepcopy(net)
    x = x.clone().requires_grad_(True)
    out = algotrading_models._tower(net, x)
    out.backward(dout)
    l1, norm, l2, head = net[0][0], net[0][1], net[0][3], net[2]
    return dict(out=out.detach(), dx=x.grad, dw1=l1.weight.grad, db1=l1.bias.grad, dgamma=norm.weight.grad,
                dbeta=norm.bias.grad, dw2=l2.weight.grad, db2=l2.bias.grad, dw3=head.weight.grad, db3=head.bias.grad,
                running_mean=norm.running_mean.clone(), running_var=norm.running_var.clone(),
                num_batches_tracked=int(norm.num_batches_tracked))


@functools.lru_cache(maxsize=None)
def route_case(index: int, training: bool, momentum) -> dict:
    rows, d_in, width, n = ROUTE_SHAPES[index]
    scale = 8.0 if rows < 16 else 1.0  # (three rows: a wide spread keeps every channel's variance off 0)
    for draw in range(64):
        seed = 500 + 10 * index + 1000 * draw
        g = gen(seed)
        net = bn_tower(d_in, width, n, momentum, seed + 1).train(training)
        net64 = copy.deepcopy(net).double()
        x = scale * torch.randn(rows, d_in, generator=g)
        for _ in range(64):
            spread, close = conditions(net64, x.double())
            if not spread or not bool(close.any()):
                break
            # (moved a little, not drawn again: a new row moves the batch statistics, hence every other row's
            # pre-activations, by about the width of the window that is being cleared)
            x[close] += 5e-3 * scale * torch.randn(int(close.sum()), d_in, generator=g)
        spread, close = conditions(net64, x.double())
        if spread and not bool(close.any()):
            break
    else:
        raise AssertionError("no well-conditioned draw")
    dout = torch.randn(rows, n, generator=g)
    ref64 = run_tower(net64, x.double(), dout.double())
    return dict(net=net, x=x, dout=dout, ref64=ref64)


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("index", range(len(ROUTE_SHAPES)))
def test_route_on_against_off_and_float64(monkeypatch, index, training, momentum):
    c = route_case(index, training, momentum)
    net, x, dout = c["net"].to(DEV), c["x"].to(DEV), c["dout"].to(DEV)
    runs = {}
    for switch in ("1", "1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        with counted() as count:
            got = run_tower(net, x, dout)
        if switch == "1" and "1" in runs:  # the second run with the kernels: the same bits
            for name in ("out",) + GRADS + ("running_mean", "running_var"):
                assert torch.equal(got[name], runs["1"][0][name]), f"{name}: two runs differ"
        runs[switch] = (got, count.ran)
    (on, ran_on), (off, ran_off) = runs["1"], runs["0"]
    want_launches = {"batchnorm_fold": 1, "mlp_narrow_forward": 1, "mlp_narrow_backward_dx": 1, "mlp_narrow_reduce": 1}
    if training:
        want_launches["tower_moments"] = 1
    assert ran_on == want_launches and ran_off == {}
    ref = c["ref64"]
    assert on["num_batches_tracked"] == off["num_batches_tracked"] == ref["num_batches_tracked"] == (4 if training else 3)
    figures: list = []
    try:
        hold("out", on["out"], ref["out"], off["out"], value=True, figures=figures)
        for name in GRADS:
            if name == "db1" and training:  # (0 up to rounding in float64: the absolute floor alone)
                assert float(on["db1"].abs().max()) <= 1e-9 + 2e-5 * float(ref["db1"].abs().max())
                continue
            hold(name, on[name], ref[name], off[name], value=False, figures=figures)
        for name in ("running_mean", "running_var"):
            hold(name, on[name], ref[name], off[name], value=True, figures=figures)
    finally:
        print(f"{ROUTE_SHAPES[index]} training {training} momentum {momentum}: " + "  ".join(figures))


def test_calls_the_route_declines_run_the_modules(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    net = bn_tower(7, 128, 3, 0.1, 5).to(DEV)
    trunk, heads = net[:2], [net[2]]
    x = torch.randn(67, 7, generator=gen(6)).to(DEV)
    with counted() as count:
        assert fused_mlp.tower_forward(trunk, heads, x[:1]) is None  # one row in training mode
        with pytest.raises(ValueError):
            algotrading_models._tower(net, x[:1])  # (torch's own)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert fused_mlp.tower_forward(trunk, heads, x) is None
        wide = torch.randn(67, 14, generator=gen(7)).to(DEV)[:, ::2]
        assert not wide.is_contiguous() and fused_mlp.tower_forward(trunk, heads, wide) is None
        assert fused_mlp.tower_forward(trunk, heads, x.double()) is None
        assert fused_mlp.tower_forward(trunk, heads, x[:0]) is None
        assert torch.equal(algotrading_models._tower(copy.deepcopy(net), wide), copy.deepcopy(net)(wide))
    assert count.ran == {}
    net.eval()
    with counted() as count:
        assert fused_mlp.tower_forward(trunk, heads, x[:1]) is not None  # (one row is fine in eval mode)
    assert count.ran == {"batchnorm_fold": 1, "mlp_narrow_forward": 1}


# --- the traders ----------------------------------------------------------------------------------------------------
NUM_ENVS, HORIZON, BATCH = 64, 32, 67


def trader_outputs(model, views, weights) -> dict:
    """Logits, values and the gradient of ``sum(w_l * logits) + sum(w_v * values)`` with respect to every parameter of
    a COPY of ``model`` on the batch ``views``."""
    model = copy.deepcopy(model)
    model.zero_grad()
    logits = model(views)["logits"]
    values = model.value_function()
    raw = logits.reshape(-1, 3)
    open_actions = raw > -1e30  # (masked logits are a constant: they carry no gradient and no information)
    scalar = (torch.where(open_actions, raw, torch.zeros_like(raw)) * weights[0].to(raw.dtype)).sum() \
        + (values.reshape(-1) * weights[1].to(values.dtype)).sum()
    scalar.backward()
    grads = {name: p.grad for name, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()), [n for n, g in grads.items() if g is None]
    return dict(logits=torch.where(open_actions, raw, torch.zeros_like(raw)).detach(), values=values.detach().reshape(-1),
                grads=grads, tracked=int(model.feature_model[0][1].num_batches_tracked))


@pytest.mark.parametrize("model_cls,width,d_in", [(MLPTrader, 128, 7), (TransformerTrader, 64, 11)])
def test_traders_on_the_route(monkeypatch, model_cls, width, d_in):
    monkeypatch.setenv(SWITCH, "0")
    torch.manual_seed(0)
    algo = AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, model_cls=model_cls, model_config={"seq_len": 4},
                           num_sgd_iters=1).build(AlgoTrading)
    algo.collect()
    model = algo.policy.model
    assert model.feature_model[0][0].in_features == d_in and model.feature_model[0][0].out_features == width
    views = model.apply_view_requirements(algo.buffer[:, :-1, ...], kind="all")
    index = torch.randperm(NUM_ENVS * HORIZON, generator=gen(11))[:BATCH].to(DEV)
    views = views[index]
    weights = (torch.randn(BATCH, 3, generator=gen(12)).to(DEV), torch.randn(BATCH, generator=gen(13)).to(DEV))
    model64 = copy.deepcopy(model).double()
    views64 = views.apply(lambda t: t.double() if t.is_floating_point() else t)
    ref = trader_outputs(model64, views64, weights)
    off = trader_outputs(model, views, weights)
    monkeypatch.setenv(SWITCH, "1")
    with counted() as count:
        on = trader_outputs(model, views, weights)
    assert count.ran == {"tower_moments": 2, "batchnorm_fold": 2, "mlp_narrow_forward": 2, "mlp_narrow_backward_dx": 2,
                         "mlp_narrow_reduce": 2}
    assert on["tracked"] == off["tracked"] == ref["tracked"]
    figures: list = []
    try:
        for name in ("logits", "values"):
            got, want, t32 = (r[name].double().cpu() for r in (on, ref, off))
            err, own = float((got - want).abs().max()), float((t32 - want).abs().max())
            figures.append(f"{name} {err:.2e} / {own:.2e} = {err / own if own else math.nan:.2f}")
            assert bool(((got - want).abs() <= 3 * own + 2e-6 + 1e-5 * want.abs()).all()), (name, err, own)
        for name, want in ref["grads"].items():
            got, want, t32 = on["grads"][name].double().cpu(), want.cpu(), off["grads"][name].double().cpu()
            err, own = float((got - want).abs().max()), float((t32 - want).abs().max())
            figures.append(f"{name} {err:.2e} / {own:.2e} = {err / own if own else math.nan:.2f}")
            if name in ("feature_model.0.0.bias", "vf_model.0.0.bias"):  # (the bias under the BatchNorm: 0 up to rounding, the absolute floor alone)
                assert err <= 1e-9 + 2e-5 * float(want.abs().max()), (name, err)
                continue
            assert err <= 3 * own + 2e-5 * float(want.abs().max()), (name, err, own)
    finally:
        print(f"{model_cls.__name__}: " + "\n  ".join(figures))

    # one collect() + step() on the route
    tracked = {}
    for switch in ("1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        torch.manual_seed(0)
        algo = AlgorithmConfig(num_envs=NUM_ENVS, horizon=HORIZON, model_cls=model_cls, model_config={"seq_len": 4},
                               num_sgd_iters=1).build(AlgoTrading)
        with counted() as collected:
            algo.collect()
        with counted() as stepped:
            stats = algo.step()
        assert all(math.isfinite(v) for v in stats.values() if isinstance(v, float)), stats
        norm = algo.policy.model.feature_model[0][1]
        tracked[switch] = (int(norm.num_batches_tracked), int(algo.policy.model.vf_model[0][1].num_batches_tracked))
        if switch == "1":
            assert collected.ran == {"tower_moments": 2 * (HORIZON + 1), "batchnorm_fold": 2 * (HORIZON + 1),
                                     "mlp_narrow_forward": 2 * (HORIZON + 1)}
            # (the embedding in front of the towers asks for dx: every backward is the dx entry)
            assert stepped.ran["mlp_narrow_backward_dx"] == stepped.ran["mlp_narrow_reduce"] >= 2
            assert "mlp_narrow_backward" not in stepped.ran
            assert stepped.ran["tower_moments"] == stepped.ran["batchnorm_fold"] == stepped.ran["mlp_narrow_forward"]
        else:
            assert collected.ran == {} and stepped.ran == {}
    assert tracked["1"] == tracked["0"] and tracked["1"][0] > HORIZON
