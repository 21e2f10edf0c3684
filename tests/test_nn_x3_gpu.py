"""The opt-in RS_GEMM_X3 route of recommender_amd/nn.py (_x3_ready, gemm_x3, _affine, the dgrad of
_LinearFn.backward, _BatchedLinearFn.forward): at a qualifying shape the Dense products go through
rs_gemm_x3 (counted on nn.gemm_x3) and agree with a float64 evaluation within the dense bound of
tests/x3_model.py; shapes and operands that do not qualify fall back to the library path,
bit-equal to the run with the flag off."""
import pytest
import torch

from recommender_amd import nn
from tests import x3_model as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def x3(monkeypatch):
    """The flag on, and a counter on nn.gemm_x3."""
    calls = []
    real = nn.gemm_x3

    def counted(*a, **kw):
        calls.append(kw.get("tb", False))
        return real(*a, **kw)

    monkeypatch.setattr(nn, "_GEMM_X3", True)
    monkeypatch.setattr(nn, "gemm_x3", counted)
    return calls


def _randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _within(got, ref, mag, rel, msg):
    worst = X.max_rel(got.cpu(), ref.cpu(), mag.cpu())
    print(f"{msg}: max err/mag {worst:.3g} (bound {rel:g})")
    assert bool(((got.double() - ref).abs() <= rel * mag).all()), f"{msg}: {worst:.3g}"


@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_takes_the_x3_route(x3, act):
    """64 x 160 -> 160: the forward (N = 160 >= 128, K = 160) and the dgrad (N = 160, K = 160)
    both qualify."""
    x = _randn(64, 160, seed=1).requires_grad_(True)
    k = (_randn(160, 160, seed=2) * 0.1).requires_grad_(True)
    b = _randn(160, seed=3).requires_grad_(True)
    g = _randn(64, 160, seed=4)
    y = nn.linear(x, k, b, act)
    assert x3 == [False]
    y.backward(g)
    assert x3 == [False, True]                      # the forward, then the dgrad with tb
    x64, k64, b64 = x.detach().double(), k.detach().double(), b.detach().double()
    z = x64 @ k64 + b64
    mag = x64.abs() @ k64.abs() + b64.abs()
    want = torch.relu(z) if act == 1 else (torch.sigmoid(z) if act == 2 else z)
    # the activations' slopes are <= 1: the pre-activation bound carries over
    _within(y.detach(), want, mag, X.REL_DENSE, "y")
    # the backward from the kernel's own y (no mask flips): dz = act'(y) g
    yd = y.detach().double()
    dz = g.double() * ((yd > 0).double() if act == 1 else (yd * (1 - yd) if act == 2 else 1.0))
    dzm = dz.abs() + (4 * X.U) * g.double().abs()   # dz itself is formed in fp32
    _within(x.grad, dz @ k64.T, dzm @ k64.abs().T, X.REL_DENSE, "dx")
    _within(k.grad, x64.T @ dz, x64.abs().T @ dzm, 4e-6, "dk (library)")
    _within(b.grad, dz.sum(0), dzm.sum(0), 4e-6, "db")


@pytest.mark.parametrize("act", [0, 1])
def test_batched_linear_takes_the_x3_route(x3, act):
    E, B, I, O = 3, 64, 160, 128
    x = _randn(E, B, I, seed=5).requires_grad_(True)
    k = (_randn(E, I, O, seed=6) * 0.1).requires_grad_(True)
    b = _randn(E, 1, O, seed=7).requires_grad_(True)
    g = _randn(E, B, O, seed=8)
    y = nn.batched_linear(x, k, b, act)
    assert x3 == [False]
    y.backward(g)
    assert x3 == [False]                            # the batched backward is the library's
    x64, k64, b64 = x.detach().double(), k.detach().double(), b.detach().double()
    z = x64 @ k64 + b64
    mag = x64.abs() @ k64.abs() + b64.abs()
    _within(y.detach(), torch.relu(z) if act else z, mag, X.REL_DENSE, "y")
    dz = g.double() * ((y.detach() > 0).double() if act else 1.0)
    _within(x.grad, dz @ k64.transpose(1, 2), dz.abs() @ k64.abs().transpose(1, 2), 4e-6, "dx")
    _within(k.grad, x64.transpose(1, 2) @ dz, x64.abs().transpose(1, 2) @ dz.abs(), 4e-6, "dk")
    _within(b.grad, dz.sum(1, keepdim=True), dz.abs().sum(1, keepdim=True), 4e-6, "db")


def _linear_case(name):
    """(x, k, b) that must not take the x3 route."""
    if name == "narrow":                      # N < 128
        return _randn(64, 160, seed=1), _randn(160, 64, seed=2), _randn(64, seed=3)
    if name == "rows_not_4":                  # a dimension that is not a multiple of 4
        return _randn(62, 160, seed=1), _randn(160, 160, seed=2), _randn(160, seed=3)
    if name == "cols_not_4":
        return _randn(64, 162, seed=1), _randn(162, 160, seed=2), _randn(160, seed=3)
    if name == "weight_view":                 # a weight that is not contiguous
        return _randn(64, 160, seed=1), _randn(160, 160, seed=2).t(), _randn(160, seed=3)
    if name == "bias_view":                   # a bias view that is not contiguous
        return _randn(64, 160, seed=1), _randn(160, 160, seed=2), _randn(320, seed=3)[::2]
    raise ValueError(name)


def _linear_run(x, k, b, act):
    x = x.clone().requires_grad_(True)
    k = k.detach().requires_grad_(True)
    y = nn.linear(x, k, b, act)
    y.backward(torch.ones_like(y))
    return y.detach(), x.grad, k.grad


@pytest.mark.parametrize("name", ["narrow", "rows_not_4", "cols_not_4", "weight_view",
                                  "bias_view"])
def test_linear_falls_back_bit_equal(monkeypatch, name):
    x, k, b = _linear_case(name)
    off = _linear_run(x, k, b, 1)
    calls = []
    monkeypatch.setattr(nn, "_GEMM_X3", True)
    real = nn.gemm_x3
    monkeypatch.setattr(nn, "gemm_x3", lambda *a, **kw: (calls.append(kw.get("tb", False)),
                                                        real(*a, **kw))[1])
    on = _linear_run(x, k, b, 1)
    # a bias view only keeps the forward off the route: the dgrad has no bias and may take it
    assert [c for c in calls if not c] == []
    if name != "bias_view":
        assert calls == []
        for a, o, what in zip(on, off, ("y", "dx", "dk")):
            assert torch.equal(a, o), f"{name}: {what} differs from the run with the flag off"
    else:
        assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])


@pytest.mark.parametrize("name", ["rows_not_4", "weight_view", "bias_view"])
def test_batched_linear_falls_back_bit_equal(monkeypatch, name):
    E = 2
    x = _randn(E, 62 if name == "rows_not_4" else 64, 160, seed=1)
    k = _randn(E, 128, 160, seed=2).transpose(1, 2) if name == "weight_view" else _randn(E, 160, 128, seed=2)
    b = _randn(E, 1, 256, seed=3)[..., ::2] if name == "bias_view" else _randn(E, 1, 128, seed=3)
    off = nn.batched_linear(x, k, b, 1)
    calls = []
    monkeypatch.setattr(nn, "_GEMM_X3", True)
    monkeypatch.setattr(nn, "gemm_x3", lambda *a, **kw: calls.append(1))
    on = nn.batched_linear(x, k, b, 1)
    assert calls == [] and torch.equal(on, off)
