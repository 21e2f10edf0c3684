"""GPU tests of recommender_amd.steps.StaticKerasAdam alone, on a toy module that reaches what
no single model's static-step test does: a table on the small densify path beside one on the
sorted path, two lookups of one table of which only one carries a grad_mask (take_grad's mixed
valid concat with its segments list), a parameter outside the loss (gradient None), and an
empty parameter. The toy has no GEMM — lookups, elementwise ops and sums only — so nothing can
pick another algorithm under capture and every comparison is torch.equal."""
import numpy as np
import pytest
import torch
from torch import nn

from recommender_amd.embedding import Embedding
from recommender_amd.optim import KerasAdam, SparseAdam
from recommender_amd.steps import StaticKerasAdam, dense_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-2
V_SMALL, D_SMALL = 8, 4      # V·dim <= 16384, dim a power of two: rs_embedding_grad_dense_small
V_BIG, D_BIG = 5000, 8       # the sorted path


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator(device=DEV).manual_seed(4)
        self.small = Embedding(V_SMALL, D_SMALL, device=DEV, generator=g)
        self.big = Embedding(V_BIG, D_BIG, device=DEV, generator=g)
        self.w = nn.Parameter(torch.randn(4, 3, device=DEV, generator=g))
        self.outside = nn.Parameter(torch.randn(5, device=DEV, generator=g))  # never in the loss
        self.empty = nn.Parameter(torch.zeros(0, device=DEV))

    def tables(self):
        return [self.small, self.big]

    def forward(self, ids_small, ids_a, mask_a, ids_b):
        # a model states with a grad_mask that the masked rows get zero gradient; here they get
        # one on purpose, so a step that dropped the validity flags would sum rows that
        # SparseAdam leaves out, and the comparison would show it
        a = self.big(ids_a, grad_mask=mask_a)
        b = self.big(ids_b)
        s = self.small(ids_small)
        mixed = (s.unsqueeze(-1) * self.w).sum(-1)  # [6, 4, 3] -> [6, 4]
        return (mixed * mixed).sum() + (a * b).sum() + 0.5 * (a * a).sum() + (b * b * b).sum()


def _ids(rng, V):
    """Six ids: 0, V-1 and one id twice (no id more often: a two-term fp32 sum is the same in
    either order, so the small path's block / lane order and the sparse apply's position order
    agree bit for bit), shuffled."""
    r, x, y = rng.choice(np.arange(1, V - 1), 3, replace=False)
    return rng.permutation(np.array([0, V - 1, r, r, x, y], dtype=np.int32))


def _batches(n=3):
    rng = np.random.default_rng(4)
    out = []
    for _ in range(n):
        mask = np.ones(6, bool)
        mask[rng.choice(6, 2, replace=False)] = False
        b = (_ids(rng, V_SMALL), _ids(rng, V_BIG), mask, _ids(rng, V_BIG))
        out.append(tuple(torch.from_numpy(x).to(DEV) for x in b))
    return out


def _state(model):
    torch.cuda.synchronize()
    st = {n: p.detach().clone() for n, p in model.named_parameters()}
    st.update({f"table{i}": t.weight.clone() for i, t in enumerate(model.tables())})
    return st


def _helper(model, comm=None):
    return StaticKerasAdam(dense_parameters(model), model.tables(),
                           SparseAdam(model.tables(), lr=LR, mode="keras"), LR, comm=comm)


def _static_step(model, helper, batch):
    helper.zero_grad()
    loss = model(*batch)
    loss.backward()
    helper.step()
    return loss.detach()


@pytest.fixture(scope="module")
def eager_static():
    """(losses, state) of three eager helper steps: the reference both tests compare with."""
    model = Toy()
    helper = _helper(model)
    # the flat buffer: the dense parameters in order without the empty one, then the tables
    assert [id(p) for p in helper.opt.params] == [id(model.w), id(model.outside),
                                                  id(model.small.weight), id(model.big.weight)]
    losses = [float(_static_step(model, helper, b)) for b in _batches()]
    assert helper.opt.iterations == 3
    return losses, _state(model)


def test_eager_helper_steps_equal_keras_adam_and_sparse_adam(eager_static):
    """Three eager helper steps equal three steps of KerasAdam + SparseAdam(mode="keras") on an
    identically seeded copy, bit for bit on every parameter and table."""
    model = Toy()
    opt_dense = KerasAdam(dense_parameters(model), lr=LR)
    opt_sparse = SparseAdam(model.tables(), lr=LR, mode="keras")
    losses = []
    for b in _batches():
        opt_dense.zero_grad(set_to_none=True)
        loss = model(*b)
        loss.backward()
        opt_dense.step()
        opt_sparse.step()
        losses.append(float(loss.detach()))
    ref, (got_losses, got) = _state(model), eager_static
    assert got_losses == losses
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
    assert not torch.equal(got["w"], Toy().w)  # the steps moved something


def test_captured_helper_steps_equal_eager_helper_steps(eager_static):
    """One eager helper step, then capture and two replays on refilled static inputs, equal
    three eager helper steps bit for bit; the replays count as steps, and the parameter outside
    the loss never moves."""
    model = Toy()
    outside0 = model.outside.detach().clone()
    helper = _helper(model)
    batches = _batches()
    losses = [float(_static_step(model, helper, batches[0]))]
    static = tuple(torch.empty_like(t) for t in batches[0])
    replay = None
    for b in batches[1:]:
        for d, s in zip(static, b):
            d.copy_(s)
        replay = replay or helper.capture(lambda: _static_step(model, helper, static))
        losses.append(float(replay()))
    ref_losses, ref = eager_static
    got = _state(model)
    assert helper.opt.iterations == 3
    assert losses == ref_losses
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
    assert torch.equal(got["outside"], outside0)


def test_no_collective_without_comm(monkeypatch):
    """comm=None, and a Comm whose collectives are off (world 1, not forced), attempt no
    all-reduce (world 2: tests/test_pinsage_gpu.py, tests/test_rccl_gpu.py)."""
    import torch.distributed as dist

    from recommender_amd import steps
    from recommender_amd.sharded import Comm

    def boom(*a, **k):
        raise AssertionError("a collective was attempted")

    monkeypatch.setattr(steps, "allreduce_mean_", boom)
    monkeypatch.setattr(dist, "all_reduce", boom)
    states = []
    for comm in (None, Comm()):
        model = Toy()
        _static_step(model, _helper(model, comm), _batches(1)[0])
        states.append(_state(model))
    for n in states[0]:
        assert torch.equal(states[0][n], states[1][n]), n
