"""Sparse Adagrad on the GPU (RS_OPT_ADAGRAD / RS_OPT_ROWWISE_ADAGRAD, optim.SparseAdagrad) against
tests/adagrad_ref.py.

Element-wise: bit-exact (the segment sums follow the oracle's tiled order and every update
operation is rounded on its own). Row-wise: the row's sum of squares is reduced across lanes in
an order the reference does not restate, so (a) the accumulator is held to the derived bound
adagrad_ref.rowwise_acc_rtol against float64, (b) the weights are bit-equal to the fp32 update
evaluated with the GPU's own new accumulator (one `a` per row, idle lanes masked), (c) two runs
agree bit for bit, (d) a zero gradient sum leaves row and accumulator as they were. Each step's
reference starts from the previous step's GPU state, so errors do not compound."""
import numpy as np
import pytest
import torch

from oracle import embedding as O
from recommender_amd import _lib as L
from recommender_amd.ctr.layers import MLP
from recommender_amd.embedding import Embedding
from recommender_amd.optim import SortedIds, SparseAdagrad, SparseAdam, SparseSGD
from tests import adagrad_ref as R
from tests.conftest import assert_close_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, EPS, ACC0 = 0.05, 1e-7, 0.1
# 128: group walk; 64; 48, 18: idle lanes at vec 4 / vec 2; 7: vec 1; 320: two chunks per lane
DIMS = [128, 64, 48, 18, 7, 320]
KINDS = ["adagrad", "rowwise_adagrad"]
RUN_LENS = [
    [31, 32, 33, 1, 1024, 1023, 1025, 2, 2048 + 7, 5, 32 * 32 * 3, 64],
    [992, 32, 1, 31, 1024 * 2 - 1, 1, 1056, 7],
    [1] * 100 + [3000] + [1] * 33,
]


def zipf_ids(rng, n, card, a=1.05):
    return np.minimum(rng.zipf(a, size=n) - 1, card - 1)


def _table(w0, rowwise, lr=LR):
    t = Embedding(w0.shape[0], w0.shape[1], device=DEV, weight=torch.from_numpy(w0))
    return t, SparseAdagrad(t, lr=lr, initial_accumulator_value=ACC0, epsilon=EPS, rowwise=rowwise)


def _state(t, opt):
    torch.cuda.synchronize()
    return t.weight.cpu().numpy(), opt.state[id(t)].cpu().numpy()


def _check_elementwise(got_w, got_acc, w, acc, ur, ug, lr=LR):
    """(w, acc): the reference state before the step. Returns the reference state after it."""
    rw, racc = R.apply_adagrad(w, acc, ur, ug, lr, EPS)
    np.testing.assert_array_equal(got_acc, racc)
    np.testing.assert_array_equal(got_w, rw)
    untouched = np.setdiff1d(np.arange(w.shape[0]), ur.astype(np.int64))
    np.testing.assert_array_equal(got_w[untouched], w[untouched])
    np.testing.assert_array_equal(got_acc[untouched], acc[untouched])
    return rw, racc


def _check_rowwise(got_w, got_acc, w, acc, ur, ug, lr=LR):
    """(w, acc): the GPU state before the step."""
    D = w.shape[1]
    u = ur.astype(np.int64)
    a64 = R.rowwise_accumulator_f64(acc, ur, ug)
    rel = np.abs(got_acc[u] - a64[u]) / a64[u]
    print(f"row-wise D={D}: accumulator max rel err {rel.max():.3g}, bound {R.rowwise_acc_rtol(D):.3g}")
    assert (rel <= R.rowwise_acc_rtol(D)).all(), (rel.max(), R.rowwise_acc_rtol(D))
    np.testing.assert_array_equal(got_w, R.rowwise_update(w, got_acc, ur, ug, lr, EPS))
    untouched = np.setdiff1d(np.arange(w.shape[0]), u)
    np.testing.assert_array_equal(got_w[untouched], w[untouched])
    np.testing.assert_array_equal(got_acc[untouched], acc[untouched])


def _step(t, opt, ids, g):
    t.accumulate_grad(torch.from_numpy(ids).to(DEV), torch.from_numpy(g).to(DEV))
    opt.step()


@pytest.mark.parametrize("dim", DIMS)
def test_elementwise_bitexact(dim, rng):
    V, n = 5000, 4000
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    t, opt = _table(w0, False)
    assert opt.kind == L.RS_OPT_ADAGRAD and tuple(opt.state[id(t)].shape) == (V, dim)
    w, acc = w0, np.full((V, dim), ACC0, np.float32)
    for _ in range(3):
        ids = zipf_ids(rng, n, V).astype(np.int64)
        g = rng.standard_normal((n, dim)).astype(np.float32)
        _step(t, opt, ids, g)
        ur, ug = R.segment_grads(ids, g, V)
        w, acc = _check_elementwise(*_state(t, opt), w, acc, ur, ug)


@pytest.mark.parametrize("dim", DIMS)
def test_rowwise_bound_bitexact_weights_and_repeatable(dim, rng):
    V, n = 5000, 4000
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    t, opt = _table(w0, True)
    t2, opt2 = _table(w0, True)  # (c): the same steps from the same state, a second time
    assert opt.kind == L.RS_OPT_ROWWISE_ADAGRAD and tuple(opt.state[id(t)].shape) == (V,)
    w, acc = w0, np.full(V, ACC0, np.float32)
    for _ in range(3):
        ids = zipf_ids(rng, n, V).astype(np.int64)
        g = rng.standard_normal((n, dim)).astype(np.float32)
        _step(t, opt, ids, g)
        _step(t2, opt2, ids, g)
        ur, ug = R.segment_grads(ids, g, V)
        gw, gacc = _state(t, opt)
        _check_rowwise(gw, gacc, w, acc, ur, ug)
        gw2, gacc2 = _state(t2, opt2)
        np.testing.assert_array_equal(gw2, gw)
        np.testing.assert_array_equal(gacc2, gacc)
        w, acc = gw, gacc


@pytest.mark.parametrize("dim", [128, 48, 7])
def test_rowwise_zero_gradient_row_stays(dim, rng):
    """(d) rows 11 and 4000 receive g and -g (row 11 inside one tile, row 4000 cut by a tile
    edge and folded by the fix-up): the sum is exactly +0, so acc += 0 and the weights do not
    move; the other rows update as usual."""
    V = 5000
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    ids = np.concatenate([[11, 11], rng.integers(100, 3000, 29), [4000, 4000],
                          rng.integers(100, 3000, 32), rng.integers(4100, V, 8)]).astype(np.int64)
    g = rng.standard_normal((ids.size, dim)).astype(np.float32)
    g[1], g[32] = -g[0], -g[31]
    order = np.argsort(ids, kind="stable")
    assert list(np.flatnonzero(ids[order] == 4000)) == [63, 64]  # last of tile 1, first of tile 2
    t, opt = _table(w0, True)
    _step(t, opt, ids, g)
    gw, gacc = _state(t, opt)
    for r in (11, 4000):
        np.testing.assert_array_equal(gw[r], w0[r])
        assert gacc[r] == np.float32(ACC0)
    ur, ug = R.segment_grads(ids, g, V)
    assert not ug[ur == 11].any() and not ug[ur == 4000].any()
    _check_rowwise(gw, gacc, w0, np.full(V, ACC0, np.float32), ur, ug)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lens,dim", [(0, 128), (1, 128), (2, 128), (0, 48)])
def test_runs_across_tile_groups(kind, lens, dim, rng):
    """The run-edge cases of test_segment_runs_across_tile_groups (runs ending on / past tile and
    group edges, runs spanning groups: the fix-up kernels finalise those rows), D = 128 through
    the group walk and D = 48 through the general walk."""
    lens = RUN_LENS[lens]
    V = 50_000
    rows = rng.choice(V, len(lens), replace=False)
    ids = np.concatenate([np.full(n, r) for n, r in zip(lens, sorted(rows))]).astype(np.int64)
    ids = ids[rng.permutation(ids.size)]
    g = rng.standard_normal((ids.size, dim)).astype(np.float32)
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    rowwise = kind == "rowwise_adagrad"
    t, opt = _table(w0, rowwise)
    _step(t, opt, ids, g)
    ur, ug = R.segment_grads(ids, g, V)
    assert ur.size == len(lens)
    acc0 = np.full((V,) if rowwise else (V, dim), ACC0, np.float32)
    (_check_rowwise if rowwise else _check_elementwise)(*_state(t, opt), w0, acc0, ur, ug)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [128, 48])
def test_valid_mask_row_scale_and_oob(kind, dim, rng):
    """~30 % of the positions masked off, a per-example row scale (scale_group = 26: one rounded
    multiply before the sum) and a few out-of-range ids, which are dropped and flagged."""
    V, B, S = 5000, 150, 26
    rowwise = kind == "rowwise_adagrad"
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    ids = zipf_ids(rng, B * S, V).reshape(B, S).astype(np.int64)
    valid = (rng.random(B * S) >= 0.3).astype(np.uint8)
    for p in (5, 1000, 3899):
        ids.reshape(-1)[p] = V + 3 + p
        valid[p] = 1
    g = rng.standard_normal((B * S, dim)).astype(np.float32)
    scale = (rng.standard_normal(B) * 0.5).astype(np.float32)
    t, opt = _table(w0, rowwise)
    opt.apply(t, torch.from_numpy(ids).to(DEV), torch.from_numpy(g).to(DEV), opt._params(),
              row_scale=torch.from_numpy(scale).to(DEV), valid=torch.from_numpy(valid).to(DEV))
    ur, ug = R.segment_grads(ids, g, V, valid=valid, row_scale=scale, scale_group=S)
    assert 0 < ur.size < np.unique(ids).size
    acc0 = np.full((V,) if rowwise else (V, dim), ACC0, np.float32)
    (_check_rowwise if rowwise else _check_elementwise)(*_state(t, opt), w0, acc0, ur, ug)
    assert t.check_errors() & L.RS_ERRBIT_OOB


@pytest.mark.parametrize("rowwise", [0, 1])
def test_one_call_matches_two_call(rowwise, rng):
    """rs_apply_adagrad is bit-identical to rs_sort_ids + rs_embedding_apply."""
    card = [50, 3, 4000, 700]
    so_np = np.concatenate([[0], np.cumsum(card)]).astype(np.int64)
    V, D, B = int(so_np[-1]), 48, 3000
    ids = np.stack([rng.integers(0, c, B) for c in card], 1).astype(np.int64)
    g = rng.standard_normal((B * 4, D)).astype(np.float32)
    so = torch.from_numpy(so_np).to(DEV)
    idt, gt = torch.from_numpy(ids).to(DEV), torch.from_numpy(g).to(DEV)
    st = L.stream_ptr(torch.device(DEV))
    n = ids.size
    ws = torch.empty(L.lib().rs_sparse_workspace_size(n, D), dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    w0 = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(DEV)
    tabs = [w0.clone(), w0.clone()]
    accs = [torch.full((V,) if rowwise else (V, D), ACC0, device=DEV) for _ in range(2)]
    L.call("rs_apply_adagrad", L.ptr(tabs[0]), L.ptr(accs[0]), V, D, L.ptr(idt), 1, n, L.ptr(so), 4,
           L.ptr(gt), 0.01, 1e-7, rowwise, L.ptr(err), L.ptr(ws), ws.numel(), st)
    s = SortedIds(idt, V, so)
    w2 = torch.empty(L.lib().rs_apply_workspace_size(n, D), dtype=torch.uint8, device=DEV)
    prm = L.AdamParams(0.01, 0, 0, 0, 0, 1e-7)
    L.call("rs_embedding_apply", L.RS_OPT_ROWWISE_ADAGRAD if rowwise else L.RS_OPT_ADAGRAD,
           L.ptr(tabs[1]), L.ptr(accs[1]), None, V, D, L.ptr(s.rows), L.ptr(s.pos), n, L.ptr(gt), prm,
           None, L.ptr(w2), w2.numel(), st)
    torch.cuda.synchronize()
    assert not torch.equal(tabs[0], w0)
    assert torch.equal(tabs[0], tabs[1]) and torch.equal(accs[0], accs[1])


@pytest.mark.parametrize("optimizer", KINDS)
def test_fused_side_stream_apply_matches_unfused(optimizer):
    """Unfused, fused, fused with the deferred join, and the latter with the next batch's sort
    prefetched: tables and accumulators bit-equal after three steps."""
    from recommender_amd.ctr.train import TrainStep, build_model
    from recommender_amd.synthetic import criteo_batch, criteo_cardinalities

    cards = criteo_cardinalities(300_000, 26)
    models, steps = [], []
    for fused, defer in ((False, False), (True, False), (True, True), (True, True)):
        g = torch.Generator(device=DEV)
        g.manual_seed(7)
        m = build_model("DLRM", 32, sum(cards), 26, 13, DEV, slot_cardinalities=cards,
                        bottom=[64, 32], top=[64, 1], generator=g)
        models.append(m)
        steps.append(TrainStep(m, optimizer, fused=fused, defer_sparse_join=defer))
        assert isinstance(steps[-1].opt_sparse, SparseAdagrad)
        assert steps[-1].opt_sparse.rowwise == (optimizer == "rowwise_adagrad")
        assert isinstance(steps[-1].opt_dense, torch.optim.Adagrad)
    r = np.random.default_rng(3)
    batches = []
    for _ in range(3):
        cat, dn, lb = criteo_batch(r, 2048, cards)
        batches.append(tuple(torch.from_numpy(x).to(DEV) for x in (cat, dn, lb)))
    for i, b in enumerate(batches):
        if i + 1 < len(batches):
            steps[3].prefetch(batches[i + 1])
        for st in steps:
            st(b)
    for m in models:
        m.embedding_layer.wait_update()
    torch.cuda.synchronize()

    def acc_of(i):
        return steps[i].opt_sparse.state[id(models[i].embedding_layer)].cpu().numpy()

    ref, ref_acc = models[0].embedding_layer.weight.cpu().numpy(), acc_of(0)
    assert (ref_acc != np.float32(0.1)).any()
    for i in range(1, 4):
        np.testing.assert_array_equal(ref, models[i].embedding_layer.weight.cpu().numpy())
        np.testing.assert_array_equal(ref_acc, acc_of(i))


@pytest.fixture
def factored_any_batch():
    old = MLP.factored_min_batch
    MLP.factored_min_batch = 0
    yield
    MLP.factored_min_batch = old


@pytest.mark.parametrize("optimizer", KINDS)
def test_fused_step_matches_autograd_path(factored_any_batch, optimizer):
    """The one-kernel DLRM step (apply_async with the unit rows and the per-example row scale) on a
    D = 64 DLRM against the same model with fused_step=False; the bounds are those of
    tests/test_fused_step_gpu.py:test_fused_step_matches_autograd_path, and so is lr = 0.05: the
    bounds judge the CHANGE of each fp32 parameter, which is resolved to one ulp of the parameter
    only (2^-27 for |p| in [1/16, 1/8)). At TrainStep's default lr = 1e-3 the MLP kernels move by
    about 1e-5, so that one ulp is 1e-3 of the change and no two summation orders could meet
    1e-4; at 0.05 the Adagrad change (about lr*g/sqrt(0.1)) is larger than the SGD test's."""
    from recommender_amd.ctr.train import TrainStep, build_model
    from recommender_amd.synthetic import criteo_batch, criteo_cardinalities

    cards = criteo_cardinalities(300_000, 26)
    bottom, top = [512, 256, 64], [512, 256, 1]

    def model():
        g = torch.Generator(device=DEV).manual_seed(3)
        return build_model("DLRM", 64, sum(cards), 26, 13, torch.device(DEV),
                           slot_cardinalities=cards, bottom=bottom, top=top, generator=g)

    rng = np.random.default_rng(11)
    batches = []
    for _ in range(3):
        cat, dn, lb = criteo_batch(rng, 2048, cards)
        batches.append(tuple(torch.from_numpy(x).to(DEV) for x in (cat, dn, lb)))
    runs = []
    for fused in (True, False):
        m = model()
        st = TrainStep(m, optimizer, lr=0.05, defer_sparse_join=True, fused_step=fused)
        assert st.fused_step_ready(batches[0]) == fused
        losses, preds = [], []
        for b in batches:
            losses.append(float(st(b).detach()))
            preds.append(st.last_pred.reshape(-1).clone())
        m.embedding_layer.wait_update()
        torch.cuda.synchronize()
        runs.append((m, losses, preds))
    (mf, lf, pf), (ma, la, pa) = runs
    for a, b in zip(lf, la):
        assert abs(a - b) <= 1e-5 * abs(b), (lf, la)
    for a, b in zip(pf, pa):
        assert_close_rel(a.cpu().numpy(), b.cpu().numpy(), 1e-5, 1e-3, "predictions")
    init = model()
    pa_, pi_ = dict(ma.named_parameters()), dict(init.named_parameters())
    for n, p in mf.named_parameters():
        if n.endswith("grad_handle"):
            continue
        d_f = (p.detach() - pi_[n].detach()).cpu().numpy()
        d_a = (pa_[n].detach() - pi_[n].detach()).cpu().numpy()
        assert_close_rel(d_f, d_a, 1e-4, np.abs(d_a).max() * 5e-2 + 1e-30, n)
    w0 = init.embedding_layer.weight
    d_f = mf.embedding_layer.weight - w0
    d_a = ma.embedding_layer.weight - w0
    touched = (d_a != 0).any(1)
    assert int(touched.sum()) > 1000
    assert_close_rel(d_f[touched].cpu().numpy(), d_a[touched].cpu().numpy(), 1e-4,
                     float(d_a.abs().max()) * 5e-2, "table change")


@pytest.mark.parametrize("dim", [128, 18])
def test_sgd_apply_unchanged(dim, rng):
    """Regression guard: test_sgd_apply_bitexact's shape, one step, same bits as the oracle."""
    V, B, S = 30_000, 512, 26
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    ids = zipf_ids(rng, B * S, V).reshape(B, S).astype(np.int64)
    g = rng.standard_normal((B * S, dim)).astype(np.float32)
    t = Embedding(V, dim, device=DEV, weight=torch.from_numpy(w0))
    opt = SparseSGD(t, lr=0.05)
    t.accumulate_grad(torch.from_numpy(ids).to(DEV), torch.from_numpy(g).to(DEV))
    opt.step()
    sr, sp, _ = O.sort_ids(ids, V)
    ur, ug = O.segment_sum_tiled(sr, sp, g, V)
    np.testing.assert_array_equal(t.weight.cpu().numpy(), O.apply_sgd(w0, ur, ug, np.float32(0.05)))


def test_lazy_adam_apply_unchanged(rng):
    """Regression guard: test_adam_apply_bitexact's shape (lazy), one step."""
    V, dim, n = 5000, 64, 4000
    w0 = rng.standard_normal((V, dim)).astype(np.float32)
    t = Embedding(V, dim, device=DEV, weight=torch.from_numpy(w0))
    opt = SparseAdam(t, lr=1e-3, mode="lazy")
    ids = zipf_ids(rng, n, V).astype(np.int64)
    g = rng.standard_normal((n, dim)).astype(np.float32)
    t.accumulate_grad(torch.from_numpy(ids).to(DEV), torch.from_numpy(g).to(DEV))
    opt.step()
    sr, sp, _ = O.sort_ids(ids, V)
    ur, ug = O.segment_sum_tiled(sr, sp, g, V)
    w, m, v = O.apply_lazy_adam(w0, np.zeros_like(w0), np.zeros_like(w0), ur, ug,
                                O.keras_adam_coefficients(1))
    mg, vg, _ = opt.state[id(t)]
    np.testing.assert_array_equal(mg.cpu().numpy(), m)
    np.testing.assert_array_equal(vg.cpu().numpy(), v)
    np.testing.assert_array_equal(t.weight.cpu().numpy(), w)
