"""GPU parity for the PinSage evaluation (pinsage/train/evaluation.py):
latest item per user, masked top-k, hit flags — bit-exact against oracle/pinsage.py. The
end-to-end recommend() uses small-integer item representations, so the fp32 similarity GEMM
is exact and the top-k (with its many ties) must match the oracle exactly too."""
import numpy as np
import pytest
import torch

from oracle import pinsage as O
from recommender_amd import _lib as L
from recommender_amd.pinsage import PinSageModel, PinSageSampler
from recommender_amd.pinsage.evaluation import (build_val_test_matrix, get_item_reprs,
                                                hit_rate_eval, latest_items, masked_topk,
                                                recommend, train_test_split_by_time)
from recommender_amd.pinsage.graph import HeteroGraph
from tests import rare_inputs as RI

pytestmark = pytest.mark.gpu
DEV = "cuda"


def graph_with_time(seed=0, n_users=80, n_items=150, n_edges=1500):
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.arange(n_users), rng.integers(0, n_users, n_edges)])
    i = rng.integers(0, n_items, u.size)
    key = np.unique(u * n_items + i)
    u, i = key // n_items, key % n_items
    ts = rng.integers(0, 40, u.size)  # many equal timestamps
    year = rng.integers(0, 12, n_items)
    genre = (rng.random((n_items, 6)) < 0.3).astype(np.int8)
    g = HeteroGraph(u, i, n_users, n_items, device=DEV, item_data={"year": year, "genre": genre},
                    edge_data={"timestamp": ts})
    return g, u, i, ts


def test_latest_item_bit_exact():
    g, u, i, ts = graph_with_time()
    got = latest_items(g, "timestamp").cpu().numpy()
    ip = g.u2i_indptr.cpu().numpy()
    ref = O.latest_item(ip, g.u2i.cpu().numpy(), g.u2i_edata["timestamp"].cpu().numpy())
    assert np.array_equal(got, ref)


def test_latest_item_missing_user_raises():
    g = HeteroGraph(np.array([0, 0]), np.array([1, 2]), 3, 4, device=DEV,
                    edge_data={"timestamp": np.array([1, 2])})
    with pytest.raises(ValueError):
        latest_items(g, "timestamp")


@pytest.mark.parametrize("R,I,K,excl", RI.COMMON_TOPK_CASES)
def test_masked_topk_bit_exact(R, I, K, excl):
    scores, eu, ei = RI.common_topk_case(R, I, K, excl)  # dense ties
    ip = it = g = None
    if excl:
        g = HeteroGraph(eu, ei, R, I, device=DEV)
        ip, it = g.u2i_indptr.cpu().numpy(), g.u2i.cpu().numpy()
    idx, val = masked_topk(torch.from_numpy(scores).to(DEV), K, 0, g, with_scores=True)
    ref = O.masked_topk(scores, K, ip, it)
    assert np.array_equal(idx.cpu().numpy(), ref)
    assert np.array_equal(val.cpu().numpy(),
                          np.take_along_axis(O.masked_topk_scores(scores, ip, it), ref, 1))


def _topk_raw(scores, ld, n_items, K, ip=None, it=None, user_base=0, with_scores=True):
    """rs_masked_topk on a device [R, ld] buffer with the CSR given as arrays; the outputs sit
    between guard elements that must come back untouched."""
    R, G = scores.shape[0], 8
    idx = torch.full((R * K + 2 * G,), -77, dtype=torch.int32, device=DEV)
    val = torch.full((R * K + 2 * G,), -77.0, device=DEV) if with_scores else None
    ipt = None if ip is None else torch.from_numpy(np.asarray(ip, np.int64)).to(DEV)
    itt = None if it is None else torch.from_numpy(np.asarray(it, np.int32)).to(DEV)
    L.call("rs_masked_topk", L.ptr(scores), ld, R, n_items, user_base, L.ptr(ipt), L.ptr(itt), K,
           L.ptr(idx[G:]), L.ptr(None if val is None else val[G:]), L.stream_ptr(scores.device))
    for o in (idx, val):
        if o is not None:
            assert (o[:G] == -77).all() and (o[-G:] == -77).all()
    return (idx[G:-G].view(R, K).cpu().numpy(),
            None if val is None else val[G:-G].view(R, K).cpu().numpy())


@pytest.mark.parametrize("name", list(RI.TOPK_CASES))
def test_masked_topk_rare_paths_bit_exact(name):
    """The candidate regimes no common input reaches (tests/test_rare_inputs_cpu.py asserts the
    regime of every row): candidate overflow in each template instance, register lists several
    entries deep, the one-wave sort's edges (ties only, K = I, fewer than K items left: the
    -inf entries in item order), exclusion bitmaps past 32 KB up to the 2^20-item limit. Half
    the rows run without an exclusion CSR, half with one."""
    scores, K, plain, (ip, it) = RI.topk_case(name)
    I = scores.shape[1]
    dev = torch.from_numpy(scores).to(DEV)
    for rows, csr in ((slice(0, plain), (None, None)), (slice(plain, None), (ip, it))):
        if scores[rows].shape[0] == 0:
            continue
        idx, val = _topk_raw(dev[rows].contiguous(), I, I, K, *csr)
        ref = O.masked_topk(scores[rows], K, *csr)
        assert np.array_equal(idx, ref)
        assert np.array_equal(val, np.take_along_axis(O.masked_topk_scores(scores[rows], *csr),
                                                      ref, 1))


@pytest.mark.parametrize("name", ["overflow_16640_33", "deep_3000_33", "wave_flat_300_64"])
def test_masked_topk_padded_rows_no_scores(name):
    """ld > n_items (the columns past n_items hold 1e30 and must not be ranked), out_scores
    NULL, and a user_base into a longer exclusion CSR."""
    scores, K, plain, (ip, it) = RI.topk_case(name)
    R, I = scores.shape
    ld = I + 77
    buf = np.full((R, ld), 1e30, np.float32)
    buf[:, :I] = scores
    # CSR over 3 + R users: users 3 + plain .. carry the case's lists, the others none
    ip_all = np.concatenate([np.zeros(3 + plain, np.int64), ip])
    idx, val = _topk_raw(torch.from_numpy(buf).to(DEV), ld, I, K, ip_all, it, user_base=3,
                         with_scores=False)
    assert val is None
    assert np.array_equal(idx, O.masked_topk(scores, K, ip_all, it, user_base=3))


def test_masked_topk_rejects_bad_sizes():
    s = torch.zeros(2, 40, device=DEV)
    for ld, I, K in ((39, 40, 5), (40, 40, 65), (40, 40, 41), ((1 << 20) + 1, (1 << 20) + 1, 5)):
        with pytest.raises(L.RecsysError):
            _topk_raw(s, ld, I, K)


def test_recommend_and_hit_rate_exact():
    g, u, i, ts = graph_with_time(seed=2)
    rng = np.random.default_rng(5)
    reprs = torch.from_numpy(rng.integers(-3, 4, (g.n_items, 16)).astype(np.float32)).to(DEV)
    for bs in (32, 100000):
        recs = recommend(g, 10, reprs, None, "user", "timestamp", bs).cpu().numpy()
        ip, u2i = g.u2i_indptr.cpu().numpy(), g.u2i.cpu().numpy()
        latest = O.latest_item(ip, u2i, g.u2i_edata["timestamp"].cpu().numpy())
        r = reprs.cpu().numpy()
        ref = O.masked_topk(r[latest] @ r.T, 10, ip, u2i)
        assert np.array_equal(recs, ref)
    val_idx = rng.choice(u.size, 200, replace=False)
    val, _ = build_val_test_matrix(u, i, val_idx, val_idx[:0], g.n_users, g.n_items)
    hr = hit_rate_eval(torch.from_numpy(ref).to(DEV), val)
    gt = val.tocsr()
    gt.sort_indices()
    assert hr == O.hit_rate(ref, gt.indptr, gt.indices)[0]


def test_recommend_in_row_chunks_exact(monkeypatch):
    """recommend() over three row chunks (32, 32 and 16 users: rs_masked_topk with user_base
    0, 32, 64 into the exclusion CSR) equals the one-chunk result and the oracle."""
    from recommender_amd.pinsage import evaluation as E

    g, u, i, ts = graph_with_time(seed=2)
    rng = np.random.default_rng(5)
    reprs = torch.from_numpy(rng.integers(-3, 4, (g.n_items, 16)).astype(np.float32)).to(DEV)
    one = recommend(g, 10, reprs, None, "user", "timestamp", 100000).cpu().numpy()
    monkeypatch.setattr(E, "_SCORE_CHUNK_BYTES", 0)
    bases = []
    real = E.masked_topk
    monkeypatch.setattr(E, "masked_topk", lambda s, k, b, *a, **kw: (bases.append((b, s.shape[0])),
                                                                     real(s, k, b, *a, **kw))[1])
    recs = recommend(g, 10, reprs, None, "user", "timestamp", 32).cpu().numpy()
    assert bases == [(0, 32), (32, 32), (64, 16)]
    ip, u2i = g.u2i_indptr.cpu().numpy(), g.u2i.cpu().numpy()
    latest = O.latest_item(ip, u2i, g.u2i_edata["timestamp"].cpu().numpy())
    r = reprs.cpu().numpy()
    ref = O.masked_topk(r[latest] @ r.T, 10, ip, u2i)
    assert np.array_equal(recs, one) and np.array_equal(recs, ref)
    val_idx = rng.choice(u.size, 200, replace=False)
    val, _ = build_val_test_matrix(u, i, val_idx, val_idx[:0], g.n_users, g.n_items)
    hr = hit_rate_eval(torch.from_numpy(recs).to(DEV), val)
    gt = val.tocsr()
    gt.sort_indices()
    assert hr == O.hit_rate(ref, gt.indptr, gt.indices)[0]


def test_item_reprs_are_per_batch_reprs():
    """get_item_reprs = model.get_repr of each batch of seeds, all at one sampler step (the
    batch-global Frobenius norm makes the result batch-size dependent, as in the reference)."""
    g, *_ = graph_with_time(seed=4)
    torch.manual_seed(0)
    model = PinSageModel(g, g.itype, 2, 8, 32, 16)
    smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=4)
    step0 = smp.step
    a = get_item_reprs(model, smp, g, g.itype, 32)
    assert a.shape == (g.n_items, 16) and smp.step == step0 + 1
    with torch.no_grad():
        for b0 in (0, 64, 128):
            smp.step = step0
            seeds = torch.arange(b0, min(g.n_items, b0 + 32), dtype=torch.int32, device=DEV)
            ref = model.get_repr(smp.generate_blocks(seeds))
            assert torch.equal(a[b0:b0 + seeds.numel()], ref)


def test_train_cli_with_hit_rate(capsys):
    from recommender_amd.pinsage.train import main

    main(["--steps", "3", "--eval_every", "2"])
    out = capsys.readouterr().out
    assert "hit_rate" in out
