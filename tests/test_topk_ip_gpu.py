"""rs_topk_ip on the GPU against tests/topk_ip_ref.py (the contract restated in NumPy), bit for
bit: score bits (the v_mfma_f32_32x32x2_f32 chain against the exact fmaf chain), the selection at
its tile, round, split and k edges, exclusion, argument errors, and the Python surfaces built on
it. Every call goes through the C entry point with 64 guard elements behind each output."""
import ctypes as C

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import topk_ip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
GUARD_ITEM = 0x5A5A5A5A
GUARD_SCORE = 0x7FC12345  # a NaN with a payload


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def padded(a, ld):
    """a's rows at stride ld, NaN in between (the kernel must not read the padding)."""
    if ld is None:
        return np.ascontiguousarray(a, f32), a.shape[1]
    out = np.full((a.shape[0], ld), np.nan, f32)
    out[:, :a.shape[1]] = a
    return out, ld


def raw_call(q, x, k, excl=None, excl_base=0, excl_one=None, n_splits=1, q_ld=None, i_ld=None,
             with_scores=True, ws_bytes=None, expect=0, offset=0):
    """rs_topk_ip → (items [Q, k], scores [Q, k] or None) as NumPy; guards checked. offset: the
    item matrix starts `offset` floats into its buffer (misaligned for 16-byte loads)."""
    lib = L.lib()
    nq, dim = q.shape
    n_items = x.shape[0]
    qa, q_ld = padded(q, q_ld)
    xa, i_ld = padded(x, i_ld)
    tq = dev(qa)
    tx_buf = torch.full((xa.size + offset + 1,), float("nan"), device=DEV)
    tx_buf[offset:offset + xa.size] = dev(xa).reshape(-1)
    tx = tx_buf[offset:]
    ip = it = None
    if excl is not None:
        ip, it = dev(excl[0], np.int64), dev(np.append(excl[1], 0), np.int32)
    one = dev(excl_one, np.int32)
    oi = torch.full((nq * k + GUARD,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    os_ = torch.full((nq * k + GUARD,), GUARD_SCORE, dtype=torch.int32, device=DEV)
    need = lib.rs_topk_ip_workspace_size(nq, n_items, k, n_splits)
    if ws_bytes is None:
        ws_bytes = need
    ws = torch.full((ws_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    st = lib.rs_topk_ip(L.ptr(tq), q_ld, nq, L.ptr(tx), i_ld, n_items, dim, excl_base, L.ptr(ip),
                        L.ptr(it), L.ptr(one), k, n_splits, L.ptr(oi),
                        L.ptr(os_) if with_scores else None, L.ptr(ws) if ws_bytes else None,
                        ws_bytes, L.stream_ptr(oi.device))
    torch.cuda.synchronize()
    assert st == expect, (st, lib.rs_last_error())
    oi, os_, ws = oi.cpu().numpy(), os_.cpu().numpy(), ws.cpu().numpy()
    assert (oi[nq * k:] == GUARD_ITEM).all() and (os_[nq * k:] == GUARD_SCORE).all()
    assert (ws[ws_bytes:] == 0xAB).all()
    if st != 0:
        assert (oi == GUARD_ITEM).all() and (os_ == GUARD_SCORE).all()  # nothing written
        return None, None
    if not with_scores:
        assert (os_ == GUARD_SCORE).all()
    return oi[:nq * k].reshape(nq, k), (os_[:nq * k].view(f32).reshape(nq, k) if with_scores else None)


def check(q, x, k, ref=None, **kw):
    """The call against topk_ref (or a precomputed ref), items exactly and scores bit for bit."""
    ref_kw = {n: kw[n] for n in ("excl", "excl_base", "excl_one") if n in kw}
    ri, rs = ref if ref is not None else R.topk_ref(q, x, k, **ref_kw)
    gi, gs = raw_call(q, x, k, **kw)
    np.testing.assert_array_equal(gi, ri)
    if gs is not None:
        assert R.same_scores(gs, rs), np.argwhere(gs.view(np.uint32) != rs.view(np.uint32))[:5]
    return gi, gs


# ---- score bits --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.DIMS)
def test_score_bits_are_the_fmaf_chain_on_random_floats(dim):
    """k = n_items = 64: every score comes back. Normal rows, subnormal rows and 1e30 rows; the
    reverse chain differs on these inputs (tests/test_topk_ip_cpu.py), so the order is checked."""
    q, x = R.random_floats(20 + dim, 33, dim), R.random_floats(40 + dim, 64, dim)
    check(q, x, 64)


@pytest.mark.parametrize("dim", R.DIMS)
def test_exact_inputs_at_every_dim(dim):
    q, x = R.exact_vectors(dim, 65, dim), R.exact_vectors(dim + 1, 129, dim)
    check(q, x, 10, n_splits=2)


# ---- shapes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cat3000():
    """33 exact queries over 3000 exact items at dim 16 and their best 64: shared, never changed."""
    q, x = R.exact_vectors(61, 33, 16), R.exact_vectors(62, 3000, 16)
    ri, rs = R.topk_ref(q, x, 64)
    for a in (q, x, ri, rs):
        a.setflags(write=False)
    return q, x, ri, rs


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 65])
def test_query_counts(nq):
    q, x = R.exact_vectors(nq, nq, 18), R.exact_vectors(99, 200, 18)
    check(q, x, 10)


@pytest.mark.parametrize("n_items", [1, 31, 32, 33, R.ROUND - 1, R.ROUND, R.ROUND + 1])
def test_item_counts_around_a_tile_and_a_round(n_items):
    q, x = R.random_floats(n_items, 33, 16, extremes=False), R.random_floats(7, n_items, 16, False)
    ref = R.topk_ref(q, x, 10)
    check(q, x, 10, ref=ref)
    if n_items <= 33:
        check(q, x, 10, ref=ref, n_splits=n_items)  # one item per range


@pytest.mark.parametrize("n_splits", [0, 1, 2, 7])
def test_three_thousand_items_by_split_count(cat3000, n_splits):
    q, x, ri, rs = cat3000
    check(q, x, 64, ref=(ri, rs), n_splits=n_splits)


@pytest.mark.parametrize("k", [1, 10, 63, 64])
def test_k_values_and_prefix(cat3000, k):
    q, x, ri, rs = cat3000
    check(q, x, k, ref=(ri[:, :k], rs[:, :k]), n_splits=2)  # k is a prefix of k = 64


def test_k_larger_than_the_catalogue():
    q, x = R.exact_vectors(1, 5, 4), R.exact_vectors(2, 40, 4)
    gi, gs = check(q, x, 64, n_splits=3)
    assert (gi[:, 40:] == -1).all() and (gs[:, 40:] == -np.inf).all()


# ---- invariance --------------------------------------------------------------------------
def test_a_query_alone_and_inside_a_batch():
    q, x = R.random_floats(70, 65, 36), R.random_floats(71, 300, 36)
    bi, bs = raw_call(q, x, 10)
    for r in (0, 40, 64):
        ai, as_ = raw_call(q[r:r + 1], x, 10)
        np.testing.assert_array_equal(ai[0], bi[r])
        assert R.same_scores(as_[0], bs[r])


@pytest.mark.parametrize("dim,q_ld,i_ld,offset", [(18, 23, 20, 0), (18, 18, 19, 0), (16, 16, 16, 1),
                                                  (36, 40, 64, 0), (255, 256, 256, 0)])
def test_strided_rows_with_nan_padding_and_misaligned_bases(dim, q_ld, i_ld, offset):
    """i_ld a multiple of 4 takes the 16-byte loads (with a partial last group at dim 18 and 255),
    an odd i_ld or a base 4 bytes off takes the element loads: same bits as contiguous rows."""
    q, x = R.random_floats(80, 33, dim), R.random_floats(81, 70, dim)
    ref = check(q, x, 64)
    gi, gs = raw_call(q, x, 64, q_ld=q_ld, i_ld=i_ld, offset=offset)
    np.testing.assert_array_equal(gi, ref[0])
    assert R.same_scores(gs, ref[1])


def test_two_runs_and_no_scores():
    q, x = R.random_floats(90, 65, 16), R.random_floats(91, 1000, 16)
    a = raw_call(q, x, 10, n_splits=7)
    b = raw_call(q, x, 10, n_splits=7)
    np.testing.assert_array_equal(a[0], b[0])
    assert R.same_scores(a[1], b[1])
    c, none = raw_call(q, x, 10, n_splits=7, with_scores=False)
    np.testing.assert_array_equal(a[0], c)
    assert none is None


# ---- selection stress --------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n_splits", [1, 2])
def test_items_sorted_by_score(descending, n_splits):
    """Ascending: every item beats the threshold, every list compacts after every round."""
    q, x = R.ramp_catalogue(3000, 16, descending)
    gi, _ = check(q, x, 64, n_splits=n_splits)
    want = np.arange(64) if descending else 2999 - np.arange(64)
    np.testing.assert_array_equal(gi[0], want)


def test_all_scores_equal():
    q, x = R.exact_vectors(3, 33, 16), np.zeros((1000, 16), f32)
    for n_splits in (1, 7):
        gi, gs = raw_call(q, x, 10, n_splits=n_splits)
        np.testing.assert_array_equal(gi, np.tile(np.arange(10), (33, 1)))
        assert (gs.view(np.uint32) == 0).all()  # +0, never -0


@pytest.mark.parametrize("n_splits", [1, 2, 7])
def test_tie_across_the_kth_place_and_a_split_boundary(n_splits):
    q, x = R.tie_catalogue(R.TIE_N, R.TIE_K, R.TIE_IDS)
    check(q, x, R.TIE_K, n_splits=n_splits)


def test_infinite_and_nan_scores():
    q, x = R.special_catalogue()
    for k in (5, 40, 64):
        check(q, x, k)
    check(q, x, 40, n_splits=3)


# ---- exclusion ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def excl_case():
    n_items, k = 100, 10
    q1, x = R.exact_vectors(5, 1, 18), R.exact_vectors(6, n_items, 18)
    top, _ = R.topk_ref(q1, x, k)
    rows = R.exclusion_rows(top[0], n_items, k)
    return np.repeat(q1, len(rows), 0), x, rows, k


def test_exclusion_rows(excl_case):
    """One query five times against: an empty row, every item, exactly its best k, an unsorted
    row with duplicates and out-of-range ids, all but k - 1 items."""
    q, x, rows, k = excl_case
    gi, gs = check(q, x, k, excl=R.csr(rows))
    assert (gi[1] == -1).all() and (gs[1] == -np.inf).all()
    assert not set(gi[2]) & set(gi[0])
    assert (gi[4, :k - 1] >= 0).all() and gi[4, k - 1] == -1
    check(q, x, k, excl=R.csr(rows), n_splits=3)


def test_exclusion_base_and_exclude_one(excl_case):
    q, x, rows, k = excl_case
    shifted = R.csr([[1, 2, 3], [], [4]] + rows)
    check(q, x, k, excl=shifted, excl_base=3)
    top = check(q, x, k)[0][0]
    one = np.array([top[0], -1, top[1], 10 ** 6, top[0]], np.int32)
    gi, _ = check(q, x, k, excl_one=one)
    assert gi[0, 0] == top[1] and gi[1, 0] == top[0] and gi[3, 0] == top[0]
    check(q, x, k, excl=R.csr(rows), excl_one=one, n_splits=2)


def test_long_exclusion_rows_over_many_rounds():
    """300-id rows (five 64-id loads each) against 3000 items: compaction meets the exclusion."""
    rng = np.random.default_rng(8)
    q, x = R.exact_vectors(8, 33, 16), R.exact_vectors(9, 3000, 16)
    s = R.scores_ref(q, x)
    rows = []
    for r in range(33):
        best = np.argsort(-s[r], kind="stable")[:150]  # half of each row is its best items
        rows.append(list(rng.permutation(np.concatenate([best, rng.integers(0, 3000, 150)]))))
    excl = R.csr(rows)
    ref = R.topk_from_scores(s, 10, excl)
    check(q, x, 10, ref=ref, excl=excl)
    check(q, x, 10, ref=ref, excl=excl, n_splits=7)


# ---- argument errors ---------------------------------------------------------------------
def test_argument_errors_write_nothing():
    q, x = R.exact_vectors(1, 5, 8), R.exact_vectors(2, 50, 8)
    bad = L.RS_E_INVALID
    for kw in (dict(k=0), dict(k=65), dict(n_splits=51), dict(n_splits=-1),
               dict(n_splits=2, ws_bytes=16)):
        raw_call(q, x, kw.pop("k", 10), expect=bad, **kw)
    lib = L.lib()
    tq, tx = dev(q), dev(x)
    oi = torch.full((50,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    s = L.stream_ptr(oi.device)

    def args(a, b, o, dim=8, n=50, q_ld=8, i_ld=8):
        return (a, q_ld, 5, b, i_ld, n, dim, 0, None, None, None, 10, 1, o, None, None, 0, s)

    assert lib.rs_topk_ip(*args(None, L.ptr(tx), L.ptr(oi))) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), None, L.ptr(oi))) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), None)) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), L.ptr(oi), dim=0)) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), L.ptr(oi), dim=257)) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), L.ptr(oi), q_ld=7)) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), L.ptr(oi), i_ld=7)) == bad
    assert lib.rs_topk_ip(*args(L.ptr(tq), L.ptr(tx), L.ptr(oi), n=2 ** 31)) == bad
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == GUARD_ITEM).all()
    assert b"rs_topk_ip" in lib.rs_last_error()


def test_no_queries_and_no_items():
    q, x = R.exact_vectors(1, 5, 8), R.exact_vectors(2, 50, 8)
    gi, gs = raw_call(q[:0], x, 10)
    assert gi.shape == (0, 10)
    gi, gs = raw_call(q, x[:0], 10)
    assert (gi == -1).all() and (gs == -np.inf).all()
    assert L.lib().rs_topk_ip_workspace_size(5, 50, 10, 1) == 0
    assert L.lib().rs_topk_ip_workspace_size(5, 50, 10, 3) >= 5 * 3 * 10 * 8


# ---- the Python surfaces -----------------------------------------------------------------
def test_topk_inner_product_surface():
    from recommender_amd.functional import topk_inner_product

    q, x = R.exact_vectors(1, 40, 18), R.exact_vectors(2, 500, 18)
    rows = [[int(i) for i in np.random.default_rng(r).integers(0, 500, r % 7)] for r in range(43)]
    ip, it = R.csr(rows)
    one = np.arange(40, dtype=np.int32)
    ri, rs = R.topk_ref(q, x, 12, excl=(ip, it), excl_base=3, excl_one=one)
    wide = torch.full((40, 32), float("nan"), device=DEV)
    wide[:, 4:22] = dev(q)
    idx, val = topk_inner_product(wide[:, 4:22], dev(x), 12, exclude=(dev(ip), dev(it)),
                                  exclude_base=3, exclude_one=dev(one), n_splits=4)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    assert R.same_scores(val.cpu().numpy(), rs)
    idx2, none = topk_inner_product(dev(q), dev(x), 12, exclude=(dev(ip), dev(it)), exclude_base=3,
                                    exclude_one=dev(one), with_scores=False)
    assert none is None
    np.testing.assert_array_equal(idx2.cpu().numpy(), ri)
    with pytest.raises(L.RecsysError):
        topk_inner_product(torch.zeros(2, 18), dev(x), 3)
    with pytest.raises(L.RecsysError):
        topk_inner_product(dev(q), dev(x), 65)


def _graph(users, items, ts, n_users, n_items):
    from recommender_amd.pinsage.graph import HeteroGraph

    return HeteroGraph(users, items, n_users, n_items, device=DEV, edge_data={"timestamp": ts})


def test_recommend_fused_equals_unfused_on_exact_reprs():
    from recommender_amd.pinsage.evaluation import recommend

    users, items, ts = R.recommend_graph(1)
    g = _graph(users, items, ts, 300, 500)
    reprs = dev(R.exact_vectors(2, 500, 16))
    a = recommend(g, 10, reprs, None, "user", "timestamp", 32)
    b = recommend(g, 10, reprs, None, "user", "timestamp", 32, fused=True)
    assert b.dtype == torch.int32 and b.shape == (300, 10)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_recommend_fused_agrees_on_random_reprs_where_the_scores_decide():
    from recommender_amd.pinsage.evaluation import recommend

    users, items, ts, reprs, latest = R.recommend_inputs()
    g = _graph(users, items, ts, 300, 500)
    k = R.RECOMMEND_K
    a = recommend(g, k, dev(reprs), None, "user", "timestamp", 32).cpu().numpy()
    b = recommend(g, k, dev(reprs), None, "user", "timestamp", 32, fused=True).cpu().numpy()
    set_ok, order_ok = R.decided_users(reprs, latest, users, items, k)
    assert (~set_ok).mean() < 0.01 and (~order_ok).mean() < 0.01
    np.testing.assert_array_equal(np.sort(a[set_ok], 1), np.sort(b[set_ok], 1))
    np.testing.assert_array_equal(a[order_ok], b[order_ok])
    ri, _ = R.topk_ref(reprs[latest], reprs, k, excl=(g.u2i_indptr.cpu().numpy(),
                                                      g.u2i.cpu().numpy()))
    np.testing.assert_array_equal(b, ri)  # the fused path itself is exact


@pytest.mark.parametrize("D", [8, 160])
def test_similar_items_over_the_three_eges_models(D):
    from recommender_amd.eges.retrieval import item_hidden, similar_items
    from recommender_amd.eges.train import build

    n = 200
    cat, brand = (np.arange(n) * 2654435761) % 11, (np.arange(n) * 40503) % 17
    query = np.array([0, 5, 199, 5, 64], np.int64)
    for model_type in ("BGE", "GES", "EGES"):
        gen = torch.Generator(device=DEV).manual_seed(3)
        model = build(model_type, n, 11, 17, embedding_size=D, generator=gen)
        hidden = item_hidden(model, cat, brand, batch=64)
        assert hidden.shape == (n, D) and not hidden.requires_grad
        whole = item_hidden(model, cat, brand)
        np.testing.assert_array_equal(hidden.cpu().numpy(), whole.cpu().numpy())
        idx, val = similar_items(hidden, dev(query), 10)
        h = hidden.cpu().numpy()
        ri, rs = R.topk_ref(h[query], h, 10, excl_one=query)
        np.testing.assert_array_equal(idx.cpu().numpy(), ri)
        assert R.same_scores(val.cpu().numpy(), rs)
        assert not (idx.cpu().numpy() == query[:, None]).any()


def test_inference_cli_writes_the_neighbours(tmp_path):
    from recommender_amd.pinsage import inference as I

    out, nb = tmp_path / "reprs.npy", tmp_path / "nbrs.npy"
    I.main(["--out", str(out), "--neighbors", "5", "--neighbors-out", str(nb)])
    reprs, nbrs = np.load(out), np.load(nb)
    assert nbrs.dtype == np.int32 and nbrs.shape == (reprs.shape[0], 5)
    rows = np.r_[0:reprs.shape[0]:8, reprs.shape[0] - 1]  # the ref on every 8th query, all items
    ri, _ = R.topk_ref(reprs[rows], reprs, 5, excl_one=rows)
    np.testing.assert_array_equal(nbrs[rows], ri)
    assert not (nbrs == np.arange(reprs.shape[0])[:, None]).any()
