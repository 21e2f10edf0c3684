"""rs_ivf_topk_ip on the GPU against tests/ivf_topk_ref.py and against rs_topk_ip, bit for bit:
equality with the exhaustive search when every list is probed, the restricted search, the tile,
grouping and sub-range edges, order, exclusion in reported ids, bad offsets, argument errors,
graph capture, and IVFIndex and the call sites built on it. Every list scan goes through the C
entry point with 64 guard elements behind each output."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import ivf_topk_ref as V
from tests import topk_ip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
GUARD_ITEM = 0x5A5A5A5A
GUARD_SCORE = 0x7FC12345  # a NaN with a payload


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).to(DEV)


def raw_ivf(q, probes, off, ids, vec, k, excl=None, excl_base=0, excl_one=None, list_splits=0,
            v_ld=None, offset=0, with_scores=True, ws_bytes=None, expect=0, n_items=None):
    """rs_ivf_topk_ip → (items [Q, k], scores [Q, k] or None) as NumPy; guards checked. v_ld /
    offset: the rows of vectors at stride v_ld (NaN between), `offset` floats into their buffer."""
    lib = L.lib()
    nq, dim = q.shape
    n = vec.shape[0] if n_items is None else n_items
    probes = np.asarray(probes, np.int32)
    assert probes.ndim == 2 and probes.shape[0] == nq
    nprobe, n_lists = probes.shape[1], len(off) - 1
    va = np.full((vec.shape[0], v_ld or dim), np.nan, f32)
    va[:, :dim] = vec
    tv_buf = torch.full((va.size + offset + 1,), float("nan"), device=DEV)
    tv_buf[offset:offset + va.size] = dev(va).reshape(-1)
    tq, tp, to, ti = dev(q, f32), dev(probes), dev(off, np.int64), dev(ids, np.int32)
    ip = it = None
    if excl is not None:
        ip, it = dev(excl[0], np.int64), dev(np.append(excl[1], 0), np.int32)
    one = dev(excl_one, np.int32)
    oi = torch.full((nq * k + GUARD,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    os_ = torch.full((nq * k + GUARD,), GUARD_SCORE, dtype=torch.int32, device=DEV)
    need = lib.rs_ivf_topk_ip_workspace_size(nq, nprobe, n_lists, k, list_splits)
    if ws_bytes is None:
        ws_bytes = need
    ws = torch.full((ws_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    st = lib.rs_ivf_topk_ip(L.ptr(tq), dim, nq, L.ptr(tp), nprobe, L.ptr(to), n_lists, L.ptr(ti),
                            L.ptr(tv_buf[offset:]), v_ld or dim, n, dim, excl_base, L.ptr(ip),
                            L.ptr(it), L.ptr(one), k, list_splits, L.ptr(oi),
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


def exhaustive(q, x, k, **kw):
    """rs_topk_ip on the same data through the Python wrapper."""
    from recommender_amd.functional import topk_inner_product

    idx, val = topk_inner_product(dev(q), dev(x), k, **kw)
    return idx.cpu().numpy(), val.cpu().numpy()


def assert_same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    if got[1] is not None:
        assert R.same_scores(got[1], want[1]), np.argwhere(
            got[1].view(np.uint32) != want[1].view(np.uint32))[:5]


def check(q, probes, off, ids, vec, k, ref=None, **kw):
    ref_kw = {n: kw[n] for n in ("excl", "excl_base", "excl_one") if n in kw}
    if ref is None:
        ref = V.ivf_topk_ref(q, probes, off, ids, vec, k, **ref_kw)
    got = raw_ivf(q, probes, off, ids, vec, k, **kw)
    assert_same(got, ref)
    return got


# ---- equals the exhaustive search ---------------------------------------------------------
DIMS = (1, 3, 4, 18, 36, 128, 255, 256)


@pytest.mark.parametrize("dim", DIMS)
def test_one_list_without_ids_is_rs_topk_ip(dim):
    q, x = R.random_floats(20 + dim, 33, dim), R.random_floats(40 + dim, 200, dim)
    want = exhaustive(q, x, 64)
    assert_same(want, R.topk_ref(q, x, 64))
    assert_same(raw_ivf(q, np.zeros((33, 1)), [0, 200], None, x, 64), want)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [1, 10, 64])
def test_eight_permuted_lists_all_probed_are_rs_topk_ip(dim, k):
    items, off, ids, vec = V.permuted_index(dim, 500, dim, 8, exact=False)
    q = R.random_floats(60 + dim, 35, dim)
    assert_same(raw_ivf(q, V.all_probes(35, 8, dim), off, ids, vec, k), exhaustive(q, items, k))


@pytest.mark.parametrize("dim,v_ld,offset", [(18, 20, 0), (18, 19, 0), (16, 16, 1), (36, 64, 0),
                                             (255, 256, 0), (256, 256, 3)])
def test_strided_and_misaligned_vectors(dim, v_ld, offset):
    """v_ld a multiple of 4 on an aligned base takes the 16-byte loads (a partial last group at
    dim 18 and 255); an odd v_ld or a base 4 or 12 bytes off takes the element loads."""
    items, off, ids, vec = V.permuted_index(dim + 1, 300, dim, 8, exact=False)
    q = R.random_floats(80, 33, dim)
    probes = V.all_probes(33, 8, 1)
    want = exhaustive(q, items, 64)
    assert_same(raw_ivf(q, probes, off, ids, vec, 64), want)
    assert_same(raw_ivf(q, probes, off, ids, vec, 64, v_ld=v_ld, offset=offset), want)


# ---- the restricted search ----------------------------------------------------------------
@pytest.fixture(scope="module")
def idx8():
    """500 exact rows at dim 18 over 8 lists, 37 exact queries, their scores: shared, unchanged."""
    items, off, ids, vec = V.permuted_index(7, 500, 18, 8)
    q = R.exact_vectors(8, 37, 18)
    s = R.scores_ref(q, vec)
    for a in (items, off, ids, vec, q, s):
        a.setflags(write=False)
    return items, off, ids, vec, q, s


@pytest.mark.parametrize("nprobe", [1, 3])
def test_fewer_probes_than_lists(idx8, nprobe):
    items, off, ids, vec, q, s = idx8
    probes = V.all_probes(37, 8, 3)[:, :nprobe]
    check(q, probes, off, ids, vec, 10,
          ref=V.ivf_topk_ref(q, probes, off, ids, vec, 10, scores=s))


def test_messy_probe_rows_and_fewer_than_k_candidates(idx8):
    items, off, ids, vec, q, s = idx8
    probes = V.messy_probes(8)
    gi, gs = check(q[:5], probes, off, ids, vec, 64,
                   ref=V.ivf_topk_ref(q[:5], probes, off, ids, vec, 64, scores=s[:5]))
    assert (gi[2] == -1).all() and (gs[2] == -np.inf).all()       # all probes -1
    assert np.bincount(gi[3]).max() == 3                          # a list probed three times
    lone = np.array([[1]], np.int32)                              # one list of fewer than k rows
    gi, _ = check(q[:1], lone, [0, 0, 7, 7], ids, vec, 10)
    assert (gi[0, :7] >= 0).all() and (gi[0, 7:] == -1).all()


# ---- tile and grouping edges --------------------------------------------------------------
@pytest.fixture(scope="module")
def lengths():
    items, off, ids, vec = V.list_length_index(2, 16)
    q = R.exact_vectors(3, 33, 16)
    return items, off, ids, vec, q, R.scores_ref(q, vec)


@pytest.mark.parametrize("list_splits", [0, 1, 2, 3, 7])
def test_list_lengths_by_sub_range_count(lengths, list_splits):
    """Lists of 0, 1, 31, 32, 33, 128, 129 and 513 rows, each probed alone by some queries and
    all probed by others; lists shorter than list_splits leave empty sub-ranges."""
    items, off, ids, vec, q, s = lengths
    n_lists = len(V.LIST_LENGTHS)
    probes = np.full((33, n_lists), -1, np.int32)
    probes[:n_lists, 0] = np.arange(n_lists)             # query l: list l alone
    probes[n_lists:] = V.all_probes(33 - n_lists, n_lists, 4)
    ref = V.ivf_topk_ref(q, probes, off, ids, vec, 10, scores=s)
    check(q, probes, off, ids, vec, 10, ref=ref, list_splits=list_splits)
    assert (ref[0][0] == -1).all() and (ref[0][1, 1:] == -1).all()  # the lists of 0 and 1 rows
    assert_same((ref[0][n_lists:], ref[1][n_lists:]), R.topk_ref(q[n_lists:], items, 10))


@pytest.mark.parametrize("list_splits", [1, 3])
def test_lists_probed_by_1_32_33_and_65_queries(list_splits):
    items, off, ids, vec = V.permuted_index(9, 300, 18, 4)
    q = R.exact_vectors(10, 65, 18)
    check(q, V.probe_count_probes(), off, ids, vec, 10, list_splits=list_splits)


def test_grouping_extremes():
    items, off, ids, vec = V.permuted_index(11, 400, 8, 70)
    q = R.exact_vectors(12, 70, 8)
    s = R.scores_ref(q, vec)
    one_list = np.full((70, 1), 5, np.int32)                      # all queries on one list
    own_list = np.arange(70, dtype=np.int32)[:, None]             # each query on its own list
    for probes in (one_list, own_list):
        check(q, probes, off, ids, vec, 10,
              ref=V.ivf_topk_ref(q, probes, off, ids, vec, 10, scores=s))
    check(q[:1], own_list[3:4], off, ids, vec, 10)                # Q = 1
    check(q[:1], [[0, 0]], [0, 400], ids, vec, 10)                # n_lists = 1, probed twice


def test_a_query_alone_and_inside_a_batch(idx8):
    items, off, ids, vec, q, s = idx8
    probes = V.all_probes(37, 8, 5)[:, :4]
    batch = raw_ivf(q, probes, off, ids, vec, 10)
    for r in (0, 20, 36):
        alone = raw_ivf(q[r:r + 1], probes[r:r + 1], off, ids, vec, 10, list_splits=2)
        assert_same(alone, (batch[0][r:r + 1], batch[1][r:r + 1]))


# ---- order --------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_equal_vectors_in_different_lists_tie_by_reported_id(descending):
    items, off, ids, vec = V.duplicate_vector_index(descending=descending)
    q = R.exact_vectors(18, 5, 4)
    probes = V.all_probes(5, 4, seed=2)
    gi, _ = check(q, probes, off, ids, vec, 10, list_splits=2)
    assert_same((gi, None), R.topk_ref(q, items, 10))
    wrong = V.ivf_topk_ref(q, probes, off, ids, vec, 10, by_position=True)
    if descending:
        assert not np.array_equal(gi, wrong[0])


def test_nan_infinite_and_signed_zero_scores():
    q, x = R.special_catalogue()
    assign = np.arange(40) % 3
    off, ids, vec = V.index_from_assignment(x, assign, 3, descending=True)
    for k in (5, 40, 64):
        got = check(q, V.all_probes(3, 3), off, ids, vec, k)
        assert_same(got, R.topk_ref(q, x, k))
    check(q, [[1], [2], [0]], off, ids, vec, 40, list_splits=3)
    # a negative product that underflows leaves -0; it ties with +0 and is written as -0
    # (dim 1: a later +0 product would turn the -0 into +0)
    zq = np.array([[1e-30]], f32)
    zx = np.array([[-1e-30], [0], [1e-30]], f32)
    gi, gs = check(zq, [[0, 1]], [0, 2, 3], [2, 0, 1], zx, 3)
    assert list(gi[0]) == [0, 1, 2] and gs.view(np.uint32)[0, 2] == 0x80000000


def test_ids_that_are_not_distinct(idx8):
    items, off, ids, vec, q, s = idx8
    shared = (np.asarray(ids) // 2).astype(np.int32)  # every id twice, with different vectors
    probes = V.all_probes(37, 8, 6)[:, :5]
    check(q, probes, off, shared, vec, 10,
          ref=V.ivf_topk_ref(q, probes, off, shared, vec, 10, scores=s))
    one = np.arange(37)  # excludes both rows that share the id
    gi, _ = check(q, probes, off, shared, vec, 10, excl_one=one,
                  ref=V.ivf_topk_ref(q, probes, off, shared, vec, 10, scores=s, excl_one=one))
    assert not (gi == one[:, None]).any()


# ---- exclusion ----------------------------------------------------------------------------
def test_exclusion_in_reported_ids(idx8):
    items, off, ids, vec, q, s = idx8
    q, s = q[:5], s[:5]
    probes = V.all_probes(5, 8, 7)
    top = V.ivf_topk_ref(q, probes, off, ids, vec, 10, scores=s)[0]
    rows = [R.exclusion_rows(top[r], 500, 10)[r] for r in range(5)]
    excl = R.csr(rows)
    one = np.array([top[0, 0], -1, top[2, 1], 10 ** 6, top[4, 0]], np.int32)
    shifted = R.csr([[1, 2, 3], [], [4]] + rows)
    for kw in (dict(excl=excl), dict(excl_one=one), dict(excl=excl, excl_one=one),
               dict(excl=shifted, excl_base=3, list_splits=3)):
        got = check(q, probes, off, ids, vec, 10,
                    ref=V.ivf_topk_ref(q, probes, off, ids, vec, 10, scores=s, **{
                        n: v for n, v in kw.items() if n != "list_splits"}), **kw)
        assert_same(got, R.topk_ref(q, items, 10, **{n: v for n, v in kw.items()
                                                      if n != "list_splits"}))
    gi, gs = raw_ivf(q, probes, off, ids, vec, 10, excl=excl)
    assert (gi[1] == -1).all() and not set(gi[2]) & set(top[2])


# ---- offsets ------------------------------------------------------------------------------
def test_bad_offsets_are_clipped(idx8):
    items, off, ids, vec, q, s = idx8
    bad = np.array(off).copy()
    bad[3], bad[4] = off[4], off[3] - 5      # lists 2 and 4 overlap their neighbours, 3 is reversed
    bad[8] = 10 ** 12                        # the last list runs far past n_items
    bad[0] = -9
    probes = V.all_probes(37, 8, 8)[:, :6]
    check(q, probes, bad, ids, vec, 10,
          ref=V.ivf_topk_ref(q, probes, bad, ids, vec, 10, scores=s), list_splits=2)


# ---- errors, sizes, determinism -----------------------------------------------------------
def test_argument_errors_write_nothing(idx8):
    items, off, ids, vec, q, s = idx8
    q, bad = q[:5], L.RS_E_INVALID
    probes = V.all_probes(5, 8)[:, :2]
    for kw in (dict(k=0), dict(k=65), dict(list_splits=-1), dict(list_splits=513),
               dict(ws_bytes=64), dict(n_items=-1), dict(n_items=2 ** 31)):
        raw_ivf(q, probes, off, ids, vec, kw.pop("k", 10), expect=bad, **kw)
    raw_ivf(q, np.zeros((5, 65)), off, ids, vec, 10, expect=bad)          # nprobe 65
    lib = L.lib()
    t = [dev(q), dev(probes), dev(off, np.int64), dev(vec)]
    oi = torch.full((50,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.rs_ivf_topk_ip_workspace_size(5, 2, 8, 10, 1), dtype=torch.uint8,
                     device=DEV)
    stream = L.stream_ptr(oi.device)

    def call(drop=None, dim=18, q_ld=18, v_ld=18, nprobe=2, n_lists=8, nq=5, base=0, out=True):
        p = [None if i == drop else L.ptr(x) for i, x in enumerate(t)]
        return lib.rs_ivf_topk_ip(p[0], q_ld, nq, p[1], nprobe, p[2], n_lists, None, p[3], v_ld,
                                  500, dim, base, None, None, None, 10, 1,
                                  L.ptr(oi) if out else None, None, L.ptr(ws), ws.numel(), stream)

    for kw in ([dict(drop=i) for i in range(4)] + [dict(out=False), dict(dim=0), dict(dim=257),
               dict(q_ld=17), dict(v_ld=17), dict(nprobe=0), dict(n_lists=-1), dict(nq=-1),
               dict(base=-1)]):
        assert call(**kw) == bad, kw
    assert b"rs_ivf_topk_ip" in lib.rs_last_error()
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == GUARD_ITEM).all()
    assert call() == 0


def test_no_queries_no_items_no_lists(idx8):
    items, off, ids, vec, q, s = idx8
    probes = V.all_probes(5, 8)[:, :2]
    gi, _ = raw_ivf(q[:0], probes[:0], off, ids, vec, 10)        # the guards stay intact
    assert gi.shape == (0, 10)
    for args in ((probes, [0] * 9, ids[:0], vec[:0]), (probes, [0], ids, vec)):
        gi, gs = raw_ivf(q[:5], *args, 10, ws_bytes=0)
        assert (gi == -1).all() and (gs == -np.inf).all()
    lib = L.lib()
    assert lib.rs_ivf_topk_ip_workspace_size(5, 2, 8, 10, 3) >= 5 * 2 * 3 * 10 * 8
    assert lib.rs_ivf_topk_ip_workspace_size(0, 2, 8, 10, 1) == 0


def test_two_runs_and_no_scores(idx8):
    items, off, ids, vec, q, s = idx8
    probes = V.all_probes(37, 8, 9)[:, :5]
    a = raw_ivf(q, probes, off, ids, vec, 10, list_splits=7)
    assert_same(raw_ivf(q, probes, off, ids, vec, 10, list_splits=7), a)
    c, none = raw_ivf(q, probes, off, ids, vec, 10, with_scores=False)
    assert none is None
    np.testing.assert_array_equal(c, a[0])


def test_captured_in_a_graph_and_replayed_on_new_queries_and_probes(idx8):
    from recommender_amd.functional import ivf_topk_inner_product

    items, off, ids, vec, q, s = idx8
    p1, p2 = V.all_probes(37, 8, 10)[:, :3], V.all_probes(37, 8, 11)[:, :3]
    q2 = R.exact_vectors(13, 37, 18)
    tq, tp = dev(q).clone(), dev(p1).clone()
    to, ti, tv = dev(off, np.int64), dev(ids, np.int32), dev(vec)
    ivf_topk_inner_product(tq, tp, to, ti, tv, 10)  # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx, val = ivf_topk_inner_product(tq, tp, to, ti, tv, 10)
    for qq, pp in ((q, p1), (q2, p2), (q, p2)):
        tq.copy_(dev(qq))
        tp.copy_(dev(pp))
        g.replay()
        torch.cuda.synchronize()
        assert_same((idx.cpu().numpy(), val.cpu().numpy()),
                    V.ivf_topk_ref(qq, pp, off, ids, vec, 10))


# ---- IVFIndex -----------------------------------------------------------------------------
def state_np(index):
    return {k: v.cpu().numpy() for k, v in index.state_dict().items()}


def test_build_invariants():
    from recommender_amd.retrieval import IVFIndex

    x = R.random_floats(30, 700, 18, extremes=False)
    a = IVFIndex.build(dev(x), 12, n_iter=4)
    sd = state_np(a)
    off, ids = sd["list_offsets"], sd["item_ids"]
    assert (a.nlist, a.n_items, a.dim) == (12, 700, 18) and off[0] == 0 and off[-1] == 700
    np.testing.assert_array_equal(a.list_sizes.cpu().numpy(), np.diff(off))
    assert sorted(ids) == list(range(700))                                  # every id once
    assert all((np.diff(ids[off[l]:off[l + 1]]) > 0).all() for l in range(12))  # ascending
    assert np.array_equal(sd["vectors"].view(np.uint32), x[ids].view(np.uint32))
    # one rounding of a float64 sum: at most one float32 ulp from any other summation order
    np.testing.assert_allclose(sd["centroid_bias"], V.centroid_bias(sd["centroids"]), rtol=2 ** -23)
    # the stored lists are the k = 1 result over the stored [centroids, bias]
    x1 = np.hstack([x, np.ones((700, 1), f32)])
    cb = np.hstack([sd["centroids"], sd["centroid_bias"][:, None]])
    nearest = R.topk_ref(x1, cb, 1)[0][:, 0]
    np.testing.assert_array_equal(np.repeat(np.arange(12), np.diff(off)), nearest[ids])
    b = state_np(IVFIndex.build(dev(x), 12, n_iter=4))
    assert all(np.array_equal(sd[k].view(np.uint8), b[k].view(np.uint8)) for k in sd)


def test_build_honours_init_and_keeps_the_centroid_of_an_empty_list():
    from recommender_amd.retrieval import IVFIndex

    items, centres, _ = V.planted_clusters()
    far = np.vstack([centres[:7], np.full((1, 16), 100, f32)])
    index = IVFIndex.build(dev(items), 8, n_iter=2, init=dev(far))
    c, assign = V.kmeans_ref(items, 8, 2, far)
    sd = state_np(index)
    np.testing.assert_array_equal(sd["centroids"][7], far[7])
    np.testing.assert_array_equal(sd["centroids"], c.astype(f32))
    assert np.diff(sd["list_offsets"])[7] == 0
    zero = IVFIndex.build(dev(items), 8, n_iter=0, init=dev(centres))
    np.testing.assert_array_equal(zero.centroids.cpu().numpy(), centres)


@pytest.mark.parametrize("with_init", [False, True])
def test_build_on_the_planted_input_equals_kmeans_ref(with_init):
    from recommender_amd.retrieval import IVFIndex

    items, centres, queries = V.planted_clusters()
    init = centres if with_init else None
    index = IVFIndex.build(dev(items), 8, n_iter=3, init=dev(init))
    c, assign = V.kmeans_ref(items, 8, 3, init)
    off, ids, vec = V.index_from_assignment(items, assign, 8)
    sd = state_np(index)
    np.testing.assert_array_equal(sd["list_offsets"], off)
    np.testing.assert_array_equal(sd["item_ids"], ids)
    np.testing.assert_array_equal(sd["centroids"], c.astype(f32))
    # nprobe = 1 already holds every query's exact top-k (tests/test_ivf_topk_cpu.py)
    exact = exhaustive(queries, items, 10)
    for nprobe in (1, 8, 11):
        idx, val = index.search(dev(queries), 10, nprobe)
        assert_same((idx.cpu().numpy(), val.cpu().numpy()), exact)


def test_search_surface_state_dict_and_dim_256():
    from recommender_amd.retrieval import IVFIndex

    x, q = R.random_floats(31, 600, 36, extremes=False), R.random_floats(32, 40, 36, False)
    index = IVFIndex.build(dev(x), 9, n_iter=3)
    one = np.arange(40, dtype=np.int32)
    excl = R.csr([[int(i) for i in np.random.default_rng(r).integers(0, 600, r % 7)]
                  for r in range(43)])
    kw = dict(exclude=(dev(excl[0]), dev(excl[1])), exclude_base=3, exclude_one=dev(one))
    idx, val = index.search(dev(q), 12, 9, list_splits=2, **kw)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    assert_same((idx.cpu().numpy(), val.cpu().numpy()), exhaustive(q, x, 12, **kw))
    # fewer probes: the reference over the probes the index chose
    sd = state_np(index)
    probes = index.probes(dev(q), 3).cpu().numpy()
    np.testing.assert_array_equal(probes, R.topk_ref(q, sd["centroids"], 3)[0])
    idx, none = index.search(dev(q), 12, 3, with_scores=False)
    assert none is None
    np.testing.assert_array_equal(idx.cpu().numpy(), V.ivf_topk_ref(
        q, probes, sd["list_offsets"], sd["item_ids"], sd["vectors"], 12)[0])
    again = IVFIndex.from_state_dict({k: v.clone() for k, v in index.state_dict().items()})
    np.testing.assert_array_equal(again.search(dev(q), 12, 3)[0].cpu().numpy(), idx.cpu().numpy())
    with pytest.raises(KeyError):
        IVFIndex.from_state_dict({"centroids": index.centroids})
    wide = R.random_floats(33, 80, 256, extremes=False)
    with pytest.raises(ValueError, match="from_assignment"):
        IVFIndex.build(dev(wide), 4)
    with pytest.raises(ValueError):
        IVFIndex.build(dev(x[:5]), 6)
    hand = IVFIndex.from_assignment(dev(wide), dev(wide[:4]), dev(np.arange(80) % 4))
    idx, val = hand.search(dev(wide[:9]), 10, 4)
    assert_same((idx.cpu().numpy(), val.cpu().numpy()), exhaustive(wide[:9], wide, 10))


# ---- call sites ---------------------------------------------------------------------------
def test_similar_items_with_an_index():
    from recommender_amd.eges.retrieval import similar_items
    from recommender_amd.retrieval import IVFIndex

    hidden = dev(R.random_floats(34, 300, 16, extremes=False))
    query = dev(np.array([0, 5, 299, 5, 64], np.int64))
    index = IVFIndex.build(hidden, 6, n_iter=2)
    a = similar_items(hidden, query, 10)
    b = similar_items(hidden, query, 10, index=index, nprobe=6)
    assert_same(tuple(t.cpu().numpy() for t in b), tuple(t.cpu().numpy() for t in a))
    c = similar_items(hidden, query, 10, index=index)  # nprobe 8 > nlist: every list, -1 padded
    assert_same(tuple(t.cpu().numpy() for t in c), tuple(t.cpu().numpy() for t in a))


def test_recommend_with_an_index():
    from recommender_amd.pinsage.evaluation import recommend
    from recommender_amd.pinsage.graph import HeteroGraph
    from recommender_amd.retrieval import IVFIndex

    users, items, ts = R.recommend_graph(1)
    g = HeteroGraph(users, items, 300, 500, device=DEV, edge_data={"timestamp": ts})
    reprs = dev(R.exact_vectors(2, 500, 16))
    index = IVFIndex.build(reprs, 7, n_iter=2)
    a = recommend(g, 10, reprs, None, "user", "timestamp", 32, fused=True)
    b = recommend(g, 10, reprs, None, "user", "timestamp", 32, fused=True, index=index, nprobe=7)
    assert b.dtype == torch.int32 and b.shape == (300, 10)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    with pytest.raises(ValueError):
        recommend(g, 10, reprs, None, "user", "timestamp", 32, index=index)


def test_inference_cli_neighbours_through_an_index(tmp_path):
    from recommender_amd.pinsage import inference as I

    exact, ivf = tmp_path / "exact.npy", tmp_path / "ivf.npy"
    I.main(["--neighbors", "5", "--neighbors-out", str(exact)])
    I.main(["--neighbors", "5", "--neighbors-out", str(ivf), "--neighbors-nlist", "4",
            "--neighbors-nprobe", "4"])
    np.testing.assert_array_equal(np.load(ivf), np.load(exact))
