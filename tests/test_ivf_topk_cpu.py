"""tests/ivf_topk_ref.py without a GPU: the restatement agrees with topk_ip_ref where the two
contracts coincide, every case builder has the property it is named for, the planted-cluster
input has the two facts the build and recall tests rest on, and a wrong restatement is caught."""
import numpy as np

from tests import ivf_topk_ref as V
from tests import topk_ip_ref as R

f32 = np.float32


def same(a, b):
    return np.array_equal(a[0], b[0]) and R.same_scores(a[1], b[1])


def test_one_list_with_identity_ids_is_topk_ref():
    q, x = R.random_floats(1, 9, 18), R.random_floats(2, 150, 18)
    probes = np.zeros((9, 1), np.int32)
    one = np.arange(9, dtype=np.int32)
    excl = R.csr([[r, 3, 149, 200, -1] for r in range(9)])
    for ids in (None, np.arange(150, dtype=np.int32)):
        assert same(V.ivf_topk_ref(q, probes, [0, 150], ids, x, 10), R.topk_ref(q, x, 10))
        assert same(V.ivf_topk_ref(q, probes, [0, 150], ids, x, 10, excl=excl, excl_one=one),
                    R.topk_ref(q, x, 10, excl=excl, excl_one=one))


def test_every_list_probed_is_topk_ref_over_the_permuted_catalogue():
    for descending in (False, True):
        items, off, ids, vec = V.permuted_index(3, 300, 8, 8, descending=descending)
        assert sorted(ids) == list(range(300)) and np.array_equal(vec, items[ids])
        q = R.exact_vectors(4, 7, 8)  # exact inputs: ties are plentiful
        got = V.ivf_topk_ref(q, V.all_probes(7, 8), off, ids, vec, 20)
        assert same(got, R.topk_ref(q, items, 20))
        inside = [np.diff(ids[off[l]:off[l + 1]]) for l in range(8)]
        assert all(((d < 0) if descending else (d > 0)).all() for d in inside)


def test_fewer_probes_see_fewer_rows():
    items, off, ids, vec = V.permuted_index(3, 300, 8, 8)
    q = R.exact_vectors(4, 3, 8)
    probes = np.array([[2, 5], [5, 5], [-1, 8]], np.int32)
    gi, gs = V.ivf_topk_ref(q, probes, off, ids, vec, 64)
    members = set(ids[off[2]:off[3]]) | set(ids[off[5]:off[6]])
    assert set(gi[0][gi[0] >= 0]) == members if len(members) <= 64 else set(gi[0]) <= members
    five = ids[off[5]:off[6]]
    counts = np.bincount(gi[1][gi[1] >= 0], minlength=300)
    assert set(np.flatnonzero(counts)) <= set(five) and counts.max() == 2  # a repeat counts twice
    assert (gi[2] == -1).all() and (gs[2] == -np.inf).all()


def test_bad_offsets_are_clipped():
    rows = V.probed_rows([0, 1, 2, 3], [-5, 3, 2, 9, 40], 10)  # non-monotone pair (3, 2); 40 > n
    assert list(rows) == [0, 1, 2] + [] + [2, 3, 4, 5, 6, 7, 8] + [9]


def test_list_length_case_has_every_length():
    items, off, ids, vec = V.list_length_index(1, 4)
    assert tuple(np.diff(off)) == V.LIST_LENGTHS == (0, 1, 31, 32, 33, 128, 129, 513)
    assert sorted(ids) == list(range(sum(V.LIST_LENGTHS))) and items.shape[0] <= 2000
    assert {31, 32, 33} <= set(V.LIST_LENGTHS) and {128, 129} <= set(V.LIST_LENGTHS)
    assert not (np.diff(ids) > 0).all()  # the ids are scattered, not the stored order


def test_probe_count_case_has_every_count():
    p = V.probe_count_probes()
    assert p.shape == (65, 4) and V.PROBE_COUNTS == (1, 32, 33, 65)
    for l, c in enumerate(V.PROBE_COUNTS):
        assert (p == l).sum() == c and ((p == l).sum(1) <= 1).all()
        if c > 1:
            assert len(set(np.argwhere(p == l)[:, 1])) > 1  # at several probe positions
    assert (p[0] == -1).sum() == 3  # a row probing one list only


def test_messy_probes():
    p = V.messy_probes(4)
    assert -1 in p[0] and 4 in p[1] and (p[2] == -1).all() and len(set(p[3])) == 1
    assert list(p[1]).count(1) == 2


def test_duplicate_vector_case():
    for descending in (False, True):
        items, off, ids, vec = V.duplicate_vector_index(descending=descending)
        lists = np.repeat(np.arange(4), np.diff(off))
        where = {int(i): int(l) for i, l in zip(ids, lists)}
        groups = [[where[b + 10 * t] for t in range(4)] for b in range(10)]
        assert all(len(set(g)) > 1 for g in groups)              # equal vectors across lists
        assert any(len(set(g)) < 4 for g in groups)              # and twice inside one list
        assert all(np.array_equal(items[b], items[b + 10]) for b in range(10))
        d = [np.diff(ids[off[l]:off[l + 1]]) for l in range(4)]
        assert all(((x < 0) if descending else (x > 0)).all() for x in d)


def test_ties_by_stored_position_is_caught():
    """Descending ids inside a list: the stored order and the id order disagree, so breaking a
    tie by position gives another result than the contract's id rule."""
    items, off, ids, vec = V.duplicate_vector_index(descending=True)
    q = R.exact_vectors(18, 5, 4)
    probes = V.all_probes(5, 4, seed=2)
    good = V.ivf_topk_ref(q, probes, off, ids, vec, 10)
    bad = V.ivf_topk_ref(q, probes, off, ids, vec, 10, by_position=True)
    assert same(good, R.topk_ref(q, items, 10))
    assert not np.array_equal(good[0], bad[0])
    assert R.same_scores(good[1], bad[1])  # the same scores, other ids at the ties


def test_planted_clusters_decide_every_assignment_and_every_query():
    items, centres, queries = V.planted_clusters()
    n_lists, per = centres.shape[0], items.shape[0] // centres.shape[0]
    assert per & (per - 1) == 0 and (items * 16 == np.round(items * 16)).all()
    truth = np.repeat(np.arange(n_lists), per)
    for init in (None, centres):
        c, assign = V.kmeans_ref(items, n_lists, 3, init)
        assert np.array_equal(assign, truth)
        # the means are exact in float32: the fp32 build holds the same centroids
        assert np.array_equal(c.astype(f32).astype(np.float64), c)
        gap, bound = V.assignment_margin(items, c)
        assert gap > 2 * bound, (gap, bound)
    # the default init picks one row of every cluster
    assert np.array_equal(truth[(np.arange(n_lists) * items.shape[0]) // n_lists], np.arange(n_lists))
    # recall at nprobe = 1: the exact top-k lies inside the first probed list
    off, ids, vec = V.index_from_assignment(items, assign, n_lists)
    first = R.topk_ref(queries, c.astype(f32), 1)[0]
    assert np.array_equal(first[:, 0], np.arange(queries.shape[0]) % n_lists)
    exact = R.topk_ref(queries, items, 10)
    assert (assign[exact[0]] == first).all()
    assert same(V.ivf_topk_ref(queries, first, off, ids, vec, 10), exact)


def test_kmeans_ref_keeps_the_centroid_of_an_empty_list():
    items, centres, _ = V.planted_clusters()
    far = np.vstack([centres[:7], np.full((1, 16), 100, f32)])  # nobody is nearest to row 7
    c, assign = V.kmeans_ref(items, 8, 2, far)
    assert (assign != 7).all() and np.array_equal(c[7], far[7].astype(np.float64))


def test_scanned_fraction():
    assert V.scanned_fraction(np.array([[0], [1], [-1]]), [0, 2, 10], 10) == (2 + 8 + 0) / 3 / 10
