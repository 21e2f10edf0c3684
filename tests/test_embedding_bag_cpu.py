"""EmbeddingBag without a GPU: the header-derived binding and the imports, hand-worked cases for
the NumPy restatement (tests/embedding_bag_ref.py), and proofs that the inputs of
tests/test_embedding_bag_gpu.py have the properties those tests rely on."""
import ctypes as C

import numpy as np

from oracle import embedding as O
from tests import embedding_bag_ref as R

f32 = np.float32


# ---- binding and imports -----------------------------------------------------------------
def test_header_declares_the_three_entry_points():
    from recommender_amd import _lib as L
    from recommender_amd._header import read_header

    consts, _, funcs = read_header(L.HEADER.read_text())
    assert consts["RS_BAG_SUM"] == 0 and consts["RS_BAG_MEAN"] == 1
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert funcs["rs_embedding_bag_fwd"] == (i32, [p, i64, i32, p, i32, i64, p, i64, i32, p, p, i32,
                                                   p, i32, p, i64, p, p, p])
    assert funcs["rs_embedding_bag_remap_pos"] == (i32, [p, i64, p, i64, i32, p, p])
    assert funcs["rs_embedding_bag_expand_grad"] == (i32, [p, i64, i32, i64, p, i64, i32, p, p, p,
                                                           p])
    assert L.RS_BAG_SUM == 0 and L.RS_BAG_MEAN == 1


def test_python_surface_imports():
    import recommender_amd
    from recommender_amd import functional
    from recommender_amd.embedding import Embedding, EmbeddingBag

    assert issubclass(EmbeddingBag, Embedding)
    assert recommender_amd.EmbeddingBag is EmbeddingBag
    assert callable(functional.embedding_bag)
    assert hasattr(Embedding, "take_bag_grad")


# ---- the restatement, by hand ------------------------------------------------------------
def test_three_bags_by_hand():
    """Bags {2, 0, 2}, {}, {1}: rows are powers of two, so every sum is exact and known."""
    table = np.array([[1, 10], [2, 20], [4, 40]], f32)
    ids = np.array([2, 0, 2, 1])
    offsets = np.array([0, 3, 3, 4], np.int64)
    out, scale, count, flag = R.bag_forward(table, ids, 3, offsets)
    np.testing.assert_array_equal(out, [[9, 90], [0, 0], [2, 20]])
    np.testing.assert_array_equal(count, [3, 0, 1])
    np.testing.assert_array_equal(scale, [f32(1) / f32(3), 0, 1])
    assert not flag
    mean, *_ = R.bag_forward(table, ids, 3, offsets, mode=R.MEAN)
    np.testing.assert_array_equal(mean, np.array([[3, 30], [0, 0], [2, 20]], f32))
    assert not np.signbit(mean[1]).any()  # the empty bag is +0, not NaN
    # remap and expansion of the same layout
    np.testing.assert_array_equal(R.bag_remap([3, 0, 2, 1], 4, 3, offsets), [2, 0, 0, 0])
    dout = np.array([[3, 6], [100, 100], [5, 7]], f32)
    rows = R.bag_expand(dout, 4, 3, offsets, scale=scale)
    third = f32(1) / f32(3)
    np.testing.assert_array_equal(rows, [[third * f32(3), third * f32(6)]] * 3 + [[5, 7]])


def test_mean_with_valid_holes_and_weights():
    table = np.array([[1.0], [2.0], [4.0], [8.0]], f32)
    ids = np.array([[0, 1, 2, 3], [3, 3, 3, 3], [1, 2, 3, 0]])
    valid = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 1]], np.uint8)
    out, scale, count, _ = R.bag_forward(table, ids, 3, bag_len=4, valid=valid, mode=R.MEAN)
    np.testing.assert_array_equal(out[:, 0], [2.5, 0.0, 4.5])  # (1+4)/2, empty, (8+1)/2
    np.testing.assert_array_equal(count, [2, 0, 2])
    np.testing.assert_array_equal(scale, [0.5, 0, 0.5])
    w = np.array([[2, 9, -1, 9], [1, 1, 1, 1], [9, 9, 0, 3]], f32)
    out, *_ = R.bag_forward(table, ids, 3, bag_len=4, valid=valid, weights=w)
    np.testing.assert_array_equal(out[:, 0], [2 * 1 - 4, 0, 0 * 8 + 3 * 1])
    # the order is the position order: 1e30 then its cancelling partner, then 1 survives
    big = np.array([[1e30], [-1e30], [1.0]], f32)
    o1, *_ = R.bag_forward(big, np.array([0, 1, 2]), 1, bag_len=3)
    o2, *_ = R.bag_forward(big, np.array([0, 2, 1]), 1, bag_len=3)
    assert o1[0, 0] == 1.0 and o2[0, 0] == 0.0


def test_slab_slot_rule_and_oob_case():
    ids, offsets, so, bad = R.oob_case()
    table = np.arange(18, dtype=f32).reshape(18, 1) + 1  # row r holds r + 1
    out, scale, count, flag = R.bag_forward(table, ids, 4, offsets, slot_offsets=so)
    # bag 0 -> slot 0 rows {0, oob, 4}; bag 1 -> slot 1 rows {5+10, oob, 5+3}; bag 2 -> slot 2
    # rows {16+1, oob, 16+0}; bag 3 -> slot 0 again rows {4, 4}
    np.testing.assert_array_equal(out[:, 0], [1 + 5, 16 + 9, 18 + 17, 5 + 5])
    np.testing.assert_array_equal(count, [3, 3, 3, 2])  # an out-of-range id still counts
    assert flag
    # the OOB positions are exactly the claimed ones: -1, the slab's row count, slot 2's size
    n_slots = len(so) - 1
    found = []
    for b in range(4):
        card = so[b % n_slots + 1] - so[b % n_slots]
        found += [p for p in range(offsets[b], offsets[b + 1]) if not 0 <= ids[p] < card]
    assert found == bad
    assert [int(ids[p]) for p in bad] == [-1, int(so[-1]), int(so[3] - so[2])]
    # with the bad positions masked nothing is flagged
    valid = np.ones(ids.size, np.uint8)
    valid[bad] = 0
    assert not R.bag_forward(table, ids, 4, offsets, valid=valid, slot_offsets=so)[3]


def test_malformed_offsets_are_empty_and_flagged():
    table = np.ones((4, 2), f32)
    ids = np.array([0, 1, 2, 3])
    for offsets in ([0, 3, 2, 4], [0, 2, 9]):  # reversed; past n_ids
        offsets = np.array(offsets, np.int64)
        out, scale, count, flag = R.bag_forward(table, ids, len(offsets) - 1, offsets)
        assert flag
        assert count[1] == 0 and not out[1].any() and scale[1] == 0
        assert count[0] > 0


# ---- what the GPU tests' inputs really are ----------------------------------------------
def test_order_sensitive_input_is_order_sensitive():
    """For every width, summing the bags in reversed and in pairwise order changes bits in at
    least one bag: a kernel that reorders the additions does not pass the bit-exact test."""
    for D in R.FWD_DIMS:
        table, ids, offsets = R.order_sensitive_bags(D)
        fwd, *_ = R.bag_forward(table, ids, len(offsets) - 1, offsets)
        rev = np.stack([R.sum_reversed(table, ids, offsets[b], offsets[b + 1])
                        for b in range(len(offsets) - 1)])
        pair = np.stack([R.sum_pairwise(table, ids, offsets[b], offsets[b + 1])
                         for b in range(len(offsets) - 1)])
        assert (fwd != rev).any(axis=1).sum() >= 1, D
        assert (fwd != pair).any(axis=1).sum() >= 1, D
        lens = np.diff(offsets)
        assert lens[0] == 0 and lens[-1] == 0 and set(R.BAG_LENS) <= set(lens.tolist())


def test_shared_id_run_crosses_tile_and_group():
    c = R.backward_cases()["shared_id"]
    sr, sp, _ = O.sort_ids(c["ids"], R.V)
    run = np.flatnonzero(sr == 7)
    assert run.size == c["n_bags"] == 1100 and (np.diff(run) == 1).all()
    a, b = run[0], run[-1]
    assert a // O.DEDUP_TILE != b // O.DEDUP_TILE  # crosses RS_DEDUP_TILE boundaries
    assert a < 1024 <= b                           # and the 1024-key group boundary
    # every position of the run lies in a different bag
    assert len(set((sp[run] // 3).tolist())) == 1100


def test_backward_cases_are_what_they_claim():
    cases = R.backward_cases()
    c = cases["dup_in_bag"]
    offs, ids = c["offsets"], c["ids"]
    dup = [b for b in range(c["n_bags"]) if offs[b + 1] - offs[b] >= 2
           and ids[offs[b]] == ids[offs[b + 1] - 1]]
    assert len(dup) > 50 and 0 in np.diff(offs)
    c = cases["distinct"]
    assert np.unique(c["ids"]).size == c["ids"].size
    assert not cases["all_masked"]["valid"].any()
    assert cases["one_bag"]["n_bags"] == 1 and cases["one_bag"]["offsets"][-1] == 300


# ---- the derived bound -------------------------------------------------------------------
def test_reorder_bound_holds_for_the_reference_path():
    """The model-level comparison (pooled history against the masked mean) is judged by
    n * 2^-23 * sum|terms| per column; the restatement's own forward and two other orders stay
    inside it against the float64 sum, on the order-sensitive inputs."""
    for D in (18, 36):
        table, ids, offsets = R.order_sensitive_bags(D)
        fwd, *_ = R.bag_forward(table, ids, len(offsets) - 1, offsets)
        for b in range(len(offsets) - 1):
            s, e = offsets[b], offsets[b + 1]
            if e == s:
                continue
            terms = table[ids[s:e]]
            bound = R.reorder_bound(terms)
            exact = terms.astype(np.float64).sum(0)
            for got in (fwd[b], R.sum_reversed(table, ids, s, e), R.sum_pairwise(table, ids, s, e)):
                assert (np.abs(got.astype(np.float64) - exact) <= bound).all(), (D, b)


def test_ref_steps_match_oracle_on_expanded_gradient():
    """ref_step is the oracle's apply on the tiled segment sums of the expanded rows."""
    r = np.random.default_rng(3)
    c = R.backward_cases()["dup_in_bag"]
    n, D = c["ids"].size, 4
    dout = r.standard_normal((c["n_bags"], D)).astype(f32)
    _, scale, _, _ = R.bag_forward(np.zeros((R.V, D), f32), c["ids"], c["n_bags"], c["offsets"],
                                   valid=c["valid"], mode=R.MEAN)
    rows = R.bag_expand(dout, n, c["n_bags"], c["offsets"], scale=scale)
    w = r.standard_normal((R.V, D)).astype(f32)
    w2, _, _ = R.ref_step("sgd", (w, None, None), c["ids"], c["valid"], rows, 0.1)
    # by hand: row u moves by lr * sum over its live positions of scale[b] * dout[b]
    u = int(c["ids"][np.flatnonzero(c["valid"])[0]])
    live = [p for p in range(n) if c["ids"][p] == u and c["valid"][p]]
    want = w[u].astype(np.float64) - 0.1 * sum(rows[p].astype(np.float64) for p in live)
    np.testing.assert_allclose(w2[u], want, rtol=1e-5, atol=1e-6)
    untouched = np.setdiff1d(np.arange(R.V), c["ids"][c["valid"] != 0])
    np.testing.assert_array_equal(w2[untouched], w[untouched])
