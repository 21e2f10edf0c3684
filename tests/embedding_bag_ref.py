"""NumPy float32 restatement of the EmbeddingBag contract (include/recsys_hip.h a-1b), written
from the contract: literal loops over bags and positions, every operation an np.float32
operation in the stated order (the columns of a row go through the same operations side by side,
as array elements). Also the inputs the GPU tests use, so tests/test_embedding_bag_cpu.py can
prove what they claim about them, and the reference optimizer steps on the expanded gradient.

tests/test_embedding_bag_cpu.py checks this file; tests/test_embedding_bag_gpu.py compares the
kernels with it."""
from __future__ import annotations

import numpy as np

from oracle import embedding as O
from tests import adagrad_ref as A

f32 = np.float32
SUM, MEAN = 0, 1


def bag_range(b, n_ids, offsets, bag_len):
    """(start, end, malformed) of bag b; a reversed range or one leaving [0, n_ids] is empty."""
    if offsets is None:
        return b * bag_len, (b + 1) * bag_len, False
    s, e = int(offsets[b]), int(offsets[b + 1])
    if s < 0 or e > n_ids or s > e:
        return 0, 0, True
    return s, e, False


def bag_forward(table, ids, n_bags, offsets=None, bag_len=0, valid=None, weights=None, mode=SUM,
                slot_offsets=None):
    """(out [n_bags, D], bag_scale [n_bags], count [n_bags], flag) — flag is True where the
    kernel sets RS_ERRBIT_OOB (an out-of-range id at a live position, or a malformed bag)."""
    table = np.asarray(table, f32)
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    n_ids, D = ids.size, table.shape[1]
    if offsets is None:
        assert n_ids == n_bags * bag_len
    out = np.zeros((n_bags, D), f32)
    scale = np.zeros(n_bags, f32)
    count = np.zeros(n_bags, np.int64)
    flag = False
    n_slots = 1 if slot_offsets is None else len(slot_offsets) - 1
    for b in range(n_bags):
        s, e, bad = bag_range(b, n_ids, offsets, bag_len)
        flag |= bad
        lo, card = 0, table.shape[0]
        if slot_offsets is not None:
            sl = b % n_slots
            lo, card = int(slot_offsets[sl]), int(slot_offsets[sl + 1] - slot_offsets[sl])
        acc = np.zeros(D, f32)  # +0.f
        for p in range(s, e):
            if valid is not None and valid.reshape(-1)[p] == 0:
                continue
            count[b] += 1
            if 0 <= ids[p] < card:
                t = table[lo + ids[p]]
            else:
                t = np.zeros(D, f32)
                flag = True
            if weights is not None:
                with np.errstate(all="ignore"):
                    t = f32(np.asarray(weights, f32).reshape(-1)[p]) * t
            with np.errstate(all="ignore"):
                acc = acc + t
        if count[b] > 0:
            scale[b] = f32(1.0) / f32(count[b])
            with np.errstate(all="ignore"):
                out[b] = acc / f32(count[b]) if mode == MEAN else acc
        else:
            out[b] = f32(0.0)
    return out, scale, count, flag


def bag_of(p, n_ids, n_bags, offsets, bag_len):
    """The bag holding position p, -1 if none (bags do not overlap)."""
    if p < 0 or p >= n_ids:
        return -1
    for b in range(n_bags):
        s, e, _ = bag_range(b, n_ids, offsets, bag_len)
        if s <= p < e:
            return b
    return -1


def bag_remap(sorted_pos, n_ids, n_bags, offsets=None, bag_len=0):
    """bag_pos[i] = bag of sorted_pos[i], 0 where it lies in no bag."""
    out = np.zeros(len(sorted_pos), np.int32)
    if offsets is None:
        for i, p in enumerate(sorted_pos):
            out[i] = p // bag_len if (0 <= p < n_ids and bag_len > 0) else 0
        return out
    # one pass over the bags instead of a search per entry: the same map
    owner = np.zeros(n_ids, np.int32)
    for b in range(n_bags):
        s, e, _ = bag_range(b, n_ids, offsets, bag_len)
        owner[s:e] = b
    for i, p in enumerate(sorted_pos):
        out[i] = owner[p] if 0 <= p < n_ids else 0
    return out


def bag_expand(dout, n_ids, n_bags, offsets=None, bag_len=0, scale=None, weights=None):
    """grad_rows [n_ids, D]: scale[b] * dout[b] (one rounded multiply; dout[b] itself without
    scale), then w[p] * that with weights; zero rows outside every bag."""
    dout = np.asarray(dout, f32)
    rows = np.zeros((n_ids, dout.shape[1]), f32)
    for b in range(n_bags):
        s, e, _ = bag_range(b, n_ids, offsets, bag_len)
        for p in range(s, e):
            g = dout[b]
            if scale is not None:
                g = f32(scale[b]) * g
            if weights is not None:
                g = f32(np.asarray(weights, f32).reshape(-1)[p]) * g
            rows[p] = g
    return rows


# ---- reference optimizer steps on the expanded gradient ---------------------------------
def ref_step(kind, state, ids, valid, rows, lr, step=1, eps=1e-7):
    """One step of `kind` in {"sgd", "lazy", "adagrad"} from state (w, m, v) (m: Adam m or the
    Adagrad accumulator) with the expanded gradient `rows` of `ids` (valid: positions left out):
    the kernel's tiled segment sums (tests/adagrad_ref.segment_grads), then the oracle's apply."""
    w, m, v = state
    ur, ug = A.segment_grads(ids, rows, w.shape[0], valid=valid)
    if kind == "sgd":
        return O.apply_sgd(w, ur, ug, lr), m, v
    if kind == "lazy":
        c = O.keras_adam_coefficients(step, lr, epsilon=eps)
        return O.apply_lazy_adam(w, m, v, ur, ug, c)
    if kind == "adagrad":
        w2, a2 = A.apply_adagrad(w, m, ur, ug, lr, eps)
        return w2, a2, v
    raise ValueError(kind)


# ---- the derived bound of a differently ordered sum -------------------------------------
def reorder_bound(terms):
    """|fl(sum in any order) - exact sum| <= (n - 1) u (1 + u)^(n-1) sum|t| < n 2^-23 sum|t| for
    fp32 (u = 2^-24, n <= 2^20): so two fp32 sums of the same n terms in different orders, or one
    of them and the exact sum, differ by at most n * 2^-23 * sum|terms|. Evaluated in float64 per
    column; terms [n, D]."""
    t = np.asarray(terms, np.float64)
    return t.shape[0] * 2.0 ** -23 * np.abs(t).sum(0)


# ---- inputs of the GPU tests -------------------------------------------------------------
FWD_DIMS = [1, 2, 3, 4, 18, 36, 64, 128, 130, 260]
BAG_LENS = [0, 1, 3, 4, 5, 8, 100, 257]
N_BAGS = [1, 3, 64, 65, 257]
V = 5000


def order_sensitive_table(D, seed=11, rows=400):
    """Rows whose magnitudes span 12 decades with mixed signs: an fp32 sum of a bag of them
    depends on the order of the additions."""
    r = np.random.default_rng(seed + D)
    return (r.standard_normal((rows, D)) * 10.0 ** r.uniform(-6, 6, (rows, D))).astype(f32)


def order_sensitive_bags(D, seed=11):
    """(table, ids, offsets): CSR bags of every length in BAG_LENS (the 0 first and last)."""
    table = order_sensitive_table(D, seed)
    r = np.random.default_rng(seed)
    lens = BAG_LENS + [7, 33, 0]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = r.integers(0, table.shape[0], offsets[-1]).astype(np.int64)
    return table, ids, offsets


def sum_reversed(table, ids, s, e):
    acc = np.zeros(table.shape[1], f32)
    for p in range(e - 1, s - 1, -1):
        acc = acc + table[ids[p]]
    return acc


def sum_pairwise(table, ids, s, e):
    if e - s == 0:
        return np.zeros(table.shape[1], f32)
    if e - s == 1:
        return table[ids[s]].copy()
    mid = (s + e) // 2
    return sum_pairwise(table, ids, s, mid) + sum_pairwise(table, ids, mid, e)


def backward_cases(seed=5):
    """name -> dict(ids, offsets | None, bag_len, n_bags, valid | None): the inputs of the
    remapped-against-expanded backward test."""
    r = np.random.default_rng(seed)
    cases = {}
    # id 7 opens every bag of 3: after the sort its run of 1100 starts at key 0 and crosses the
    # 32-key tiles and the 1024-key group
    nb = 1100
    ids = r.integers(8, V, (nb, 3))
    ids[:, 0] = 7
    cases["shared_id"] = dict(ids=ids.reshape(-1), offsets=None, bag_len=3, n_bags=nb, valid=None)
    # CSR bags of 0..6 ids, every bag of >= 2 holding its first id twice
    lens = r.integers(0, 7, 300)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = r.integers(0, V, offs[-1])
    for b in range(300):
        if lens[b] >= 2:
            ids[offs[b] + lens[b] - 1] = ids[offs[b]]
    valid = (r.random(offs[-1]) < 0.8).astype(np.uint8)
    cases["dup_in_bag"] = dict(ids=ids, offsets=offs, bag_len=0, n_bags=300, valid=valid)
    lens = r.integers(1, 9, 200)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cases["distinct"] = dict(ids=r.permutation(V)[:offs[-1]], offsets=offs, bag_len=0, n_bags=200,
                             valid=None)
    cases["all_masked"] = dict(ids=r.integers(0, V, 40 * 5), offsets=None, bag_len=5, n_bags=40,
                               valid=np.zeros(200, np.uint8))
    cases["one_bag"] = dict(ids=r.integers(0, V, 300), offsets=np.array([0, 300], np.int64),
                            bag_len=0, n_bags=1, valid=None)
    for c in cases.values():
        c["ids"] = np.asarray(c["ids"], np.int64)
    return cases


def oob_case():
    """(ids, offsets, slot_offsets, expected bad positions): a 3-slot slab (cardinalities 5, 11,
    2) with 4 bags; the out-of-range ids are exactly -1 (bag 0), the slab's row count 18 (bag 1,
    whose own slot holds 11), and slot 2's cardinality 2 (bag 2). Bag 3 wraps to slot 0."""
    slot_offsets = np.array([0, 5, 16, 18], np.int64)
    ids = np.array([0, -1, 4,    10, 18, 3,    1, 2, 0,    4, 4], np.int64)
    offsets = np.array([0, 3, 6, 9, 11], np.int64)
    return ids, offsets, slot_offsets, [1, 4, 7]
