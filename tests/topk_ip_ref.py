"""NumPy restatement of rs_topk_ip's contract (include/recsys_hip.h, "Top-k inner-product
retrieval") and the builders of every input tests/test_topk_ip_gpu.py uses; the properties those
tests rely on are asserted without a GPU in tests/test_topk_ip_cpu.py.

fmaf32      the correctly rounded float32 fma, exactly: the product of two float32 is exact in
            float64 (24 + 24 bits), TwoSum gives the float64 sum and its error, an inexact sum is
            turned into its round-to-odd neighbour, and the cast to float32 then rounds once
            (53 >= 24 + 2 bits: round-to-odd makes the double rounding innocuous).
scores_ref  acc = +0; acc = fmaf32(q[d], x[d], acc) for d ascending, vectorised over (query, item).
topk_ref    exclusion, NaN -> -inf for ranking, stable sort by (-score, item), padding (-1, -inf).
"""
import numpy as np

f32 = np.float32
TILE = 32           # queries per block, items per wave tile
ROUND = 128         # items one block scores between two compaction checks
K_MAX = 64
DIMS = (1, 2, 3, 4, 16, 18, 36, 128, 160, 255, 256)
PAD_ITEM = -1


# ---- arithmetic --------------------------------------------------------------------------
def fmaf32(a, b, c):
    """round_to_nearest_even_f32(a * b + c) with a single rounding; float32 arrays (broadcast)."""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                      # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
        s, err = np.broadcast_arrays(s, err)
        s = s.copy()
        inexact = np.isfinite(s) & (err != 0)
        # round to odd: truncate toward zero (one ulp back when s overshot in magnitude: the error
        # points toward zero), then set the low mantissa bit
        overshoot = inexact & ((err < 0) == (s > 0))
        bits = s.view(np.uint64)
        bits[overshoot] -= np.uint64(1)
        bits[inexact] |= np.uint64(1)
        return s.astype(f32)


def scores_ref(queries, items):
    """[n_queries, n_items] float32: the ascending-d fmaf chain from +0."""
    q, x = np.asarray(queries, f32), np.asarray(items, f32)
    acc = np.zeros((q.shape[0], x.shape[0]), f32)
    for d in range(q.shape[1]):
        acc = fmaf32(q[:, d:d + 1], x[None, :, d], acc)
    return acc


def scores_f64(queries, items):
    return np.asarray(queries, np.float64) @ np.asarray(items, np.float64).T


def gamma(dim):
    """The standard bound of a length-dim fp32 chain: |s - exact| <= gamma * sum |q_d x_d|."""
    u = dim * 2.0 ** -24
    return u / (1 - u)


def candidate_mask(n_queries, n_items, excl=None, excl_base=0, excl_one=None):
    ok = np.ones((n_queries, n_items), bool)
    for r in range(n_queries):
        if excl is not None:
            indptr, idx = excl
            row = np.asarray(idx[indptr[excl_base + r]:indptr[excl_base + r + 1]], np.int64)
            ok[r, row[(row >= 0) & (row < n_items)]] = False
        if excl_one is not None and 0 <= excl_one[r] < n_items:
            ok[r, excl_one[r]] = False
    return ok


def topk_from_scores(scores, k, excl=None, excl_base=0, excl_one=None):
    """(items int32 [n, k], scores float32 [n, k]) of a score matrix under the contract's order."""
    scores = np.asarray(scores, f32)
    n, n_items = scores.shape
    ok = candidate_mask(n, n_items, excl, excl_base, excl_one)
    out_i = np.full((n, k), PAD_ITEM, np.int32)
    out_s = np.full((n, k), -np.inf, f32)
    for r in range(n):
        cand = np.flatnonzero(ok[r])
        s = scores[r, cand]
        rank = np.where(np.isnan(s), f32(-np.inf), s)
        order = np.lexsort((cand, -rank))[:k]  # by -rank, then item; -0 == +0
        out_i[r, :order.size] = cand[order]
        out_s[r, :order.size] = s[order]
    return out_i, out_s


def topk_ref(queries, items, k, excl=None, excl_base=0, excl_one=None):
    return topk_from_scores(scores_ref(queries, items), k, excl, excl_base, excl_one)


def same_scores(a, b):
    """Bit equality, any NaN matching any NaN (the payload of a generated NaN is not specified)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(
        ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def csr(rows):
    """(indptr int64, indices int32) of a list of id lists."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = [i for r in rows for i in r]
    return indptr, np.asarray(flat, np.int32).reshape(-1)


# ---- input builders ----------------------------------------------------------------------
def exact_vectors(seed, n, dim):
    """Multiples of 2^-4 in [-2, 2): every partial sum of a dot product of up to 256 of them is a
    multiple of 2^-8 below 2^10, exact in float32 in any order; ties are plentiful."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 32, (n, dim)) / 16.0).astype(f32)


def random_floats(seed, n, dim, extremes=True):
    """Standard normal rows; with extremes, row 1 (mod 11) is scaled into the subnormals and row 5
    (mod 13) to 1e30."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(f32)
    if extremes:
        x[1::11] *= f32(1e-39)
        x[5::13] *= f32(1e30)
    return x


def ramp_catalogue(n_items, dim, descending=False):
    """(query [1, dim], items): item i scores exactly i (or -i): strictly monotone in the id. The
    other columns hold exact noise that the query's zeros cancel."""
    items = exact_vectors(7, n_items, dim)
    items[:, 0] = np.arange(n_items, dtype=f32) * (-1 if descending else 1)
    q = np.zeros((1, dim), f32)
    q[0, 0] = 1
    return q, items


def tie_catalogue(n_items, k, tie_ids, dim=4):
    """(queries [2, dim], items): score 2 for the first k - len(tie_ids) // 2 ids outside the tie
    that are congruent 3 mod 5, score 1 for tie_ids, 0 elsewhere: the k-th place falls inside the tie."""
    items = np.zeros((n_items, dim), f32)
    tie = set(int(t) for t in tie_ids)
    high = [i for i in range(n_items) if i % 5 == 3 and i not in tie][:k - len(tie) // 2]
    items[high, 1] = 2
    items[sorted(tie), 1] = 1
    q = np.zeros((2, dim), f32)
    q[:, 1] = 1
    return q, items


def special_catalogue(dim=4):
    """(queries [3, dim], items [40, dim]): +inf and -inf scores, a NaN item row (12), a NaN query
    row (2); query 1 sees the infinities negated."""
    items = exact_vectors(11, 40, dim)
    items[3, 0] = items[20, 0] = np.inf
    items[7, 0] = items[33, 0] = -np.inf
    items[12, :] = np.nan
    q = np.zeros((3, dim), f32)
    q[0, 0], q[0, 1] = 1, 0.5
    q[1, 0], q[1, 1] = -1, 0.25
    q[2, :] = np.nan
    return q, items


TIE_N, TIE_K, TIE_IDS = 3000, 10, tuple(range(1498, 1506))  # n_splits = 2 cuts at item 1500


def exclusion_rows(top, n_items, k):
    """Five exclusion rows for a query whose unexcluded best k are `top`: nothing; every item;
    exactly the best k; unsorted with duplicates and out-of-range ids around top[0] and top[2];
    all but k - 1 items (k is larger than the remaining candidates by one)."""
    top = [int(t) for t in top[:k]]
    messy = [top[2], n_items + 5, top[0], -3, top[2], 2 ** 31 - 1, top[0], n_items]
    kept = set(list(range(n_items))[::max(n_items // (k - 1), 1)][:k - 1])
    return [[], list(range(n_items)), top, messy, [i for i in range(n_items) if i not in kept]]


def recommend_graph(seed, n_users=300, n_items=500, per_user=6):
    """(users, items, timestamps) int64 edge arrays: per_user distinct items per user, distinct
    timestamps per user (the latest item is unambiguous)."""
    rng = np.random.default_rng(seed)
    users = np.repeat(np.arange(n_users), per_user)
    items = np.concatenate([rng.choice(n_items, per_user, replace=False) for _ in range(n_users)])
    ts = np.concatenate([rng.permutation(per_user) for _ in range(n_users)])
    return users.astype(np.int64), items.astype(np.int64), ts.astype(np.int64)


RECOMMEND_SEED = 3      # random-reprs seed of the recommend(fused=True) comparison
RECOMMEND_K = 10
RECOMMEND_DIM = 16


def recommend_inputs(seed=RECOMMEND_SEED, n_users=300, n_items=500):
    """The graph, the random item representations and the latest item of each user."""
    users, items, ts = recommend_graph(seed, n_users, n_items)
    reprs = random_floats(seed + 100, n_items, RECOMMEND_DIM, extremes=False)
    latest = np.empty(n_users, np.int64)
    for u in range(n_users):
        e = np.flatnonzero(users == u)
        latest[u] = items[e[np.argmax(ts[e])]]
    return users, items, ts, reprs, latest


def decided_users(reprs, latest, users, items, k):
    """(set_decided, order_decided) bool [n_users]. Any fp32 evaluation of a score, in any order,
    lies within b = gamma_D * sum|q_d x_d| of the float64 score, so two of them can rank a pair
    differently only if its float64 gap is <= 2b. set_decided: the k-th and (k+1)-th float64
    scores (after exclusion) are further apart than that, so both paths pick the same set;
    order_decided: so is every adjacent pair of the best k + 1, so the order agrees too."""
    q = reprs[latest].astype(np.float64)
    s = q @ reprs.astype(np.float64).T
    mag = np.abs(q) @ np.abs(reprs.astype(np.float64)).T
    s[users, items] = -np.inf
    part = -np.sort(-s, axis=1)[:, :k + 1]
    gaps = part[:, :-1] - part[:, 1:]
    bound = 2 * gamma(reprs.shape[1]) * mag.max(axis=1)
    return gaps[:, k - 1] > bound, gaps.min(axis=1) > bound
