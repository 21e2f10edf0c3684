"""NumPy restatement of the int8 candidate retrieval contract (include/recsys_hip.h, "Int8
candidate retrieval with an exact re-rank") and the builders of every input
tests/test_topk_i8_gpu.py uses; the properties those tests rely on are asserted without a GPU in
tests/test_topk_i8_cpu.py.

quantize_ref  rule 1 in float32 IEEE operations: amax, amax / 127, rint(x / scale), the clamp.
int_scores    I = cq · codes in int64.
keys_ref      (float32) I * scales, one float32 product.
scan_ref      rs_topk_ip_i8: the query codes, the keys, topk_ip_ref's order and exclusions.
rerank_ref    rs_rerank_ip: topk_ip_ref's exact fmaf chain over the valid candidates, its order.
"""
from fractions import Fraction

import numpy as np

from tests import topk_ip_ref as R

f32 = np.float32
DIMS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 160, 255, 256)  # 16-byte and K = 32 chunk edges
QUANT_DIMS = (1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 129, 255, 256)


def row_bytes(dim):
    return 0 if dim <= 0 else (dim + 15) // 16 * 16


# ---- the contract ------------------------------------------------------------------------
def quantize_ref(x):
    """(codes int8 [n, dim], scales float32 [n], nonfinite bool [n]) of float32 rows."""
    x = np.asarray(x, f32)
    n, dim = x.shape
    bad = ~np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        amax = np.abs(np.where(np.isfinite(x), x, f32(0))).max(axis=1).astype(f32)
        scale = (amax / f32(127)).astype(f32)
        scale[bad] = 0
        live = scale != 0
        q = np.zeros((n, dim), f32)
        q[live] = np.rint(x[live] / scale[live, None])  # float32 division, ties to even
        q = np.minimum(np.maximum(q, f32(-127)), f32(127))
    return q.astype(np.int8), scale, bad


def int_scores(cq, codes):
    return np.asarray(cq, np.int64) @ np.asarray(codes, np.int64).T


def keys_ref(cq, codes, scales):
    """[n_queries, n_items] float32: (float) I * scales[i], one rounded product."""
    i = int_scores(cq, codes)
    assert np.abs(i).max(initial=0) <= 2 ** 22
    with np.errstate(all="ignore"):
        return i.astype(f32) * np.asarray(scales, f32)[None, :]


def scan_ref(queries, codes, scales, kc, excl=None, excl_base=0, excl_one=None):
    """(items int32 [Q, kc], keys float32 [Q, kc]) of rs_topk_ip_i8."""
    cq, _, _ = quantize_ref(queries)
    return R.topk_from_scores(keys_ref(cq, codes, scales), kc, excl, excl_base, excl_one)


def rerank_ref(queries, items, cand, k):
    """(items int32 [Q, k], scores float32 [Q, k]) of rs_rerank_ip."""
    queries, items, cand = np.asarray(queries, f32), np.asarray(items, f32), np.asarray(cand)
    n = queries.shape[0]
    out_i = np.full((n, k), -1, np.int32)
    out_s = np.full((n, k), -np.inf, f32)
    for r in range(n):
        ids = cand[r][(cand[r] >= 0) & (cand[r] < items.shape[0])].astype(np.int64)
        if not ids.size:
            continue
        s = R.scores_ref(queries[r:r + 1], items[ids])[0]
        rank = np.where(np.isnan(s), f32(-np.inf), s)
        order = np.lexsort((ids, -rank))[:k]
        out_i[r, :order.size] = ids[order]
        out_s[r, :order.size] = s[order]
    return out_i, out_s


# ---- plain-Python definitions the restatement is proved against ------------------------------
def _round_half_even(fr):
    """The integer nearest to a Fraction, ties to even."""
    fl = fr.numerator // fr.denominator
    rem = fr - fl
    return fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2) else 0)


def f32_of_fraction(fr):
    """The float32 nearest to a Fraction (ties to even, subnormals included; no overflow here),
    as a Fraction: one rounding of the exact value, which float(fr) -> float32 would do twice."""
    if fr == 0:
        return Fraction(0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    m = _round_half_even(a / quantum) * quantum
    return m if fr > 0 else -m


def quantize_row_python(row):
    """Rule 1 on one row in exact rational arithmetic: (codes, scale as a Fraction, nonfinite).
    Each IEEE operation is the exact result rounded once to float32."""
    if any(v != v or abs(v) == float("inf") for v in map(float, row)):
        return [0] * len(row), Fraction(0), True
    vals = [Fraction(float(f32(v))) for v in row]
    scale = f32_of_fraction(max(abs(v) for v in vals) / 127)
    if scale == 0:
        return [0] * len(row), Fraction(0), False
    codes = [max(-127, min(127, _round_half_even(f32_of_fraction(v / scale)))) for v in vals]
    return codes, scale, False


def order_quadratic(keys, ids):
    """The order by its definition: position = the number of pairs that are strictly better
    (key descending with NaN as -inf and -0 == +0, then id ascending)."""
    rank = [float("-inf") if k != k else float(k) for k in keys]
    pos = []
    for a in range(len(ids)):
        better = sum(1 for b in range(len(ids))
                     if rank[b] > rank[a] or (rank[b] == rank[a] and ids[b] < ids[a]))
        pos.append(better)
    return pos


# ---- input builders ----------------------------------------------------------------------
def planted_exact(seed, n, dim):
    """Integer-valued rows in [-127, 127] with amax exactly 127: scale = 1, codes = values, and
    with |score| <= 256 * 127^2 < 2^24 the fp32 chain is exact, so key == score."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-127, 128, (n, dim)).astype(f32)
    x[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-127, 127], n)
    return x


def gaussian_mixture(seed, n, dim, centres):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, dim)).astype(f32)
    return (c[rng.integers(0, centres, n)] + f32(0.5) * rng.standard_normal((n, dim))).astype(f32)


def coded_catalogue(seed, n, dim, c_ld=None, garbage=True):
    """(codes int8 [n, c_ld], scales float32 [n]) straight from a generator: any int8 value,
    -128 included; padding bytes hold garbage the scan must ignore. Scales are positive, a
    handful of distinct values so that equal keys happen."""
    rng = np.random.default_rng(seed)
    c_ld = row_bytes(dim) if c_ld is None else c_ld
    codes = rng.integers(-128, 128, (n, c_ld)).astype(np.int8)
    if not garbage:
        codes[:, dim:] = 0
    scales = rng.choice(np.asarray([0.25, 0.5, 1.0, 3.0], f32), n).astype(f32)
    return codes, scales


def small_int_queries(seed, n, dim):
    """Rows of small integers with amax 127 somewhere: their codes are the values themselves."""
    return planted_exact(seed, n, dim)


def extreme_codes(n_fill=61, dim=256):
    """(queries [4, dim], codes [3 + n_fill, dim], scales): items 0..2 are all +127, all -127 and
    all -128; queries are constant +c / -c rows (codes ±127). |I| reaches 256 * 127 * 128."""
    rng = np.random.default_rng(5)
    codes = rng.integers(-100, 101, (3 + n_fill, dim)).astype(np.int8)
    codes[0], codes[1], codes[2] = 127, -127, -128
    q = np.stack([np.full(dim, 2.5, f32), np.full(dim, -2.5, f32), np.full(dim, 1e-3, f32),
                  np.full(dim, -7.0, f32)])
    return q, codes, np.ones(len(codes), f32)


def one_hot_case(dim=256, n_items=200):
    """(queries [dim, dim] one-hot, codes [n_items, dim], scales of 1): column d holds a distinct
    code per item, so query d's keys are 127 * codes[:, d], all distinct: K position d is
    checked on its own."""
    i, d = np.arange(n_items)[:, None], np.arange(dim)[None, :]
    codes = ((i * 7 + d * 13) % 255 - 127).astype(np.int8)
    return np.eye(dim, dtype=f32), codes, np.ones(n_items, f32)


def tie_case(n_items=513, dim=32):
    """(queries [2, dim], codes, scales): every item has the same key except a few better ones, so
    the kc-th place falls inside a tie that spans tiles, rounds and split boundaries."""
    codes = np.zeros((n_items, dim), np.int8)
    codes[:, 0] = 1
    codes[[5, 130, 257, 400, 512], 0] = 2
    q = np.zeros((2, dim), f32)
    q[0, 0], q[1, 0] = 1, -1
    return q, codes, np.ones(n_items, f32)


def special_scales(n_items=70, dim=16):
    """(queries [3, dim], codes, scales): scales of 0, negative, +inf, NaN and a subnormal."""
    codes, scales = coded_catalogue(17, n_items, dim, garbage=False)
    scales[3], scales[9], scales[20], scales[33], scales[40] = 0, -2, np.inf, np.nan, 1e-42
    scales[50] = -np.inf
    return small_int_queries(18, 3, dim), codes, scales
