"""rs_group_auc's contract (include/recsys_hip.h) restated in NumPy, and the inputs its tests
share. Two independent statements of the counts:

  counts_brute   straight from the definition: per group, every (positive, negative) pair
                 compared as floats (NaN above everything, NaNs tied), O(n²);
  counts_fast    the float → uint32 key, one lexsort and cumulative negative counts, for large n.

gauc_exact is the weighted mean of the per-group ratios in fractions.Fraction. Every generator
returns (pred float32 [n], label float32 [n], group int array [n] or None)."""
from fractions import Fraction

import numpy as np

f32 = np.float32
WEIGHTS = ("impressions", "positives", "uniform")
# sizes at which the kernels change path: the per-run block and its waves, the sort's 512- and
# 1024-key tiles (the latter from n = 2^17 on), the scan's 4096-element tile
SORT_TILE_TINY, SORT_TILE_SMALL, SORT_SMALL_FROM = 512, 1024, 1 << 17
SCAN_TILE, WAVE, RUN_BLOCK = 4096, 64, 1024
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
KEYS_I64 = [INT64_MIN, INT64_MAX, -1, 0, 1 << 32, (1 << 32) + 1, (1 << 63) - (1 << 32)]
SPECIAL_PREDS = np.array([-1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, -np.inf], f32)


def pred_key(pred):
    """The order-preserving uint32 of a float32: -0 → +0, negatives bit-flipped, the others with
    the top bit set, NaN → 0xFFFFFFFF."""
    b = np.ascontiguousarray(pred, f32).view(np.uint32).copy()
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    b[b == 0x80000000] = 0
    k = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0xFFFFFFFF
    return k


def _groups(group, n):
    return np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64)


def counts_brute(pred, label, group=None):
    """(keys int64, n int32, pos int32, w2 int64), groups in ascending signed key order."""
    pred, label = np.asarray(pred, f32), np.asarray(label, f32)
    g = _groups(group, pred.size)
    keys = np.unique(g)
    n, pos, w2 = [], [], []
    for k in keys:
        m = g == k
        p, y = pred[m], label[m] != 0
        a, b = p[y][:, None], p[~y][None, :]
        an, bn = np.isnan(a), np.isnan(b)
        with np.errstate(invalid="ignore"):
            gt = ((a > b) & ~an & ~bn) | (an & ~bn)
            eq = ((a == b) & ~an & ~bn) | (an & bn)
        n.append(int(m.sum()))
        pos.append(int(y.sum()))
        w2.append(2 * int(gt.sum()) + int(eq.sum()))
    return keys.astype(np.int64), np.array(n, np.int32), np.array(pos, np.int32), np.array(w2, np.int64)


def counts_fast(pred, label, group=None):
    pred, label = np.asarray(pred, f32), np.asarray(label, f32)
    n = pred.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    g, k = _groups(group, n), pred_key(pred)
    order = np.lexsort((k, g))
    g, k, neg = g[order], k[order], (label[order] == 0).astype(np.int64)
    negcum = np.concatenate([[0], np.cumsum(neg)])
    ghead = np.concatenate([[True], g[1:] != g[:-1]])
    rhead = ghead | np.concatenate([[True], k[1:] != k[:-1]])
    gs = np.flatnonzero(ghead)
    rs = np.flatnonzero(rhead)
    re = np.concatenate([rs[1:], [n]])
    g_of_run = np.cumsum(ghead)[rs] - 1
    neg_before = negcum[rs] - negcum[gs[g_of_run]]
    neg_in = negcum[re] - negcum[rs]
    pos_in = (re - rs) - neg_in
    w2 = np.zeros(gs.size, np.int64)
    np.add.at(w2, g_of_run, pos_in * (2 * neg_before + neg_in))
    ge = np.concatenate([gs[1:], [n]])
    cnt = ge - gs
    pos = cnt - (negcum[ge] - negcum[gs])
    return g[gs].astype(np.int64), cnt.astype(np.int32), pos.astype(np.int32), w2


def gauc_exact(keys, n, pos, w2, weight="impressions"):
    """Σ w_u·AUC_u / Σ w_u over the groups with 0 < pos < n, as a Fraction (0 when none)."""
    assert weight in WEIGHTS
    num, den = Fraction(0), 0
    for nu, pu, wu in zip(map(int, n), map(int, pos), map(int, w2)):
        if 0 < pu < nu:
            w = nu if weight == "impressions" else pu if weight == "positives" else 1
            num += Fraction(w * wu, 2 * pu * (nu - pu))
            den += w
    return num / den if den else Fraction(0)


# ---- case generators -------------------------------------------------------------------------
def random_case(rng, n, n_groups, dtype=np.int64, levels=None, p_pos=0.4):
    """n examples over <= n_groups random keys; levels: predictions drawn from that many distinct
    values (ties), None: continuous."""
    pred = (rng.random(n) if levels is None else rng.integers(0, levels, n) / max(levels, 1)).astype(f32)
    label = (rng.random(n) < p_pos).astype(f32)
    lo, hi = (INT32_MIN, INT32_MAX) if dtype == np.int32 else (INT64_MIN, INT64_MAX)
    keys = rng.integers(lo, hi, n_groups, dtype=dtype, endpoint=True)
    return pred, label, keys[rng.integers(0, n_groups, n)]


def own_group_case(rng, n, dtype=np.int32):
    """Every example its own group."""
    pred, label, _ = random_case(rng, n, 1)
    return pred, label, rng.permutation(n).astype(dtype) - n // 2


def split_case(rng, n, split, dtype=np.int32, keys=(-7, 9)):
    """Two groups: the one with the smaller key holds exactly `split` examples, so in sorted order
    the second group starts at position `split`."""
    pred, label, _ = random_case(rng, n, 1, levels=37)
    group = np.full(n, keys[1], dtype)
    group[rng.permutation(n)[:split]] = keys[0]
    return pred, label, group


def lone_between_case(rng, big, dtype=np.int64):
    """A group of one between two groups of `big`."""
    n = 2 * big + 1
    pred, label, _ = random_case(rng, n, 1, levels=50)
    group = np.concatenate([np.full(big, -5), [0], np.full(big, 5)]).astype(dtype)
    perm = rng.permutation(n)
    return pred[perm], label[perm], group[perm]


def one_label_groups_case(rng, n):
    """Group 0 all positive, group 1 all negative, group 2 mixed."""
    pred, label, _ = random_case(rng, n, 1)
    group = rng.integers(0, 3, n).astype(np.int32)
    label = np.where(group == 0, 1.0, np.where(group == 1, 0.0, label)).astype(f32)
    return pred, label, group


def zipf_case(rng, n, n_groups, a=1.3, dtype=np.int64):
    """n examples over n_groups users with Zipf(a) membership (a few users own most of them)."""
    w = 1.0 / np.arange(1, n_groups + 1) ** a
    users = rng.choice(n_groups, n, p=w / w.sum())
    keys = rng.permutation(n_groups).astype(dtype) * 7919 - 3 * n_groups
    pred, label, _ = random_case(rng, n, 1, levels=4096)
    return pred, label, keys[users]


def all_equal_case(rng, n, n_groups):
    """Every prediction equal: one tie run per group, w2 = pos·neg."""
    _, label, group = random_case(rng, n, n_groups, np.int32)
    return np.full(n, 0.25, f32), label, group


def tie_run_case(rng, n, at, half=6):
    """One group of n distinct predictions except one tie run covering sorted positions
    [at - half, at + half): it crosses position `at`."""
    assert half <= at and at + half <= n
    vals = np.arange(n, dtype=np.float64)
    vals[at - half:at + half] = vals[at - half]
    perm = rng.permutation(n)
    return (vals / n).astype(f32)[perm], (rng.random(n) < 0.5).astype(f32), None


def tie_run_span(pred, group=None):
    """[(start, end)] of the tie runs longer than one, as sorted positions."""
    g, k = _groups(group, len(pred)), pred_key(pred)
    order = np.lexsort((k, g))
    g, k = g[order], k[order]
    head = np.concatenate([[True], (g[1:] != g[:-1]) | (k[1:] != k[:-1])])
    s = np.flatnonzero(head)
    e = np.concatenate([s[1:], [len(pred)]])
    return [(int(a), int(b)) for a, b in zip(s, e) if b - a > 1]


def run_groups_case(rng, run_counts, dtype=np.int32):
    """Groups with run_counts[i] tie runs each (every run of one or two examples), in key order:
    with one thread per run, group i covers run indices [Σ_{<i}, Σ_{<=i})."""
    pred, label, group = [], [], []
    for i, r in enumerate(run_counts):
        size = rng.integers(1, 3, r)
        pred.append(np.repeat(rng.permutation(r), size) / f32(max(r, 1)))
        label.append(rng.random(size.sum()) < 0.5)
        group.append(np.full(size.sum(), 10 * i - 20))
    pred, label, group = (np.concatenate(x) for x in (pred, label, group))
    perm = rng.permutation(pred.size)
    return pred[perm].astype(f32), label[perm].astype(f32), group[perm].astype(dtype)


def run_index_ranges(pred, group):
    """[(first run index, one past the last)] per group in key order."""
    g, k = _groups(group, len(pred)), pred_key(pred)
    order = np.lexsort((k, g))
    g, k = g[order], k[order]
    ghead = np.concatenate([[True], g[1:] != g[:-1]])
    rhead = ghead | np.concatenate([[True], k[1:] != k[:-1]])
    ridx = np.cumsum(rhead) - 1
    first = ridx[np.flatnonzero(ghead)]
    return list(zip(first.tolist(), np.concatenate([first[1:], [ridx[-1] + 1]]).tolist()))


def interleaved_case(n):
    """One group, ascending predictions, labels 0, 1, 0, 1, …"""
    return (np.arange(n) / f32(n)).astype(f32), (np.arange(n) % 2).astype(f32), None


def special_values_case(rng, reps=6):
    """-1, -0.0, +0.0, 1e-45, 1, ±inf, each with both labels several times, two groups."""
    pred = np.tile(SPECIAL_PREDS, 2 * reps)
    label = np.repeat([0.0, 1.0], SPECIAL_PREDS.size * reps).astype(f32)
    group = rng.integers(0, 2, pred.size).astype(np.int32)
    perm = rng.permutation(pred.size)
    return pred[perm], label[perm], group[perm]


def signed_preds_case(rng, n):
    """Predictions of both signs: mapped keys with the top bit clear (negative) and set."""
    pred = rng.standard_normal(n).astype(f32)
    return pred, (rng.random(n) < 0.5).astype(f32), rng.integers(-3, 3, n).astype(np.int32)


def nan_case(rng, n, n_nan):
    pred, label, group = random_case(rng, n, 5, np.int32, levels=20)
    pred[rng.permutation(n)[:n_nan]] = np.nan
    if n_nan > 1:  # a NaN with another payload and sign: still the same tie
        pred[np.flatnonzero(np.isnan(pred))[0]] = np.array([0xFFC00001], np.uint32).view(f32)[0]
    pred[np.flatnonzero(~np.isnan(pred))[0]] = np.inf
    return pred, label, group


def separated_case(n, tied=False):
    """One group, half positives, every positive above every negative: w2 = 2·(n/2)² (tied: all
    predictions equal, w2 = (n/2)²). Sorted against the labels: positives first, descending."""
    h = n // 2
    label = np.concatenate([np.ones(h), np.zeros(n - h)]).astype(f32)
    pred = np.full(n, 0.5, f32) if tied else (np.arange(n, 0, -1) / f32(n)).astype(f32)
    return pred, label, None


def odd_labels_case(rng, n):
    """Labels 2.0, -1.0 (positive) and -0.0, 0.0 (negative)."""
    pred, _, group = random_case(rng, n, 4, np.int32, levels=30)
    return pred, rng.choice(np.array([2.0, -1.0, -0.0, 0.0], f32), n), group


def keys_case(rng, keys, per_key, dtype):
    """per_key examples for each of the given keys, shuffled."""
    n = len(keys) * per_key
    pred, label, _ = random_case(rng, n, 1, levels=17)
    group = np.repeat(np.array(keys, dtype), per_key)
    return pred, label, group[rng.permutation(n)]


def small_cases(rng):
    """{name: case} of every family at brute-force size."""
    c = {f"random_n{n}": random_case(rng, n, max(n // 7, 1)) for n in (1, 2, 63, 64, 65, 700)}
    c["random_i32_ties"] = random_case(rng, 900, 11, np.int32, levels=9)
    c["own_group"] = own_group_case(rng, 300)
    c["one_group_none"] = random_case(rng, 500, 1, levels=40)[:2] + (None,)
    c["one_group_const"] = random_case(rng, 500, 1, levels=40)[:2] + (np.full(500, -3, np.int64),)
    c["split_wave"] = split_case(rng, 200, WAVE)
    c["split_tile"] = split_case(rng, 1300, SORT_TILE_TINY)
    c["lone_between"] = lone_between_case(rng, 300)
    c["one_label_groups"] = one_label_groups_case(rng, 400)
    c["zipf"] = zipf_case(rng, 3000, 200)
    c["all_equal"] = all_equal_case(rng, 600, 7)
    c["tie_run_64"] = tie_run_case(rng, 200, WAVE)
    c["tie_run_1024"] = tie_run_case(rng, 1100, RUN_BLOCK)
    c["run_groups"] = run_groups_case(rng, [40, 100, 1200, 3])
    c["interleaved"] = interleaved_case(501)
    c["special_values"] = special_values_case(rng)
    c["signed_preds"] = signed_preds_case(rng, 800)
    c["one_nan"] = nan_case(rng, 300, 1)
    c["many_nans"] = nan_case(rng, 300, 90)
    c["separated"] = separated_case(400)
    c["separated_tied"] = separated_case(400, tied=True)
    c["odd_labels"] = odd_labels_case(rng, 500)
    c["keys_i32_extremes"] = keys_case(rng, [INT32_MIN, INT32_MAX, -1, 0, 1], 40, np.int32)
    c["keys_i64_words"] = keys_case(rng, KEYS_I64, 40, np.int64)
    return c
