"""Top-k inner-product retrieval without a GPU: the exact float32 fma of tests/topk_ip_ref.py
against rational arithmetic, topk_ref against a brute-force loop, the header-derived binding, and
proofs that the inputs of tests/test_topk_ip_gpu.py have the properties those tests rely on."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import topk_ip_ref as R

f32 = np.float32


# ---- fmaf32 ------------------------------------------------------------------------------
def round_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational x, ties to even, from first principles."""
    if x == 0:
        return f32(0)
    with np.errstate(over="ignore"):
        g = f32(float(x))  # within an ulp: pick the best of it and its neighbours
    if not np.isfinite(g):
        g = f32(np.finfo(f32).max) * (1 if x > 0 else -1)
    cands = {g, np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(-np.inf))}
    cands = [c for c in cands if np.isfinite(c)]
    best = min(abs(Fraction(float(c)) - x) for c in cands)
    win = [c for c in cands if abs(Fraction(float(c)) - x) == best]
    if len(win) > 1:
        win = [c for c in win if (c.view(np.uint32) & 1) == 0]
    top = Fraction(float(np.finfo(f32).max)) + Fraction(2) ** 103  # past it rounds to inf
    if abs(x) >= top:
        return f32(np.inf) if x > 0 else f32(-np.inf)
    return win[0]


def fma_exact(a, b, c):
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:  # an exact zero: IEEE's sign rule, which float64 follows (nothing rounds here)
        return f32(np.float64(a) * np.float64(b) + np.float64(c))
    return round_f32(x)


def midpoint_triples():
    """a*b + c whose float64 sum lands exactly on a float32 midpoint while the exact value does
    not: a*b = ±2^-24 (1 - 2^-46) against c = ±(1 + 2^-23), scaled by powers of two."""
    out = []
    for e in (-20, -3, 0, 5, 40):
        for sa in (1, -1):
            for sc in (1, -1):
                a = f32(sa * 2.0 ** (e - 24) * (1 + 2.0 ** -23))
                b = f32(1 - 2.0 ** -23)
                c = f32(sc * 2.0 ** e * (1 + 2.0 ** -23))
                out.append((a, b, c))
    return out


def test_fmaf32_matches_rational_arithmetic_on_random_triples():
    rng = np.random.default_rng(0)
    n = 3000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(f32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-18, 18, n)).astype(f32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(f32)
    # a third cancels almost completely, a tenth meets the subnormals
    c[::3] = -(a[::3].astype(np.float64) * b[::3]).astype(f32)
    a[::10] *= f32(1e-30)
    b[::10] *= f32(1e-12)
    c[::10] *= f32(1e-38)
    got = R.fmaf32(a, b, c)
    ref = np.array([fma_exact(*t) for t in zip(a, b, c)], f32)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (np.abs(got[np.isfinite(got)]) < 1.2e-38).sum() > 20  # subnormal results were met


def test_fmaf32_on_float32_midpoints_where_double_rounding_fails():
    naive_wrong = 0
    for a, b, c in midpoint_triples():
        ref = fma_exact(a, b, c)
        got = R.fmaf32(a, b, c)
        assert got.view(np.uint32) == ref.view(np.uint32), (a, b, c)
        naive = f32(np.float64(a) * np.float64(b) + np.float64(c))
        naive_wrong += naive.view(np.uint32) != ref.view(np.uint32)
    assert naive_wrong >= 1


def test_fmaf32_specials():
    inf, nan = f32(np.inf), f32(np.nan)
    assert R.fmaf32(inf, f32(1), f32(1)) == inf
    assert np.isnan(R.fmaf32(inf, f32(0), f32(1)))
    assert np.isnan(R.fmaf32(inf, f32(1), -inf))
    assert np.isnan(R.fmaf32(nan, f32(1), f32(1)))
    assert R.fmaf32(f32(3e38), f32(2), f32(0)) == inf
    z = R.fmaf32(f32(0), f32(0), f32(0))
    assert z == 0 and not np.signbit(z)
    assert not np.signbit(R.fmaf32(f32(-1), f32(0), f32(0)))  # -0 + +0 = +0


# ---- the exact-arithmetic inputs ---------------------------------------------------------
@pytest.mark.parametrize("dim", R.DIMS)
def test_exact_vectors_make_every_order_agree(dim):
    q, x = R.exact_vectors(1, 9, dim), R.exact_vectors(2, 70, dim)
    for v in (q, x):
        assert (v * 16 == np.round(v * 16)).all() and v.min() >= -2 and v.max() < 2
    fwd = R.scores_ref(q, x)
    rev = R.scores_ref(q[:, ::-1], x[:, ::-1])
    f64 = R.scores_f64(q, x)
    np.testing.assert_array_equal(fwd.view(np.uint32), rev.view(np.uint32))
    np.testing.assert_array_equal(fwd.astype(np.float64), f64)
    assert not np.signbit(fwd[fwd == 0]).any()
    if dim == 1:  # 64 distinct item values: ties among 70 items are certain
        assert all(np.unique(row).size < row.size for row in fwd)


def test_exact_catalogue_of_3000_has_ties_inside_the_best_64():
    """The shared catalogue of the GPU tests (seeds 61 / 62): float64 is exact on it."""
    s = R.scores_f64(R.exact_vectors(61, 33, 16), R.exact_vectors(62, 3000, 16))
    best = -np.sort(-s, axis=1)[:, :65]
    tied_rows = (np.diff(best, axis=1) == 0).any(axis=1)
    assert tied_rows.sum() >= 16                       # most queries rank a tie by item id
    assert (best[:, 9] == best[:, 10]).any() or (best[:, 63] == best[:, 64]).any()


def test_random_floats_are_order_sensitive_and_cover_the_extremes():
    q, x = R.random_floats(3, 5, 36), R.random_floats(4, 60, 36)
    fwd = R.scores_ref(q, x)
    rev = R.scores_ref(q[:, ::-1], x[:, ::-1])
    assert (fwd.view(np.uint32) != rev.view(np.uint32)).any()  # the chain order is observable
    assert (np.abs(x[1]) < 1.2e-38).all() and (np.abs(x[1]) > 0).any()  # subnormal row
    assert np.abs(x[5]).max() > 1e29
    finite = np.isfinite(fwd) & np.isfinite(R.scores_f64(q, x))
    mag = np.abs(q.astype(np.float64)) @ np.abs(x.astype(np.float64)).T
    err = np.abs(fwd.astype(np.float64) - R.scores_f64(q, x))
    assert (err[finite] <= R.gamma(36) * mag[finite] + 1e-45).all()  # the derived bound holds
    # a negative product that underflows leaves -0: a chain from +0 CAN end at -0, and the GPU
    # test at dim 1 (these seeds) meets it; an odd dim's zero padding must keep that sign
    s1 = R.scores_ref(R.random_floats(21, 33, 1), R.random_floats(41, 64, 1))
    assert np.signbit(s1[s1 == 0]).any()


# ---- topk_ref ----------------------------------------------------------------------------
def brute_topk(scores, k, excluded):
    out = []
    for r, row in enumerate(scores):
        cand = [(-(float("-inf") if np.isnan(s) else float(s)), i) for i, s in enumerate(row)
                if i not in excluded[r]]
        cand.sort()
        ids = [i for _, i in cand[:k]]
        out.append(ids + [-1] * (k - len(ids)))
    return np.array(out, np.int32)


def test_topk_ref_against_a_brute_force_loop():
    nan, inf = np.nan, np.inf
    scores = np.array([[1, 3, 3, 2, 3, 0],          # ties by item
                       [5, 4, 3, 2, 1, 0],          # everything excluded
                       [0, -0.0, nan, -inf, 1, nan],  # NaN ranks as -inf; -0 ties with +0
                       [2, 2, 2, 2, 2, 2]], f32)     # k > candidates
    excl_rows = [[], [5, 4, 3, 2, 1, 0, 0, 9, -1], [4], [0, 1, 2, 3]]
    excl = R.csr(excl_rows)
    for k in (1, 3, 6, 8):
        items, vals = R.topk_from_scores(scores, k, excl)
        np.testing.assert_array_equal(items, brute_topk(scores, k, [set(r) for r in excl_rows]))
        for r in range(4):
            for c in range(k):
                if items[r, c] < 0:
                    assert vals[r, c] == -inf
                else:
                    assert R.same_scores(vals[r, c], scores[r, items[r, c]])
    items, vals = R.topk_from_scores(scores, 6, excl)
    np.testing.assert_array_equal(items[0], [1, 2, 4, 3, 0, 5])
    np.testing.assert_array_equal(items[1], [-1] * 6)
    np.testing.assert_array_equal(items[2], [0, 1, 2, 3, 5, -1])
    assert np.isnan(vals[2, 2]) and vals[2, 3] == -inf and np.isnan(vals[2, 4])
    np.testing.assert_array_equal(items[3], [4, 5, -1, -1, -1, -1])
    # excl_base and excl_one
    items, _ = R.topk_from_scores(scores[:2], 2, excl, excl_base=2, excl_one=np.array([1, -1]))
    np.testing.assert_array_equal(items, [[2, 3], [4, 5]])


# ---- binding -----------------------------------------------------------------------------
def test_header_declares_both_entry_points():
    from recommender_amd import _lib as L
    from recommender_amd._header import read_header

    _, _, funcs = read_header(L.HEADER.read_text())
    p, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    assert funcs["rs_topk_ip_workspace_size"] == (sz, [i32, i64, i32, i32])
    assert funcs["rs_topk_ip"] == (i32, [p, i64, i32, p, i64, i64, i32, i64, p, p, p, i32, i32,
                                         p, p, p, sz, p])
    assert len(funcs["rs_topk_ip"][1]) == 18
    assert {"rs_topk_ip", "rs_topk_ip_workspace_size"} <= set(L.header_symbols())


def test_python_surface_imports():
    import inspect

    from recommender_amd import functional
    from recommender_amd.eges import retrieval
    from recommender_amd.pinsage import evaluation

    sig = inspect.signature(functional.topk_inner_product)
    assert list(sig.parameters) == ["queries", "items", "k", "exclude", "exclude_base",
                                    "exclude_one", "with_scores", "n_splits"]
    assert inspect.signature(evaluation.recommend).parameters["fused"].default is False
    assert callable(retrieval.item_hidden) and callable(retrieval.similar_items)


# ---- the GPU tests' inputs ---------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_ramp_catalogue_is_strictly_monotone(descending):
    q, x = R.ramp_catalogue(3000, 16, descending)
    s = R.scores_ref(q, x)[0]
    d = np.diff(s)
    assert (d < 0).all() if descending else (d > 0).all()
    np.testing.assert_array_equal(s, R.scores_f64(q, x)[0])


def test_tie_catalogue_straddles_the_kth_place_and_the_split_boundary():
    q, x = R.tie_catalogue(R.TIE_N, R.TIE_K, R.TIE_IDS)
    s = R.scores_ref(q, x)
    items, vals = R.topk_from_scores(s, R.TIE_K + 1)
    assert vals[0, R.TIE_K - 1] == vals[0, R.TIE_K] == 1  # the cut falls inside the tie
    assert (s[0] == 1).sum() == len(R.TIE_IDS) >= 8
    cut = R.TIE_N // 2  # where n_splits = 2 divides the items
    chosen = [i for i in items[0, :R.TIE_K] if i in R.TIE_IDS]
    left_out = [i for i in R.TIE_IDS if i not in chosen]
    assert min(chosen) < cut <= max(chosen)       # chosen tie members on both sides
    assert min(left_out) >= cut                   # the rest lose on the item id alone
    assert chosen == sorted(R.TIE_IDS)[:len(chosen)]


def test_special_catalogue_has_the_stated_scores():
    q, x = R.special_catalogue()
    s = R.scores_ref(q, x)
    assert s[0, 3] == s[0, 20] == np.inf and s[0, 7] == s[0, 33] == -np.inf
    assert s[1, 3] == s[1, 20] == -np.inf and s[1, 7] == s[1, 33] == np.inf
    assert np.isnan(s[:, 12]).all() and np.isnan(s[2]).all()
    assert np.isnan(s[0]).sum() == 1 and np.isfinite(s[0]).sum() == 35
    items, vals = R.topk_from_scores(s, 40)
    np.testing.assert_array_equal(items[0, :2], [3, 20])
    np.testing.assert_array_equal(items[0, -3:], [7, 12, 33])  # NaN ties with -inf, by item
    np.testing.assert_array_equal(items[2], np.arange(40))


def test_exclusion_rows_leave_the_stated_candidates():
    n_items, k = 100, 10
    q, x = R.exact_vectors(5, 1, 18), R.exact_vectors(6, n_items, 18)
    s = R.scores_ref(q, x)
    top, _ = R.topk_from_scores(s, k)
    rows = R.exclusion_rows(top[0], n_items, k)
    left = [R.candidate_mask(1, n_items, R.csr([row]))[0].sum() for row in rows]
    assert left == [n_items, 0, n_items - k, n_items - 2, k - 1]
    assert rows[3] != sorted(rows[3]) and len(set(rows[3])) < len(rows[3])
    assert any(i < 0 for i in rows[3]) and any(i >= n_items for i in rows[3])
    got, _ = R.topk_from_scores(s, k, R.csr([rows[2]]))
    assert not set(got[0]) & set(top[0])
    got, _ = R.topk_from_scores(s, k, R.csr([rows[4]]))
    assert (got[0, :k - 1] >= 0).all() and got[0, k - 1] == -1


def test_recommend_seed_leaves_under_one_percent_undecided():
    users, items, ts, reprs, latest = R.recommend_inputs()
    assert users.max() + 1 <= 300 and reprs.shape[0] <= 500
    set_ok, order_ok = R.decided_users(reprs, latest, users, items, R.RECOMMEND_K)
    assert (~set_ok).mean() < 0.01 and (~order_ok).mean() < 0.01
    # every user has a unique latest item and fewer training items than the catalogue
    for u in (0, 17, 299):
        e = np.flatnonzero(users == u)
        assert np.unique(ts[e]).size == e.size and np.unique(items[e]).size == e.size
