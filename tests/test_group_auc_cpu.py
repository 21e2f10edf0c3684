"""The NumPy statements of rs_group_auc's contract against each other (tests/group_auc_ref.py),
the key map's monotonicity, the host arithmetic of GroupAUC.result(), the case generators'
named properties, and the new names on every layer. No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import group_auc_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return R.small_cases(np.random.default_rng(11))


def test_fast_counts_equal_brute_force_on_every_small_family(cases):
    for name, (pred, label, group) in cases.items():
        fast, brute = R.counts_fast(pred, label, group), R.counts_brute(pred, label, group)
        for a, b, what in zip(fast, brute, ("keys", "n", "pos", "w2")):
            assert a.dtype == b.dtype, (name, what)
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: {what}")
        assert (np.diff(fast[0]) > 0).all(), name  # ascending signed keys


def test_key_map_is_strictly_monotone_with_the_zeros_tied():
    tiny = np.array([1e-45, 2e-45, 1.1754942e-38, 1.17549435e-38], f32)  # subnormals, min normal
    base = np.concatenate([[0.0, 1.0, 0.5, 3.4028235e38, 1e-30, 65504.0, np.inf], tiny,
                           np.random.default_rng(0).standard_normal(200)]).astype(f32)
    v = np.concatenate([base, -base])
    with np.errstate(over="ignore"):  # the neighbours of ±FLT_MAX are ±inf
        v = np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])
    v = np.unique(v[~np.isnan(v)])  # sorted by value; np.unique keeps one of ±0
    assert np.isinf(v[0]) and np.isinf(v[-1]) and (np.abs(v) < 1.2e-38).sum() > 8
    k = R.pred_key(v).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert R.pred_key(np.array([-0.0], f32))[0] == R.pred_key(np.array([0.0], f32))[0] == 0x80000000
    nans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32).view(f32)
    assert (R.pred_key(nans) == 0xFFFFFFFF).all() and k.max() < 0xFFFFFFFF
    assert k.min() < 0x80000000 <= k.max()  # keys with the top bit clear and set


def test_result_arithmetic_is_the_fraction_rounded_to_float64(cases):
    from recommender_amd.metrics import gauc_from_counts

    rng = np.random.default_rng(5)
    sets = [R.counts_fast(*cases[name]) for name in ("zipf", "random_n700", "own_group", "keys_i64_words")]
    sets.append(R.counts_fast(*R.zipf_case(rng, 40000, 3000)))
    for keys, n, pos, w2 in sets:
        for weight in R.WEIGHTS:
            exact = R.gauc_exact(keys, n, pos, w2, weight)
            got = gauc_from_counts(n, pos, w2, weight)
            assert got == float(exact), (weight, got, float(exact))
            assert 0.0 <= got <= 1.0
    assert gauc_from_counts(np.array([3]), np.array([3]), np.array([0]), "uniform") == 0.0
    assert gauc_from_counts(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)) == 0.0
    with pytest.raises(ValueError):
        gauc_from_counts(n, pos, w2, "clicks")


def test_gauc_exact_on_a_hand_case():
    # user 1: positives {0.9, 0.4}, negatives {0.4, 0.1}: pairs 2+2+1+2 = 7 of 8 → AUC 7/8;
    # user 2: positive 0.2 below negative 0.3 → 0; user 3: one label only → left out
    pred = np.array([0.9, 0.4, 0.4, 0.1, 0.2, 0.3, 0.5, 0.6], f32)
    label = np.array([1, 1, 0, 0, 1, 0, 1, 1], f32)
    group = np.array([1, 1, 1, 1, 2, 2, 3, 3], np.int32)
    out = R.counts_brute(pred, label, group)
    np.testing.assert_array_equal(out[3], [7, 0, 0])
    assert R.gauc_exact(*out, "impressions") == Fraction(4 * 7, 8 * 6)
    assert R.gauc_exact(*out, "positives") == Fraction(2 * 7, 8 * 3)
    assert R.gauc_exact(*out, "uniform") == Fraction(7, 16)


def test_generators_have_the_properties_they_are_named_for(cases):
    rng = np.random.default_rng(3)
    for at, name in ((R.WAVE, "tie_run_64"), (R.RUN_BLOCK, "tie_run_1024")):
        (s, e), = R.tie_run_span(cases[name][0])
        assert s < at < e, name  # the tie run crosses the position
    # run-index ranges: a group inside one wave, one across lane 64, one across the block
    # boundary that also covers whole waves, and a short tail
    rr = R.run_index_ranges(*cases["run_groups"][::2])
    assert rr == [(0, 40), (40, 140), (140, 1340), (1340, 1343)]
    assert rr[1][0] < R.WAVE < rr[1][1] and rr[2][0] < R.RUN_BLOCK < rr[2][1]
    assert rr[2][1] - rr[2][0] > 3 * R.WAVE
    # pair counts past 32 bits
    pred, label, group = R.separated_case(1 << 17)
    assert R.counts_fast(pred, label, group)[3][0] == 1 << 33 > 1 << 32
    assert R.counts_fast(*R.separated_case(1 << 17, tied=True))[3][0] == 1 << 32
    # int64 keys that differ only in the high word / only in the low word, of both signs
    k = np.array(R.KEYS_I64, np.int64).view(np.uint64)
    lo, hi = (k & 0xFFFFFFFF).tolist(), (k >> 32).tolist()
    assert any(lo[i] == lo[j] and hi[i] != hi[j] for i in range(len(k)) for j in range(i))
    assert any(lo[i] != lo[j] and hi[i] == hi[j] for i in range(len(k)) for j in range(i))
    assert sorted(R.KEYS_I64) != sorted(R.KEYS_I64, key=lambda v: v % (1 << 64))  # sign matters
    np.testing.assert_array_equal(R.counts_fast(*cases["keys_i64_words"])[0], sorted(R.KEYS_I64))
    # splits land where they are named
    for name, at in (("split_wave", R.WAVE), ("split_tile", R.SORT_TILE_TINY)):
        assert R.counts_fast(*cases[name])[1][0] == at
    out = R.counts_fast(*cases["lone_between"])
    np.testing.assert_array_equal(out[1], [300, 1, 300])
    out = R.counts_fast(*cases["one_label_groups"])
    assert out[2][0] == out[1][0] and out[2][1] == 0 and out[3][0] == out[3][1] == 0 < out[3][2]
    out = R.counts_fast(*cases["all_equal"])
    np.testing.assert_array_equal(out[3], out[2].astype(np.int64) * (out[1] - out[2]))
    out = R.counts_fast(*cases["own_group"])
    assert (out[1] == 1).all() and out[0].size == 300
    pred, label, group = cases["signed_preds"]
    k = R.pred_key(pred)
    assert (k < 0x80000000).any() and (k >= 0x80000000).any()
    # the two zeros tie: a +0 positive against a -0 negative counts 1, not 2 or 0
    np.testing.assert_array_equal(
        R.counts_brute(np.array([0.0, -0.0], f32), np.array([1, 0], f32))[3], [1])
    # a NaN ranks above +inf and ties with every other NaN
    nan2 = np.array([0xFFC00001], np.uint32).view(f32)[0]
    out = R.counts_fast(np.array([np.nan, np.inf, nan2], f32), np.array([1, 0, 0], f32))
    assert out[3][0] == 2 + 1
    assert np.isnan(cases["one_nan"][0]).sum() == 1 and np.isnan(cases["many_nans"][0]).sum() == 90
    # odd labels: -0.0 is negative, 2.0 and -1.0 positive
    out = R.counts_brute(np.array([0.5, 0.6, 0.7, 0.1], f32), np.array([-0.0, 2.0, -1.0, 0.0], f32))
    assert (out[2][0], out[3][0]) == (2, 8)
    pred, label, group = R.zipf_case(rng, 20000, 1000)
    cnt = R.counts_fast(pred, label, group)[1]
    assert cnt.max() > 50 * np.median(cnt)  # a few users own most of the examples


def test_new_entry_points_are_declared_in_the_header():
    from recommender_amd import _lib as L

    assert {"rs_group_auc", "rs_group_auc_workspace_size", "rs_dien_users"} <= set(L.header_symbols())
    res, args = L.SIGNATURES["rs_group_auc"]
    assert len(args) == 14


def test_python_surface_exists():
    from recommender_amd import functional, metrics
    from recommender_amd.data import amazon

    assert callable(functional.group_auc_counts) and callable(amazon.read_dien_users)
    assert issubclass(metrics.ExactAUC, metrics.GroupAUC)
    for w in R.WEIGHTS:
        assert w in metrics.GroupAUC.WEIGHTS
    with pytest.raises(ValueError):
        metrics.GroupAUC(weight="clicks", device="cpu")
