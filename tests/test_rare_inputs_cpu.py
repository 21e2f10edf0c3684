"""The inputs of tests/rare_inputs.py reach the kernel paths their names claim (CPU models of
rs_masked_topk's candidate count and of the tables' linear probing): without this, a GPU test
that passes says nothing about the path it was written for."""
import numpy as np
import pytest

from tests import rare_inputs as RI


def test_common_topk_cases_stay_on_the_usual_paths():
    """Documents the gap the rare cases close: test_masked_topk_bit_exact never collects more
    than 75 candidates (one wave's sort, or one candidate per thread)."""
    worst = 0
    for R, I, K, excl in RI.COMMON_TOPK_CASES:
        scores, u, it = RI.common_topk_case(R, I, K, excl)
        for r in range(R):
            row = RI.masked_row(scores[r], it[u == r] if excl else None)
            worst = max(worst, RI.topk_candidates(row, K))
    assert 64 < worst <= 75


@pytest.mark.parametrize("I,K,nc", [(8448, 64, 2080), (27278, 64, 6742), (16640, 33, 2081),
                                    (33024, 17, 2065), (70000, 9, 2193), (80000, 8, 2192),
                                    (70000, 8, 1919), (140000, 4, 1642)])
def test_hot_row_candidate_count(I, K, nc):
    """nc = (K - 1) · (items per hot thread) + 1."""
    assert RI.topk_candidates(RI.hot_row(I, K, np.random.default_rng(1)), K) == nc


@pytest.mark.parametrize("name", list(RI.TOPK_CASES))
def test_topk_case_regime(name):
    regime, I, K, *_ = RI.TOPK_CASES[name]
    rows, k = RI.topk_case_rows(name)
    assert k == K and len(rows) in (2, 4) and all(r.size == I for r in rows)
    assert [RI.topk_regime(r, K) for r in rows] == [regime] * len(rows)
    scores, _, plain, (ip, it) = RI.topk_case(name)
    assert ip[-1] > 0 and plain in (0, len(rows) // 2)  # half the rows (or all) exclude items
    if name.startswith("wave_bitmap"):
        assert (I + 31) // 32 * 4 > 32 * 1024  # the bitmap alone is past 32 KB
        for r in range(len(rows)):
            assert (it[ip[r]:ip[r + 1]] >= (I - 1) // 32 * 32).any()  # its last word is used
    if "one_thread" in name:  # the top K of every row (exclusions applied) belong to thread 0
        for r in rows:
            top = np.lexsort((np.arange(I), -r.astype(np.float64)))[:K]
            assert (top % RI.TOPK_THREADS == 0).all()
    if "wave3" in name:  # every hot item belongs to a thread of the block's last wave
        hot = np.flatnonzero(scores[0] >= 400) % RI.TOPK_THREADS
        assert hot.min() >= 192


def test_three_left_case_needs_excluded_items():
    rows, K = RI.topk_case_rows("wave_three_left_300_10")
    assert all(np.isfinite(r).sum() == 3 < K for r in rows)


@pytest.mark.parametrize("name", list(RI.HASH_CASES) + ["overfull"])
def test_hash_case_properties(name):
    cap, keys, stream = RI.hash_case(name)
    nd = RI.HASH_OVERFULL[1] if name == "overfull" else RI.HASH_CASES[name][1]
    assert np.unique(RI.table_key(keys)).size == keys.size == nd
    d = RI.hash_counts(stream)
    assert set(d) == set(RI.table_key(keys).tolist())  # every key occurs
    slot_of, dropped, wrapped = RI.probe_table(stream, cap)
    assert wrapped  # a probe chain runs past the last slot
    if name == "overfull":
        assert nd > cap and len(dropped) == nd - cap and len(slot_of) == cap
    else:
        assert not dropped and len(slot_of) == nd
        assert (nd == cap) == name.endswith("full")  # exactly full / load ~0.9
        assert 0.89 < nd / cap <= 1.0
    # the key edge cases: 0, and ~0 with ~0 - 1 (one table key)
    assert (stream == 0).any() and (stream == RI.EMPTY).any() and (stream == RI.EMPTY - RI.U64(1)).any()
    # counts on both sides of min_count
    counts = sorted(c for c, _ in d.values())
    assert RI.MIN_COUNT in counts and RI.MIN_COUNT + 1 in counts
    # wave_key_group: runs over a wave and a block boundary, a whole wave, 200 in a row, a tail
    assert np.unique(stream[50:80]).size == 1 and np.unique(stream[250:270]).size == 1
    assert np.unique(stream[320:384]).size == 1 and np.unique(stream[400:600]).size == 1
    assert stream.size % 64 != 0
    # absent keys are absent, and some start probing in the last slots
    absent = RI.absent_hashes(keys, cap, 64, seed=1)
    assert absent.size == 64 and not np.isin(RI.table_key(absent), RI.table_key(keys)).any()
    assert (RI.vslot(absent, cap - 1) >= cap - 4).sum() >= 8


def test_vslot_is_the_table_slot_function():
    # 0x9E3779B97F4A7C15 · 1 >> 32 = 0x9E3779B9; · 2 mod 2^64 = 0x3C6EF372FE94F82A
    assert RI.vslot(RI.U64(1), 0xFFFFFFFF) == 0x9E3779B9
    assert RI.vslot(RI.U64(2), 1023) == 0x3C6EF372 & 1023
    assert RI.vslot(np.array([0], RI.U64), 63)[0] == 0
    assert RI.table_key(RI.EMPTY) == RI.EMPTY - RI.U64(1) and RI.table_key(RI.U64(5)) == 5
