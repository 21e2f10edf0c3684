"""rs_group_auc on the GPU against tests/group_auc_ref.py, bit for bit on integers: sizes at
every tile edge of the sort, the scan and the per-run kernel, group shapes, key dtypes and
signs, prediction ties and special values, NaN, counts past 32 bits, labels, argument errors,
and the Python layer on top (functional.group_auc_counts, metrics.GroupAUC / ExactAUC, the DIEN
CLI). Every raw call has 64 guard elements behind each output and prefilled tails."""
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import group_auc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def raw_call(pred, label, group, ws_bytes=None, expect=0, null_pred=False, dtype=None, n=None):
    """rs_group_auc → ((keys, n, pos, w2) as NumPy, error flag); guards and unwritten tails
    checked. A failing status must leave every output untouched."""
    lib = L.lib()
    n = len(pred) if n is None else n
    cap = max(len(pred), 0)
    tp = torch.from_numpy(np.ascontiguousarray(pred, f32)).to(DEV)
    ty = torch.from_numpy(np.ascontiguousarray(label, f32)).to(DEV)
    tg = None if group is None else torch.from_numpy(np.ascontiguousarray(group)).to(DEV)
    if dtype is None:
        dtype = L.RS_ID_I32 if tg is None else L.id_dtype_code(tg)
    key = torch.full((cap + GUARD,), FILL64, dtype=torch.int64, device=DEV)
    cnt = torch.full((cap + GUARD,), FILL32, dtype=torch.int32, device=DEV)
    pos = torch.full((cap + GUARD,), FILL32, dtype=torch.int32, device=DEV)
    w2 = torch.full((cap + GUARD,), FILL64, dtype=torch.int64, device=DEV)
    ng = torch.full((1 + GUARD,), FILL32, dtype=torch.int32, device=DEV)
    err = torch.full((1 + GUARD,), FILL32, dtype=torch.int32, device=DEV)
    err[0] = 0
    need = lib.rs_group_auc_workspace_size(n)
    if ws_bytes is None:
        ws_bytes = need
    ws = torch.full((ws_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    st = lib.rs_group_auc(None if null_pred else L.ptr(tp), L.ptr(ty), L.ptr(tg), dtype, n,
                          L.ptr(key), L.ptr(cnt), L.ptr(pos), L.ptr(w2), L.ptr(ng), L.ptr(err),
                          L.ptr(ws), ws_bytes, L.stream_ptr(ws.device))
    torch.cuda.synchronize()
    assert st == expect, (st, lib.rs_last_error())
    key, cnt, pos, w2, ng, err, ws = (t.cpu().numpy() for t in (key, cnt, pos, w2, ng, err, ws))
    assert (ws[ws_bytes:] == 0xAB).all()
    assert (ng[1:] == FILL32).all() and (err[1:] == FILL32).all()
    G = 0 if st != 0 else int(ng[0])
    if st != 0:
        assert ng[0] == FILL32 and err[0] == 0
    assert 0 <= G <= cap
    for a, fill in ((key, FILL64), (cnt, FILL32), (pos, FILL32), (w2, FILL64)):
        assert (a[G:] == fill).all()  # tails j >= n_groups and the guards
    return (key[:G], cnt[:G], pos[:G], w2[:G]), int(err[0])


def check(pred, label, group, nan=False):
    got, err = raw_call(pred, label, group)
    ref = R.counts_fast(pred, label, group)
    for a, b, what in zip(got, ref, ("keys", "n", "pos", "w2")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert err == (L.RS_ERRBIT_NONFINITE if nan else 0)
    return got


@pytest.fixture(scope="module")
def cases():
    return R.small_cases(np.random.default_rng(11))


# ---- sizes and determinism --------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65,
         R.SORT_TILE_TINY - 1, R.SORT_TILE_TINY, R.SORT_TILE_TINY + 1,
         R.SORT_TILE_SMALL - 1, R.SORT_TILE_SMALL, R.SORT_TILE_SMALL + 1,
         R.SCAN_TILE - 1, R.SCAN_TILE, R.SCAN_TILE + 1,
         R.SORT_SMALL_FROM - 1, R.SORT_SMALL_FROM, R.SORT_SMALL_FROM + 1,
         R.SORT_SMALL_FROM + R.SORT_TILE_SMALL - 1, R.SORT_SMALL_FROM + R.SORT_TILE_SMALL + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_the_tile_edges(n):
    rng = np.random.default_rng(n)
    check(*R.random_case(rng, n, max(n // 50, 1), np.int64, levels=max(n // 3, 2)))
    if n <= R.SCAN_TILE + 1:
        check(*R.random_case(rng, n, max(n // 9, 1), np.int32))


def test_n_zero_stores_zero_groups():
    e = np.zeros(0, f32)
    got, err = raw_call(e, e, np.zeros(0, np.int32))
    assert got[0].size == 0 and err == 0
    assert L.lib().rs_group_auc_workspace_size(0) == 0


def test_same_inputs_twice_are_bit_equal():
    case = R.zipf_case(np.random.default_rng(2), 50000, 300)
    a, b = raw_call(*case)[0], raw_call(*case)[0]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a, R.counts_fast(*case)):
        np.testing.assert_array_equal(x, y)


def test_call_replays_from_a_captured_graph():
    """No host sync and nothing sized by the data: the call records into a HIP graph, and a
    replay on refilled inputs gives that input's counts."""
    lib = L.lib()
    rng = np.random.default_rng(22)
    n = 3000
    first, second = R.zipf_case(rng, n, 40), R.random_case(rng, n, 300, np.int64, levels=25)
    tp, ty, tg = (torch.from_numpy(a).to(DEV) for a in first)
    key = torch.zeros(n, dtype=torch.int64, device=DEV)
    cnt, pos = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
    w2 = torch.zeros(n, dtype=torch.int64, device=DEV)
    info = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.rs_group_auc_workspace_size(n), dtype=torch.uint8, device=DEV)

    def call():
        st = lib.rs_group_auc(L.ptr(tp), L.ptr(ty), L.ptr(tg), L.RS_ID_I64, n, L.ptr(key), L.ptr(cnt),
                              L.ptr(pos), L.ptr(w2), L.ptr(info), L.ptr(info[1:]), L.ptr(ws),
                              ws.numel(), L.stream_ptr(ws.device))
        assert st == 0, lib.rs_last_error()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for case in (second, first):
        for dst, src in zip((tp, ty, tg), case):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize()
        G, err = info.tolist()
        assert err == 0
        for a, b in zip((key, cnt, pos, w2), R.counts_fast(*case)):
            np.testing.assert_array_equal(a[:G].cpu().numpy(), b)


# ---- the shared small families (each also checked against brute force on the CPU) --------------
FAMILIES = ["own_group", "one_group_none", "one_group_const", "split_wave", "split_tile",
            "lone_between", "one_label_groups", "zipf", "all_equal", "tie_run_64", "tie_run_1024",
            "run_groups", "interleaved", "special_values", "signed_preds", "separated",
            "separated_tied", "odd_labels", "keys_i32_extremes", "keys_i64_words",
            "random_i32_ties"]


@pytest.mark.parametrize("name", FAMILIES)
def test_family(cases, name):
    got = check(*cases[name])
    assert (np.diff(got[0]) > 0).all()  # ascending signed keys


def test_one_group_as_null_and_as_constant_agree(cases):
    pred, label, _ = cases["one_group_none"]
    a = check(pred, label, None)
    b = check(pred, label, np.full(pred.size, 0, np.int64))
    c = check(pred, label, np.full(pred.size, 0, np.int32))
    for x, y, z in zip(a, b, c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    assert a[0].tolist() == [0]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_groups_split_at_wave_and_tile_boundaries(dtype):
    rng = np.random.default_rng(8)
    for n, split in ((200, 64), (1300, 512), (3000, 1024), (1 << 17, 1024), (9000, 4096)):
        got = check(*R.split_case(rng, n, split, dtype))
        assert got[1].tolist() == [split, n - split]


def test_thousand_zipf_groups():
    got = check(*R.zipf_case(np.random.default_rng(6), 60000, 1000))
    assert 500 < got[0].size <= 1000


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_every_example_its_own_group(dtype):
    got = check(*R.own_group_case(np.random.default_rng(7), 5000, dtype))
    assert got[0].size == 5000 and (got[3] == 0).all()


def test_int64_keys_order_by_both_words():
    rng = np.random.default_rng(9)
    got = check(*R.keys_case(rng, R.KEYS_I64, 700, np.int64))
    assert got[0].tolist() == sorted(R.KEYS_I64)
    got = check(*R.keys_case(rng, [R.INT32_MIN, R.INT32_MAX, -1, 0], 700, np.int32))
    assert got[0].tolist() == [R.INT32_MIN, -1, 0, R.INT32_MAX]


# ---- predictions ------------------------------------------------------------------------------
def test_tie_runs_across_wave_and_block_positions():
    rng = np.random.default_rng(10)
    for n, at, half in ((5000, 64, 6), (5000, 1024, 30), (5000, 256, 200), (9000, 4096, 64)):
        case = R.tie_run_case(rng, n, at, half)
        (s, e), = R.tie_run_span(case[0])
        assert s < at < e
        check(*case)


def test_groups_whose_runs_cross_waves_and_blocks():
    rng = np.random.default_rng(12)
    for counts in ([40, 100, 1200, 3], [63, 1, 64, 896, 1, 1023, 2048, 5], [1024, 1024, 1]):
        case = R.run_groups_case(rng, counts)
        assert [b - a for a, b in R.run_index_ranges(case[0], case[2])] == counts
        check(*case)


def test_full_width_sort_keys():
    """Predictions of both signs give prediction keys with the top bit clear and set; negative
    group ids give group words with it clear: every radix pass sees all 32 bits."""
    pred, label, group = R.signed_preds_case(np.random.default_rng(13), 20000)
    k = R.pred_key(pred)
    assert (k < 0x80000000).any() and (k >= 0x80000000).any()
    check(pred, label, group)
    check(pred, label, group.astype(np.int64) * (1 << 40))


@pytest.mark.parametrize("name", ["one_nan", "many_nans"])
def test_nan_sets_the_flag_and_ranks_as_the_top_tie(cases, name):
    check(*cases[name], nan=True)


def test_nan_in_every_wave_of_a_large_input():
    rng = np.random.default_rng(14)
    pred, label, group = R.random_case(rng, 3000, 4, np.int32, levels=50)
    pred[::50] = np.nan
    check(pred, label, group, nan=True)


# ---- counts past 32 bits ----------------------------------------------------------------------
def test_pair_counts_past_32_bits():
    n = 1 << 17
    got = check(*R.separated_case(n))
    assert got[3].tolist() == [1 << 33] and got[2].tolist() == [n // 2]
    got = check(*R.separated_case(n, tied=True))
    assert got[3].tolist() == [1 << 32]
    got = check(*R.separated_case(n + 1))
    assert got[3].tolist() == [2 * (n // 2) * (n // 2 + 1)]


# ---- argument errors --------------------------------------------------------------------------
def test_argument_errors():
    rng = np.random.default_rng(15)
    pred, label, group = R.random_case(rng, 100, 5, np.int32)
    raw_call(pred, label, group, n=-1, expect=L.RS_E_INVALID)
    raw_call(pred, label, group, dtype=7, expect=L.RS_E_INVALID)
    raw_call(pred, label, group, null_pred=True, expect=L.RS_E_INVALID)
    need = L.lib().rs_group_auc_workspace_size(100)
    raw_call(pred, label, group, ws_bytes=need - 1, expect=L.RS_E_WORKSPACE)
    check(pred, label, group)


# ---- Python layer -----------------------------------------------------------------------------
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_functional_counts_and_nan():
    from recommender_amd.functional import group_auc_counts

    pred, label, group = R.zipf_case(np.random.default_rng(16), 7000, 100)
    got = group_auc_counts(t(pred).view(70, 100), t(label).view(70, 100), t(group))
    for a, b in zip(got, R.counts_fast(pred, label, group)):
        assert a.dtype == torch.from_numpy(b).dtype
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    pred[5] = np.nan
    with pytest.raises(ValueError):
        group_auc_counts(t(pred), t(label), t(group))
    with pytest.raises(ValueError):
        group_auc_counts(t(pred)[:-1], t(label), t(group))
    e = torch.empty(0, device=DEV)
    assert [x.numel() for x in group_auc_counts(e, e)] == [0, 0, 0, 0]


def test_group_auc_metric_against_the_exact_fraction():
    from recommender_amd.metrics import GroupAUC

    pred, label, group = R.zipf_case(np.random.default_rng(17), 9000, 150)
    ref = R.counts_fast(pred, label, group)
    for weight in R.WEIGHTS:
        m = GroupAUC(weight=weight)
        assert m.result() == 0.0 and m.groups()[0].size == 0
        m.update_state(t(label), t(pred), t(group))
        for a, b in zip(m.groups(), ref):
            np.testing.assert_array_equal(a, b)
        assert m.result() == float(R.gauc_exact(*ref, weight))
    with pytest.raises(ValueError):
        m.update_state(t(label)[:-1], t(pred), t(group))


def test_result_does_not_depend_on_how_updates_were_split():
    from recommender_amd.metrics import GroupAUC

    rng = np.random.default_rng(18)
    pred, label, group = R.zipf_case(rng, 5000, 80)
    results = []
    for parts in (1, 3, 17):
        m = GroupAUC()
        perm = rng.permutation(pred.size)
        for idx in np.array_split(perm, parts):
            m.update_state(t(label[idx]).view(-1, 1), t(pred[idx]).view(-1, 1), t(group[idx].astype(np.int32)))
        results.append((m.groups(), m.result()))
    for g, r in results[1:]:
        for a, b in zip(g, results[0][0]):
            np.testing.assert_array_equal(a, b)
        assert r == results[0][1]
    assert results[0][1] == float(R.gauc_exact(*R.counts_fast(pred, label, group)))
    m.reset_states()
    assert m.size == 0 and m.result() == 0.0 and m.groups()[0].size == 0
    m.update_state(t(label[:10]), t(pred[:10]), t(group[:10]))
    for a, b in zip(m.groups(), R.counts_fast(pred[:10], label[:10], group[:10])):
        np.testing.assert_array_equal(a, b)


def test_exact_auc_is_the_one_group_count():
    from recommender_amd.metrics import ExactAUC

    pred, label, _ = R.random_case(np.random.default_rng(19), 6000, 1, levels=500)
    m = ExactAUC()
    m.update_state(t(label[:1000]), t(pred[:1000]))
    m.update_state(t(label[1000:]), t(pred[1000:]))
    keys, n, pos, w2 = R.counts_fast(pred, label, None)
    for a, b in zip(m.groups(), (keys, n, pos, w2)):
        np.testing.assert_array_equal(a, b)
    assert m.result() == float(Fraction(int(w2[0]), 2 * int(pos[0]) * int(n[0] - pos[0])))


def test_exact_auc_meets_keras_auc_where_the_grid_cannot_matter():
    from oracle.metrics import keras_auc
    from recommender_amd.metrics import ExactAUC

    rng = np.random.default_rng(20)
    T = 20000
    step = 1.0 / (T - 1)
    neg, pos = rng.uniform(0.1, 0.3, 30).astype(f32), rng.uniform(0.6, 0.9, 25).astype(f32)
    # precondition: perfectly separated, at least two grid steps between the labels, in [0, 1]
    assert pos.min() - neg.max() >= 2 * step and 0 <= neg.min() and pos.max() <= 1
    pred = np.concatenate([neg, pos])
    label = np.concatenate([np.zeros(30), np.ones(25)]).astype(f32)
    perm = rng.permutation(pred.size)
    m = ExactAUC()
    m.update_state(t(label[perm]), t(pred[perm]))
    assert m.result() == 1.0
    assert keras_auc(label[perm], pred[perm], num_thresholds=T)[0] == 1.0


def test_dien_cli_reports_gauc_only_when_asked(capsys):
    from recommender_amd.dien.train import main

    argv = ["--model_type", "BASE", "--epochs", "1", "--steps_per_epoch", "3", "--train_batch_size",
            "64", "--history_max_length", "8", "--item_vocab", "300", "--cat_vocab", "20",
            "--hip_graph", "0"]
    main(argv)
    plain = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(r"epoch 1 loss \d+\.\d{4} auc \d\.\d{4} \d+ ex/s", plain), plain
    main(argv + ["--gauc_users", "50"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    mt = re.fullmatch(r"epoch 1 loss \d+\.\d{4} auc \d\.\d{4} gauc (\d\.\d{4}) \d+ ex/s", line)
    assert mt, line
    assert 0.0 <= float(mt[1]) <= 1.0
