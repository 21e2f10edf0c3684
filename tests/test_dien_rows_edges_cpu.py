"""The references of tests/dien_rows_edges.py against brute-force loops, and every case list of
tests/test_dien_rows_edges_gpu.py reaching the kernel path it names — all without a GPU."""
import numpy as np
import pytest
import torch

from tests import dien_rows_edges as E


def _rng():
    return np.random.default_rng(17)


# ---- 1. the valid-row list ---------------------------------------------------------------------
@pytest.mark.parametrize("R", E.VR_RS)
def test_vr_masks_have_their_rows(R):
    rng = _rng()
    for kind in E.VR_KINDS:
        m = E.vr_mask(kind, R, rng)
        assert m.dtype == np.uint8 and m.shape == (R,)
        want = [r for r in range(R) if m[r] != 0]  # the brute-force list
        assert E.valid_rows_ref(m).tolist() == want
        if kind == "all":
            assert want == list(range(R))
        elif kind == "none":
            assert want == []
        elif kind == "row0":
            assert want == [0]
        elif kind == "last":
            assert want == [R - 1]
        elif kind.startswith("first"):
            s = int(kind[5:])
            assert want == list(range(0, R, s))
        elif kind.startswith("last"):
            s = int(kind[4:])
            assert want == list(range(s - 1, R, s))
        elif kind == "bytes":
            assert set(np.unique(m)) <= {0, 2, 255} and (R < 64 or {2, 255} <= set(np.unique(m)))


def test_vr_sizes_sit_on_the_chunk_edges():
    """R on, one before and one after the 64-row ballot chunk, the 1024-row wave and the
    4096-row block; 8193: three blocks, the last holding one row."""
    for s in (64, 1024, 4096):
        assert {s - 1, s, s + 1} <= set(E.VR_RS)
    assert -(-8193 // 4096) == 3 and 8193 % 4096 == 1 and 1 in E.VR_RS


# ---- 2. the products ---------------------------------------------------------------------------
def test_count_mask_is_exact():
    rng = _rng()
    for R, c in ((1, 0), (1, 1), (5, 5), (70, 33), (200, 2), (9000, 8193), (40, 0)):
        m = E.count_mask(R, c, rng, values=(1, 2, 255))
        assert int((m != 0).sum()) == c
        if 2 <= c:
            assert m[0] and m[R - 1]


def test_proj_pairs_reach_every_instance():
    got = {E.proj_class(K, N) for K, N in E.PROJ_PAIRS}
    assert got == {(km, nb) for km in (16, 36, 64) for nb in (1, 2, 3)}
    assert len(E.PROJ_PAIRS) >= 10
    assert {K for K, _ in E.PROJ_PAIRS} >= {1, 16, 17, 36, 37, 64}
    assert {N for _, N in E.PROJ_PAIRS} >= {1, 64, 65, 128, 129, 192}
    # both sides of every dispatch threshold
    assert E.proj_class(16, 64) == (16, 1) and E.proj_class(17, 65) == (36, 2)
    assert E.proj_class(36, 128) == (36, 2) and E.proj_class(37, 129) == (64, 3)
    # counts around one wave (32 rows) and one block (128 rows) of the projection
    assert {0, 1, 31, 32, 33, 127, 128, 129} == set(E.PROJ_COUNTS)


def test_dx_sizes_reach_every_instance():
    assert [E.dx_class(N) for N in E.DX_NS] == [64, 64, 112, 112, 128, 128, 192, 192]
    assert set(E.DX_KS) == {1, 36, 63, 64}
    assert set(E.DX_COUNTS) == {0, 15, 16, 17, 63, 64, 65}
    for c in E.DX_COUNTS:
        rs = E.dx_rs(c)
        assert (c in rs) == (c > 0)
        assert any(r % 16 for r in rs if r != c) and any(r % 16 == 0 and r % 64 for r in rs)
        assert all(r >= c and r > 0 for r in rs)


def test_wgrad_pairs_take_both_instantiations():
    items = {p: E.wgrad_items(*p) for p in E.WGRAD_PAIRS}
    assert items[(36, 108)] == 999 and items[(36, 112)] == 1036
    assert items[(63, 64)] == 1024 and items[(64, 192)] == 3120
    assert items[(1, 1)] == 2 and items[(20, 109)] == 588
    assert any(v <= 1024 for v in items.values()) and any(v > 1024 for v in items.values())
    assert 1024 in items.values()  # the threshold itself stays on 256 threads
    assert max(items.values()) <= 4 * 1024  # four outputs per thread at 1024 threads
    assert any(N % 4 for _, N in E.WGRAD_PAIRS) and any(K == 64 for K, _ in E.WGRAD_PAIRS)
    per = [E.wgrad_per(c) for c in E.WGRAD_COUNTS]
    assert set(per) == {0, 16, 32}
    assert E.wgrad_per(8192) == 16 and E.wgrad_per(8193) == 32
    # one block, two blocks (a 1-row tail), more than 64 rows only in the last case
    assert E.wgrad_per(17) == 16 and E.wgrad_per(16) == 16


def test_product_references_vs_loops():
    rng = _rng()
    R, K, N = 13, 5, 7
    x, W, b = rng.standard_normal((R, K)), rng.standard_normal((K, N)), rng.standard_normal(N)
    d, add = rng.standard_normal((R, N)), rng.standard_normal((R, K))
    rows = np.array([0, 3, 4, 9, 12])
    y, by = E.proj_ref(x, W, b, rows)
    y0, by0 = E.proj_ref(x, W, None, rows)
    dx, bdx = E.dx_ref(d, W, add, rows)
    dx0, bdx0 = E.dx_ref(d, W, None, rows)
    for i, r in enumerate(rows):
        for n in range(N):
            s = sum(x[r, k] * W[k, n] for k in range(K))
            mg = sum(abs(x[r, k] * W[k, n]) for k in range(K))
            assert abs(y[i, n] - (s + b[n])) < 1e-12 and abs(y0[i, n] - s) < 1e-12
            assert np.isclose(by[i, n], (K + 2) * E.U24 * (mg + abs(b[n])))
            assert np.isclose(by0[i, n], (K + 1) * E.U24 * mg)
        for k in range(K):
            s = sum(d[r, n] * W[k, n] for n in range(N))
            mg = sum(abs(d[r, n] * W[k, n]) for n in range(N))
            assert abs(dx[i, k] - (s + add[r, k])) < 1e-12 and abs(dx0[i, k] - s) < 1e-12
            assert np.isclose(bdx[i, k], (N + 2) * E.U24 * (mg + abs(add[r, k])))
            assert np.isclose(bdx0[i, k], (N + 1) * E.U24 * mg)
    for shift in (0, 4):
        C, s, bC, bs = E.wgrad_ref(x, d, rows, shift)
        C2, s2 = np.zeros((K, N)), np.zeros(N)
        M2 = np.zeros((K, N))
        for r in rows:
            a = x[r] if shift == 0 else (x[r - 1] if r % shift else np.zeros(K))
            C2 += np.outer(a, d[r])
            M2 += np.abs(np.outer(a, d[r]))
            s2 += d[r]
        assert np.allclose(C, C2, atol=1e-12) and np.allclose(s, s2, atol=1e-12)
        assert np.allclose(bC, (len(rows) + 1) * E.U24 * M2)
    C, s, bC, bs = E.wgrad_ref(x, d, np.zeros(0, np.int64))
    assert (C == 0).all() and (s == 0).all() and (bC == 0).all()


def test_shift_mask_has_first_steps_and_unlisted_predecessors():
    B, T = 6, 9
    m = E.shift_mask(B, T, _rng())
    rows = E.valid_rows_ref(m)
    first = rows[rows % T == 0]
    assert len(first) >= 1 and len(first) < B  # some sequences start listed, some do not
    pred_unlisted = [r for r in rows if r % T and not m.reshape(-1)[r - 1]]
    pred_listed = [r for r in rows if r % T and m.reshape(-1)[r - 1]]
    assert pred_unlisted and pred_listed


# ---- 3. the aux loss ---------------------------------------------------------------------------
def test_aux_masks_have_their_shape():
    rng = _rng()
    for L in E.AUX_LS:
        for kind in E.AUX_KINDS:
            if kind == "dead_tile" and L < 34:
                continue
            m = E.aux_mask(kind, 5, L, rng)
            v = m != 0
            assert (v[:, 1:].sum(1) > 0).all()
            if kind == "post":
                lens = v.sum(1)
                assert (v == (np.arange(L)[None] < lens[:, None])).all()
                want = sorted({min(max(s, 1), L - 1) for s in (L - 1, 16, 17)})
                assert sorted(set(lens - 1)) == want
            elif kind == "only1":
                assert (v[:, 1:].sum(1) == 1).all() and v[:, 1].all()
            elif kind == "only_last":
                assert (v[:, 1:].sum(1) == 1).all() and v[:, L - 1].all()
            elif kind == "late":
                assert not v[:, 0].any()
            elif kind == "bytes":
                assert set(np.unique(m)) <= {0, 1, 2, 255} and (L < 16 or m.max() > 1)
            elif kind == "dead_tile":
                assert not v[:, 17:33].any() and v[:, 1:17].any(1).all() and v[:, 33].all()
                B = 5
                live = E.aux_live_items(m)
                assert [i for i in live if i // B == 1] == []  # the tile between two live ones
                assert len([i for i in live if i // B == 0]) == B
                assert len([i for i in live if i // B == 2]) == B


def test_aux_cases_cover_the_tile_edges():
    specs = [s for s in E.AUX_CASES if s[0] == 36]
    assert len(set(E.AUX_CASES)) == len(E.AUX_CASES)
    for L in E.AUX_LS:
        assert {s[1] for s in specs if s[2] == L} == set(E.AUX_BS), L
        kinds = {s[3] for s in specs if s[2] == L}
        assert kinds >= set(E.AUX_KINDS) - ({"dead_tile"} if L < 34 else set()), L
    assert {s[2] for s in E.AUX_CASES if s[0] == 16} == set(E.AUX_LS)
    # the last aux row (t = L - 2) and the last hidden row (t = L - 1) on, before and after a
    # tile edge; forward tiles over t <= L - 2, backward tiles over t < L
    assert [E.fwd_tiles(L) for L in E.AUX_LS] == [1, 1, 1, 1, 2, 2, 2, 3]
    assert [E.bwd_tiles(L) for L in E.AUX_LS] == [1, 1, 1, 2, 2, 2, 3, 3]
    for L in (17, 33):  # the last backward tile holds hidden row L - 1 alone: never live
        m = np.ones((2, L), np.uint8)
        assert max(E.aux_live_items(m)) // 2 == E.bwd_tiles(L) - 2


def test_aux_live_item_counts_odd_and_single():
    n = {s: len(E.aux_live_items(E.aux_inputs(*s)["mask"])) for s in E.AUX_CASES}
    assert n[(36, 1, 2, "all")] == 1 and n[(36, 3, 3, "all")] == 3
    assert any(v % 2 for v in n.values()) and any(v % 2 == 0 for v in n.values())
    assert 1 in n.values()
    # an example without a valid aux row: every tile live (0 / 0, as the reference)
    m = E.nan_case()["mask"]
    B, L = m.shape
    live = E.aux_live_items(m)
    assert [i for i in live if i % B == 2] == [t * B + 2 for t in range(E.bwd_tiles(L))]
    assert (m[2, 1:] == 0).all() and ((m[[0, 1, 3, 4], 1:] != 0).sum(1) > 0).all()


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
def test_persistent_cases_loop(cus):
    bwd, fwd, odd = E.persistent_cases(cus)
    H, B, L, _ = odd
    if cus == 8:
        assert len(E.aux_live_items(np.ones((B, L), np.uint8))) == B
    assert B % 2 == 1 and E.bwd_tiles(L) == 1
    last_pair = (B + 1) // 2 - 1  # holds item B - 1 alone
    assert last_pair // cus >= 2 and E.bwd_rounds(B, cus)[0] >= 3
    H, B, L, _ = bwd
    m = np.ones((B, L), np.uint8)
    if cus == 8:
        assert len(E.aux_live_items(m)) == 2 * B
    n_live = 2 * B  # tiles 0 and 1 of every example
    if cus == 256:
        assert B == 700 and n_live == 1400
    pairs = (n_live + 1) // 2
    assert pairs >= 2.5 * cus
    hi, lo = E.bwd_rounds(n_live, cus)
    assert hi >= 3 and lo >= 2  # the two-rounds-ahead item_of and the one-ahead fetch both run
    H, B, L, _ = fwd
    assert B % 2 == 1 and L == 3 and B == 6 * cus + 3
    hi, lo, grid = E.fwd_rounds(B, cus)
    assert grid == 3 * cus and hi == 2 and lo == 1
    # the small cases: fewer pairs than blocks, so some blocks have no pair at all
    assert E.bwd_rounds(3, cus) == (1, 0)


def test_aux_daux_spans_six_decades():
    d = E.aux_daux(5, _rng())
    assert d[3] == 0 and (d > 0).any() and (d < 0).any()
    nz = np.abs(d[d != 0])
    assert nz.max() >= 1e3 and nz.min() <= 1e-3
    big = E.aux_daux(700, _rng())
    assert np.abs(big[big != 0]).min() >= 1e-3 * 0.999 and np.abs(big).max() <= 1e3 * 1.001


def _aux_loops(d):
    """aux_b by explicit loops in float64 (dien/layers.py:89-108)."""
    f = {k: np.asarray(v, np.float64) for k, v in d.items() if k != "mask"}
    m = d["mask"] != 0
    B, L = m.shape
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    out = np.zeros(B)
    for b in range(B):
        tot, cnt = 0.0, 0
        for t in range(L - 1):
            if not m[b, t + 1]:
                continue
            cnt += 1
            for e, y in ((f["pos"], 1.0), (f["neg"], 0.0)):
                x = np.concatenate([f["hidden"][b, t], e[b, t + 1]])
                z = float(sig(sig(x @ f["W1"] + f["b1"]) @ f["W2"] + f["b2"]) @ f["W3"][:, 0]
                          + f["b3"][0])
                tot += max(z, 0.0) - z * y + np.log1p(np.exp(-abs(z)))
        out[b] = tot / (2.0 * cnt)
    return out


@pytest.mark.parametrize("spec", [(36, 3, 18, "random"), (16, 5, 34, "dead_tile"),
                                  (36, 2, 3, "bytes"), (36, 5, 17, "late")])
def test_aux_reference_vs_loops(spec):
    d = E.aux_inputs(*spec)
    r64 = E.aux_eval(d, torch.float64)
    assert np.allclose(r64["aux"], _aux_loops(d), rtol=1e-12, atol=0)
    # the masked rows (of another scale) are read by nothing: zero gradients, and the loss does
    # not move when they change
    v = d["mask"] != 0
    assert (r64["dpos"][:, 0] == 0).all() and (r64["dneg"][:, 0] == 0).all()
    assert (r64["dhidden"][:, -1] == 0).all()
    assert (r64["dpos"][~v] == 0).all() and (r64["dneg"][~v] == 0).all()
    assert (r64["dhidden"][:, :-1][~v[:, 1:]] == 0).all()
    d2 = dict(d)
    d2["hidden"] = d["hidden"].copy()
    d2["hidden"][:, :-1][~v[:, 1:]] = 3.0
    d2["hidden"][:, -1] = -3.0
    d2["pos"] = np.where(v[:, :, None], d["pos"], 3.0).astype(np.float32)
    assert (E.aux_eval(d2, torch.float64)["aux"] == r64["aux"]).all()
    # the parameter-gradient magnitudes: per example, and their sum bounds the gradient
    mag = E.aux_param_magnitude(d)
    for n in E.AUX_PARAMS:
        assert (np.abs(r64["d" + n]) <= mag["d" + n] * (1 + 1e-12) + 1e-300).all()
    mag4 = E.aux_param_magnitude(d, 2)
    for n in E.AUX_PARAMS:
        assert (mag4["d" + n] <= mag["d" + n] * (1 + 1e-12)).all()


def test_scales_and_control():
    ref = np.array([[1.0, -4.0], [0.0, 0.0], [0.5, 0.25]])
    assert (E.example_scale(ref) == [[5.0, 8.0], [0.0, 0.0], [1.0, 0.75]]).all()
    assert (E.example_scale(np.array([2.0, -3.0])) == [4.0, 6.0]).all()
    assert E.worst_ratio(np.array([0.0, 1.0]), np.array([0.0, 4.0])) == 0.25
    assert E.worst_ratio(np.array([1e-30]), np.array([0.0])) == np.inf
    # the control (the oracle in fp32) over a slice of the case list: finite, above zero, and by
    # definition within its own pooled worst ratio
    specs = E.AUX_CASES[:12]
    rho = E.rho32(specs)
    print(f"rho32 over {len(specs)} cases: {rho:.3g}")
    assert 0 < rho < np.inf
    for s in specs:
        assert max(E.aux_case(s)[3].values()) <= rho


def test_nan_pattern_of_the_reference():
    """An example without a valid aux row: NaN in dhidden[b, :L-1], dpos[b, 1:], dneg[b, 1:],
    its aux and every parameter gradient; exactly 0 in dhidden[b, L-1], dpos[b, 0], dneg[b, 0];
    the other examples finite."""
    d = E.nan_case()
    r = E.aux_eval(d, torch.float64)
    assert np.isnan(r["aux"][2]) and np.isfinite(np.delete(r["aux"], 2)).all()
    assert np.isnan(r["dhidden"][2, :-1]).all() and (r["dhidden"][2, -1] == 0).all()
    for n in ("dpos", "dneg"):
        assert np.isnan(r[n][2, 1:]).all() and (r[n][2, 0] == 0).all()
    for n in ("dhidden", "dpos", "dneg"):
        assert np.isfinite(np.delete(r[n], 2, 0)).all()
    for n in E.AUX_PARAMS:
        assert np.isnan(r["d" + n]).all()
