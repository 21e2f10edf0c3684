"""The inputs of tests/test_head_edges_gpu.py have the property their name claims, and the bounds
those tests state hold for a plain fp32 reference — all without a GPU."""
import numpy as np
import pytest

from oracle import ctr as OC
from oracle.metrics import keras_auc
from tests import head_edges as E


# ---- 1. activation backward + column sums ----------------------------------------------------
def test_colsum_cases_cover_every_edge():
    cases = E.COLSUM_CASES
    assert 55 <= len(cases) <= 65 and len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(E.COLSUM_N)
    assert {c[1] for c in cases} == set(E.COLSUM_B)
    for N in E.COLSUM_N:
        bs = {b for n, b, _ in cases if n == N}
        assert bs & {511, 512} and 513 in bs, f"N = {N}: no B on either side of the chunk edge"
        assert {a for n, _, a in cases if n == N} == {0, 1, 2}
    for vec in (True, False):  # every chunk count under the float4 and under the scalar kernel
        got = {E.n_chunks(b) for n, b, _ in cases if (n % 4 == 0) == vec}
        assert got >= {1, 2, 3, 4, 5, 9}, (vec, got)
    assert {E.n_chunks(b) for b in E.COLSUM_B} == {1, 2, 3, 4, 5, 9}


def test_colsum_depth_is_the_codes_chain():
    assert [E.colsum_depth(k) for k in (1, 2, 3, 4, 5, 9)] == [52, 52, 52, 52, 53, 54]


@pytest.mark.parametrize("N,B,act", [c for c in E.COLSUM_CASES if c[2] == 1])
def test_relu_outputs_hold_both_zeros(N, B, act):
    dy, y = E.colsum_inputs(N, B, act)
    assert y.dtype == np.float32 and (y >= 0).all()
    neg0 = (y == 0) & np.signbit(y)
    pos0 = (y == 0) & ~np.signbit(y)
    if y.size >= 8:
        assert neg0.any() and pos0.any() and (y > 0).any()
    if B >= 4:
        assert pos0[1].all() and neg0[2].all()
    dz = E.act_bwd_f64(dy, y, 1)
    assert (dz[y == 0] == 0).all() and (dz[y > 0] == dy[y > 0]).all()


def test_sigmoid_outputs_and_bound():
    """A plain fp32 evaluation of dy·(y·(1-y)) stays within SIGMOID_RTOL of float64."""
    for N, B, act in [c for c in E.COLSUM_CASES if c[2] == 2]:
        dy, y = E.colsum_inputs(N, B, act)
        assert ((y > 0) & (y < 1)).all()
        ref = E.act_bwd_f64(dy, y, 2)
        f32 = dy * (y * (np.float32(1) - y))
        assert (np.abs(f32 - ref) <= E.SIGMOID_RTOL * np.abs(ref)).all()


@pytest.mark.parametrize("N,B,act", E.COLSUM_CASES[::7])
def test_db_bound_holds_for_the_kernels_order_in_fp32(N, B, act):
    """The kernel's summation order, replayed in NumPy fp32, stays inside colsum_db_bound; so
    does a plain fp32 column sum."""
    dy, y = E.colsum_inputs(N, B, act)
    dz = E.act_bwd_f64(dy, y, act).astype(np.float32)
    nch = E.n_chunks(B)
    part = np.zeros((nch, N), np.float32)
    for c in range(nch):
        blk = dz[c * 512:(c + 1) * 512]
        lanes = np.zeros((16, N), np.float32)
        for r in range(blk.shape[0]):
            lanes[r % 16] += blk[r]
        for i in range(16):
            part[c] += lanes[i]
    waves = np.zeros((4, N), np.float32)
    for c in range(nch):
        waves[c % 4] += part[c]
    db = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    ref, bound = dz.astype(np.float64).sum(0), E.colsum_db_bound(dz, nch)
    assert (np.abs(db - ref) <= bound).all()
    assert (np.abs(dz.sum(0, dtype=np.float32) - ref) <= bound).all()


@pytest.mark.parametrize("N", E.COLSUM_N)
def test_v4_predicate_of_each_path(N):
    """Which kernel each of the three runs of a case takes: aligned and contiguous → float4 iff
    N % 4 == 0; one float off, or a stride that is no multiple of 4 → scalar, always."""
    for act in (0, 1, 2):
        assert E.takes_v4(N, act) == (N % 4 == 0)
        assert not E.takes_v4(N, act, dy_off=1, y_off=1, dz_off=1)
        lg, ly, lz = E.misaligned_lds(N)
        assert min(lg, ly, lz) > N and lg % 4 != 0
        assert not E.takes_v4(N, act, ld_dy=lg, ld_y=ly, ld_dz=lz)
        vg, vy, vz = E.vector_lds(N)
        assert len({vg, vy, vz}) == 3 and min(vg, vy, vz) >= N
        assert E.takes_v4(N, act, ld_dy=vg, ld_y=vy, ld_dz=vz) == (N % 4 == 0)
    # act 0 reads neither y nor dz: their alignment does not matter; dy's does
    assert E.takes_v4(4, 0, y_off=1, dz_off=1) and not E.takes_v4(4, 1, y_off=1)
    assert not E.takes_v4(4, 1, dz_off=2) and not E.takes_v4(4, 0, dy_off=3)


def test_esmm_blocks_and_groups():
    assert [sum(b) for b in E.ESMM_BLOCKS] == [20, 16, 19]
    # a block that starts at column 8 or 6 of a row of 20, 16 or 19 floats: 8 of 20 is 16-byte
    # aligned with ld % 4 == 0 (float4 for N = 12), the others are not
    assert E.takes_v4(12, 1, y_off=8, dz_off=8, ld_y=20, ld_dz=20)
    assert not E.takes_v4(10, 1, y_off=6, dz_off=6, ld_y=16, ld_dz=16)
    assert not E.takes_v4(8, 1, ld_y=19, ld_dz=19)
    assert {g * c for g, c in E.GROUP_SHAPES} == {1, 3, 6, 20, 8}


# ---- 2. batch norm ---------------------------------------------------------------------------
def test_bn_cases():
    assert len(E.BN_CASES) == 40
    assert {-(-B // E.BN_ROWS) for B in E.BN_B} == {1, 2, 3, 5}
    assert {B % E.BN_ROWS for B in E.BN_B} >= {1, 2, 3, 5, 63, 0}  # tails of 1, 2 and 3 rows


@pytest.mark.parametrize("C,B", [c for c in E.BN_CASES if c[0] >= 4])
def test_bn_structured_columns(C, B):
    d = E.bn_inputs(C, B)
    x = d["x"]
    x64 = x.astype(np.float64)
    # constant column: variance exactly 0, in float64 and in an fp32 two-pass evaluation
    assert x64[:, E.COL_CONST].var() == 0 and E.var_two_pass_f32(x)[E.COL_CONST] == 0
    # step column: constant inside every 64-row chunk, changing exactly at rows 64 and 128
    s = x[:, C - 1]
    for k in range(0, B, E.BN_ROWS):
        assert np.ptp(s[k:k + E.BN_ROWS]) == 0
    assert list(np.flatnonzero(np.diff(s)) + 1) == [r for r in (64, 128) if r < B]
    # the other columns stay ordinary
    o = np.delete(x64, [E.COL_CONST, E.COL_BIG, C - 1], axis=1)
    if B >= 63:
        assert (np.abs(o.mean(0) - 1) < 2).all() and (o.std(0) > 1.5).all()
    assert (d["gamma"] < 0).any() and (d["gamma"] > 0).any() and (np.abs(d["gamma"]) >= 0.5).all()


@pytest.mark.parametrize("B", E.BN_B)
def test_bn_big_column_bound_is_reachable_in_fp32_but_not_in_one_pass(B):
    """The variance of 1000 + 0.01·N(0,1) against 1e-5 relative of float64 plus the spread of the
    two eager fp32 samples (torch's var: about 1e-7 relative here, so the bound is the 1e-5).
    A two-pass fp32 evaluation with a mean off by δ errs by δ²: it meets the bound when its mean
    is within half an ulp of 1000 (3e-5)² / 1e-4 = 9e-6, which NumPy's fp32 sum of the raw values
    does not always deliver (figures printed); the same two passes on x - x[0], all fp32, meet it
    at every B. The one-pass E[x²] - E[x]² misses the bound by more than 100x."""
    C = 65
    d = E.bn_inputs(C, B)
    x = d["x"]
    v64 = x.astype(np.float64).var(0)[E.COL_BIG]
    assert 0 < v64 < 3e-4
    samples = E.bn_eager_samples(d, 0.0, True)
    spread = max(abs(float(s["var"][E.COL_BIG]) - v64) for s in samples)
    bound = 1e-5 * v64 + spread
    raw = abs(float(E.var_two_pass_f32(x)[E.COL_BIG]) - v64)
    two = abs(float(E.var_two_pass_f32(x - x[0])[E.COL_BIG]) - v64)
    one = abs(float(E.var_one_pass_f32(x)[E.COL_BIG]) - v64)
    print(f"  B {B}: var {v64:.4g} bound {bound:.3g} errors: two-pass shifted {two:.3g} raw {raw:.3g} "
          f"one-pass {one:.3g}")
    assert (x - x[0]).dtype == np.float32 and two <= bound
    assert one > 100 * bound


@pytest.mark.parametrize("C,B", [(65, 129), (4, 5), (129, 257)])
@pytest.mark.parametrize("training", [True, False])
def test_bn_eager_samples_bracket_float64(C, B, training):
    """The eager fallback (two row orders) agrees with the float64 restatement to fp32 rounding,
    apart from y's intrinsic term: a float mean is off by up to an ulp, which moves y by
    ulp32(mean)·invstd·|gamma|."""
    d = E.bn_inputs(C, B)
    r = E.bn_fwd_f64(d["x"], d["gamma"], d["beta"], d["mm"], d["mv"], 0.99, training)
    for s in E.bn_eager_samples(d, 0.99, training):
        tol = 1e-5 * np.abs(r["y"]) + 1e-5 + 2 * E.ulp32(r["mean"]) * r["invstd"] * np.abs(d["gamma"])
        assert (np.abs(s["y"] - r["y"]) <= tol).all()
        np.testing.assert_allclose(s["mm"], r["mm"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(s["mv"], r["mv"], rtol=1e-4, atol=1e-6)


def test_bn_bwd_restatement_is_the_gradient():
    """bn_bwd with the true batch statistics is the gradient of the forward (autograd, float64);
    its fp32 evaluations are close to it."""
    import torch

    d = E.bn_inputs(65, 129)
    x = torch.from_numpy(d["x"]).double().requires_grad_()
    g = torch.from_numpy(d["gamma"]).double().requires_grad_()
    b = torch.from_numpy(d["beta"]).double().requires_grad_()
    mean, var = x.mean(0), x.var(0, unbiased=False)
    y = (x - mean) * torch.rsqrt(var + E.BN_EPS) * g + b
    y.backward(torch.from_numpy(d["dy"]).double())
    r = 1.0 / np.sqrt(var.detach().numpy() + E.BN_EPS)
    got = E.bn_bwd(d["dy"], d["x"], mean.detach().numpy(), r, d["gamma"], True)
    np.testing.assert_allclose(got["dx"], x.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got["dgamma"], g.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got["dbeta"], b.grad.numpy(), rtol=1e-9, atol=1e-9)
    f32 = E.bn_bwd(d["dy"], d["x"], mean.detach().numpy().astype(np.float32), r.astype(np.float32),
                   d["gamma"], True, np.float32, np.random.default_rng(0).permutation(129))
    assert f32["dx"].dtype == np.float32
    ordinary = [c for c in range(65) if c != E.COL_BIG]
    np.testing.assert_allclose(f32["dgamma"][ordinary], got["dgamma"][ordinary], rtol=1e-4, atol=1e-4)


# ---- 3. BCE ----------------------------------------------------------------------------------
def test_bce_planted_values_sit_on_the_clip_edges():
    e, h = E.BCE_EPS, E.BCE_HI
    p = E.bce_planted()
    assert p.dtype == np.float32 and len(p) == 9
    assert float(h) == 0.9999998807907104 and h == np.float32(0.99999988)
    assert p[2] == e and p[3] < e and np.nextafter(p[3], np.float32(1)) == e
    assert p[4] == h and p[5] > h and np.nextafter(p[5], np.float32(0)) == h
    inside = (p >= e) & (p <= h)
    assert list(inside) == [False, False, True, False, True, False, True, False, False]
    for y in (0.0, 1.0, 0.3):
        d, _ = E.bce_grad_f64(p, np.full(9, y, np.float32))
        assert (d[~inside] == 0).all() and (d[inside] != 0).all()


def test_bce_sizes_reach_the_block_caps():
    """2^20: the forward's 1024 blocks exactly, the pass count of smaller sizes; 2^20 + 1: one
    more grid-stride pass; 2^21 + 5: the backward's 2048 blocks and one more pass."""
    f = {n: (E.bce_fwd_blocks(n), E.bce_passes(n, E.bce_fwd_blocks(n))) for n in E.BCE_N if n}
    assert f[1025] == (2, 3) and f[1024] == (1, 4)
    assert f[2 ** 20] == (1024, 4) and f[2 ** 20 + 1] == (1024, 5)
    b = {n: (E.bce_bwd_blocks(n), E.bce_passes(n, E.bce_bwd_blocks(n))) for n in E.BCE_N if n}
    assert b[2 ** 20 + 1] == (1025, 4) and b[2 ** 21 + 5] == (2048, 5)
    assert E.bce_sum_depth(1) == 10 and E.bce_sum_depth(2 ** 20 + 1) == 5 + 8 + 1024


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("n", [1, 257, 1025, 2 ** 20 + 1])
def test_bce_bounds_hold_for_plain_fp32(n, soft):
    """The restatement equals oracle.ctr.bce; an fp32 NumPy evaluation of the kernel's formula
    meets the per-element bound, its fp32 sum the sum bound, its gradient the gradient bound."""
    p, y, g, pos = E.bce_inputs(n, soft)
    assert len(pos) == min(n, 9) and (p[pos] == E.bce_planted()[: len(pos)]).all()
    l64 = E.bce_f64(p, y)
    np.testing.assert_allclose(l64, OC.bce(y.astype(np.float64), p.astype(np.float64)), rtol=1e-6,
                               atol=1e-7)  # the oracle's eps is the double 1e-7
    e, one = E.BCE_EPS, np.float32(1)
    pc = np.minimum(np.maximum(p, e), one - e)
    l32 = -(y * np.log(pc + e) + (one - y) * np.log((one - pc) + e))
    assert l32.dtype == np.float32 and (np.abs(l32 - l64) <= E.bce_elem_tol(l64)).all()
    assert abs(float(l32.sum(dtype=np.float32)) - l64.sum()) <= E.bce_sum_tol(l64)
    d64, mag = E.bce_grad_f64(p, y)
    d32 = (-(y / (pc + e)) + (one - y) / ((one - pc) + e)) * ((p >= e) & (p <= one - e))
    assert (np.abs(g * d32 - g.astype(np.float64) * d64) <= E.BCE_RTOL * np.abs(g) * mag).all()
    if soft:
        assert (y[::3] == np.float32(0.3)).all()
    else:
        assert set(np.unique(y)) <= {0.0, 1.0}


def test_bce_nan_is_nan_in_the_oracle():
    p = np.array([0.3, np.nan, 0.9])
    y = np.array([1.0, 0.0, 0.3])
    assert list(np.isnan(OC.bce(y, p))) == [False, True, False]
    assert list(np.isnan(OC.bce_grad(y, p))) == [False, True, False]
    l = E.bce_f64(p.astype(np.float32), y.astype(np.float32))
    d, _ = E.bce_grad_f64(p.astype(np.float32), y.astype(np.float32))
    assert list(np.isnan(l)) == [False, True, False] and list(np.isnan(d)) == [False, True, False]


# ---- 4. AUC ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", E.AUC_T)
def test_auc_inputs_sit_on_the_thresholds(T):
    from recommender_amd.metrics import keras_thresholds

    thr = E.keras_thresholds(T)
    assert thr.dtype == np.float32 and np.array_equal(thr, keras_thresholds(T))
    assert (np.diff(thr) > 0).all(), "thresholds not strictly increasing"
    p, y, neg, pos, roc = E.auc_reference(T)
    assert p.size == 3 * (T - 2) + 3 and ((p >= 0) & (p <= 1)).all()
    assert np.isin(thr[1:-1], p).all() and np.signbit(p[p == 0]).any()
    assert set(np.unique(y)) == set(E.AUC_LABELS.tolist()) or p.size < 5
    # the bucket of every prediction under the literal comparison: #thresholds < p. A prediction
    # equal to a threshold lies in the bucket below the one its upper neighbour lies in
    bucket = (thr[None, :] < p[:, None]).sum(1) if T <= 200 else None
    if bucket is not None:
        assert np.array_equal(np.bincount(bucket[y != 0], minlength=T + 1), pos)
        assert np.array_equal(np.bincount(bucket[y == 0], minlength=T + 1), neg)
        for i in range(1, T - 1):
            assert bucket[p == thr[i]][0] == i
            assert bucket[p == np.nextafter(thr[i], np.float32(2))][0] == i + 1
            assert bucket[p == np.nextafter(thr[i], np.float32(-1))][0] == i
    assert neg.sum() + pos.sum() == p.size and pos.sum() == (y != 0).sum()
    assert neg[0] == 0 and pos[0] == 0 and neg[T] + pos[T] == 0  # all in range
    assert neg[1] + pos[1] >= 2 + (T > 2)  # 0, -0.0 (and the first threshold's lower neighbour)
    assert 0.0 <= roc <= 1.0


@pytest.mark.parametrize("T", [2, 3, 200])
def test_auc_literal_counts_are_the_oracles(T):
    """literal_tp_fp (chunked) and the trapezoid equal oracle.metrics.keras_auc; at T = 20000 on a
    sample of the predictions (the whole matrix would hold 1.2e9 entries)."""
    p, y, neg, pos, roc = E.auc_reference(T)
    ref, tp, fp = keras_auc(y, p, T)
    got_tp, got_fp = E.literal_tp_fp(p, y, E.keras_thresholds(T), chunk=97)
    assert np.array_equal(got_tp, tp.astype(np.int64)) and np.array_equal(got_fp, fp.astype(np.int64))
    assert abs(roc - ref) < 1e-15
    # buckets → cumulative → buckets
    assert np.array_equal(np.cumsum(pos[::-1])[::-1][1:], got_tp)


def test_auc_literal_counts_at_20000_on_a_sample():
    p, y, *_ = E.auc_reference(20000)
    ps, ys = p[::29], y[::29]
    ref, tp, fp = keras_auc(ys, ps, 20000)
    got_tp, got_fp = E.literal_tp_fp(ps, ys, E.keras_thresholds(20000))
    assert np.array_equal(got_tp, tp.astype(np.int64)) and np.array_equal(got_fp, fp.astype(np.int64))
    assert abs(E.roc_from_tp_fp(got_tp, got_fp, int((ys != 0).sum()), int((ys == 0).sum())) - ref) < 1e-15


def test_auc_searchsorted_would_not_tell_the_comparisons_apart():
    """Why the reference is the literal matrix: on these inputs a search with `<=` (side =
    'right') moves every on-threshold prediction one bucket up."""
    p, y, neg, pos, _ = E.auc_reference(200)
    thr = E.keras_thresholds(200)
    left, right = np.searchsorted(thr, p, side="left"), np.searchsorted(thr, p, side="right")
    assert np.array_equal(np.flatnonzero(left != right), np.flatnonzero(np.isin(p, thr)))
    assert (left != right).sum() == 198
    assert not np.array_equal(np.bincount(right[y != 0], minlength=201), pos)


def test_tie_heavy_input():
    p, y = E.tie_heavy()
    assert np.unique(p).size <= 12 and np.isin(p, E.keras_thresholds(200)).mean() > 0.2
    assert 0.2 < y.mean() < 0.8 and ((p >= 0) & (p <= 1)).all()
