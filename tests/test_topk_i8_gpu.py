"""rs_quantize_rows_i8, rs_topk_ip_i8 and rs_rerank_ip on the GPU against tests/topk_i8_ref.py
(the contract restated in NumPy), items exactly and key / score bits: the quantiser at its width
and row-kind edges, the int8 MFMA scan at its 16-byte fragment, K = 32 chunk, tile, round and
split edges, the re-rank against rs_topk_ip restricted to the candidate set, the planted exact
case end to end against rs_topk_ip, and the Python surfaces. Every call goes through the C entry
point with 64 guard elements behind each output, and is run twice and compared bit for bit."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import topk_i8_ref as T
from tests import topk_ip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
GUARD_ITEM = 0x5A5A5A5A
GUARD_SCORE = 0x7FC12345  # a NaN with a payload
GUARD_BYTE = 0x5A


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).to(DEV)


def padded(a, ld):
    """a's rows at stride ld, NaN in between (the kernel must not read the padding)."""
    if ld is None:
        return np.ascontiguousarray(a, f32), a.shape[1]
    out = np.full((a.shape[0], ld), np.nan, f32)
    out[:, :a.shape[1]] = a
    return out, ld


def at_offset(flat_u8, offset):
    """A device copy of a byte array that starts `offset` bytes into a 16-byte aligned buffer."""
    buf = torch.full((flat_u8.size + offset + 16,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[offset:offset + flat_u8.size] = dev(flat_u8)
    return buf, buf[offset:]


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        if x is not None:
            assert x.dtype == y.dtype and (x.view(np.uint8) == y.view(np.uint8)).all()
    return a


# ---- rs_quantize_rows_i8 -----------------------------------------------------------------
def quant_call(x, ld=None, c_ld=None, offset=0, flag=True, expect=0):
    """→ (codes int8 [n, c_ld], scales [n], flag value or None); guards checked. offset: codes
    starts that many bytes into its buffer (4: misaligned for 16-byte stores)."""
    def run():
        lib = L.lib()
        n, dim = x.shape
        xa, ld_ = padded(x, ld)
        cl = T.row_bytes(dim) if c_ld is None else c_ld
        tx = dev(xa)
        cbuf = torch.full((n * cl + offset + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        sc = torch.full((n + GUARD,), GUARD_SCORE, dtype=torch.int32, device=DEV)
        fl = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
        st = lib.rs_quantize_rows_i8(L.ptr(tx), ld_, n, dim, L.ptr(cbuf[offset:]), cl, L.ptr(sc),
                                     L.ptr(fl) if flag else None, L.stream_ptr(tx.device))
        torch.cuda.synchronize()
        assert st == expect, (st, lib.rs_last_error())
        c, s, f = cbuf.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()
        assert (c[:offset] == GUARD_BYTE).all() and (c[offset + n * cl:] == GUARD_BYTE).all()
        assert (s[n:] == GUARD_SCORE).all() and not f[1:].any()
        return (c[offset:offset + n * cl].view(np.int8).reshape(n, cl), s[:n].view(f32),
                f[:1] if flag else None)
    return twice(run)


def check_quant(x, **kw):
    """Both access widths against the restatement: codes, zero padding, scales, the flag."""
    rc, rs, bad = T.quantize_ref(x)
    dim = x.shape[1]
    for off in (0, 4):
        c, s, f = quant_call(x, offset=off, **kw)
        np.testing.assert_array_equal(c[:, :dim], rc)
        assert not c[:, dim:].any()
        assert (s.view(np.uint32) == rs.view(np.uint32)).all()
        if f is not None:
            assert f[0] == (L.RS_ERRBIT_NONFINITE if bad.any() else 0)


def row_kinds(dim):
    """Rows of every kind at one width: zero, constant, one element, ±amax ties, subnormal,
    exact .5 quotients, random."""
    tiny = f32(2.0 ** -149)
    x = R.random_floats(dim, 24, dim)
    x[0] = 0
    x[2] = -3.25
    x[3] = 0
    x[3, dim - 1] = -1e-3
    x[4, 0], x[4, dim - 1] = 7.5, -7.5
    x[5] = tiny * f32(190) * np.sign(x[5])
    x[6] = np.arange(dim, dtype=f32) % 5 * tiny
    x[7] = (np.arange(dim) % 255 - 127) * 0.5
    x[7, 0] = 127
    x[8] = -0.0
    return x


@pytest.mark.parametrize("dim", T.QUANT_DIMS)
def test_quantise_every_row_kind_at_every_width(dim):
    check_quant(row_kinds(dim))


@pytest.mark.parametrize("dim,ld,c_ld", [(3, 5, 4), (17, 20, 20), (17, 17, 48), (33, 64, 36),
                                         (129, 131, 160), (255, 256, 256)])
def test_quantise_strides_above_the_minimum(dim, ld, c_ld):
    """c_ld % 16 != 0 takes the 4-byte stores at any base; the whole row [dim, c_ld) reads 0."""
    check_quant(row_kinds(dim), ld=ld, c_ld=c_ld)


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 4097])
def test_quantise_row_counts(n_rows):
    check_quant(R.random_floats(n_rows + 3, n_rows, 20))


def test_quantise_nonfinite_rows_set_the_flag_or_not_with_a_null_flag():
    x = row_kinds(33)
    x[1, 5], x[9, 32], x[10, 0] = np.nan, np.inf, -np.inf
    check_quant(x)
    check_quant(x, flag=False)
    c, s, _ = quant_call(x)
    assert not c[[1, 9, 10]].any() and not s[[1, 9, 10]].any()


# ---- rs_topk_ip_i8 -----------------------------------------------------------------------
def scan_call(q, codes, scales, kc, excl=None, excl_base=0, excl_one=None, n_splits=1, q_ld=None,
              offset=0, with_keys=True, ws_bytes=None, expect=0):
    """rs_topk_ip_i8 → (items [Q, kc], keys [Q, kc] or None) as NumPy; guards checked. codes is
    int8 [n, c_ld], padding included; offset: it starts that many bytes into its buffer."""
    def run():
        lib = L.lib()
        nq, dim = q.shape
        n_items, c_ld = codes.shape
        qa, q_ld_ = padded(q, q_ld)
        tq = dev(qa)
        _, tc = at_offset(np.ascontiguousarray(codes).view(np.uint8).reshape(-1), offset)
        ts = dev(np.append(scales, f32(np.nan)), f32)
        ip = it = None
        if excl is not None:
            ip, it = dev(excl[0], np.int64), dev(np.append(excl[1], 0), np.int32)
        one = dev(excl_one, np.int32)
        oi = torch.full((nq * kc + GUARD,), GUARD_ITEM, dtype=torch.int32, device=DEV)
        ok = torch.full((nq * kc + GUARD,), GUARD_SCORE, dtype=torch.int32, device=DEV)
        need = lib.rs_topk_ip_i8_workspace_size(nq, n_items, kc, n_splits)
        wb = need if ws_bytes is None else ws_bytes
        ws = torch.full((wb + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
        st = lib.rs_topk_ip_i8(L.ptr(tq), q_ld_, nq, L.ptr(tc), c_ld, L.ptr(ts), n_items, dim,
                               excl_base, L.ptr(ip), L.ptr(it), L.ptr(one), kc, n_splits,
                               L.ptr(oi), L.ptr(ok) if with_keys else None,
                               L.ptr(ws) if wb else None, wb, L.stream_ptr(oi.device))
        torch.cuda.synchronize()
        assert st == expect, (st, lib.rs_last_error())
        oi_, ok_, ws_ = oi.cpu().numpy(), ok.cpu().numpy(), ws.cpu().numpy()
        assert (oi_[nq * kc:] == GUARD_ITEM).all() and (ok_[nq * kc:] == GUARD_SCORE).all()
        assert (ws_[wb:] == 0xAB).all()
        if st != 0:
            assert (oi_ == GUARD_ITEM).all() and (ok_ == GUARD_SCORE).all()  # nothing written
            return None, None
        if not with_keys:
            assert (ok_ == GUARD_SCORE).all()
        return (oi_[:nq * kc].reshape(nq, kc),
                ok_[:nq * kc].view(f32).reshape(nq, kc) if with_keys else None)
    return twice(run) if expect == 0 else run()


def check_scan(q, codes, scales, kc, ref=None, widths=(0, 4), **kw):
    """The call against scan_ref (or a precomputed ref) at both access widths (a base 4 bytes off
    takes the 4-byte loads), items exactly and keys bit for bit."""
    dim = q.shape[1]
    ref_kw = {n: kw[n] for n in ("excl", "excl_base", "excl_one") if n in kw}
    ri, rk = ref if ref is not None else T.scan_ref(q, codes[:, :dim], scales, kc, **ref_kw)
    for off in widths:
        gi, gk = scan_call(q, codes, scales, kc, offset=off, **kw)
        np.testing.assert_array_equal(gi, ri)
        if gk is not None:
            assert R.same_scores(gk, rk), np.argwhere(gk.view(np.uint32) != rk.view(np.uint32))[:5]
    return ri, rk


@pytest.mark.parametrize("dim", T.DIMS)
def test_scan_at_every_fragment_and_chunk_edge(dim):
    """kc = 64 of 129 items over two ranges, garbage in the padding bytes and NaN in the padding
    columns; every int8 value occurs in the codes."""
    q = R.random_floats(dim, 33, dim)
    codes, scales = T.coded_catalogue(dim + 1, 129, dim)
    check_scan(q, codes, scales, 64, n_splits=2, q_ld=dim + 3)


@pytest.mark.parametrize("dim,c_ld", [(17, 48), (17, 20), (33, 36), (160, 164), (255, 256)])
def test_scan_code_strides_above_the_minimum(dim, c_ld):
    q = T.small_int_queries(dim, 33, dim)
    codes, scales = T.coded_catalogue(dim + 2, 70, dim, c_ld=c_ld)
    check_scan(q, codes, scales, 10)


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 65])
def test_scan_query_counts(nq):
    q = R.random_floats(nq, nq, 33)
    codes, scales = T.coded_catalogue(3, 200, 33)
    check_scan(q, codes, scales, 10)


@pytest.mark.parametrize("n_items", [0, 1, 31, 32, 33, 127, 128, 129, 513])
def test_scan_item_counts_around_a_tile_and_a_round(n_items):
    q = R.random_floats(n_items, 33, 17, extremes=False)
    codes, scales = T.coded_catalogue(7, n_items, 17)
    ref = check_scan(q, codes, scales, 10)
    if 0 < n_items <= 33:
        check_scan(q, codes, scales, 10, ref=ref, n_splits=n_items)  # one item per range
    if n_items == 0:
        assert (ref[0] == -1).all() and (ref[1] == -np.inf).all()


@pytest.fixture(scope="module")
def cat3000():
    """33 queries over 3000 coded items at dim 64 and their best 64: shared, never changed."""
    q = R.random_floats(61, 33, 64, extremes=False)
    codes, scales = T.coded_catalogue(62, 3000, 64)
    ri, rk = T.scan_ref(q, codes, scales, 64)
    for a in (q, codes, scales, ri, rk):
        a.setflags(write=False)
    return q, codes, scales, ri, rk


@pytest.mark.parametrize("n_splits", [0, 1, 2, 7])
def test_scan_three_thousand_items_by_split_count(cat3000, n_splits):
    q, codes, scales, ri, rk = cat3000
    check_scan(q, codes, scales, 64, ref=(ri, rk), n_splits=n_splits)


@pytest.mark.parametrize("kc", [1, 10, 63, 64])
def test_scan_kc_values_and_prefix(cat3000, kc):
    q, codes, scales, ri, rk = cat3000
    check_scan(q, codes, scales, kc, ref=(ri[:, :kc], rk[:, :kc]), n_splits=2)


def test_scan_a_query_alone_and_inside_a_batch(cat3000):
    q, codes, scales, ri, rk = cat3000
    for r in (0, 31, 32):
        check_scan(q[r:r + 1], codes, scales, 64, ref=(ri[r:r + 1], rk[r:r + 1]), widths=(0,))


def test_scan_largest_integer_scores():
    """All +127, all -127 and all -128 code rows at dim 256 against ±127 queries: a dropped,
    doubled or mis-permuted K fragment changes |I| = 256 * 127 * 128."""
    q, codes, scales = T.extreme_codes()
    ri, rk = check_scan(q, codes, scales, 64)
    assert ri[0, 0] == 0 and rk[0, 0] == 256 * 127 * 127 and ri[1, 0] == 2
    assert rk[1, 0] == 256 * 127 * 128 and ri[0, -1] == 2 and rk[0, -1] == -256 * 127 * 128


def test_scan_one_hot_queries_check_every_k_position():
    q, codes, scales = T.one_hot_case()
    check_scan(q, codes, scales, 64)


@pytest.mark.parametrize("n_splits", [1, 2, 7])
def test_scan_equal_keys_across_tiles_rounds_and_splits(n_splits):
    q, codes, scales = T.tie_case()
    check_scan(q, codes, scales, 10, n_splits=n_splits)
    check_scan(q, codes, scales, 64, n_splits=n_splits, widths=(0,))


def test_scan_special_scales():
    q, codes, scales = T.special_scales()
    for kc in (5, 64):
        check_scan(q, codes, scales, kc)
    check_scan(q, codes, scales, 40, n_splits=3)


def test_scan_zero_and_nan_query_rows_give_the_items_in_ascending_order():
    codes, scales = T.coded_catalogue(23, 300, 20)
    q = R.random_floats(24, 4, 20, extremes=False)
    q[1] = 0
    q[2, 7] = np.nan
    q[3] = f32(2.0 ** -149)  # amax / 127 rounds to 0
    ri, rk = check_scan(q, codes, scales, 10, n_splits=2)
    for r in (1, 2, 3):
        np.testing.assert_array_equal(ri[r], np.arange(10))
        assert (rk[r] == 0).all()


def test_scan_fewer_than_kc_candidates():
    q = R.random_floats(30, 5, 16)
    codes, scales = T.coded_catalogue(31, 40, 16)
    ri, rk = check_scan(q, codes, scales, 64, n_splits=3)
    assert (ri[:, 40:] == -1).all() and (rk[:, 40:] == -np.inf).all()


@pytest.fixture(scope="module")
def excl_case():
    n_items, kc = 100, 10
    q1 = R.random_floats(5, 1, 18, extremes=False)
    codes, scales = T.coded_catalogue(6, n_items, 18)
    top, _ = T.scan_ref(q1, codes[:, :18], scales, kc)
    rows = R.exclusion_rows(top[0], n_items, kc)
    return np.repeat(q1, len(rows), 0), codes, scales, rows, kc


def test_scan_exclusion_rows(excl_case):
    """One query five times against: an empty row, every item, exactly its best kc, an unsorted
    row with duplicates and out-of-range ids, all but kc - 1 items."""
    q, codes, scales, rows, kc = excl_case
    ri, rk = check_scan(q, codes, scales, kc, excl=R.csr(rows))
    assert (ri[1] == -1).all() and (rk[1] == -np.inf).all()
    assert not set(ri[2]) & set(ri[0])
    assert (ri[4, :kc - 1] >= 0).all() and ri[4, kc - 1] == -1
    check_scan(q, codes, scales, kc, excl=R.csr(rows), n_splits=3)


def test_scan_exclusion_base_and_exclude_one(excl_case):
    q, codes, scales, rows, kc = excl_case
    shifted = R.csr([[1, 2, 3], [], [4]] + rows)
    check_scan(q, codes, scales, kc, excl=shifted, excl_base=3)
    top = check_scan(q, codes, scales, kc)[0][0]
    one = np.array([top[0], -1, top[1], 10 ** 6, top[0]], np.int32)
    ri, _ = check_scan(q, codes, scales, kc, excl_one=one)
    assert ri[0, 0] == top[1] and ri[1, 0] == top[0] and ri[3, 0] == top[0]
    check_scan(q, codes, scales, kc, excl=R.csr(rows), excl_one=one, n_splits=2)


def test_scan_long_exclusion_rows_over_many_rounds(cat3000):
    q, codes, scales, ri, _ = cat3000
    rng = np.random.default_rng(8)
    rows = [list(rng.permutation(np.concatenate([ri[r], rng.integers(0, 3000, 236)])))
            for r in range(33)]
    check_scan(q, codes, scales, 10, excl=R.csr(rows), n_splits=7, widths=(0,))


def test_scan_without_keys(cat3000):
    q, codes, scales, ri, _ = cat3000
    for n_splits in (1, 7):
        gi, none = scan_call(q, codes, scales, 64, n_splits=n_splits, with_keys=False)
        assert none is None
        np.testing.assert_array_equal(gi, ri)


def test_scan_argument_errors_write_nothing():
    q = R.random_floats(1, 5, 8)
    codes, scales = T.coded_catalogue(2, 50, 8)
    bad = L.RS_E_INVALID
    for kw in (dict(kc=0), dict(kc=65), dict(n_splits=51), dict(n_splits=-1),
               dict(n_splits=2, ws_bytes=16), dict(offset=2)):
        scan_call(q, codes, scales, kw.pop("kc", 10), expect=bad, **kw)
    scan_call(q, codes[:, :10], scales, 10, expect=bad)  # c_ld % 4 != 0
    scan_call(q, codes[:, :4], scales, 10, expect=bad)   # c_ld < dim
    lib = L.lib()
    tq, tc, ts = dev(q), dev(codes), dev(scales)
    oi = torch.full((50,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    s = L.stream_ptr(oi.device)

    def args(a, b, c, o, dim=8, n=50):
        return (a, 8, 5, b, 16, c, n, dim, 0, None, None, None, 10, 1, o, None, None, 0, s)

    full = (L.ptr(tq), L.ptr(tc), L.ptr(ts), L.ptr(oi))
    for hole in range(4):
        assert lib.rs_topk_ip_i8(*args(*[None if i == hole else p
                                         for i, p in enumerate(full)])) == bad
    assert lib.rs_topk_ip_i8(*args(*full, dim=0)) == bad
    assert lib.rs_topk_ip_i8(*args(*full, dim=257)) == bad
    assert lib.rs_topk_ip_i8(*args(*full, n=2 ** 31)) == bad
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == GUARD_ITEM).all()
    assert b"rs_topk_ip_i8" in lib.rs_last_error()
    gi, _ = scan_call(q[:0], codes, scales, 10)
    assert gi.shape == (0, 10)


def test_scan_captured_in_a_graph_and_replayed_on_refilled_queries():
    from recommender_amd.functional import topk_inner_product_i8

    codes, scales = T.coded_catalogue(41, 3000, 36, garbage=False)
    q1, q2 = R.random_floats(42, 37, 36), R.random_floats(43, 37, 36)
    tq, tc, ts = dev(q1).clone(), dev(codes), dev(scales)
    topk_inner_product_i8(tq, tc, ts, 10)  # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx, key = topk_inner_product_i8(tq, tc, ts, 10)
    for qq in (q1, q2, q1):
        tq.copy_(dev(qq))
        g.replay()
        torch.cuda.synchronize()
        ri, rk = T.scan_ref(qq, codes[:, :36], scales, 10)
        np.testing.assert_array_equal(idx.cpu().numpy(), ri)
        assert R.same_scores(key.cpu().numpy(), rk)


# ---- rs_rerank_ip ------------------------------------------------------------------------
def rerank_call(q, x, cand, k, q_ld=None, i_ld=None, with_scores=True, expect=0):
    def run():
        lib = L.lib()
        nq, dim = q.shape
        qa, q_ld_ = padded(q, q_ld)
        xa, i_ld_ = padded(x, i_ld)
        tq, tx, tcand = dev(qa), dev(xa), dev(cand, np.int32)
        kc = cand.shape[1]
        oi = torch.full((nq * k + GUARD,), GUARD_ITEM, dtype=torch.int32, device=DEV)
        os_ = torch.full((nq * k + GUARD,), GUARD_SCORE, dtype=torch.int32, device=DEV)
        st = lib.rs_rerank_ip(L.ptr(tq), q_ld_, nq, L.ptr(tx), i_ld_, x.shape[0], dim,
                              L.ptr(tcand), kc, k, L.ptr(oi), L.ptr(os_) if with_scores else None,
                              L.stream_ptr(oi.device))
        torch.cuda.synchronize()
        assert st == expect, (st, lib.rs_last_error())
        oi_, os__ = oi.cpu().numpy(), os_.cpu().numpy()
        assert (oi_[nq * k:] == GUARD_ITEM).all() and (os__[nq * k:] == GUARD_SCORE).all()
        if st != 0:
            assert (oi_ == GUARD_ITEM).all() and (os__ == GUARD_SCORE).all()
            return None, None
        if not with_scores:
            assert (os__ == GUARD_SCORE).all()
        return (oi_[:nq * k].reshape(nq, k),
                os__[:nq * k].view(f32).reshape(nq, k) if with_scores else None)
    return twice(run) if expect == 0 else run()


def topk_ip_call(q, x, k):
    """The existing exhaustive call, through its C entry point."""
    lib = L.lib()
    nq, dim = q.shape
    tq, tx = dev(q, f32), dev(x, f32)
    oi = torch.empty(nq * k, dtype=torch.int32, device=DEV)
    os_ = torch.empty(nq * k, device=DEV)
    st = lib.rs_topk_ip(L.ptr(tq), dim, nq, L.ptr(tx), dim, x.shape[0], dim, 0, None, None, None,
                        k, 1, L.ptr(oi), L.ptr(os_), None, 0, L.stream_ptr(oi.device))
    torch.cuda.synchronize()
    assert st == 0, lib.rs_last_error()
    return oi.cpu().numpy().reshape(nq, k), os_.cpu().numpy().reshape(nq, k)


def restricted_topk(q, x, cand, k):
    """rs_topk_ip of every query over the catalogue restricted to its valid candidates (distinct
    ids, ascending, so the restricted row number orders like the id), mapped back to ids."""
    out_i = np.full((q.shape[0], k), -1, np.int32)
    out_s = np.full((q.shape[0], k), -np.inf, f32)
    for r in range(q.shape[0]):
        ids = np.unique(cand[r][(cand[r] >= 0) & (cand[r] < x.shape[0])])
        if not ids.size:
            continue
        gi, gs = topk_ip_call(q[r:r + 1], x[ids], k)
        out_i[r] = np.where(gi[0] >= 0, ids[np.maximum(gi[0], 0)], -1)
        out_s[r] = gs[0]
    return out_i, out_s


@pytest.mark.parametrize("dim", T.DIMS)
def test_rerank_equals_topk_ip_restricted_to_the_candidates(dim):
    """Distinct candidates with -1 and out-of-range entries among them, random floats with
    subnormal and 1e30 rows: items and score bits of the existing kernel, and the restatement."""
    rng = np.random.default_rng(dim)
    q, x = R.random_floats(dim, 6, dim), R.random_floats(dim + 1, 90, dim)
    for kc in (1, 33, 64):
        cand = np.stack([rng.permutation(90)[:kc] for _ in range(6)]).astype(np.int32)
        cand[rng.random(cand.shape) < 0.15] = -1
        cand[rng.random(cand.shape) < 0.05] = 90 + kc
        k = min(10, kc)
        gi, gs = rerank_call(q, x, cand, k, q_ld=dim + 1, i_ld=dim + 5)
        ri, rs = restricted_topk(q, x, cand, k)
        np.testing.assert_array_equal(gi, ri)
        assert R.same_scores(gs, rs)
        ti, ts = T.rerank_ref(q, x, cand, k)
        np.testing.assert_array_equal(gi, ti)
        assert R.same_scores(gs, ts)


def test_rerank_repeated_ids_special_scores_and_no_scores():
    q, x = R.special_catalogue()
    x[5, 0], q[0, 2], x[6, 2] = -0.0, 1e-30, -1e-30  # a chain that ends at -0
    cand = np.tile(np.array([3, 12, 7, 7, 20, 33, -1, 12, 5, 6, 40, 2 ** 31 - 1, 0, 3], np.int32),
                   (3, 1))
    for k in (1, 5, 14):
        gi, gs = rerank_call(q, x, cand, k)
        ti, ts = T.rerank_ref(q, x, cand, k)
        np.testing.assert_array_equal(gi, ti)
        assert R.same_scores(gs, ts)
    gi2, none = rerank_call(q, x, cand, 14, with_scores=False)
    assert none is None
    np.testing.assert_array_equal(gi2, gi)
    assert list(gi[0][:2]) == [3, 3] and (gi[0] == 7).sum() == 2  # repeats stay repeated


def test_rerank_argument_errors_write_nothing():
    q, x = R.random_floats(1, 5, 8), R.random_floats(2, 50, 8)
    cand = np.zeros((5, 10), np.int32)
    bad = L.RS_E_INVALID
    rerank_call(q, x, cand, 0, expect=bad)
    rerank_call(q, x, cand, 11, expect=bad)
    rerank_call(q, x, np.zeros((5, 65), np.int32), 10, expect=bad)
    lib = L.lib()
    tq, tx, tc = dev(q), dev(x), dev(cand)
    oi = torch.full((25,), GUARD_ITEM, dtype=torch.int32, device=DEV)
    s = L.stream_ptr(oi.device)

    def args(a, b, c, o, q_ld=8, i_ld=8, dim=8, n=50):
        return (a, q_ld, 5, b, i_ld, n, dim, c, 10, 5, o, None, s)

    full = (L.ptr(tq), L.ptr(tx), L.ptr(tc), L.ptr(oi))
    for hole in range(4):
        assert lib.rs_rerank_ip(*args(*[None if i == hole else p
                                        for i, p in enumerate(full)])) == bad
    for kw in (dict(q_ld=7), dict(i_ld=7), dict(dim=0), dict(dim=257), dict(n=2 ** 31)):
        assert lib.rs_rerank_ip(*args(*full, **kw)) == bad
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == GUARD_ITEM).all()
    assert b"rs_rerank_ip" in lib.rs_last_error()
    gi, _ = rerank_call(q[:0], x, cand[:0], 5)
    assert gi.shape == (0, 5)


# ---- the planted exact case, end to end against the existing kernel ---------------------------
@pytest.mark.parametrize("dim", [16, 64, 160, 256])
def test_planted_exact_scan_then_rerank_equals_topk_ip(dim):
    x, q = T.planted_exact(dim, 513, dim), T.planted_exact(dim + 1, 33, dim)
    codes, scales, _ = quant_call(x)
    assert (scales == 1).all()
    exact = {k: topk_ip_call(q, x, k) for k in (1, 10, 64)}
    for k in (1, 10, 64):
        for kc in sorted({k, 64}):
            ci, ck = scan_call(q, codes, scales, kc, n_splits=2)
            gi, gs = rerank_call(q, x, ci, k)
            np.testing.assert_array_equal(gi, exact[k][0])
            assert R.same_scores(gs, exact[k][1])
            if kc == k:
                assert R.same_scores(ck + f32(0), exact[k][1] + f32(0))  # key == score


# ---- the Python surfaces -----------------------------------------------------------------
def test_int8_index_search_state_dict_and_the_c_calls():
    from recommender_amd.functional import (quantize_rows_i8, rerank_inner_product,
                                            topk_inner_product_i8)
    from recommender_amd.retrieval import Int8Index

    x, q = R.random_floats(1, 500, 36, extremes=False), R.random_floats(2, 40, 36, extremes=False)
    index = Int8Index.from_float(dev(x))
    assert index.n_items == 500 and index.dim == 36
    rc, rs, _ = T.quantize_ref(x)
    assert index.codes.dtype == torch.int8 and tuple(index.codes.shape) == (500, 48)
    np.testing.assert_array_equal(index.codes.cpu().numpy()[:, :36], rc)
    np.testing.assert_array_equal(index.scales.cpu().numpy(), rs)
    codes, scales = quantize_rows_i8(dev(x))
    assert torch.equal(codes, index.codes) and torch.equal(scales, index.scales)
    one = np.arange(40, dtype=np.int32)
    rows = [[int(i) for i in np.random.default_rng(r).integers(0, 500, r % 7)] for r in range(43)]
    ip, it = R.csr(rows)
    kw = dict(exclude=(dev(ip), dev(it)), exclude_base=3, exclude_one=dev(one))
    idx, val = index.search(dev(q), 10, n_candidates=32, **kw)
    ci, ck = T.scan_ref(q, rc, rs, 32, excl=(ip, it), excl_base=3, excl_one=one)
    cand, keys = topk_inner_product_i8(dev(q), index.codes, index.scales, 32, n_splits=3, **kw)
    np.testing.assert_array_equal(cand.cpu().numpy(), ci)
    assert R.same_scores(keys.cpu().numpy(), ck)
    ri, rs_ = T.rerank_ref(q, x, ci, 10)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    assert R.same_scores(val.cpu().numpy(), rs_)
    idx2, val2 = rerank_inner_product(dev(q), dev(x), cand, 10)
    assert torch.equal(idx, idx2) and R.same_scores(val.cpu().numpy(), val2.cpu().numpy())
    again = Int8Index.from_state_dict({k: v.clone() for k, v in index.state_dict().items()})
    idx3, none = again.search(dev(q), 10, n_candidates=32, with_scores=False, **kw)
    assert none is None and torch.equal(idx, idx3)
    with pytest.raises(KeyError):
        Int8Index.from_state_dict({"codes": index.codes})
    with pytest.raises(ValueError):
        index.search(dev(q), 10, n_candidates=5)


def test_similar_items_with_an_int8_index_on_planted_exact_rows():
    from recommender_amd.eges.retrieval import similar_items
    from recommender_amd.retrieval import Int8Index

    hidden = dev(T.planted_exact(3, 400, 24))
    query = dev(np.array([0, 5, 399, 5, 64], np.int64))
    want = similar_items(hidden, query, 10)
    got = similar_items(hidden, query, 10, index=Int8Index.from_float(hidden), n_candidates=10,
                        nprobe=3)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    again = similar_items(hidden, query, 10, index=None)
    assert torch.equal(want[0], again[0]) and torch.equal(want[1], again[1])


def test_recommend_fused_with_an_int8_index_on_planted_exact_reprs():
    from recommender_amd.pinsage.evaluation import recommend
    from recommender_amd.pinsage.graph import HeteroGraph
    from recommender_amd.retrieval import Int8Index

    users, items, ts = R.recommend_graph(1)
    g = HeteroGraph(users, items, 300, 500, device=DEV, edge_data={"timestamp": ts})
    reprs = dev(T.planted_exact(2, 500, 16))
    want = recommend(g, 10, reprs, None, "user", "timestamp", 32, fused=True)
    got = recommend(g, 10, reprs, None, "user", "timestamp", 32, fused=True,
                    index=Int8Index.from_float(reprs), n_candidates=16)
    assert got.dtype == torch.int32 and torch.equal(want, got)
    with pytest.raises(ValueError):
        recommend(g, 10, reprs, None, "user", "timestamp", 32, index=Int8Index.from_float(reprs))


def test_inference_cli_int8_neighbours_are_the_rerank_of_the_int8_candidates(tmp_path):
    from recommender_amd.pinsage import inference as I

    out, nb, nb8 = tmp_path / "reprs.npy", tmp_path / "nbrs.npy", tmp_path / "nbrs8.npy"
    out8 = tmp_path / "reprs8.npy"
    I.main(["--out", str(out), "--neighbors", "5", "--neighbors-out", str(nb)])
    I.main(["--out", str(out8), "--neighbors", "5", "--neighbors-out", str(nb8),
            "--neighbors-int8", "64"])
    reprs, nbrs, nbrs8 = np.load(out), np.load(nb), np.load(nb8)
    np.testing.assert_array_equal(np.load(out8).view(np.uint32), reprs.view(np.uint32))
    assert nbrs8.dtype == np.int32 and nbrs8.shape == nbrs.shape
    rows = np.r_[0:reprs.shape[0]:8, reprs.shape[0] - 1]
    codes, scales, _ = T.quantize_ref(reprs)
    ci, _ = T.scan_ref(reprs[rows], codes, scales, 64, excl_one=rows)
    ri, _ = T.rerank_ref(reprs[rows], reprs, ci, 5)
    np.testing.assert_array_equal(nbrs8[rows], ri)
    ei, _ = R.topk_ref(reprs[rows], reprs, 5, excl_one=rows)
    np.testing.assert_array_equal(nbrs[rows], ei)  # without the flag: the exact result, as before
