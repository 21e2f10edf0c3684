"""Row-wise int8 tables on the GPU against tests/embedding_q8_ref.py (the contract restated in
NumPy), bit for bit: quantise, dequantise, lookup, bag, the argument errors and the Python
surface. Every output has 64 guard elements of a fixed pattern behind it and the same pattern
in its row padding; both are checked untouched."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from recommender_amd.embedding import Embedding, EmbeddingBag, SlabEmbedding
from recommender_amd.functional import embedding_bag_q8, embedding_lookup_q8, quantize_rows
from recommender_amd.quantized import (QuantizedEmbedding, QuantizedEmbeddingBag, from_float,
                                       quantize_embeddings)
from tests import embedding_q8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
NAN_BITS = 0x7FC00A5A  # the float guard: a NaN with a payload no kernel produces
BYTE = 0xA5            # the byte guard


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def float_buf(n):
    """n + GUARD floats of the guard NaN (a flat tensor: callers carve rows out of it)."""
    return torch.full((n + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def read_rows(buf, n, dim, ld):
    """(rows [n, dim] as uint32 bits, True when the padding and the guard are untouched)."""
    bits = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    body = bits[:n * ld].reshape(n, ld) if n else bits[:0].reshape(0, ld)
    clean = (body[:, dim:] == NAN_BITS).all() and (bits[n * ld:] == NAN_BITS).all()
    return body[:, :dim], bool(clean)


def stream():
    return L.stream_ptr(torch.device(DEV))


def gpu_quantize(src, q_ld, ld=None, offset=0):
    """rs_quantize_rows_q8 of src [n, dim] held at row stride ld (NaN in its padding: the
    kernel must not read it into the minimum), into a buffer `offset` bytes past an aligned base:
    (qtable [n, q_ld], error bits)."""
    n, dim = src.shape
    ld = ld or dim + 3
    wide = np.full((n, ld), np.nan, f32)
    wide[:, :dim] = src
    t = dev(wide)
    buf = torch.full((offset + n * q_ld + GUARD,), BYTE, dtype=torch.uint8, device=DEV)
    q = buf[offset:]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("rs_quantize_rows_q8", L.ptr(t), ld, n, dim, L.ptr(q), q_ld, L.ptr(err), stream())
    got = buf.cpu().numpy()
    assert (got[:offset] == BYTE).all() and (got[offset + n * q_ld:] == BYTE).all()
    return got[offset:offset + n * q_ld].reshape(n, q_ld), int(err.item())


def q_on_device(q, offset=0):
    """A quantised table on the device, `offset` bytes past an aligned base."""
    buf = torch.zeros(offset + q.size + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + q.size] = dev(q.reshape(-1))
    return buf[offset:]


def gpu_dequantize(q, dim, out_ld=None, offset=0):
    n, q_ld = q.shape
    out_ld = out_ld or dim
    out = float_buf(n * out_ld)
    L.call("rs_dequantize_rows_q8", L.ptr(q_on_device(q, offset)), n, dim, q_ld, L.ptr(out),
           out_ld, stream())
    rows, clean = read_rows(out, n, dim, out_ld)
    assert clean
    return rows


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- quantise and dequantise ---------------------------------------------------------------
@pytest.mark.parametrize("dim", R.QUANT_DIMS)
def test_quantize_dequantize_bitexact(dim):
    """Every row family and edge row, flagged rows first, last and inside; n_rows 1, 2, 1000; the
    default q_ld, default + 16, the smallest multiple of 4, and the default at a base 4 bytes off
    (the 4-byte path on the same data): codes, header and padding equal the restatement's, two
    runs agree, and the dequantised rows equal the restatement's with out_ld = dim and dim + 3."""
    for n in R.N_ROWS:
        src = R.table(dim, n)
        lds = [(R.row_bytes(dim), 0), (R.row_bytes(dim) + 16, 0), (R.narrow_ld(dim), 0),
               (R.row_bytes(dim), 4)]
        first = None
        for q_ld, offset in lds:
            ref, flagged = R.quantize(src, q_ld)
            got, err = gpu_quantize(src, q_ld, offset=offset)
            np.testing.assert_array_equal(got, ref, err_msg=f"n={n} q_ld={q_ld} offset={offset}")
            assert not got[:, 8 + dim:].any()                       # the padding is zero
            assert err == (L.RS_ERRBIT_NONFINITE if flagged.any() else 0)
            again, _ = gpu_quantize(src, q_ld, offset=offset)
            np.testing.assert_array_equal(again, got)              # reproducible
            if first is None:
                first = got
            np.testing.assert_array_equal(got[:, :8 + dim], first[:, :8 + dim])  # the paths agree
            table = bits(R.dequantize(ref, dim))
            np.testing.assert_array_equal(gpu_dequantize(got, dim, offset=offset), table)
            np.testing.assert_array_equal(gpu_dequantize(got, dim, dim + 3, offset), table)
        clean = R.table(dim, n, flagged=False)
        got, err = gpu_quantize(clean, R.row_bytes(dim), ld=dim)
        np.testing.assert_array_equal(got, R.quantize(clean)[0])
        assert err == 0                                             # set for flagged rows only


def test_quantize_keeps_the_other_error_bits():
    src = R.table(8, 3)
    t = dev(src)
    q = torch.empty(3, 16, dtype=torch.uint8, device=DEV)
    err = torch.full((1,), L.RS_ERRBIT_OOB | L.RS_ERRBIT_RANGE, dtype=torch.int32, device=DEV)
    L.call("rs_quantize_rows_q8", L.ptr(t), 8, 3, 8, L.ptr(q), 16, L.ptr(err), stream())
    assert int(err.item()) == L.RS_ERRBIT_OOB | L.RS_ERRBIT_RANGE | L.RS_ERRBIT_NONFINITE
    L.call("rs_quantize_rows_q8", L.ptr(t), 8, 3, 8, L.ptr(q), 16, None, stream())  # NULL flag
    torch.cuda.synchronize()


def test_zero_rows_have_positive_zero_bias():
    z = R.families(12)["zeros"]
    got, err = gpu_quantize(z, R.row_bytes(12))
    assert not got.any() and err == 0


# ---- lookup --------------------------------------------------------------------------------
def rows_per_block(dim, pw=4):
    """The rows one block of the lookup takes per pass: its lane groups read the codes in 4-byte
    pieces (recommender_amd/csrc/embedding_q8.hip)."""
    pieces = (dim + pw - 1) // pw
    lanes = 1
    while lanes < pieces and lanes < 64:
        lanes *= 2
    return 256 // lanes * 4  # lane groups per block, four rows each per pass


def gpu_lookup(q, dim, ids, slot_offsets=None, out_ld=None, offset=0):
    n, out_ld = ids.numel(), out_ld or dim
    out = float_buf(n * out_ld)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    so = dev(slot_offsets)
    L.call("rs_embedding_q8_fwd", L.ptr(q_on_device(q, offset)), q.shape[0], dim, q.shape[1],
           L.ptr(ids), L.id_dtype_code(ids), n, L.ptr(so),
           1 if so is None else so.numel() - 1, L.ptr(out), out_ld, L.ptr(err), stream())
    rows, clean = read_rows(out, n, dim, out_ld)
    assert clean
    return rows, int(err.item())


def float_gather(q, dim, ids, slot_offsets, out_ld):
    """rs_embedding_fwd_strided over rs_dequantize_rows_q8's output."""
    table = torch.empty(q.shape[0], dim, device=DEV)
    L.call("rs_dequantize_rows_q8", L.ptr(q_on_device(q)), q.shape[0], dim, q.shape[1],
           L.ptr(table), dim, stream())
    n = ids.numel()
    out = float_buf(n * out_ld)
    so = dev(slot_offsets)
    L.call("rs_embedding_fwd_strided", L.ptr(table), q.shape[0], dim, L.ptr(ids),
           L.id_dtype_code(ids), n, L.ptr(so), 1 if so is None else so.numel() - 1, L.ptr(out),
           out_ld, None, stream())
    return read_rows(out, n, dim, out_ld)[0]


@pytest.mark.parametrize("slots", [None, [1, 7, 1000]])
@pytest.mark.parametrize("dim", [1, 18, 64, 128, 130])
def test_lookup_bitexact(dim, slots, rng):
    cards = slots or [1008]
    so = None if slots is None else np.concatenate([[0], np.cumsum(cards)]).astype(np.int64)
    n_slots = len(cards)
    q, _ = R.quantize(R.table(dim, 1008, flagged=False))
    rpb = rows_per_block(dim)
    for id_dtype in (np.int64, np.int32):
        edge = [-1, np.iinfo(id_dtype).min]
        if id_dtype == np.int64:
            edge += [2 ** 32 + 1]
        for n_ids in (0, 1, rpb - 1, rpb + 1, 3 * rpb + 5):
            ids = np.empty(n_ids, id_dtype)
            for p in range(n_ids):
                c = cards[p % n_slots]
                ids[p] = [c - 1, c, rng.integers(0, c), edge[p % len(edge)]][(p // n_slots) % 4]
            for out_ld in (dim, dim + 3):
                for qq, offset in ((q, 0), (q, 4)):
                    ref, flag = R.lookup(qq, dim, ids, so)
                    got, err = gpu_lookup(qq, dim, dev(ids), so, out_ld, offset)
                    np.testing.assert_array_equal(got, bits(ref).reshape(n_ids, dim))
                    assert err == (L.RS_ERRBIT_OOB if flag else 0)
                if n_ids:
                    np.testing.assert_array_equal(got, float_gather(q, dim, dev(ids), so, out_ld))


def test_lookup_all_in_range_sets_nothing(rng):
    q, _ = R.quantize(R.table(20, 50, flagged=False))
    ids = rng.integers(0, 50, 333)
    got, err = gpu_lookup(q, 20, dev(ids))
    assert err == 0
    np.testing.assert_array_equal(got, bits(R.dequantize(q, 20))[ids])


# ---- bag -----------------------------------------------------------------------------------
def gpu_bag(q, dim, ids, n_bags, offsets=None, bag_len=0, valid=None, weights=None, mode=R.SUM,
            slot_offsets=None, id_dtype=np.int64, out_ld=None, offset=0, float_table=None):
    """rs_embedding_bag_q8_fwd, or rs_embedding_bag_fwd over float_table: (out bits, bag_scale,
    error bits)."""
    out_ld = out_ld or dim
    i = dev(np.asarray(ids).reshape(-1), id_dtype)
    o, v, w, so = dev(offsets, np.int64), dev(valid, np.uint8), dev(weights, f32), dev(slot_offsets)
    out = float_buf(n_bags * out_ld)
    scale = float_buf(n_bags)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tail = (L.ptr(i), L.id_dtype_code(i), i.numel(), L.ptr(o), n_bags, bag_len, L.ptr(v), L.ptr(w),
            mode, L.ptr(so), 1 if so is None else so.numel() - 1, L.ptr(out), out_ld,
            L.ptr(scale), L.ptr(err), stream())
    if float_table is None:
        L.call("rs_embedding_bag_q8_fwd", L.ptr(q_on_device(q, offset)), q.shape[1], q.shape[0],
               dim, *tail)
    else:
        L.call("rs_embedding_bag_fwd", L.ptr(float_table), q.shape[0], dim, *tail)
    rows, clean = read_rows(out, n_bags, dim, out_ld)
    sc, sclean = read_rows(scale, n_bags, 1, 1)
    assert clean and sclean
    return rows, sc.reshape(-1), int(err.item())


def check_bag(q, dim, ids, n_bags, **kw):
    """Against the restatement, against rs_embedding_bag_fwd over the dequantised table, and the
    4-byte path against both, bit for bit."""
    ref_kw = {k: v for k, v in kw.items() if k not in ("id_dtype", "out_ld")}
    ref, rscale, _, flag = R.bag_forward(q, dim, ids, n_bags, **ref_kw)
    table = torch.empty(q.shape[0], dim, device=DEV)
    L.call("rs_dequantize_rows_q8", L.ptr(q_on_device(q)), q.shape[0], dim, q.shape[1],
           L.ptr(table), dim, stream())
    for variant in (dict(), dict(offset=4), dict(float_table=table)):
        out, scale, err = gpu_bag(q, dim, ids, n_bags, **kw, **variant)
        np.testing.assert_array_equal(out, bits(ref).reshape(n_bags, dim), err_msg=str(variant))
        np.testing.assert_array_equal(scale, bits(rscale), err_msg=str(variant))
        assert bool(err & L.RS_ERRBIT_OOB) == flag and not err & ~L.RS_ERRBIT_OOB
    return ref


BAG_LENS = [0, 1, 3, 4, 5, 300, 0, 0, 2, 0]  # empty bags first, last and adjacent


def bag_table(dim, rows=400):
    """Quantised rows whose scales span 12 decades: a bag's fp32 sum depends on the order."""
    r = np.random.default_rng(dim)
    t = r.standard_normal((rows, dim)) * 10.0 ** r.uniform(-6, 6, (rows, 1))
    return R.quantize(t.astype(f32))[0]


@pytest.mark.parametrize("mode", [R.SUM, R.MEAN])
@pytest.mark.parametrize("dim", [1, 4, 18, 128, 130, 260])
def test_bag_bitexact_lengths_and_empties(dim, mode, rng):
    q = bag_table(dim)
    offsets = np.concatenate([[0], np.cumsum(BAG_LENS)]).astype(np.int64)
    ids = rng.integers(0, 400, offsets[-1])
    nb = len(BAG_LENS)
    check_bag(q, dim, ids, nb, offsets=offsets, mode=mode)
    check_bag(q, dim, ids, nb, offsets=offsets, mode=mode, id_dtype=np.int32, out_ld=dim + 3)
    # without offsets: bag_len 0, 1, 5
    for bl in (0, 1, 5):
        check_bag(q, dim, ids[:60 * bl].reshape(60, bl), 60, bag_len=bl, mode=mode)


@pytest.mark.parametrize("dim", [18, 128])
def test_bag_masks_and_weights(dim, rng):
    q = bag_table(dim)
    ids = rng.integers(0, 400, (33, 6))
    valid = (rng.random((33, 6)) < 0.6).astype(np.uint8)
    valid[0] = [1, 0, 1, 0, 0, 1]
    valid[5] = 0                                   # an all-dead bag
    valid[-1] = 0
    ref = check_bag(q, dim, ids, 33, bag_len=6, valid=valid, mode=R.MEAN)
    assert not ref[5].any()
    check_bag(q, dim, ids, 33, bag_len=6, valid=valid, mode=R.SUM, id_dtype=np.int32)
    w = rng.standard_normal((33, 6)).astype(f32)
    w[1] = [0.0, -1.5, 1e30, -1e30, 1e-42, 2.0]
    check_bag(q, dim, ids, 33, bag_len=6, weights=w, mode=R.SUM)
    check_bag(q, dim, ids, 33, bag_len=6, weights=w, valid=valid, mode=R.SUM)
    offsets = np.array([0, 0, 7, 7, 100, 198], np.int64)
    check_bag(q, dim, ids.reshape(-1), 5, offsets=offsets, weights=w.reshape(-1), mode=R.SUM)


@pytest.mark.parametrize("offsets", [[0, 3, 2, 6, 8], [0, 2, 50, 8], [-1, 4, 8]])
def test_bag_malformed_offsets(offsets, rng):
    q = bag_table(4)
    ids = rng.integers(0, 400, 8)
    offsets = np.array(offsets, np.int64)
    _, _, err = gpu_bag(q, 4, ids, len(offsets) - 1, offsets=offsets)
    assert err & L.RS_ERRBIT_OOB
    check_bag(q, 4, ids, len(offsets) - 1, offsets=offsets, mode=R.MEAN)


@pytest.mark.parametrize("dim", [3, 36, 128])
def test_bag_slots_strided_out_and_out_of_range(dim, rng):
    so = np.array([0, 1, 8, 311], np.int64)
    card = np.diff(so)
    q = bag_table(dim, rows=311)
    ids = np.stack([rng.integers(0, card[b % 3], 9) for b in range(64)])
    check_bag(q, dim, ids, 64, bag_len=9, slot_offsets=so, mode=R.MEAN, out_ld=dim + 4)
    ids[4, 2] = card[1]            # bag 4 reads slot 1: its cardinality is out of range
    ids[5, 0] = -1
    ids[6, 8] = 311
    ref = check_bag(q, dim, ids, 64, bag_len=9, slot_offsets=so, mode=R.MEAN, out_ld=dim + 1)
    assert R.bag_forward(q, dim, ids, 64, bag_len=9, slot_offsets=so, mode=R.MEAN)[3]
    assert ref.shape == (64, dim)


# ---- argument errors -------------------------------------------------------------------------
def test_argument_errors():
    lib = L.lib()
    t = torch.zeros(4, 8, device=DEV)
    q = torch.zeros(4, 16, dtype=torch.uint8, device=DEV)
    o = torch.zeros(6, 8, device=DEV)
    i = torch.zeros(6, dtype=torch.int64, device=DEV)
    w = torch.ones(6, device=DEV)
    E = L.RS_E_INVALID

    def quant(table=t, ld=8, n=4, dim=8, qt=q, q_ld=16):
        return lib.rs_quantize_rows_q8(L.ptr(table), ld, n, dim, L.ptr(qt), q_ld, None, None)

    def deq(qt=q, n=4, dim=8, q_ld=16, out=o, out_ld=8):
        return lib.rs_dequantize_rows_q8(L.ptr(qt), n, dim, q_ld, L.ptr(out), out_ld, None)

    def look(qt=q, dim=8, q_ld=16, ids=i, n_ids=6, out=o, out_ld=8, dtype=1):
        return lib.rs_embedding_q8_fwd(L.ptr(qt), 4, dim, q_ld, L.ptr(ids), dtype, n_ids, None, 1,
                                       L.ptr(out), out_ld, None, None)

    def bag(qt=q, q_ld=16, dim=8, ids=i, n_ids=6, n_bags=2, bag_len=3, mode=0, out=o, out_ld=8,
            weights=None):
        return lib.rs_embedding_bag_q8_fwd(L.ptr(qt), q_ld, 4, dim, L.ptr(ids), 1, n_ids, None,
                                           n_bags, bag_len, None, L.ptr(weights), mode, None, 1,
                                           L.ptr(out), out_ld, None, None, None)

    for f in (quant, deq, look, bag):
        assert f() == 0
        assert f(dim=0) == E and f(dim=-1) == E
        assert f(q_ld=15) == E               # < 8 + dim
        assert f(q_ld=12) == E               # < 8 + dim, a multiple of 4
        assert f(q_ld=18) == E               # not a multiple of 4
        assert f(qt=None) == E
    assert quant(table=None) == E and quant(ld=7) == E
    assert deq(out=None) == E and deq(out_ld=7) == E
    assert look(out=None) == E and look(ids=None) == E and look(out_ld=7) == E
    assert look(dtype=2) == E
    assert bag(out=None) == E and bag(ids=None) == E and bag(out_ld=7) == E
    assert bag(mode=2) == E and bag(mode=1, weights=w) == E and bag(n_ids=5) == E
    # no-ops: nothing is read or written, null pointers included
    assert quant(n=0, table=None, qt=None) == 0 and deq(n=0, qt=None, out=None) == 0
    assert look(n_ids=0, ids=None, out=None) == 0 and bag(n_ids=0, n_bags=0, out=None) == 0
    torch.cuda.synchronize()


# ---- modules ---------------------------------------------------------------------------------
def test_from_float_slab_lookup_and_state_round_trip(rng):
    cards = [1, 7, 1000]
    w = R.table(18, 1008, flagged=False)
    slab = SlabEmbedding(cards, 18, device=DEV, weight=torch.from_numpy(w))
    qm = from_float(slab)
    assert type(qm) is QuantizedEmbedding
    assert (qm.input_dim, qm.output_dim, qm.n_slots, qm.mask_zero) == (1008, 18, 3, False)
    ref_q, _ = R.quantize(w)
    np.testing.assert_array_equal(qm.qweight.cpu().numpy(), ref_q)
    ids = np.stack([rng.integers(0, c, 64) for c in cards], 1)
    ids[3, 1] = 7                                        # out of range in slot 1
    out = qm(dev(ids))
    assert out.shape == (64, 3, 18) and not out.requires_grad
    ref, _ = R.lookup(ref_q, 18, ids, np.array([0, 1, 8, 1008]))
    np.testing.assert_array_equal(bits(out.cpu().numpy()).reshape(-1, 18), bits(ref))
    assert qm.oob_detected()
    qm.reset_oob()
    assert not qm.oob_detected() and qm.check_errors() == 0
    np.testing.assert_array_equal(bits(qm.dequantize().cpu().numpy()), bits(R.dequantize(ref_q, 18)))
    assert embedding_lookup_q8(qm, dev(ids)).equal(out)
    np.testing.assert_array_equal(quantize_rows(slab.weight).cpu().numpy(), ref_q)
    # state_dict round trip into an empty module
    fresh = QuantizedEmbedding(1008, 18, device=DEV, slot_offsets=slab.slot_offsets)
    assert not fresh(dev(ids)).any()
    fresh.load_state_dict(qm.state_dict())
    assert set(qm.state_dict()) == {"qweight", "slot_offsets", "err_flag"}
    assert fresh(dev(ids)).equal(out)
    # mask_zero travels, and the mask with it
    e = Embedding(50, 4, mask_zero=True, device=DEV)
    qe = from_float(e)
    m = qe.compute_mask(dev(np.array([0, 3, 0])))
    assert m.tolist() == [False, True, False] and qm.compute_mask(dev(ids)) is None


def test_from_float_bag_matches_float_bag_over_dequantized(rng):
    w = R.table(36, 300, flagged=False)
    for mode in ("sum", "mean"):
        bag = EmbeddingBag(300, 36, mode=mode, device=DEV, weight=torch.from_numpy(w))
        qb = from_float(bag)
        assert type(qb) is QuantizedEmbeddingBag and qb.mode == mode
        ids = dev(rng.integers(0, 300, (40, 7)))
        valid = dev((rng.random((40, 7)) < 0.7).astype(np.uint8))
        bag.weight.copy_(qb.dequantize())
        with torch.no_grad():
            want = bag(ids, valid=valid)
        got = qb(ids, valid=valid)
        assert got.equal(want) and not got.requires_grad
        assert embedding_bag_q8(qb, ids, mode=mode, valid=valid).equal(got)
        offs = dev(np.array([0, 0, 100, 280], np.int64))
        with torch.no_grad():
            want = bag(ids.reshape(-1), offs)
        assert qb(ids.reshape(-1), offs).equal(want)


def test_from_float_refuses_a_non_finite_table():
    w = R.table(8, 20, flagged=False)
    w[11, 3] = np.nan
    e = Embedding(20, 8, device=DEV, weight=torch.from_numpy(w))
    with pytest.raises(ValueError, match="quantised"):
        from_float(e)
    with pytest.raises(TypeError):
        from_float(torch.nn.Linear(2, 2))


def _pair(build):
    """The same model twice (one seed): the second keeps its float table."""
    ms = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        ms.append(build(g))
    return ms


def _check_swapped(qmodel, fmodel, table_of, feats):
    """quantize_embeddings' predictions against the float model run on dequantize()."""
    assert table_of(qmodel).weight.equal(table_of(fmodel).weight)
    assert quantize_embeddings(qmodel) is qmodel
    qt = table_of(qmodel)
    assert isinstance(qt, QuantizedEmbedding) and not hasattr(qt, "weight")
    table_of(fmodel).weight.copy_(qt.dequantize())
    with torch.no_grad():
        got, want = qmodel(feats), fmodel(feats)
    assert got.equal(want) and got.shape[0] == 64
    assert not qt.oob_detected()
    assert all(not isinstance(m, Embedding) for m in qmodel.modules())


def test_quantize_embeddings_deepfm():
    from recommender_amd.ctr.train import build_model
    from recommender_amd.synthetic import criteo_batch

    cards = [3, 7, 1000, 50]
    q, f = _pair(lambda g: build_model("DeepFM", 16, 0, 4, 13, DEV, slot_cardinalities=cards,
                                       mlp_units=[64, 32, 1], generator=g))
    cat, dense, _ = criteo_batch(np.random.default_rng(1), 64, cards)
    feats = {"cat_features": dev(cat), "int_features": dev(dense)}
    _check_swapped(q, f, lambda m: m.embedding_layer, feats)


@pytest.mark.parametrize("kind", ["ESMM", "MMOE"])
def test_quantize_embeddings_esmm_family(kind):
    from recommender_amd.esmm import FEAT_VOCAB
    from recommender_amd.esmm.train import build
    from recommender_amd.synthetic import aliccp_batch

    vocab = {k: min(v, 300) for k, v in FEAT_VOCAB.items()}
    q, f = _pair(lambda g: build(kind, vocab, 18, DEV, g))
    feats, _ = aliccp_batch(np.random.default_rng(5), 64, vocab)
    feats = {k: dev(v) for k, v in feats.items()}
    _check_swapped(q, f, lambda m: m.embedding_layer.slab, feats)


def test_quantize_embeddings_refusals():
    from recommender_amd.ctr.train import build_model
    from recommender_amd.optim import SparseSGD

    dlrm = build_model("DLRM", 16, 100, 4, 13, DEV, bottom=[32, 16], top=[32, 1])
    with pytest.raises(TypeError, match="DLRM"):
        quantize_embeddings(dlrm)
    assert isinstance(dlrm.embedding_layer, Embedding)               # nothing was swapped
    deepfm = build_model("DeepFM", 16, 100, 4, 13, DEV, mlp_units=[32, 1])
    SparseSGD(deepfm.embedding_layer, lr=0.1, fused=True)
    with pytest.raises(TypeError, match="fused optimizer"):
        quantize_embeddings(deepfm)
    assert isinstance(deepfm.embedding_layer, Embedding)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.table = Embedding(10, 4, device=DEV)

    with pytest.raises(TypeError, match="forward"):
        quantize_embeddings(Holder())
    h = quantize_embeddings(Holder(), forward_only=(Holder,))
    assert isinstance(h.table, QuantizedEmbedding)
