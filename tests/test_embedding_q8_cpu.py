"""What tests/test_embedding_q8_gpu.py relies on, proved without a GPU: the exports exist in the
derived binding, the NumPy restatement (tests/embedding_q8_ref.py) does what the header says on
the rows chosen to show it, and its accuracy bound holds on every input family."""
import numpy as np
import pytest

from recommender_amd import _lib as L
from tests import embedding_q8_ref as R

f32 = np.float32


def test_exports_in_the_derived_binding():
    for name in ("rs_q8_row_bytes", "rs_quantize_rows_q8", "rs_dequantize_rows_q8",
                 "rs_embedding_q8_fwd", "rs_embedding_bag_q8_fwd"):
        assert name in L.SIGNATURES and name in L.header_symbols()
    assert L.RS_ERRBIT_NONFINITE == 8
    assert {L.RS_ERRBIT_OOB, L.RS_ERRBIT_FORMAT, L.RS_ERRBIT_RANGE} == {1, 2, 4}
    # the bag's argument list is rs_embedding_bag_fwd's with (qtable, q_ld) in place of table
    bag, qbag = L.SIGNATURES["rs_embedding_bag_fwd"], L.SIGNATURES["rs_embedding_bag_q8_fwd"]
    assert qbag[0] == bag[0] and len(qbag[1]) == len(bag[1]) + 1 and qbag[1][2:] == bag[1][1:]
    lib = L.load()
    assert [lib.rs_q8_row_bytes(d) for d in (1, 8, 9, 120, 128, 136)] == [16, 16, 32, 128, 144, 144]
    assert all(lib.rs_q8_row_bytes(d) == R.row_bytes(d) for d in R.QUANT_DIMS)
    assert lib.rs_q8_row_bytes(0) == 0


@pytest.mark.parametrize("dim", [4, 20, 128, 260])
def test_tie_row_rounds_to_even(dim):
    row = R.tie_row(dim)[None]
    lo, hi, scale, flagged = R.row_stats(row)
    assert (lo[0], hi[0], scale[0], flagged[0]) == (0.0, 255.0, 1.0, False)
    q, _ = R.quantize(row)
    codes = q[0, 8:8 + dim]
    assert codes[0] == 0 and codes[1] == 255            # the minimum and the maximum
    halves = row[0, 2:]
    assert (halves % 1 == 0.5).all()
    assert (codes[2:] % 2 == 0).all()                   # the even neighbour of k + 0.5
    assert (np.abs(codes[2:].astype(f32) - halves) == 0.5).all()
    up = codes[2:] > halves
    assert up.any() and not up.all()                    # some up, some down: no fixed direction


@pytest.mark.parametrize("dim", R.QUANT_DIMS)
def test_extremes_get_the_end_codes_when_scale_is_normal(dim):
    t = R.table(dim, 400, flagged=False)
    lo, hi, scale, _ = R.row_stats(t)
    q, _ = R.quantize(t)
    codes = q[:, 8:8 + dim]
    normal = scale >= np.finfo(f32).tiny
    assert normal.sum() > 100 or dim == 1               # a one-column row is constant
    for r in np.nonzero(normal)[0]:
        assert (codes[r][t[r] == lo[r]] == 0).all()
        assert (codes[r][t[r] == hi[r]] == 255).all()


def test_clamp_row_needs_the_clamp():
    for dim in (2, 5, 128):
        row = R.clamp_row(dim)[None]
        _, _, scale, _ = R.row_stats(row)
        assert 0 < scale[0] < np.finfo(f32).tiny        # subnormal
        assert R.raw_quotient(row).max() == 382          # past 255
        assert R.quantize(row)[0][0, 8:8 + dim].max() == 255
    # and the tables the GPU tests quantise hold such rows, besides the one built for it
    worst = max(R.raw_quotient(R.table(dim, 400, flagged=False)).max() for dim in (2, 17, 128))
    assert worst > 255


@pytest.mark.parametrize("dim", [1, 2, 7, 33, 128, 260])
def test_accuracy_bound_on_every_family(dim):
    for name, rows in R.families(dim, rows=64).items():
        q, flagged = R.quantize(rows)
        assert not flagged.any(), name
        err = np.abs(R.dequantize(q, dim).astype(np.float64) - rows.astype(np.float64))
        ratio = (err / R.bound(rows)).max()
        assert ratio <= 1.0, (name, dim, ratio)


def test_constant_and_zero_rows():
    fam = R.families(9)
    q, _ = R.quantize(fam["constant"])
    scale, bias = R.header(q)
    assert (scale == 0).all() and (q[:, 8:] == 0).all()
    np.testing.assert_array_equal(R.dequantize(q, 9), fam["constant"])   # exact
    z = fam["zeros"]
    assert np.signbit(z).any() and not np.signbit(z).all() and np.signbit(z[0]).all()
    q, _ = R.quantize(z)
    assert not q.any()                                   # scale +0, bias +0, codes 0
    q, _ = R.quantize(fam["two_valued"])
    assert set(np.unique(q[:, 8:8 + 9])) <= {0, 255}


@pytest.mark.parametrize("dim", [1, 2, 16, 128])
def test_flagged_rows_are_classified(dim):
    bad = R.flagged_rows(dim)
    q, flagged = R.quantize(bad)
    want = [True, True, True, dim > 1]
    assert flagged.tolist() == want
    assert not q[flagged].any()                          # scale 0, bias 0, codes 0
    for n in R.N_ROWS:
        _, fl = R.quantize(R.table(dim, n))
        assert fl[0] and (n == 1 or fl[-1]) and (n < 5 or fl[n // 2])
        assert not R.quantize(R.table(dim, n, flagged=False))[1].any()


def test_padding_and_layout():
    t = R.table(5, 7, flagged=False)
    for q_ld in (R.row_bytes(5), R.row_bytes(5) + 16, R.narrow_ld(5)):
        q, _ = R.quantize(t, q_ld)
        assert q.shape == (7, q_ld) and not q[:, 13:].any()
        lo, _, scale, _ = R.row_stats(t)
        s, b = R.header(q)
        np.testing.assert_array_equal(s.view(np.uint32), scale.view(np.uint32))
        np.testing.assert_array_equal(b.view(np.uint32), lo.view(np.uint32))
    assert (R.narrow_ld(5), R.narrow_ld(8), R.narrow_ld(130)) == (16, 16, 140)


def test_lookup_and_bag_restatements():
    t = R.table(6, 30, flagged=False)
    q, _ = R.quantize(t)
    table = R.dequantize(q, 6)
    so = np.array([0, 1, 8, 30], np.int64)
    ids = np.array([0, 6, 21, 0, 7, 22, 1, -1, 5], np.int64)
    out, flag = R.lookup(q, 6, ids, so)
    assert flag
    np.testing.assert_array_equal(out[:3], table[[0, 7, 29]])
    assert not out[[4, 5, 6, 7]].any() and out[8].tolist() == table[13].tolist()
    out, *_ = R.bag_forward(q, 6, np.array([[3, 4], [5, 5]]), 2, bag_len=2, mode=R.SUM)
    np.testing.assert_array_equal(out[0], (np.zeros(6, f32) + table[3]) + table[4])
