"""Sparse Adagrad without a GPU: the C ABI's constants, export and argument checks, and the NumPy
reference (tests/adagrad_ref.py) against a float64 evaluation on a hand-sized case."""
import ctypes as C

import numpy as np
import pytest

from recommender_amd import _lib as L
from tests import adagrad_ref as R


def test_constants_and_export(lib):
    assert L.RS_OPT_ADAGRAD == 3 and L.RS_OPT_ROWWISE_ADAGRAD == 4
    assert hasattr(lib, "rs_apply_adagrad")
    assert "rs_apply_adagrad" in L.header_symbols() and "rs_apply_adagrad" in L.SIGNATURES
    text = L.HEADER.read_text()
    assert "#define RS_OPT_ADAGRAD 3" in text and "#define RS_OPT_ROWWISE_ADAGRAD 4" in text


@pytest.mark.parametrize("kind", [3, 4])
def test_null_accumulator_is_invalid_and_named(lib, kind):
    prm = L.AdamParams(1e-3, 0, 0, 0, 0, 1e-7)
    st = lib.rs_embedding_apply(kind, None, None, None, 10, 8, None, None, 0, None, C.byref(prm),
                                None, None, 0, None)
    assert st == -1
    assert "accumulator" in lib.rs_last_error().decode()
    st = lib.rs_embedding_apply_scaled(kind, None, None, None, 10, 8, None, None, 0, None, None, 1,
                                       C.byref(prm), None, None, 0, None)
    assert st == -1
    assert "accumulator" in lib.rs_last_error().decode()


def test_one_call_null_accumulator_is_invalid(lib):
    st = lib.rs_apply_adagrad(None, None, 10, 8, None, 1, 0, None, 1, None, 1e-3, 1e-7, 1, None,
                              None, 0, None)
    assert st == -1
    assert "accumulator" in lib.rs_last_error().decode()


def test_unknown_kind_still_rejected(lib):
    prm = L.AdamParams(1e-3, 0, 0, 0, 0, 1e-7)
    st = lib.rs_embedding_apply(5, None, None, None, 10, 8, None, None, 0, None, C.byref(prm),
                                None, None, 0, None)
    assert st == -1
    assert "unknown optimizer" in lib.rs_last_error().decode()


def _hand_case():
    """V = 6, D = 3: id 4 twice, id 9 out of range, id 1 once; rows 0, 2, 3, 5 untouched."""
    V, D = 6, 3
    ids = np.array([4, 1, 9, 4], np.int64)
    g = np.array([[0.5, -1.25, 2.0], [0.1, 0.2, -0.3], [7.0, 7.0, 7.0], [0.25, 0.75, -1.0]],
                 np.float32)
    w = (np.arange(V * D, dtype=np.float32).reshape(V, D) - 8) / 4
    return V, D, ids, g, w


def test_segment_grads_dedup_and_oob():
    V, D, ids, g, _ = _hand_case()
    ur, ug = R.segment_grads(ids, g, V)
    np.testing.assert_array_equal(ur, [1, 4])
    np.testing.assert_array_equal(ug, np.stack([g[1], g[0] + g[3]]))  # the OOB row is dropped
    ur, ug = R.segment_grads(ids, g, V, valid=np.array([1, 1, 1, 0]),
                             row_scale=np.array([2.0, 0.5], np.float32), scale_group=2)
    np.testing.assert_array_equal(ur, [1, 4])
    np.testing.assert_array_equal(ug, np.stack([g[1] * np.float32(2), g[0] * np.float32(2)]))


@pytest.mark.parametrize("rowwise", [False, True])
def test_reference_matches_float64(rowwise):
    """Two steps from acc = 0.1. Every fp32 result is a chain of fewer than 8 rounded operations
    on the exact inputs, so it lies within 8 * 2^-24 of the float64 value relative to the
    magnitudes involved (|w| + |update| for the weights, whose subtraction may cancel)."""
    V, D, ids, g, w0 = _hand_case()
    lr, eps = 0.05, 1e-7
    acc0 = np.full((V,) if rowwise else (V, D), 0.1, np.float32)
    f = R.apply_rowwise_adagrad if rowwise else R.apply_adagrad
    f64 = R.apply_rowwise_adagrad_f64 if rowwise else R.apply_adagrad_f64
    ur, ug = R.segment_grads(ids, g, V)
    w, acc = w0, acc0
    for _ in range(2):
        w_new, acc_new = f(w, acc, ur, ug, lr, eps)
        w64, acc64 = f64(w, acc, ur, ug, lr, eps)  # from the same fp32 state: no compounding
        assert w_new.dtype == np.float32 and acc_new.dtype == np.float32
        u = 8 * 2.0 ** -24
        assert (np.abs(acc_new - acc64) <= u * np.abs(acc64)).all()
        upd = np.abs(w64 - w)
        assert (np.abs(w_new - w64) <= u * (np.abs(w64) + upd)).all()
        untouched = np.setdiff1d(np.arange(V), ur)
        np.testing.assert_array_equal(w_new[untouched], w[untouched])
        np.testing.assert_array_equal(acc_new[untouched], acc[untouched])
        assert (acc_new[ur] > acc[ur]).all() and (w_new[ur] != w[ur]).any()
        w, acc = w_new, acc_new
    if rowwise:  # one accumulator per row: the mean of the squared gradient, by hand for row 4
        s = np.float64(0.75) ** 2 + np.float64(0.5) ** 2 + 1.0
        a1 = float(np.float32(0.1)) + s / 3
        assert abs(float(R.rowwise_accumulator(acc0, ur, ug)[4]) - a1) <= R.rowwise_acc_rtol(D) * a1


def test_sharded_slab_rejects_adagrad():
    """TrainStep refuses the two Adagrad names on a row-sharded slab (the owner-side apply has
    its own ordering and oracle); the type alone decides, before any communicator is used."""
    import torch

    from recommender_amd import sharded
    from recommender_amd.ctr import train as T

    class _Emb(sharded.ShardedSlabEmbedding):
        shard = None

        def __init__(self):  # no communicator: TrainStep only looks at the type before raising
            torch.nn.Module.__init__(self)

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding_layer = _Emb()
            self.lin = torch.nn.Linear(2, 1)

    for name in ("adagrad", "rowwise_adagrad"):
        with pytest.raises(ValueError, match="row-sharded slab does not support Adagrad"):
            T.TrainStep(_Model(), name)
