"""CPU tests of the DLRM scoring entry points (rs_dlrm_score, rs_dlrm_score_q8): the symbols and
their signatures, every argument error from the C entry point without a GPU, and the proofs of
what tests/test_dlrm_score_gpu.py relies on (tests/dlrm_score_ref.py): the magnitude bound of the
pre-activation, the quantisation bound, and the edge ids."""
import ctypes as C

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import dlrm_edges as E
from tests import dlrm_score_ref as R
from tests import embedding_q8_ref as Q

NAMES = ("rs_dlrm_score", "rs_dlrm_score_q8")


def test_symbols_declared_exported_and_typed(lib):
    i32, i64, p = C.c_int32, C.c_int64, C.c_void_p
    tail = [p, i32, i32, p, p, i64, p, p, i32, p, p, p]   # ids ... stream
    for n in NAMES:
        assert n in L.header_symbols()
        assert hasattr(lib, n)
    assert L.SIGNATURES["rs_dlrm_score"] == (i32, [p, i64, i32] + tail)
    assert L.SIGNATURES["rs_dlrm_score_q8"] == (i32, [p, i64, i64, i32] + tail)


# ---- argument errors: no device access, so fake (aligned, non-null) addresses serve ----------
A = 0x10000


def f32_args(**over):
    a = dict(table=A, n_rows=100, D=128, ids=A, id_dtype=L.RS_ID_I32, n_slots=4,
             slot_offsets=None, dense=A, batch=8, q=A, c=A, act=2, y=A, err_flag=None, stream=None)
    a.update(over)
    return list(a.values())


def q8_args(**over):
    a = dict(qtable=A, q_ld=144, n_rows=100, D=128, ids=A, id_dtype=L.RS_ID_I32, n_slots=4,
             slot_offsets=None, dense=A, batch=8, q=A, c=A, act=2, y=A, err_flag=None, stream=None)
    a.update(over)
    return list(a.values())


COMMON_ERRORS = [
    (dict(ids=None), L.RS_E_INVALID), (dict(dense=None), L.RS_E_INVALID),
    (dict(q=None), L.RS_E_INVALID), (dict(c=None), L.RS_E_INVALID), (dict(y=None), L.RS_E_INVALID),
    (dict(id_dtype=2), L.RS_E_INVALID), (dict(id_dtype=-1), L.RS_E_INVALID),
    (dict(act=3), L.RS_E_INVALID), (dict(act=-1), L.RS_E_INVALID),
    (dict(n_slots=0), L.RS_E_INVALID), (dict(n_slots=32), L.RS_E_INVALID),
    (dict(n_rows=0), L.RS_E_INVALID), (dict(n_rows=-5), L.RS_E_INVALID),
    (dict(batch=-1), L.RS_E_INVALID), (dict(dense=A + 4), L.RS_E_INVALID),
    (dict(D=32), L.RS_E_UNSUPPORTED), (dict(D=16), L.RS_E_UNSUPPORTED),
    (dict(D=256, q_ld=272), L.RS_E_UNSUPPORTED), (dict(D=120), L.RS_E_UNSUPPORTED),
]


@pytest.mark.parametrize("over,code", COMMON_ERRORS)
def test_argument_errors_without_gpu(lib, over, code):
    f32_over = {k: v for k, v in over.items() if k != "q_ld"}
    assert lib.rs_dlrm_score(*f32_args(**f32_over)) == code
    assert lib.rs_last_error()
    assert lib.rs_dlrm_score_q8(*q8_args(**over)) == code


def test_table_errors_without_gpu(lib):
    assert lib.rs_dlrm_score(*f32_args(table=None)) == L.RS_E_INVALID
    assert lib.rs_dlrm_score(*f32_args(table=A + 8)) == L.RS_E_INVALID        # not 16-byte aligned
    assert lib.rs_dlrm_score_q8(*q8_args(qtable=None)) == L.RS_E_INVALID
    assert lib.rs_dlrm_score_q8(*q8_args(qtable=A + 2)) == L.RS_E_INVALID     # not 4-byte aligned
    assert lib.rs_dlrm_score_q8(*q8_args(q_ld=135)) == L.RS_E_INVALID         # < 8 + D
    assert lib.rs_dlrm_score_q8(*q8_args(q_ld=138)) == L.RS_E_INVALID         # not a multiple of 4
    assert lib.rs_dlrm_score_q8(*q8_args(D=64, q_ld=68)) == L.RS_E_INVALID
    assert lib.rs_dlrm_score_q8(*q8_args(D=0, q_ld=16)) == L.RS_E_INVALID


def test_empty_batch_is_a_no_op_without_gpu(lib):
    none = dict(ids=None, dense=None, q=None, c=None, y=None, batch=0)
    assert lib.rs_dlrm_score(*f32_args(table=None, n_rows=0, **none)) == L.RS_OK
    assert lib.rs_dlrm_score_q8(*q8_args(qtable=None, n_rows=0, **none)) == L.RS_OK
    # the argument errors still come first
    assert lib.rs_dlrm_score(*f32_args(batch=0, act=5)) == L.RS_E_INVALID
    assert lib.rs_dlrm_score_q8(*q8_args(batch=0, D=32)) == L.RS_E_UNSUPPORTED


# ---- the magnitude bound of the pre-activation -------------------------------------------------
@pytest.mark.parametrize("S,D,shared", [(1, 64, True), (3, 128, False), (17, 64, False)])
def test_magnitude_bound_is_the_sum_of_absolute_terms(S, D, shared):
    """head_dx_reference's hm equals Σ|terms| written out pair by pair, bounds |h|, and an fp32
    evaluation in another order than the kernel's lies within 1e-5 · hm of the float64 value: the
    bound of the 1e-5 comparison is the right size for fp32."""
    B = 9
    table, ids, offs, dense, q, c = R.score_inputs(B, S, D, False, seed=S, shared=shared, oob=True)
    _, _, y, hm, _, _, has_oob = E.head_dx_reference(table, ids, offs, dense, q, c, S, 0)
    h, m = R.preact_terms(table, ids, offs, dense, q, c, S)
    assert has_oob
    np.testing.assert_allclose(y.numpy(), h, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(hm.numpy(), m, rtol=1e-12)
    assert (np.abs(h) <= m).all()
    X, _ = E.gather_x(table, ids, offs, dense, S)
    X32 = X.float()
    iu = torch.triu_indices(S + 1, S + 1, 1)
    z32 = (X32 @ X32.transpose(1, 2))[:, iu[0], iu[1]]
    h32 = torch.cat([z32, dense], 1) @ q + c
    E.close(h32, y, hm, "fp32 in torch's order")
    # the sigmoid and relu tolerances: Lipschitz constants 1/4 and 1
    for act, lip in ((1, 1.0), (2, 0.25)):
        f = {1: lambda v: np.maximum(v, 0), 2: lambda v: 1 / (1 + np.exp(-v))}[act]
        d = 1e-5 * m
        assert (np.abs(f(h + d) - f(h)) <= lip * d * (1 + 1e-9)).all()
        assert (R.y_tolerance(m, f(h), act) >= lip * d * (1 - 1e-12)).all()


# ---- the quantisation bound --------------------------------------------------------------------
@pytest.mark.parametrize("D", R.DIMS)
def test_quantisation_bound_holds_on_the_test_tables(D):
    """|h(dequantised) − h(float)| <= Σ|q_o||Δz_o| with Δz from the per-element bound e_i, on the
    families the GPU tests use and on a trained-like gaussian table."""
    S, B = 4, 40
    g = torch.Generator().manual_seed(D)
    for name, src in (("families", R.mild_families(D)),
                      ("gauss", (torch.randn(64, D, generator=g) * 0.5).numpy())):
        src = np.asarray(src, np.float32)
        V = src.shape[0]
        qt, flagged = Q.quantize(src)
        assert not flagged.any()
        deq = Q.dequantize(qt, D)
        e = Q.bound(src)
        assert (np.abs(deq.astype(np.float64) - src.astype(np.float64)) <= e).all(), name
        ids = torch.randint(0, V, (B, S), generator=g)
        ids[3, 1] = V            # an out-of-range id: a zero row, no error from it
        dense = E.relu_dense(B, D, g)
        q = torch.randn(E.nzc_of(S + 1) + D, generator=g) * 0.05
        c = torch.tensor([0.1])
        hf, _ = R.preact_terms(src, ids, None, dense, q, c, S)
        hq, _ = R.preact_terms(deq, ids, None, dense, q, c, S)
        bound = R.quant_bound(src, ids, None, dense, q, S)
        assert (np.abs(hq - hf) <= bound).all(), name
        if name == "gauss":      # and the bound is not vacuous: within 100x of what is seen
            assert np.abs(hq - hf).max() * 100 > bound.max()


def test_q8_table_has_the_edge_rows():
    """The RS_Q8 test table holds a constant row (scale 0) and rows with a subnormal scale."""
    for D in R.DIMS:
        src, qt = R.q8_table(D, 90)
        scale, _ = Q.header(qt)
        assert (scale == 0).any()
        assert ((scale > 0) & (scale < np.float32(2.0 ** -126))).any()
        const = np.flatnonzero(src.max(1) == src.min(1))
        assert const.size and (scale[const] == 0).all()
        assert (Q.dequantize(qt, D)[const] == src[const]).all()
        # the default stride allows the 16-byte reads, 8 + D + 4 only the 4-byte ones
        assert Q.row_bytes(D) % 8 == 0 and (8 + D + 4) % 8 == 4


# ---- the edge ids ------------------------------------------------------------------------------
@pytest.mark.parametrize("id64", [False, True])
def test_edge_ids_are_what_they_claim(id64):
    S = 4
    cards = R.uneven_cards(S)
    assert 1 in cards and len(set(cards)) > 1
    B = 2 + (5 if id64 else 3) * S + 1
    ids, bad = E.edge_ids(B, cards, id64, seed=1)
    v = ids.numpy().astype(object)
    for s, card in enumerate(cards):
        col = list(v[:, s])
        assert card - 1 in col and not bad[col.index(card - 1), s]      # the last valid id
        for out in [card, -1] + ([2 ** 32 + 1, E.I64_MIN] if id64 else []):
            assert out in col and bad[col.index(out), s]
    assert bad[B - 1].all()                                              # no valid id at all
    assert not bad[0].any()
    if id64:
        # truncated to 32 bits, 2^32 + 1 would be the valid id 1 of a slot with more than one row
        assert (2 ** 32 + 1) % 2 ** 32 == 1 and max(cards) > 1
