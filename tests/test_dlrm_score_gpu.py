"""The DLRM scoring kernels through their C entry points (rs_dlrm_score, rs_dlrm_score_q8) and
through DLRM.score / quantize_embeddings. Inputs and bounds come from tests/dlrm_score_ref.py
(proven in tests/test_dlrm_score_cpu.py). y is prefilled and has 64 guard elements of a fixed NaN
bit pattern behind it. The contract's equalities (the fp32 kernel against
rs_dlrm_interaction_fwd_head's y, the RS_Q8 kernel against the fp32 one over the dequantised
table, whatever the access width; two runs) are bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from recommender_amd.functional import dequantize_rows
from tests import dlrm_edges as E
from tests import dlrm_score_ref as R
from tests import embedding_q8_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def stream():
    return L.stream_ptr(torch.device(DEV))


class Y:
    """y [B] prefilled with NaN, E.GUARD guard elements behind it."""

    def __init__(self, B):
        self.B = B
        self.buf = torch.full((B + E.GUARD,), E.GUARD_BITS, dtype=torch.int32, device=DEV)
        self.t = self.buf[:B].view(torch.float32)
        self.t.fill_(NAN)
        self.before = self.buf.clone()

    def ptr(self):
        return L.ptr(self.buf)

    def check(self):
        assert bool((self.buf[self.B:] == E.GUARD_BITS).all()), "written past y[batch)"

    def untouched(self):
        return torch.equal(self.buf, self.before)


def bits(t):
    return t.contiguous().view(torch.int32)


def run_head(table, ids, offs, dense, q, c, S, act):
    """rs_dlrm_interaction_fwd_head's (y, err) at D = 128 (q padded to the row stride)."""
    B, D = dense.shape
    w = E.nzc_of(S + 1) + D
    out = torch.empty(B, w, device=DEV)
    y = Y(B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("rs_dlrm_interaction_fwd_head", L.ptr(table), table.shape[0], D, L.ptr(ids),
           L.id_dtype_code(ids), S, L.ptr(offs), L.ptr(dense), B, L.ptr(out), w, L.ptr(q), L.ptr(c),
           act, y.ptr(), L.ptr(err), stream())
    torch.cuda.synchronize()
    y.check()
    return y.t.clone(), int(err.item())


def run_score(table, ids, offs, dense, q, c, S, act, err_flag=True, y=None):
    B, D = dense.shape
    y = y or Y(B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if err_flag else None
    L.call("rs_dlrm_score", L.ptr(table), table.shape[0], D, L.ptr(ids), L.id_dtype_code(ids), S,
           L.ptr(offs), L.ptr(dense), B, L.ptr(q), L.ptr(c), act, y.ptr(), L.ptr(err), stream())
    torch.cuda.synchronize()
    y.check()
    return y.t.clone(), (int(err.item()) if err_flag else None)


class QTable:
    """RS_Q8 bytes on the device, the table starting `shift` bytes into its allocation."""

    def __init__(self, qt, shift=0):
        self.n_rows, self.q_ld = qt.shape
        self.buf = torch.zeros(qt.size + 16, dtype=torch.uint8, device=DEV)
        self.view = self.buf[shift:shift + qt.size].view(self.n_rows, self.q_ld)
        self.view.copy_(torch.from_numpy(qt))
        assert self.buf.data_ptr() % 16 == 0
        self.addr = self.buf.data_ptr() + shift

    def ptr(self):
        return C.c_void_p(self.addr)

    def dequantized(self, D):
        return dequantize_rows(self.view.contiguous(), D)


def run_score_q8(qt, ids, offs, dense, q, c, S, act, err_flag=True):
    B, D = dense.shape
    y = Y(B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if err_flag else None
    L.call("rs_dlrm_score_q8", qt.ptr(), qt.q_ld, qt.n_rows, D, L.ptr(ids), L.id_dtype_code(ids), S,
           L.ptr(offs), L.ptr(dense), B, L.ptr(q), L.ptr(c), act, y.ptr(), L.ptr(err), stream())
    torch.cuda.synchronize()
    y.check()
    return y.t.clone(), (int(err.item()) if err_flag else None)


def combos():
    """(B, id64, shared, act, oob): every batch with both id widths and both table layouts, the
    activation and the out-of-range ids in turn."""
    k = 0
    for B in R.BATCHES:
        for id64 in (False, True):
            for shared in (False, True):
                yield B, id64, shared, k % 3, k % 2 == 0
                k += 1


# ---- 1. rs_dlrm_score == rs_dlrm_interaction_fwd_head's y, D = 128 -----------------------------
@pytest.mark.parametrize("S", R.SLOTS)
def test_score_equals_fwd_head_bit_for_bit(S):
    acts = set()
    for B, id64, shared, act, oob in combos():
        inp = dev(*R.score_inputs(B, S, 128, id64, seed=S * 100 + B, shared=shared, oob=oob))
        for a in ((act,) if B != 67 else (0, 1, 2)):
            acts.add(a)
            want, werr = run_head(*inp, S, a)
            got, gerr = run_score(*inp, S, a)
            assert torch.equal(bits(got), bits(want)), f"B {B} id64 {id64} shared {shared} act {a}"
            assert gerr == werr
    assert acts == {0, 1, 2}


# ---- 2. rs_dlrm_score against float64 ----------------------------------------------------------
@pytest.mark.parametrize("D", R.DIMS)
@pytest.mark.parametrize("S", R.SLOTS)
def test_score_against_float64(S, D):
    for B, id64, shared, act, oob in combos():
        inp = R.score_inputs(B, S, D, id64, seed=S * 100 + B + D, shared=shared, oob=oob)
        _, _, y, hm, _, _, has_oob = E.head_dx_reference(*inp, S, act)
        got, err = run_score(*dev(*inp), S, act)
        assert (err != 0) == has_oob and err in (0, L.RS_ERRBIT_OOB)
        tol = R.y_tolerance(hm, y, act)
        d = (got.cpu().double() - y).abs()
        print(f"S {S} D {D} B {B} act {act}: max err/tol {float((d / (tol + 1e-30)).max()):.3g}")
        assert bool((d <= tol + 1e-30).all()), f"B {B} id64 {id64} shared {shared} act {act}"


# ---- 3. rs_dlrm_score_q8 == rs_dlrm_score over the dequantised table ---------------------------
Q8_LAYOUTS = [("default", None, 0), ("narrow", "narrow", 0), ("shift4", None, 4),
              ("shift8", None, 8), ("narrow_shift8", "narrow", 8)]


@pytest.mark.parametrize("D", R.DIMS)
@pytest.mark.parametrize("S", R.SLOTS)
def test_score_q8_equals_score_over_dequantised_bit_for_bit(S, D):
    """Every access width: the default q_ld at shifts 0 and 8 takes the 16-byte reads, a shift of
    4 or q_ld = 8 + D + 4 the 4-byte ones. The table holds every family of embedding_q8_ref (its
    overflowing rows give infinities and NaNs: equal bits are asked of those too)."""
    cards = R.uneven_cards(S)
    V = max(sum(cards), 90)
    tables = {}
    for name, ld, shift in Q8_LAYOUTS:
        _, qt = R.q8_table(D, V, None if ld is None else 8 + D + 4)
        tables[name] = QTable(qt, shift)
    deq = {name: t.dequantized(D) for name, t in tables.items()}
    for name in tables:
        assert torch.equal(bits(deq[name]), bits(deq["default"]))
    for B, id64, shared, act, oob in combos():
        _, ids, offs, dense, q, c = R.score_inputs(B, S, D, id64, seed=S * 100 + B + D,
                                                    shared=shared, oob=oob)
        ids, offs, dense, q, c = dev(ids, offs, dense, q, c)
        want, werr = run_score(deq["default"], ids, offs, dense, q, c, S, act)
        for name, t in tables.items():
            got, gerr = run_score_q8(t, ids, offs, dense, q, c, S, act)
            assert torch.equal(bits(got), bits(want)), \
                f"{name}: B {B} id64 {id64} shared {shared} act {act}"
            assert gerr == werr


@pytest.mark.parametrize("D", R.DIMS)
def test_score_q8_within_the_quantisation_bound(D):
    """Over rows whose products stay finite: the RS_Q8 kernel lies within the CPU-proven
    quantisation bound plus the fp32 bound of the float64 value over the float table."""
    S, B = 5, 67
    src = R.mild_families(D)
    V = src.shape[0]
    qt, _ = Q.quantize(src)
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, (B, S), generator=g).to(torch.int32)
    dense = E.relu_dense(B, D, g)
    q = torch.randn(E.nzc_of(S + 1) + D, generator=g) * 0.05
    c = torch.tensor([0.1])
    table = torch.from_numpy(src)
    _, _, y, hm, _, _, _ = E.head_dx_reference(table, ids, None, dense, q, c, S, 0)
    qb = torch.from_numpy(R.quant_bound(src, ids, None, dense, q, S))
    got, err = run_score_q8(QTable(qt), *dev(ids, None, dense, q, c), S, 0)
    assert err == 0
    d = (got.cpu().double() - y).abs()
    tol = qb + 1e-5 * (hm + qb)
    print(f"D {D}: max err/tol {float((d / tol).max()):.3g}")
    assert bool((d <= tol).all())


# ---- 4. ids ------------------------------------------------------------------------------------
@pytest.mark.parametrize("id64", [False, True])
@pytest.mark.parametrize("D", R.DIMS)
def test_id_edges(D, id64):
    S = 4
    cards = R.uneven_cards(S)
    B = 2 + (5 if id64 else 3) * S + 1
    table, _, offs, dense, q, c = R.score_inputs(B, S, D, id64, seed=7)
    ids, bad = E.edge_ids(B, cards, id64, seed=1)
    _, _, y, hm, _, _, has_oob = E.head_dx_reference(table, ids, offs, dense, q, c, S, 2)
    assert has_oob
    dtable, dids, doffs, ddense, dq, dc = dev(table, ids, offs, dense, q, c)
    got, err = run_score(dtable, dids, doffs, ddense, dq, dc, S, 2)
    assert err == L.RS_ERRBIT_OOB
    E.close(got.cpu(), y, 0.25 * hm + 0.03 * y, "edge ids, sigmoid")
    # the example with no valid id: act(dense·q_d + c), no table row in it
    nz = E.nzc_of(S + 1)
    lin, _ = run_score(dtable, dids, doffs, ddense, dq, dc, S, 0)
    dn, qd = dense[B - 1].double(), q[nz:nz + D].double()
    E.close(lin[B - 1:].cpu(), (dn @ qd + float(c)).reshape(1),
            (dn.abs() @ qd.abs() + abs(float(c))).reshape(1), "no valid id")
    # a NULL err_flag: the same y
    again, none = run_score(dtable, dids, doffs, ddense, dq, dc, S, 2, err_flag=False)
    assert none is None and torch.equal(bits(again), bits(got))
    # the same ids over an RS_Q8 table: a zero row and the flag as well
    src, qt = R.q8_table(D, sum(cards))
    qtab = QTable(qt)
    want, werr = run_score(qtab.dequantized(D), dids, doffs, ddense, dq, dc, S, 2)
    got8, err8 = run_score_q8(qtab, dids, doffs, ddense, dq, dc, S, 2)
    assert err8 == werr == L.RS_ERRBIT_OOB and torch.equal(bits(got8), bits(want))
    got8n, _ = run_score_q8(qtab, dids, doffs, ddense, dq, dc, S, 2, err_flag=False)
    assert torch.equal(bits(got8n), bits(want))
    # in-range ids set no flag
    clean = torch.from_numpy(np.stack([np.arange(B) % cd for cd in cards], 1)).to(ids.dtype).to(DEV)
    assert run_score(dtable, clean, doffs, ddense, dq, dc, S, 2)[1] == 0
    assert run_score_q8(qtab, clean, doffs, ddense, dq, dc, S, 2)[1] == 0


# ---- 5. repeatability --------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.DIMS)
def test_two_runs_are_bit_identical(D):
    S, B = 26, 67
    table, ids, offs, dense, q, c = dev(*R.score_inputs(B, S, D, True, seed=3, oob=True))
    a, _ = run_score(table, ids, offs, dense, q, c, S, 2)
    b, _ = run_score(table, ids, offs, dense, q, c, S, 2)
    assert torch.equal(bits(a), bits(b))
    _, qt = R.q8_table(D, table.shape[0])
    for shift in (0, 4):
        t = QTable(qt, shift)
        a, _ = run_score_q8(t, ids, offs, dense, q, c, S, 2)
        b, _ = run_score_q8(t, ids, offs, dense, q, c, S, 2)
        assert torch.equal(bits(a), bits(b))


# ---- 6. argument errors ------------------------------------------------------------------------
def test_argument_errors_leave_y_untouched():
    S, B, D = 4, 8, 128
    table, ids, offs, dense, q, c = dev(*R.score_inputs(B, S, D, False, seed=2))
    _, qt = R.q8_table(D, table.shape[0])
    qtab = QTable(qt)
    y = Y(B)
    st = stream()

    def f32(**o):
        a = dict(table=L.ptr(table), n_rows=table.shape[0], D=D, ids=L.ptr(ids), id_dtype=0,
                 n_slots=S, slot_offsets=L.ptr(offs), dense=L.ptr(dense), batch=B, q=L.ptr(q),
                 c=L.ptr(c), act=2, y=y.ptr(), err_flag=None, stream=st)
        a.update(o)
        return L.lib().rs_dlrm_score(*a.values())

    def q8(**o):
        a = dict(qtable=qtab.ptr(), q_ld=qtab.q_ld, n_rows=qtab.n_rows, D=D, ids=L.ptr(ids),
                 id_dtype=0, n_slots=S, slot_offsets=L.ptr(offs), dense=L.ptr(dense), batch=B,
                 q=L.ptr(q), c=L.ptr(c), act=2, y=y.ptr(), err_flag=None, stream=st)
        a.update(o)
        return L.lib().rs_dlrm_score_q8(*a.values())

    inv, uns = L.RS_E_INVALID, L.RS_E_UNSUPPORTED
    off4 = C.c_void_p(dense.data_ptr() + 4)
    for fn in (f32, q8):
        for over, code in ((dict(ids=None), inv), (dict(dense=None), inv), (dict(q=None), inv),
                           (dict(c=None), inv), (dict(id_dtype=2), inv), (dict(act=3), inv),
                           (dict(act=-1), inv), (dict(n_slots=0), inv), (dict(n_slots=32), inv),
                           (dict(n_rows=0), inv), (dict(batch=-1), inv), (dict(dense=off4), inv),
                           (dict(D=32), uns), (dict(D=16), uns)):
            assert fn(**over) == code, (fn.__name__, over)
    assert f32(table=None) == inv
    assert f32(table=C.c_void_p(table.data_ptr() + 4)) == inv
    assert f32(y=None) == inv and q8(y=None) == inv
    assert q8(qtable=None) == inv
    assert q8(qtable=C.c_void_p(qtab.addr + 2)) == inv
    assert q8(q_ld=8 + D - 4) == inv and q8(q_ld=8 + D + 2) == inv
    assert q8(D=256) == inv                      # q_ld < 8 + D comes first
    assert q8(D=256, q_ld=272) == uns
    assert f32(batch=0) == L.RS_OK and q8(batch=0) == L.RS_OK
    torch.cuda.synchronize()
    assert y.untouched()
    assert f32() == L.RS_OK and q8() == L.RS_OK  # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    y.check()
    assert not bool(torch.isnan(y.t).any())


# ---- 7. modules --------------------------------------------------------------------------------
def make_model(D, slab, seed=5, S=4, **kw):
    from recommender_amd.ctr.train import build_model

    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    cards = R.uneven_cards(S) if slab else None
    cards = None if cards is None else [c + 20 for c in cards]
    return build_model("DLRM", D, 120, S, E.NI, torch.device(DEV, 0), slot_cardinalities=cards,
                       bottom=[32, D], top=[32, 16, 1], generator=g, **kw), cards


def model_batch(B, S, cards, seed=9):
    g = torch.Generator().manual_seed(seed)
    if cards is None:
        ids = torch.randint(0, 120, (B, S), generator=g)
    else:
        ids = torch.stack([torch.randint(0, c, (B,), generator=g) for c in cards], 1)
    return {"cat_features": ids.to(torch.int32).to(DEV),
            "int_features": torch.rand(B, E.NI, generator=g).to(DEV)}


def model_reference(model, x, table):
    """float64 y and the tolerance parts (hm over Σ|terms| of the composed chain, the
    quantisation bound's q) from the model's parameters and its own fp32 bottom output."""
    S = model.num_cat_fea
    with torch.no_grad():
        dense = model.bottom_mlp(x["int_features"].float()).cpu()
    q, c, qm, cm = R.composed_qc(list(model.top_mlp.mlp), model.compact_rows)
    so = model.embedding_layer.slot_offsets
    offs = None if so is None else so.cpu()
    ids = x["cat_features"].cpu()
    table = table.detach().cpu()
    _, _, y, _, _, _, _ = E.head_dx_reference(table, ids, offs, dense, q, c, S, 2)
    _, _, _, hm, _, _, _ = E.head_dx_reference(table, ids, offs, dense, qm, cm, S, 2)
    return y, hm, (table, ids, offs, dense, q)


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("D", R.DIMS)
def test_model_score(D, slab):
    from recommender_amd.quantized import QuantizedEmbedding, quantize_embeddings

    B, S = 67, 4
    model, cards = make_model(D, slab)
    twin, _ = make_model(D, slab)
    x = model_batch(B, S, cards)
    y, hm, (table, ids, offs, dense, q) = model_reference(model, x, model.embedding_layer.weight)
    tol = R.y_tolerance(hm, y, 2)
    got = model.score(x)
    assert got.shape == (B,) and got.grad_fn is None and not got.requires_grad
    d = (got.cpu().double() - y).abs()
    print(f"score vs float64: max err/tol {float((d / tol).max()):.3g}")
    assert bool((d <= tol).all())
    with torch.no_grad():
        fwd = model(x)
    d = (got.cpu().double() - fwd.cpu().double()).abs()
    print(f"score vs forward: max err/tol {float((d / (2 * tol)).max()):.3g}")
    assert bool((d <= 2 * tol).all())
    # the quantised model: forward is score() over the RS_Q8 table
    assert quantize_embeddings(model) is model
    assert isinstance(model.embedding_layer, QuantizedEmbedding)
    with torch.no_grad():
        qy = model(x)
    assert qy.grad_fn is None and model(x).grad_fn is None     # with grad enabled too
    with torch.no_grad():
        twin.embedding_layer.weight.copy_(model.embedding_layer.dequantize())
    assert torch.equal(bits(qy), bits(twin.score(x)))
    qb = 0.25 * torch.from_numpy(R.quant_bound(table.numpy(), ids, offs, dense, q.abs(), S))
    d = (qy.cpu().double() - got.cpu().double()).abs()
    print(f"quantised vs float: max err/tol {float((d / (qb + 2 * tol)).max()):.3g}")
    assert bool((d <= qb + 2 * tol).all())
    assert model.embedding_layer.check_errors() == 0


def test_quantize_embeddings_dlrm_refusals():
    from recommender_amd.ctr.model import DLRM
    from recommender_amd.ctr.train import build_model
    from recommender_amd.embedding import Embedding
    from recommender_amd.quantized import quantize_embeddings

    d0 = torch.device(DEV, 0)
    loose = DLRM([32, 64], [32, 16, 1], 64, 120, 4, E.NI, device=d0, compact=False)
    narrow = build_model("DLRM", 32, 120, 4, E.NI, d0, bottom=[32, 32], top=[32, 16, 1])
    wide = build_model("DLRM", 64, 120, 32, E.NI, d0, bottom=[32, 64], top=[32, 16, 1])
    nobias, _ = make_model(64, False)
    nobias.top_mlp.mlp[1].bias = None
    for m, why in ((loose, "compact"), (narrow, "32"), (wide, "slots"), (nobias, "biases")):
        with pytest.raises(TypeError, match="DLRM") as ei:
            quantize_embeddings(m)
        assert why in str(ei.value)
        assert isinstance(m.embedding_layer, Embedding)          # nothing was swapped
    x = model_batch(5, 4, None)
    for m in (loose, narrow, nobias):
        with pytest.raises(ValueError):
            m.score(x)
