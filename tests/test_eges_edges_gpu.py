"""The kernels of csrc/eges.hip at their edges: the fused match logits, the side pooling in its
scalar, half-wave vector and multi-task forms, and the pair sampler. Inputs, float64
restatements and bounds come from tests/eges_edges.py, whose properties
tests/test_eges_edges_cpu.py proves.

The C ABI is called directly (L.call) wherever the Python wrappers hide the edge: alignment,
strides, null pointers, leading dimensions. Every output is prefilled with a NaN bit pattern
(SENT; SENT_I for ids) and has a tail behind it; strided buffers have the same pattern in their
padding. Tails, padding and inputs must come back bit-unchanged.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import eges as O
from recommender_amd import _lib as L
from recommender_amd.eges.model import match_logits, side_pool
from recommender_amd.embedding import Embedding
from recommender_amd.esmm.mmoe import _ptrs
from tests import eges_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC12345   # a quiet NaN with a payload no kernel produces
SENT_I = -0x5A5A5A5  # an id no sampler produces
TAIL = 8
GUARD = 256         # bytes behind a workspace


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent_buf(n):
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENT)
    return t


def is_sent(t):
    return bool((t.view(torch.int32) == SENT).all())


def id_buf(n):
    return torch.full((n,), SENT_I, dtype=torch.int32, device=DEV)


def bits(a):
    return E.bits(a)


def stream():
    return L.stream_ptr(torch.device(DEV))


def same_bits(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    bad = bits(got) != bits(want)
    assert not bad.any(), (f"{msg}: {int(bad.sum())} / {bad.size} elements differ in bits; first at "
                           f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} != {want[bad][0]!r}")


# =============================================================================================
# 1. match logits
def run_match(table, ids, hidden, g, id64, n_rows=None):
    """rs_match_logits_fwd and _bwd on one input → dict(logits [B, M], flag, grad_rows
    [B, M, D], grad_hidden [B, D])."""
    B, M = ids.shape
    D = table.shape[1]
    n_rows = table.shape[0] if n_rows is None else n_rows
    t, h, gg = dev(table), dev(hidden), dev(g)
    idt = dev(ids.astype(np.int64 if id64 else np.int32))
    code = L.RS_ID_I64 if id64 else L.RS_ID_I32
    logits, rows, gh = sent_buf(B * M + TAIL), sent_buf(B * M * D + TAIL), sent_buf(B * D + TAIL)
    flag = torch.tensor([0, SENT_I], dtype=torch.int32, device=DEV)
    L.call("rs_match_logits_fwd", L.ptr(t), n_rows, D, L.ptr(idt), code, M, L.ptr(h), B,
           L.ptr(logits), L.ptr(flag), stream())
    L.call("rs_match_logits_bwd", L.ptr(t), n_rows, D, L.ptr(idt), code, M, L.ptr(h), L.ptr(gg), B,
           L.ptr(rows), L.ptr(gh), stream())
    torch.cuda.synchronize()
    assert is_sent(logits[B * M:]) and is_sent(rows[B * M * D:]) and is_sent(gh[B * D:]), \
        "an output was written past its end"
    assert int(flag[1]) == SENT_I, "the word behind the error flag was written"
    assert torch.equal(t, dev(table)) and torch.equal(h, dev(hidden)) and torch.equal(gg, dev(g))
    return dict(logits=logits[:B * M].view(B, M).cpu().numpy(), flag=int(flag[0]),
                grad_rows=rows[:B * M * D].view(B, M, D).cpu().numpy(),
                grad_hidden=gh[:B * D].view(B, D).cpu().numpy())


def check_match(got, r, msg):
    E.within(got["logits"], r["logits"], E.RTOL * r["logits_mag"], f"{msg} logits")
    E.within(got["grad_hidden"], r["grad_hidden"], E.RTOL * r["grad_hidden_mag"], f"{msg} grad_hidden")
    same_bits(got["grad_rows"], r["grad_rows32"], f"{msg} grad_rows (one fp32 multiply)")


@pytest.mark.parametrize("D,M,B,id64,kind", E.MATCH_CASES)
def test_match_logits_edges(D, M, B, id64, kind):
    """The lane-stride remainder (D = 1 .. 130: zero, one, two passes of the 64 lanes and ragged
    ones), the empty waves of the last block (B = 1 .. 9), both id widths; Gaussian values, a
    cancelling set judged on Σ|terms|, an example whose M slots hold one row."""
    table, ids, hidden, g = E.match_inputs(D, M, B, kind)
    got = run_match(table, ids, hidden, g, id64)
    check_match(got, E.match_ref(table, ids, hidden, g), f"match D {D} M {M} B {B} {kind}")
    assert got["flag"] == 0, "the error flag is set though every id is valid"
    if kind == "same_row":
        same_bits(got["logits"][B - 1], np.repeat(got["logits"][B - 1, :1], M), "one row, M logits")


OOB_CASES = [(n, v, id64) for n, v, needs64 in E.oob_values() for id64 in (False, True)
             if id64 or not needs64]  # -1 and n_rows in both widths, the two 64-bit values as int64


@pytest.mark.parametrize("name,value,id64", OOB_CASES,
                         ids=[f"{n}-{'int64' if w else 'int32'}" for n, _, w in OOB_CASES])
def test_match_out_of_range_id(name, value, id64):
    """One id out of range (-1, n_rows, 2^32 + 1, the smallest int64) in one slot of one example:
    its logit is exactly 0, the flag is set, grad_hidden gets nothing from it, everything else is
    as the reference says. 2^32 + 1 and the smallest int64 alias rows 1 and 0 if truncated."""
    D, M, B = 65, 6, 5
    table, ids, hidden, g = E.match_inputs(D, M, B, "gauss")
    ids[2, 3] = value
    got = run_match(table, ids, hidden, g, id64)
    r = E.match_ref(table, ids, hidden, g)
    assert not r["valid"][2, 3] and r["valid"].sum() == B * M - 1
    assert bits(got["logits"][2, 3]) == 0, f"logit of the {name} id is {got['logits'][2, 3]!r}, not +0.0"
    assert got["flag"] & L.RS_ERRBIT_OOB, "the error flag is not set"
    check_match(got, r, f"match with id {name}")


def test_match_logits_wrapper_equals_direct_call():
    """match_logits (the autograd node) gives the direct call's bits, registers g·h as the table's
    sparse gradient rows, and raises the table's flag for an id out of range."""
    D, M, B = 130, 6, 9
    table, ids, hidden, g = E.match_inputs(D, M, B, "gauss")
    direct = run_match(table, ids, hidden, g, True)
    t = Embedding(E.MATCH_ROWS, D, device=DEV)
    with torch.no_grad():
        t.weight.copy_(dev(table))
    h = dev(hidden).view(B, 1, D).requires_grad_()
    out = match_logits(t, dev(ids), h)
    out.backward(dev(g))
    same_bits(out.detach().cpu().numpy(), direct["logits"], "logits")
    same_bits(h.grad.view(B, D).cpu().numpy(), direct["grad_hidden"], "grad_hidden")
    gid, rows = t.take_grad()
    assert np.array_equal(gid.cpu().numpy(), ids.reshape(-1))
    same_bits(rows.cpu().numpy().reshape(B, M, D), direct["grad_rows"], "grad rows")
    assert int(t.err_flag.item()) == 0
    bad = ids.copy()
    bad[0, 0] = -1
    match_logits(t, dev(bad), h.detach())
    assert int(t.err_flag.item()) & L.RS_ERRBIT_OOB


def test_match_argument_edges():
    table, ids, hidden, g = E.match_inputs(3, 1, 3, "gauss")
    t, h, gg, idt = dev(table), dev(hidden), dev(g), dev(ids)
    out, rows, gh = sent_buf(16), sent_buf(32), sent_buf(16)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fwd(n_rows, D, M, B):
        L.call("rs_match_logits_fwd", L.ptr(t), n_rows, D, L.ptr(idt), L.RS_ID_I64, M, L.ptr(h), B,
               L.ptr(out), L.ptr(flag), stream())

    def bwd(n_rows, D, M, B):
        L.call("rs_match_logits_bwd", L.ptr(t), n_rows, D, L.ptr(idt), L.RS_ID_I64, M, L.ptr(h),
               L.ptr(gg), B, L.ptr(rows), L.ptr(gh), stream())

    for f in (fwd, bwd):
        f(E.MATCH_ROWS, 3, 1, 0)  # B = 0: nothing to do
        for bad in ((0, 3, 1, 3), (E.MATCH_ROWS, 0, 1, 3), (E.MATCH_ROWS, 3, 0, 3), (E.MATCH_ROWS, 3, 1, -1)):
            with pytest.raises(L.RecsysError):
                f(*bad)
    torch.cuda.synchronize()
    assert is_sent(out) and is_sent(rows) and is_sent(gh) and int(flag) == 0


# =============================================================================================
# 2. side pooling
class SideBuf:
    """side[b, s, :] at b·sb + s·ss, `off` floats into a 16-byte aligned, SENT-filled buffer with
    a tail; everything outside the rows is padding nobody may write."""

    def __init__(self, B, S, D, layout, data=None, off=0):
        self.sb, self.ss, n = E.layout_strides(layout, B, S, D)
        self.shape, self.off = (B, S, D), off
        self.flat = sent_buf(off + n + TAIL)
        assert self.flat.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.flat, self.shape, (self.sb, self.ss, 1), off)
        if data is not None:
            self.view.copy_(dev(data))

    @property
    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + 4 * self.off)

    def numpy(self):
        return self.view.cpu().numpy()

    def padding_untouched(self):
        pad = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(pad, self.shape, (self.sb, self.ss, 1), self.off).fill_(False)
        return bool((self.flat.view(torch.int32)[pad] == SENT).all())

    def untouched(self):
        return is_sent(self.flat)


def run_pool_fwd(side, wl, layout="dense", off=0):
    """rs_side_pool_fwd_strided → (hidden [B, D], attn [B, S] or None in mean mode)."""
    B, S, D = side.shape
    X = SideBuf(B, S, D, layout, side, off)
    w = None if wl is None else dev(wl)
    hidden, attn = sent_buf(B * D + TAIL), sent_buf(B * S + TAIL)
    L.call("rs_side_pool_fwd_strided", X.ptr, X.sb, X.ss, L.ptr(w), B, S, D, L.ptr(hidden),
           L.ptr(attn), stream())
    torch.cuda.synchronize()
    assert is_sent(hidden[B * D:]) and is_sent(attn[B * S:]), "an output was written past its end"
    same_bits(X.numpy(), side, "the side rows were modified")
    assert X.padding_untouched(), "the side rows' padding was written"
    if wl is None:
        assert is_sent(attn), "mean mode wrote attn"
        return hidden[:B * D].view(B, D).cpu().numpy(), None
    assert torch.equal(w, dev(wl))
    return hidden[:B * D].view(B, D).cpu().numpy(), attn[:B * S].view(B, S).cpu().numpy()


def run_pool_bwd(side, attn32, g, layout="dense", off=0):
    """rs_side_pool_bwd_strided → (grad_side [B, S, D], grad_w [B, S] or None in mean mode)."""
    B, S, D = side.shape
    X = SideBuf(B, S, D, layout, side, off)
    G = SideBuf(B, S, D, layout, None, off)
    a = None if attn32 is None else dev(attn32)
    gg = dev(g)
    gw = sent_buf(B * S + TAIL)
    L.call("rs_side_pool_bwd_strided", X.ptr, X.sb, X.ss, L.ptr(a), L.ptr(gg), B, S, D, G.ptr,
           L.ptr(gw), stream())
    torch.cuda.synchronize()
    assert is_sent(gw[B * S:]), "grad_weight_logits was written past its end"
    same_bits(X.numpy(), side, "the side rows were modified")
    assert X.padding_untouched() and G.padding_untouched(), "padding of side / grad_side was written"
    assert torch.equal(gg, dev(g))
    if attn32 is None:
        assert is_sent(gw), "mean mode wrote grad_weight_logits"
        return G.numpy(), None
    return G.numpy(), gw[:B * S].view(B, S).cpu().numpy()


def check_pool(D, B, S, mode, layout="dense", off=0):
    side, wl, g = E.pool_inputs(D, B, S, mode)
    sb, ss, _ = E.layout_strides(layout, B, S, D)
    tag = f"pool D {D} B {B} S {S} {mode} {layout} off {off} ({E.pool_route(D, S, sb, ss, (off,))})"
    fwd = E.pool_fwd_ref(side, wl)
    hidden, attn = run_pool_fwd(side, wl, layout, off)
    if mode == "mean":
        bwd = E.pool_bwd_ref(side, None, g)
        same_bits(hidden, fwd["hidden32"], f"{tag} hidden (sum s ascending, one division)")
        gs, _ = run_pool_bwd(side, None, g, layout, off)
        same_bits(gs, bwd["grad_side32"], f"{tag} grad_side (g / float(S))")
        return
    assert np.isfinite(attn).all() and np.isfinite(hidden).all(), f"{tag}: NaN / inf in the forward"
    E.pool_check_fwd(attn, hidden, fwd, tag)
    # the backward on weights of our own (the float64 softmax rounded), not the forward's output
    bwd = E.pool_bwd_ref(side, fwd["attn32"], g)
    gs, gw = run_pool_bwd(side, fwd["attn32"], g, layout, off)
    assert np.isfinite(gs).all() and np.isfinite(gw).all(), f"{tag}: NaN / inf in the backward"
    E.pool_check_bwd(gs, gw, bwd, tag)
    same_bits(gs, fwd["attn32"][:, :, None] * g[:, None, :], f"{tag} grad_side (one fp32 multiply)")
    r = np.arange(B)
    if mode == "equal":
        same_bits(attn, np.repeat(attn[:, :1], S, 1), f"{tag}: equal logits, unequal weights")
    if mode == "spread60":
        assert (attn[r, (r + 1) % S] == 1).all() and attn.sum() == B, f"{tag}: not saturated to 1 / 0"
        same_bits(hidden, side[r, (r + 1) % S], f"{tag}: weight 1 must return the row itself")
    if mode == "neg1e30" and S >= 2:
        assert (bits(attn[r, r % S]) == 0).all(), f"{tag}: the -1e30 entry's weight is not +0.0"
        assert (gw[r, r % S] == 0).all(), f"{tag}: the -1e30 entry's grad_w is not 0"
        assert (gs[r, r % S] == 0).all()


@pytest.mark.parametrize("D,B,S,mode", E.POOL_SCALAR_CASES)
def test_side_pool_scalar_form(D, B, S, mode):
    """pool_fwd_kernel / pool_bwd_kernel: the lane-stride remainder (D = 1 .. 200), the empty
    waves of the last block, S = 1 .. 16, every logit set (the max subtraction, the underflowed
    and the -1e30 weight) and the mean."""
    check_pool(D, B, S, mode)


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("D,B,S,mode", E.POOL_VECTOR_CASES)
def test_side_pool_vector_form(D, B, S, mode, layout):
    """pool_fwd_vec_kernel / pool_bwd_vec_kernel: the half-wave tail of an odd B, the lanes past
    D / 4, dense rows, MMOE's [E, B, H] layout and padded rows (a padding write shows in the
    sentinels of side and grad_side)."""
    check_pool(D, B, S, mode, layout)


@pytest.mark.parametrize("B,S,mode", [(1, 1, "gauss"), (3, 16, "gauss"), (7, 3, "offset1e4"),
                                      (8, 15, "neg1e30"), (9, 2, "spread60"), (9, 3, "mean")])
def test_side_pool_forms_agree_at_d64(B, S, mode):
    """The same dense D = 64 rows through the vector form and, from a copy one float off 16 bytes,
    through the scalar form: the float64 bounds hold for both, hidden, attn and grad_side are
    bit-identical (the claim of csrc/eges.hip for the vector form); grad_w only meets the bound
    (the two forms fold the D sum in different orders)."""
    D = 64
    assert E.pool_route(D, S, S * D, D, (0,)) == "vector" and E.pool_route(D, S, S * D, D, (1,)) == "scalar"
    check_pool(D, B, S, mode, "dense", 0)
    check_pool(D, B, S, mode, "dense", 1)
    side, wl, g = E.pool_inputs(D, B, S, mode)
    hv, av = run_pool_fwd(side, wl, "dense", 0)
    hs, as_ = run_pool_fwd(side, wl, "dense", 1)
    same_bits(hv, hs, "hidden: vector vs scalar form")
    a32 = None
    if mode != "mean":
        same_bits(av, as_, "attn: vector vs scalar form")
        a32 = av
    gv, wv = run_pool_bwd(side, a32, g, "dense", 0)
    gs, ws_ = run_pool_bwd(side, a32, g, "dense", 1)
    same_bits(gv, gs, "grad_side: vector vs scalar form")
    if mode != "mean":
        bwd = E.pool_bwd_ref(side, a32, g)
        for w in (wv, ws_):
            E.within(w, bwd["grad_w"], E.RTOL * bwd["grad_w_mag"], "grad_w on the forward's weights")


def test_side_pool_wrapper_layouts():
    """side_pool (the autograd node) over MMOE's [E, B, H] buffer seen as [B, E, H] reads and
    writes that layout in place with the direct call's bits; a layout the kernels refuse (D = 33
    transposed) is made contiguous first."""
    for D, B, S in ((80, 7, 8), (33, 5, 3)):
        side, wl, g = E.pool_inputs(D, B, S, "gauss")
        ebh = dev(side.transpose(1, 0, 2))  # [S, B, D] contiguous
        x = ebh.transpose(0, 1).requires_grad_()
        w = dev(wl).view(B, 1, S).requires_grad_()
        out = side_pool(x, w)
        out.backward(dev(g).view(B, 1, D))
        layout = "ebh" if D % 4 == 0 else "dense"
        hidden, attn = run_pool_fwd(side, wl, layout)
        gs, gw = run_pool_bwd(side, attn, g, layout)
        same_bits(out.detach().view(B, D).cpu().numpy(), hidden, "hidden")
        same_bits(x.grad.cpu().numpy(), gs, "grad_side")
        same_bits(w.grad.view(B, S).cpu().numpy(), gw, "grad_w")
        fwd = E.pool_fwd_ref(side, wl)
        E.pool_check_fwd(attn, hidden, fwd, f"wrapper D {D}")
        # the chain the model runs: the backward on the forward's own weights
        bwd = E.pool_bwd_ref(side, attn, g)
        E.pool_check_bwd(gs, gw, bwd, f"wrapper D {D}")


def test_side_pool_routes_and_rejections():
    """Everything strided that the vector form cannot take is refused, not read with the wrong
    strides; S = 17 is refused, not overrun; a refused call writes nothing."""
    B = 3
    g = dev(np.zeros((B, 256), np.float32))
    hidden, attn, gw = sent_buf(B * 256), sent_buf(B * 32), sent_buf(B * 32)

    def both(X, G, S, D, wl):
        with pytest.raises(L.RecsysError):
            L.call("rs_side_pool_fwd_strided", X.ptr, X.sb, X.ss, L.ptr(wl), B, S, D, L.ptr(hidden),
                   L.ptr(attn), stream())
        with pytest.raises(L.RecsysError):
            L.call("rs_side_pool_bwd_strided", X.ptr, X.sb, X.ss, L.ptr(wl), L.ptr(g), B, S, D, G.ptr,
                   L.ptr(gw), stream())
        torch.cuda.synchronize()
        assert G.untouched() and is_sent(hidden) and is_sent(attn) and is_sent(gw)

    S = 3
    wl = dev(np.zeros((B, 32), np.float32))
    for D, layout, off in ((33, "padded", 0), (33, "ebh", 0), (132, "padded", 0), (200, "ebh", 0),
                           (2, "padded", 0), (64, "padded", 1), (64, "ebh", 2)):
        sb, ss, _ = E.layout_strides(layout, B, S, D)
        assert E.pool_route(D, S, sb, ss, (off,)) == "rejected"
        side = np.zeros((B, S, D), np.float32)
        both(SideBuf(B, S, D, layout, side, off), SideBuf(B, S, D, layout, None, off), S, D, wl)
    # strides that are no multiple of 4 floats at D = 64
    X, G = SideBuf(B, S, 64, "padded", np.zeros((B, S, 64), np.float32)), SideBuf(B, S, 64, "padded")
    X.sb = G.sb = X.sb + 2
    both(X, G, S, 64, wl)
    # S = 17 (and 0), in the dense and the strided entry points, both modes
    for D in (64, 33):
        for S_bad in (17, 0):
            Xd, Gd = SideBuf(B, 17, D, "dense", np.zeros((B, 17, D), np.float32)), SideBuf(B, 17, D, "dense")
            both(Xd, Gd, S_bad, D, wl)
            both(Xd, Gd, S_bad, D, None)
            for fn, args in (("rs_side_pool_fwd", (Xd.ptr, L.ptr(wl), B, S_bad, D, L.ptr(hidden), L.ptr(attn))),
                             ("rs_side_pool_bwd", (Xd.ptr, L.ptr(wl), L.ptr(g), B, S_bad, D, Gd.ptr, L.ptr(gw)))):
                with pytest.raises(L.RecsysError):
                    L.call(fn, *args, stream())
    # B = 0 does nothing, and the dense entry points route as the strided ones do
    L.call("rs_side_pool_fwd_strided", None, 12, 4, None, 0, 3, 4, None, None, stream())
    side, wlg, gg = E.pool_inputs(64, 7, 3, "gauss")
    s, w, h, a = dev(side), dev(wlg), sent_buf(7 * 64), sent_buf(7 * 3)
    L.call("rs_side_pool_fwd", L.ptr(s), L.ptr(w), 7, 3, 64, L.ptr(h), L.ptr(a), stream())
    torch.cuda.synchronize()
    hv, av = run_pool_fwd(side, wlg)
    same_bits(h.view(7, 64).cpu().numpy(), hv, "rs_side_pool_fwd vs _strided")
    same_bits(a.view(7, 3).cpu().numpy(), av, "rs_side_pool_fwd vs _strided")
    assert is_sent(hidden) and is_sent(attn) and is_sent(gw)


# ---- multi form ----------------------------------------------------------------------------
def run_multi(side, wl, g, layout, bias=None, attn_in=None):
    """rs_side_pool_fwd_multi then rs_side_pool_bwd_multi (on attn_in, default the forward's own
    weights) → dict(side (after the call), hidden [T], attn [T], grad_side, grad_w [T])."""
    T, B, S = wl.shape
    D = side.shape[2]
    ld = T * S + E.MULTI_EXTRA_LD
    X = SideBuf(B, S, D, layout, side)
    Z = sent_buf(B * ld + TAIL)  # the unused columns hold NaN: reading one poisons a softmax
    Zv = Z[:B * ld].view(B, ld)
    for t in range(T):
        Zv[:, t * S:(t + 1) * S] = dev(wl[t])
    z_before = Z.clone()
    hid = [sent_buf(B * D + TAIL) for _ in range(T)]
    att = [sent_buf(B * S + TAIL) for _ in range(T)]
    bt = None if bias is None else dev(bias)
    st = stream()
    L.call("rs_side_pool_fwd_multi", X.ptr, X.sb, X.ss, B, S, D, T,
           _ptrs([Zv[:, t * S:] for t in range(T)]), ld, _ptrs(hid), _ptrs(att), L.ptr(bt), st)
    torch.cuda.synchronize()
    assert torch.equal(Z.view(torch.int32), z_before.view(torch.int32)), "the logits were modified"
    assert all(is_sent(h[B * D:]) for h in hid) and all(is_sent(a[B * S:]) for a in att)
    assert X.padding_untouched(), "the side rows' padding was written"
    side_after = X.numpy()
    if bias is None:
        same_bits(side_after, side, "the side rows were modified without a bias")
    a_in = [a[:B * S].clone() for a in att] if attn_in is None else [dev(a).reshape(-1) for a in attn_in]
    gh = [dev(g[t]) for t in range(T)]
    G = SideBuf(B, S, D, layout)
    dZ = sent_buf(B * ld + TAIL)
    dZv = dZ[:B * ld].view(B, ld)
    L.call("rs_side_pool_bwd_multi", X.ptr, X.sb, X.ss, B, S, D, T, _ptrs(a_in), _ptrs(gh), G.ptr,
           _ptrs([dZv[:, t * S:] for t in range(T)]), ld, st)
    torch.cuda.synchronize()
    assert G.padding_untouched() and X.padding_untouched()
    assert is_sent(dZ[B * ld:]) and is_sent(dZv[:, T * S:].contiguous()), \
        "the logit gradient's extra columns were written"
    same_bits(X.numpy(), side_after, "the backward modified the side rows")
    return dict(side=side_after,
                hidden=[h[:B * D].view(B, D).cpu().numpy() for h in hid],
                attn=[a[:B * S].view(B, S).cpu().numpy() for a in att],
                grad_side=G.numpy(),
                grad_w=[dZv[:, t * S:(t + 1) * S].cpu().numpy() for t in range(T)])


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("layout", ["ebh", "padded"])
@pytest.mark.parametrize("T,Ex,H,B,kind", E.MULTI_CASES)
def test_side_pool_multi_form(T, Ex, H, B, kind, layout, bias):
    """pool_fwd_multi_kernel / pool_bwd_multi_kernel against the float64 reference of T
    independent poolings and the task-ordered sum of their side gradients, and bit-equal to T
    single-task calls; the leading dimensions of the logit buffers are wider than the tasks'
    blocks; with a bias the rows become relu(z + bias[s]) in place, bit for bit."""
    z, wl, g, b = E.multi_inputs(T, Ex, H, B, kind, with_bias=bias)
    got = run_multi(z, wl, g, layout, b)
    side = z
    if bias:
        side = E.relu_bias32(z, b)
        same_bits(got["side"], side, "side after relu(z + bias[s]) in place")
    tag = f"multi T {T} E {Ex} H {H} B {B} {kind} {layout}"
    singles = []
    for t in range(T):
        fwd = E.pool_fwd_ref(side, wl[t])
        E.pool_check_fwd(got["attn"][t], got["hidden"][t], fwd, f"{tag} task {t}")
        bwd = E.pool_bwd_ref(side, got["attn"][t], g[t])
        E.within(got["grad_w"][t], bwd["grad_w"], E.RTOL * bwd["grad_w_mag"], f"{tag} task {t} grad_w")
        h1, a1 = run_pool_fwd(side, wl[t], layout)
        gs1, gw1 = run_pool_bwd(side, a1, g[t], layout)
        same_bits(got["hidden"][t], h1, f"{tag} task {t} hidden vs the single-task call")
        same_bits(got["attn"][t], a1, f"{tag} task {t} attn vs the single-task call")
        same_bits(got["grad_w"][t], gw1, f"{tag} task {t} grad_w vs the single-task call")
        singles.append(gs1)
    ref, mag = E.multi_grad_side_ref(got["attn"], list(g))
    E.within(got["grad_side"], ref, E.RTOL * mag, f"{tag} grad_side")
    acc = singles[0]
    for s in singles[1:]:
        acc = (acc + s).astype(np.float32)
    same_bits(got["grad_side"], acc, f"{tag} grad_side vs the single-task calls summed in task order")
    same_bits(got["grad_side"], E.multi_grad_side_sum32(got["attn"], list(g)),
              f"{tag} grad_side vs the fp32 products summed in task order")
    assert all(np.isfinite(a).all() for a in got["attn"] + got["hidden"] + got["grad_w"])


def test_side_pool_multi_rejections():
    """T = 5, S = 17, D = 132 / 6, a misaligned side_bias, hidden[t], grad_hidden[t] or grad_side
    and a leading dimension below S are refused; a refused call writes nothing."""
    B, S, D = 3, 4, 8
    X, G = SideBuf(B, 17, D, "dense", np.zeros((B, 17, D), np.float32)), SideBuf(B, 17, D, "dense")
    wl = dev(np.zeros((B, 64), np.float32))
    hid = [sent_buf(B * D + 4) for _ in range(5)]
    att = [sent_buf(B * 17) for _ in range(5)]
    gws = [sent_buf(B * 17) for _ in range(5)]
    bias = sent_buf(17 * D + 4)
    x_before = X.flat.clone()

    def off1(t):
        return t[1:]  # 4 bytes past a 16-byte boundary

    def fwd(S=S, D=D, T=2, ld=64, h=hid, b=None, sb=None):
        L.call("rs_side_pool_fwd_multi", X.ptr, S * D if sb is None else sb, D, B, S, D, T,
               _ptrs([wl] * 5), ld, _ptrs(h), _ptrs(att), L.ptr(b), stream())

    def bwd(S=S, D=D, T=2, ld=64, gh=hid, gs=None):
        L.call("rs_side_pool_bwd_multi", X.ptr, S * D, D, B, S, D, T, _ptrs(att), _ptrs(gh),
               G.ptr if gs is None else L.ptr(gs), _ptrs(gws), ld, stream())

    for f in (fwd, bwd):
        for kw in (dict(T=5), dict(T=0), dict(S=17), dict(S=0), dict(D=132), dict(D=6), dict(ld=S - 1)):
            with pytest.raises(L.RecsysError):
                f(**kw)
    with pytest.raises(L.RecsysError):
        fwd(b=off1(bias))
    with pytest.raises(L.RecsysError):
        fwd(h=[hid[0], off1(hid[1])] + hid[2:])
    with pytest.raises(L.RecsysError):
        fwd(sb=S * D + 2)
    with pytest.raises(L.RecsysError):
        bwd(gh=[hid[0], off1(hid[1])] + hid[2:])
    with pytest.raises(L.RecsysError):
        bwd(gs=off1(G.flat))
    torch.cuda.synchronize()
    assert torch.equal(X.flat.view(torch.int32), x_before.view(torch.int32)) and G.untouched()
    assert all(is_sent(t) for t in hid + att + gws + [bias])


# =============================================================================================
# 3. pair sampler
SENT_D = 0x7FF8000012345678  # a float64 NaN pattern


def graph_on_device(n_nodes):
    indptr, indices, w = E.edge_graph(n_nodes)
    return dev(indptr), dev(indices), dev(w)


def run_prefix(n_nodes):
    ip, _, w = graph_on_device(n_nodes)
    cum = torch.empty(w.numel() + TAIL, dtype=torch.float64, device=DEV)
    cum.view(torch.int64).fill_(SENT_D)
    L.call("rs_csr_weight_prefix", L.ptr(ip), L.ptr(w), n_nodes, L.ptr(cum), stream())
    torch.cuda.synchronize()
    assert bool((cum[w.numel():].view(torch.int64) == SENT_D).all()), "prefix written past the edges"
    return cum


@pytest.mark.parametrize("n_nodes", E.GRAPH_NODES)
def test_weight_prefix_bit_exact(n_nodes):
    """Node counts on both sides of a 256-thread block; empty nodes, a 1200-edge node, a denormal
    and a 1e30 weight: the sequential float64 prefix of the oracle, bit for bit."""
    indptr, _, w = E.edge_graph(n_nodes)
    cum = run_prefix(n_nodes)[:w.size].cpu().numpy()
    assert np.array_equal(cum.view(np.uint64), O.weight_prefix(indptr, w).view(np.uint64))
    # fewer nodes than the graph has: the edges of the others are left alone
    ip, _, wt = graph_on_device(n_nodes)
    part = torch.zeros(w.size, dtype=torch.float64, device=DEV)
    L.call("rs_csr_weight_prefix", L.ptr(ip), L.ptr(wt), 2, L.ptr(part), stream())
    L.call("rs_csr_weight_prefix", L.ptr(ip), L.ptr(wt), 0, L.ptr(part), stream())
    torch.cuda.synchronize()
    assert np.array_equal(part.cpu().numpy()[:indptr[2]], cum[:indptr[2]]) and not part[int(indptr[2]):].any()


@pytest.mark.parametrize("n_nodes", E.GRAPH_NODES)
@pytest.mark.parametrize("length", E.WALK_LENGTHS)
@pytest.mark.parametrize("n_walks", E.WALK_COUNTS)
def test_walks_edges(n_walks, length, n_nodes):
    """n_walks around one 256-thread block, lengths 0, 1 and 12, n_items = 2 (every walk starts
    at node 1, the 1200-edge hub), a walk base past 2^31: bit-exact against the oracle, every
    step along an edge of positive weight (a weight-0 edge first, last or inside a node's list
    leads to node 0, which nothing else reaches), -1 from a dead end on."""
    g = indptr, indices, w = E.edge_graph(n_nodes)
    ip, ix, _ = graph_on_device(n_nodes)
    cum = run_prefix(n_nodes)
    n = n_walks * (length + 1)
    tr = id_buf(n + TAIL)
    L.call("rs_eges_walks", L.ptr(ip), L.ptr(ix), L.ptr(cum), 2, E.WALK_BASE, n_walks, length, E.SEED,
           E.STEP, L.ptr(tr), stream())
    torch.cuda.synchronize()
    assert bool((tr[n:] == SENT_I).all()), "traces written past their end"
    got = tr[:n].view(n_walks, length + 1).cpu().numpy()
    assert (got[:, 0] == 1).all()
    E.check_walks(g, got, 2)
    ref = O.weighted_walks(indptr, indices, O.weight_prefix(indptr, w), 2, E.WALK_BASE, n_walks, length,
                           E.SEED, E.STEP)
    assert np.array_equal(got, ref)
    if n_walks >= 255 and length == 12:
        assert (got == -1).any() and E.N_OOV not in got


def test_walks_argument_edges():
    ip, ix, _ = graph_on_device(200)
    cum = run_prefix(200)
    tr = id_buf(64)
    for n_items, n_walks, length in ((1, 4, 3), (2, -1, 3), (2, 4, -1)):
        with pytest.raises(L.RecsysError):
            L.call("rs_eges_walks", L.ptr(ip), L.ptr(ix), L.ptr(cum), n_items, 0, n_walks, length, E.SEED,
                   E.STEP, L.ptr(tr), stream())
    L.call("rs_eges_walks", L.ptr(ip), L.ptr(ix), L.ptr(cum), 2, 0, 0, 3, E.SEED, E.STEP, L.ptr(tr), stream())
    torch.cuda.synchronize()
    assert bool((tr == SENT_I).all())


@pytest.mark.parametrize("name,n_traces,length,window,fill", E.SKIPGRAM_CASES,
                         ids=[c[0] for c in E.SKIPGRAM_CASES])
def test_skipgram_pairs_edges(name, n_traces, length, window, fill):
    """len = 1 (no slot), window >= len, window 1, no traces, 0 and -1 at the first, the last and
    an inner position, all valid, all dead, and slot counts on both sides of the scan's 4096
    tile: the count, the pairs in enumeration order, nothing written behind them."""
    traces = E.skipgram_traces(n_traces, length, fill)
    slots = E.skipgram_slots(length, window)
    cap = n_traces * slots
    t = dev(traces) if n_traces else id_buf(4)
    nbytes = L.lib().rs_skipgram_workspace_size(n_traces, length, window)
    ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    tgt, ctx = id_buf(cap + TAIL), id_buf(cap + TAIL)
    cnt = torch.tensor([SENT_I, SENT_I], dtype=torch.int32, device=DEV)
    L.call("rs_skipgram_pairs", L.ptr(t), n_traces, length, window, L.ptr(tgt), L.ptr(ctx), L.ptr(cnt),
           L.ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    rt, rc = E.skipgram_ref(traces, window)
    ot, oc = O.skipgram_pairs(traces, window)
    m = int(cnt[0])
    assert int(cnt[1]) == SENT_I and bool((ws[nbytes:] == 0xA5).all()), "count / workspace overrun"
    assert m == rt.size == ot.size, f"{name}: n_pairs {m}, expected {rt.size}"
    got_t, got_c = tgt[:m].cpu().numpy(), ctx[:m].cpu().numpy()
    assert np.array_equal(got_t, rt) and np.array_equal(got_c, rc), f"{name}: pairs differ"
    assert np.array_equal(got_t, ot) and np.array_equal(got_c, oc), f"{name}: pairs differ from the oracle"
    assert bool((tgt[m:] == SENT_I).all()) and bool((ctx[m:] == SENT_I).all()), \
        f"{name}: written behind n_pairs"
    if n_traces:
        assert torch.equal(t, dev(traces))


def test_skipgram_argument_edges():
    t, out, cnt = id_buf(16), id_buf(64), id_buf(2)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    for n, ln, wd in ((-1, 4, 2), (2, 0, 2), (2, 4, 0)):
        with pytest.raises(L.RecsysError):
            L.call("rs_skipgram_pairs", L.ptr(t), n, ln, wd, L.ptr(out), L.ptr(out), L.ptr(cnt), L.ptr(ws),
                   4096, stream())
    need = L.lib().rs_skipgram_workspace_size(4, 4, 2)
    with pytest.raises(L.RecsysError, match="workspace too small"):
        L.call("rs_skipgram_pairs", L.ptr(t), 4, 4, 2, L.ptr(out), L.ptr(out), L.ptr(cnt), L.ptr(ws),
               need - 512, stream())
    torch.cuda.synchronize()
    assert bool((out == SENT_I).all()) and bool((cnt == SENT_I).all())


def run_negatives(cdf, range_max, n_pairs, ns, base=E.NEG_PAIR_BASE):
    table = dev(np.asarray(cdf, np.uint32).view(np.int32))
    out = id_buf(n_pairs * ns + TAIL)
    err = torch.tensor([0, SENT_I], dtype=torch.int32, device=DEV)
    L.call("rs_log_uniform_sample", L.ptr(table), range_max, base, n_pairs, ns, E.SEED, E.STEP,
           L.ptr(out), L.ptr(err), stream())
    torch.cuda.synchronize()
    assert bool((out[n_pairs * ns:] == SENT_I).all()) and int(err[1]) == SENT_I, "output overrun"
    return out[:n_pairs * ns].view(n_pairs, ns).cpu().numpy(), int(err[0])


@pytest.mark.parametrize("range_max,ns,n_pairs", E.NEG_CASES)
def test_log_uniform_negatives_edges(range_max, ns, n_pairs):
    """One- and two-class tables, num_sampled == range_max (a permutation of every class), a
    2^20 + 3 class table (the float inverse-CDF guess misses and the walk along the table takes
    over), n_pairs around one block, a pair base past 2^31: bit-exact ids, distinct, in range,
    no error."""
    cdf = E.log_uniform_cdf(range_max)
    out, err = run_negatives(cdf, range_max, n_pairs, ns)
    assert err == 0
    E.check_negatives(out, range_max, ns)
    assert np.array_equal(out, E.log_uniform_ref(cdf, E.NEG_PAIR_BASE, n_pairs, ns, E.SEED, E.STEP))
    if n_pairs * ns <= 1500:  # the oracle itself where its Python loop is short
        assert np.array_equal(out, O.log_uniform_sample(cdf, E.NEG_PAIR_BASE, n_pairs, ns, E.SEED, E.STEP))


@pytest.mark.parametrize("kind", ["down", "up"])
def test_log_uniform_guess_far_from_the_answer(kind):
    """Hand-made tables (tests/eges_edges.py skewed_cdf) on which the float inverse-CDF guess is
    hundreds of classes above ('down') or below ('up') the first class whose entry exceeds the
    draw: the walk along the table in either direction, and its stop at the last class when no
    entry exceeds the draw. Bit-exact against the oracle's search of the same table."""
    cdf = E.skewed_cdf(kind)
    out, err = run_negatives(cdf, E.SKEW_RANGE, E.SKEW_PAIRS, E.SKEW_SAMPLED)
    assert err == 0
    E.check_negatives(out, E.SKEW_RANGE, E.SKEW_SAMPLED)
    assert np.array_equal(out, O.log_uniform_sample(cdf, E.NEG_PAIR_BASE, E.SKEW_PAIRS, E.SKEW_SAMPLED,
                                                    E.SEED, E.STEP))
    if kind == "down":
        assert out.max() <= 30
    else:
        assert (out == E.SKEW_RANGE - 1).any(1).mean() > 0.9  # the clamp to the last class


def test_log_uniform_bounded_retry():
    """A table of 0xFFFFFFFF in all four classes makes class 0 the only one a draw can give: after
    the kernel's own bound of 4096 · num_sampled draws every row is [0, 0] and the error flag is
    set (the oracle has no such bound and would not return)."""
    cdf = np.full(E.RETRY_RANGE, 0xFFFFFFFF, np.uint32)
    out, err = run_negatives(cdf, E.RETRY_RANGE, E.RETRY_PAIRS, E.RETRY_SAMPLED)
    assert np.array_equal(out, np.zeros((E.RETRY_PAIRS, E.RETRY_SAMPLED), np.int32))
    assert err & L.RS_ERRBIT_OOB, "the error flag is not set"


def test_log_uniform_argument_edges():
    table, out = dev(E.log_uniform_cdf(4).view(np.int32)), id_buf(32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for rng_max, n, ns in ((0, 2, 1), (4, 2, 0), (4, 2, 5), (4, -1, 2)):
        with pytest.raises(L.RecsysError):
            L.call("rs_log_uniform_sample", L.ptr(table), rng_max, 0, n, ns, E.SEED, E.STEP, L.ptr(out),
                   L.ptr(err), stream())
    L.call("rs_log_uniform_sample", L.ptr(table), 4, 0, 0, 2, E.SEED, E.STEP, L.ptr(out), L.ptr(err),
           stream())
    torch.cuda.synchronize()
    assert bool((out == SENT_I).all()) and int(err) == 0
