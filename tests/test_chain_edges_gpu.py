"""The factored MLP-chain kernels of csrc/dense.hip at their dispatch and fold edges:
rs_chain_reduce (vec, quad and outer kernels, the two-level fold), rs_chain3_vec_grads,
rs_chain3_vec_compose, rs_chain_aug_product, rs_chain_rt_product, rs_chain_outer,
rs_affine_narrow_fwd, rs_rowdot_act and the grouped rs_dlrm_dense_tail. Cases, inputs,
references and bounds come from tests/chain_edges.py, whose properties
tests/test_chain_edges_cpu.py proves.

The C ABI is called directly. Two kinds of input per kernel: small integers, whose result is
exact in fp32 in any summation order and is compared bit for bit with the int64 evaluation (a
dropped, doubled or mis-indexed row, phase, chunk, segment or wave shows), and Gaussians, compared
with float64 within the derived summation bound. Every buffer sits between guard words of a NaN
bit pattern (SENT) that must come back untouched, every output and workspace is prefilled with
it (an unwritten partial that is read shows), the workspace is passed with its reported size, and
every call is made twice: the results are bit-identical.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from recommender_amd import nn as NN
from tests import chain_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC12345  # a quiet NaN with a payload no kernel produces
GUARD = 64         # floats of guard on either side (a multiple of 4: alignment is `off` alone)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent_buf(n):
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENT)
    return t


def is_sent(t):
    return bool((t.contiguous().view(torch.int32) == SENT).all())


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def exact(got, ref64):
    """Bit for bit against the integer evaluation, up to the sign of a zero (x + 0 turns -0 into
    +0 and leaves every other value, a NaN guard pattern included, alone)."""
    want = np.asarray(ref64, np.float64).astype(F32)
    return got.shape == want.shape and np.array_equal(bits(got + F32(0)), bits(want + F32(0)))


def stream():
    return L.stream_ptr(torch.device(DEV))


class Buf:
    """`shape` floats that start `off` floats past a 16-byte boundary, inside a SENT-filled
    buffer with GUARD floats on either side; data None leaves the floats SENT (an output)."""

    def __init__(self, shape, data=None, off=0):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.n = int(np.prod(self.shape))
        self.lo = GUARD + off
        self.flat = sent_buf(self.lo + self.n + GUARD)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.lo:self.lo + self.n].view(self.shape)
        if data is not None:
            assert tuple(data.shape) == self.shape, (data.shape, self.shape)
            self.view.copy_(dev(np.asarray(data, F32)))

    @property
    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + 4 * self.lo)

    def at(self, k):
        """Pointer to float k of the data."""
        return C.c_void_p(self.flat.data_ptr() + 4 * (self.lo + k))

    def numpy(self):
        return self.view.cpu().numpy()

    def guards_ok(self):
        return is_sent(self.flat[:self.lo]) and is_sent(self.flat[self.lo + self.n:])

    def untouched(self):
        return is_sent(self.flat)

    def reset(self):
        self.flat.view(torch.int32).fill_(SENT)


def opt(buf):
    return None if buf is None else buf.ptr


def ratio(err, bound):
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0).max(initial=0))


def within(got, ref, bound, msg):
    err = np.abs(got.astype(np.float64) - ref)
    print(f"  {msg}: max err/bound {ratio(err, bound):.3g}")
    assert np.isfinite(got).all() and (err <= bound).all(), \
        f"{msg}: {int((~(err <= bound)).sum())} / {err.size} elements off ({ratio(err, bound):.3g} x bound)"


def twice(outs, call, ws=None):
    """Run `call` twice from SENT-filled outputs (and workspace) → {name: array} of the first
    run; the second is bit-identical and no guard word changed."""
    res = []
    for _ in range(2):
        for b in outs.values():
            b.reset()
        if ws is not None:
            ws.view(torch.int32).fill_(SENT)
        call()
        torch.cuda.synchronize()
        res.append({k: b.numpy() for k, b in outs.items()})
    for k, b in outs.items():
        assert b.guards_ok(), f"{k}: guard written"
        assert same_bits(res[0][k], res[1][k]), f"{k}: a second call differs"
    return res[0]


def inputs_intact(*pairs):
    for b, data in pairs:
        if b is not None:
            assert b.guards_ok() and same_bits(b.numpy(), np.asarray(data, F32)), "an input was modified"


# =============================================================================================
# 1. rs_chain_reduce
def run_reduce(c, act, x, dy, y, with_g=True):
    """→ (out [n0·nl + nl], G [B, nl] or None)."""
    B, n0, nl = c.B, c.n0, c.nl
    X, DY, Y = Buf(x.shape, x), Buf(dy.shape, dy, c.dy_off), Buf(y.shape, y, c.y_off)
    outs = dict(out=Buf(n0 * nl + nl))
    if with_g:
        outs["g"] = Buf((B, nl), off=c.g_off)
    nbytes = L.lib().rs_chain_reduce_workspace_size(B, n0, nl)
    assert nbytes == E.reduce_workspace_bytes(B, n0, nl)
    ws = sent_buf(nbytes // 4 + GUARD)
    r = twice(outs, lambda: L.call("rs_chain_reduce", X.ptr, x.shape[1], n0, DY.ptr, Y.ptr, nl, act, B,
                                   outs["out"].ptr, opt(outs.get("g")), L.ptr(ws), nbytes, stream()), ws)
    assert is_sent(ws[nbytes // 4:]), "workspace guard written"
    inputs_intact((X, x), (DY, dy), (Y, y))
    return r["out"], r.get("g")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("c", E.REDUCE_CASES, ids=str)
def test_reduce_integer_exact(c, act):
    """A, s and G of integer inputs equal the int64 evaluation bit for bit, with g_out given and
    with g_out NULL (for the g_out-misaligned cases that is the quad kernel instead of outer)."""
    x, dy, y = E.reduce_inputs(c, act, "int")
    ref, G, mag = E.reduce_ref(x, dy, y, act, c.n0)
    assert mag.max(initial=0) < E.TWO24
    out, g = run_reduce(c, act, x, dy, y)
    reg = E.case_regime(c)
    assert exact(out, ref), f"{reg}: out differs at {np.flatnonzero(out != ref.astype(F32))[:8]}"
    assert exact(g, G), "g_out differs"
    out2, _ = run_reduce(c, act, x, dy, y, with_g=False)
    assert exact(out2, ref), f"g_out NULL ({E.case_regime(c, has_g=False)['kernel']}): out differs"


@pytest.mark.parametrize("c", E.REDUCE_CASES, ids=str)
def test_reduce_sigmoid_within_the_summation_bound(c):
    x, dy, y = E.reduce_inputs(c, 2, "gauss")
    ref, G, mag = E.reduce_ref(x, dy, y, 2, c.n0)
    out, g = run_reduce(c, 2, x, dy, y)
    reg = E.case_regime(c)
    within(g, G, E.SIGMOID_RTOL * np.abs(G), f"G {tuple(c)}")
    within(out, ref, E.reduce_bound(mag, reg, c.B, 2), f"out {reg['kernel']} {tuple(c)}")
    out2, _ = run_reduce(c, 2, x, dy, y, with_g=False)
    within(out2, ref, E.reduce_bound(mag, E.case_regime(c, has_g=False), c.B, 2), "out, g_out NULL")


REFUSALS = {  # name: (n0, nl, ldx, act, x_off, y NULL, bytes short)
    "n0 33 nl 2": (33, 2, 33, 0, 0, False, 0),
    "nl 257": (1, 257, 1, 0, 0, False, 0),
    "nl 1 n0 1028": (1028, 1, 1028, 0, 0, False, 0),
    "nl 1 n0 6": (6, 1, 8, 0, 0, False, 0),
    "nl 1 ldx n0+2": (4, 1, 6, 0, 0, False, 0),
    "nl 1 x misaligned": (4, 1, 4, 0, 1, False, 0),
    "act 3": (4, 4, 4, 3, 0, False, 0),
    "act 1 y NULL": (4, 4, 4, 1, 0, True, 0),
    "workspace one byte short": (4, 4, 4, 1, 0, False, 1),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_reduce_refusals_leave_the_outputs_untouched(name):
    n0, nl, ldx, act, x_off, y_null, short = REFUSALS[name]
    B = 5
    assert short or not E.reduce_accepts(n0, nl, ldx, act, B, not y_null, x_off)
    assert E.reduce_accepts(4, 4, 4, 1, B) and E.reduce_accepts(4, 1, 4, 0, B)  # the neighbours
    X, DY, Y = Buf((B, ldx), np.ones((B, ldx), F32), x_off), Buf((B, nl), np.ones((B, nl), F32)), \
        Buf((B, nl), np.ones((B, nl), F32))
    OUT, G = Buf(n0 * nl + nl), Buf((B, nl))
    nbytes = L.lib().rs_chain_reduce_workspace_size(B, n0, nl)
    ws = sent_buf(nbytes // 4 + GUARD)
    with pytest.raises(L.RecsysError, match="rs_chain_reduce"):
        L.call("rs_chain_reduce", X.ptr, ldx, n0, DY.ptr, None if y_null else Y.ptr, nl, act, B,
               OUT.ptr, G.ptr, L.ptr(ws), nbytes - short, stream())
    torch.cuda.synchronize()
    assert OUT.untouched() and G.untouched() and is_sent(ws)


def _count_calls(monkeypatch):
    calls, orig = [], L.call

    def spy(fn, *a):
        calls.append(fn)
        return orig(fn, *a)

    monkeypatch.setattr(L, "call", spy)
    return calls


@pytest.mark.parametrize("n0,nl,pad,x_off,act", [
    (4, 1, 0, 0, 2), (512, 1, 4, 0, 0), (32, 2, 3, 0, 1), (17, 12, 0, 1, 2),   # fused
    (33, 2, 0, 0, 2), (4, 1, 0, 1, 2), (6, 1, 2, 0, 0), (4, 1, 2, 0, 1)])       # torch fallback
def test_nn_chain_reduce_routes_by_the_restated_predicate(monkeypatch, n0, nl, pad, x_off, act):
    """nn.chain_reduce takes the fused call exactly when nn_routes_fused says so; either way A, s
    and G are within the Gaussian bound (129 rows: any summation order of 129 terms is no deeper
    than the bound's depth, so it holds for the fallback's library GEMM too)."""
    B = 129
    c = E.RC(n0, nl, pad, B)
    x, dy, y = E.reduce_inputs(c, act, "gauss")
    ref, G, mag = E.reduce_ref(x, dy, y, act, n0)
    X = Buf(x.shape, np.nan_to_num(x), x_off)
    xt = torch.as_strided(X.flat, (B, n0), (n0 + pad, 1), X.lo)
    assert xt.data_ptr() % 16 == 4 * x_off
    calls = _count_calls(monkeypatch)
    g, A, s = NN.chain_reduce(xt, dev(dy), None if act == 0 else dev(y), act)
    torch.cuda.synchronize()
    fused = E.nn_routes_fused(n0, nl, n0 + pad, x_off)
    assert ("rs_chain_reduce" in calls) == fused, calls
    if fused:
        assert calls == ["rs_chain_reduce"]
        assert E.reduce_accepts(n0, nl, n0 + pad, act, B, True, x_off)
    if fused:
        reg = E.reduce_regime(n0, nl)
    else:  # the bound of the nearest fused shape: at least as deep as any order of B terms
        reg = E.reduce_regime(min(n0, 32), nl) if nl > 1 else E.reduce_regime(4 * (n0 // 4), 1)
        assert E.reduce_depth(reg, B) >= B
    bound = E.reduce_bound(mag, reg, B, act)
    assert tuple(A.shape) == (n0, nl) and tuple(s.shape) == (nl,)
    got = np.concatenate([A.cpu().numpy().reshape(-1), s.cpu().numpy()])
    within(got, ref, bound, f"A, s (fused {fused})")
    within(g.cpu().numpy(), G, E.SIGMOID_RTOL * np.abs(G) if act == 2 else 0 * G, "G")


# =============================================================================================
# 2. rs_chain3_vec_grads / rs_chain3_vec_compose
def _i32(a):
    return None if a is None else dev(a.astype(np.int32))


GRAD_OUTS = ("dK1", "db1", "dK2", "db2", "dK3", "db3", "p")


def run_chain3(c, d):
    """Both entry points on one set of inputs → {dK1, db1, dK2, db2, dK3, db3, p, q, c}."""
    nf, n0, n1, n2 = d["n_full0"], c.n0, c.n1, c.n2
    I = {k: (None if d[k] is None else Buf(d[k].shape, d[k])) for k in ("K1", "K2", "K3", "b1", "b2", "b3", "A", "s")}
    rows, inv = _i32(d["rows"]), _i32(d["inv"])
    outs = dict(dK1=Buf((nf, n1)), db1=Buf(n1), dK2=Buf((n1, n2)), db2=Buf(n2), dK3=Buf(n2), db3=Buf(1),
                p=Buf(n0))
    nb = (2 * n1 + 2 * n2) * 4
    ws = sent_buf(nb // 4 + GUARD)
    r = twice(outs, lambda: L.call(
        "rs_chain3_vec_grads", I["K1"].ptr, L.ptr(rows), L.ptr(inv), nf, n0, opt(I["b1"]), I["K2"].ptr,
        opt(I["b2"]), I["K3"].ptr, n1, n2, I["A"].ptr, I["s"].ptr, *(outs[k].ptr for k in GRAD_OUTS),
        L.ptr(ws), nb, stream()), ws)
    assert is_sent(ws[nb // 4:]), "grads: workspace guard written"
    outs2 = dict(q=Buf(n0), c=Buf(1))
    nb2 = (n1 + 1) * 4
    ws2 = sent_buf(nb2 // 4 + GUARD)
    r.update(twice(outs2, lambda: L.call(
        "rs_chain3_vec_compose", I["K1"].ptr, L.ptr(rows), n0, opt(I["b1"]), I["K2"].ptr, opt(I["b2"]),
        I["K3"].ptr, opt(I["b3"]), n1, n2, outs2["q"].ptr, outs2["c"].ptr, L.ptr(ws2), nb2, stream()), ws2))
    assert is_sent(ws2[nb2 // 4:]), "compose: workspace guard written"
    inputs_intact(*((I[k], d[k]) for k in I))
    return r


def chain3_refs(d):
    v, e, _ = E.chain3_grads_ref(d)
    vc, ec, _ = E.chain3_compose_ref(d)
    return {**v, **vc}, {**e, **ec}


@pytest.mark.parametrize("c", E.CHAIN3_CASES, ids=str)
def test_chain3_integer_exact(c):
    """Every output of both entry points; with a rows subset the rows of dK1 outside it are 0."""
    d = E.chain3_inputs(c, "int")
    v, _ = chain3_refs(d)
    r = run_chain3(c, d)
    for k in GRAD_OUTS + ("q", "c"):
        assert exact(r[k], v[k]), f"{k} differs"
    assert same_bits(r["q"], r["p"])
    if c.subset:
        outside = np.setdiff1d(np.arange(d["n_full0"]), d["rows"])
        assert not bits(r["dK1"][outside]).any(), "dK1 rows outside `rows` are not +0"


@pytest.mark.parametrize("c", E.CHAIN3_CASES, ids=str)
def test_chain3_gaussian_within_the_bounds(c):
    d = E.chain3_inputs(c, "gauss")
    v, e = chain3_refs(d)
    r = run_chain3(c, d)
    for k in GRAD_OUTS + ("q", "c"):
        within(r[k], v[k], e[k], f"{k} {tuple(c)}")


# =============================================================================================
# 3. rs_chain_aug_product, rs_chain_rt_product, rs_chain_outer
def run_aug(c, d):
    M, K = Buf(d["M"].shape, d["M"]), Buf(d["K"].shape, d["K"])
    cin = None if d["cin"] is None else Buf(c.k, d["cin"])
    b = None if d["b"] is None else Buf(c.n, d["b"])
    outs = dict(out=Buf((c.m + 1, c.n)))
    r = twice(outs, lambda: L.call("rs_chain_aug_product", M.ptr, c.k + c.pad, c.m, opt(cin), K.ptr, c.k,
                                   c.n, opt(b), outs["out"].ptr, stream()))
    inputs_intact((M, d["M"]), (K, d["K"]), (cin, d["cin"]), (b, d["b"]))
    return r["out"]


@pytest.mark.parametrize("c", E.AUG_CASES, ids=str)
def test_aug_product(c):
    d = E.aug_inputs(c, "int")
    ref, _, mag = E.aug_ref(d)
    assert mag.max() < E.TWO24
    assert exact(run_aug(c, d), ref), "integer product differs"
    d = E.aug_inputs(c, "gauss")
    ref, err, _ = E.aug_ref(d)
    within(run_aug(c, d), ref, err, f"aug {tuple(c)}")


@pytest.mark.parametrize("m,k,n,null_m", [(33, 4, 4, False), (0, 16897, 1, False), (0, 4, 4, True)])
def test_aug_product_refusals(m, k, n, null_m):
    """m = 33, (m + 1)·k = 16897, and m = 0 with neither M nor cin (the staging loop would read
    through M)."""
    assert null_m or not E.aug_accepts(m, k, n, k)
    M, K, out = Buf((m, k), np.ones((m, k), F32)), Buf((k, n), np.ones((k, n), F32)), Buf((m + 1, n))
    with pytest.raises(L.RecsysError, match="rs_chain_aug_product"):
        L.call("rs_chain_aug_product", None if null_m else M.ptr, k, m, None, K.ptr, k, n, None, out.ptr,
               stream())
    torch.cuda.synchronize()
    assert out.untouched()


def run_rt(m, k, n, P, K):
    Pb, Kb = Buf(P.shape, P), Buf(K.shape, K)
    outs = dict(out=Buf((m + 1, n)))
    r = twice(outs, lambda: L.call("rs_chain_rt_product", Pb.ptr, m, Kb.ptr, k, n, outs["out"].ptr, stream()))
    inputs_intact((Pb, P), (Kb, K))
    return r["out"]


@pytest.mark.parametrize("m,k,n", E.RT_CASES)
def test_rt_product(m, k, n):
    P, K = E.rt_inputs(m, k, n, "int")
    ref, _, mag = E.rt_ref(P, K)
    assert mag.max() < E.TWO24
    assert exact(run_rt(m, k, n, P, K), ref), "integer product differs"
    P, K = E.rt_inputs(m, k, n, "gauss")
    ref, err, _ = E.rt_ref(P, K)
    within(run_rt(m, k, n, P, K), ref, err, f"rt {(m, k, n)}")


def run_outer(c, R, rlast, P):
    Rb, Pb = Buf(R.shape, R), Buf(P.shape, P)
    rl = None if rlast is None else Buf(c.na, rlast)
    outs = dict(out=Buf((c.na, c.nb)))
    r = twice(outs, lambda: L.call("rs_chain_outer", Rb.ptr, c.na + c.pad, c.m, opt(rl), c.na, Pb.ptr, c.nb,
                                   outs["out"].ptr, stream()))
    inputs_intact((Rb, R), (Pb, P), (rl, rlast))
    return r["out"]


@pytest.mark.parametrize("c", E.OUTER_CASES, ids=str)
def test_outer(c):
    """Without rlast, row m of P holds NaN and is not read; m = 0 without rlast gives zeros."""
    R, rlast, P = E.outer_inputs(c, "int")
    ref, _, mag = E.outer_ref(R, rlast, P, c.na)
    assert mag.max(initial=0) < E.TWO24
    out = run_outer(c, R, rlast, P)
    assert exact(out, ref), "integer product differs"
    if c.m == 0 and not c.rlast:
        assert not bits(out).any()
    R, rlast, P = E.outer_inputs(c, "gauss")
    ref, err, _ = E.outer_ref(R, rlast, P, c.na)
    within(run_outer(c, R, rlast, P), ref, err, f"outer {tuple(c)}")


# =============================================================================================
# 4. rs_affine_narrow_fwd, rs_rowdot_act
def run_narrow(n0, n, B, pady, act, x, Qa, x_off=0):
    X, Q = Buf(x.shape, x, x_off), Buf(Qa.shape, Qa)
    outs = dict(y=Buf((B, n + pady)))
    r = twice(outs, lambda: L.call("rs_affine_narrow_fwd", X.ptr, x.shape[1], B, n0, Q.ptr, n, act,
                                   outs["y"].ptr, n + pady, stream()))
    inputs_intact((X, x), (Q, Qa))
    assert is_sent(outs["y"].view[:, n:]), "padding columns of y written"
    return r["y"][:, :n]


@pytest.mark.parametrize("c", E.FWD_CASES, ids=str)
def test_narrow_forward(c):
    """relu and linear on integers, exact; the three activations on Gaussians, within the bound.
    x starts one float past a 16-byte boundary on the cases with padded rows."""
    x_off = 1 if c.padx else 0
    x, Qa = E.narrow_inputs(c.n0, c.n, c.B, c.padx, "int")
    for act in (0, 1):
        ref, _, mag = E.narrow_ref(x, Qa, act)
        assert mag.max(initial=0) < E.TWO24
        assert exact(run_narrow(c.n0, c.n, c.B, c.pady, act, x, Qa, x_off), ref), f"act {act} differs"
    x, Qa = E.narrow_inputs(c.n0, c.n, c.B, c.padx, "gauss")
    for act in (0, 1, 2):
        ref, err, _ = E.narrow_ref(x, Qa, act)
        within(run_narrow(c.n0, c.n, c.B, c.pady, act, x, Qa, x_off), ref, err, f"narrow act {act} {tuple(c)}")


def test_narrow_forward_second_grid_stride_trip():
    """B = 4096·64 + 65: blocks 0 and 1 take a second trip (64 rows and one row) on rows the
    prefetch loaded during the first."""
    B, n0, n = E.FWD_BIG
    assert E.narrow_trips(B) == (4096, 2)
    x, Qa = E.narrow_inputs(n0, n, B, 0, "int")
    ref, _, mag = E.narrow_ref(x, Qa, 1)
    assert mag.max() < E.TWO24
    y = run_narrow(n0, n, B, 0, 1, x, Qa)
    assert exact(y, ref), f"rows {np.flatnonzero((y != ref.astype(F32)).any(1))[:8]} differ"
    x, Qa = E.narrow_inputs(n0, n, B, 0, "gauss")
    ref, err, _ = E.narrow_ref(x, Qa, 2)
    within(run_narrow(n0, n, B, 0, 2, x, Qa), ref, err, "sigmoid")


def run_rowdot(n0, B, act, x, q, c):
    X, Q, Cc = Buf(x.shape, x), Buf(n0, q), Buf(1, c)
    outs = dict(y=Buf(B))
    r = twice(outs, lambda: L.call("rs_rowdot_act", X.ptr, x.shape[1], B, n0, Q.ptr, Cc.ptr, act,
                                   outs["y"].ptr, stream()))
    inputs_intact((X, x), (Q, q), (Cc, c))
    return r["y"]


@pytest.mark.parametrize("n0,B,pad,_act", E.ROWDOT_CASES)
def test_rowdot_act(n0, B, pad, _act):
    x, q, c = E.rowdot_inputs(n0, B, pad, "int")
    for act in (0, 1):
        ref, _, mag = E.rowdot_ref(x, q, c, act)
        assert mag.max(initial=0) < E.TWO24
        assert exact(run_rowdot(n0, B, act, x, q, c), ref), f"act {act} differs"
    x, q, c = E.rowdot_inputs(n0, B, pad, "gauss")
    for act in (0, 1, 2):
        ref, err, _ = E.rowdot_ref(x, q, c, act)
        within(run_rowdot(n0, B, act, x, q, c), ref, err, f"rowdot act {act} {(n0, B, pad)}")


# =============================================================================================
# 5. rs_dlrm_dense_tail against the separate calls
PARAMS = [f"top_{k}{i}" for i in range(3) for k in "kb"] + [f"bot_{k}{i}" for i in range(3) for k in "kb"]


def _tail_bufs(c, d, comp2):
    """Fresh device copies of everything the tail reads or writes."""
    b = {}
    for side in ("top", "bot"):
        for i in range(3):
            b[f"{side}_k{i}"] = Buf(d[f"{side}_k"][i].shape, d[f"{side}_k"][i])
            b[f"{side}_b{i}"] = Buf(d[f"{side}_b"][i].shape, d[f"{side}_b"][i])
    b.update(A=Buf(c.n0, d["A"]), s=Buf(1, d["s"]), P=Buf(d["P"].shape, d["P"], c.p_off),
             comp2=Buf(comp2.shape, comp2))
    for i, k in enumerate(("K1", "K2", "K3")):
        b[f"top_dk{i}"] = Buf(d["top_k"][i].shape)
        b[f"top_db{i}"] = Buf(d["top_b"][i].shape)
    b.update(dk2=Buf((c.b1, c.b2)), dk3=Buf((c.b2, c.b3)), P2=Buf((c.m + 1, c.b2)), P1=Buf((c.m + 1, c.b1)),
             comp2n=Buf((c.m + 1, c.b2)), comp3n=Buf((c.m + 1, c.b3)), q=Buf(c.n0), c=Buf(1))
    return b


TAIL_OUTS = PARAMS + [f"top_dk{i}" for i in range(3)] + [f"top_db{i}" for i in range(3)] + \
    ["dk2", "dk3", "P2", "P1", "comp2n", "comp3n", "q", "c"]


def _tail_args(c, d, b, rows, inv):
    a = L.DlrmTailArgs()
    for i in range(3):
        a.top_k[i], a.top_b[i] = b[f"top_k{i}"].ptr.value, b[f"top_b{i}"].ptr.value
        a.top_dk[i], a.top_db[i] = b[f"top_dk{i}"].ptr.value, b[f"top_db{i}"].ptr.value
        a.bot_k[i], a.bot_b[i] = b[f"bot_k{i}"].ptr.value, b[f"bot_b{i}"].ptr.value
    a.top_rows = None if rows is None else rows.data_ptr()
    a.top_inv = None if inv is None else inv.data_ptr()
    a.top_n_full0, a.top_n0, a.top_n1, a.top_n2 = d["n_full0"], c.n0, c.n1, c.n2
    a.top_A, a.top_s, a.top_q, a.top_c = (b[k].ptr.value for k in ("A", "s", "q", "c"))
    a.bot_n0, a.bot_n1, a.bot_n2, a.bot_n3 = c.m, c.b1, c.b2, c.b3
    a.bot_P, a.bot_comp2 = b["P"].ptr.value, b["comp2"].ptr.value
    a.bot_dk2, a.bot_dk3, a.bot_P2, a.bot_P1 = (b[k].ptr.value for k in ("dk2", "dk3", "P2", "P1"))
    a.bot_comp2_next, a.bot_comp3_next = b["comp2n"].ptr.value, b["comp3n"].ptr.value
    a.lr = E.TAIL_LR
    return a


def _compose2(c, b, dst):
    """dst = [K1; b1]·K2 + [0; b2] of the bottom chain in b (rs_chain_aug_product)."""
    L.call("rs_chain_aug_product", b["bot_k0"].ptr, c.b1, c.m, b["bot_b0"].ptr, b["bot_k1"].ptr, c.b1, c.b2,
           b["bot_b1"].ptr, dst.ptr, stream())


def tail_fused(c, d, comp2, rows, inv):
    b = _tail_bufs(c, d, comp2)
    nb = L.lib().rs_dlrm_dense_tail_workspace_size(c.n0, c.n1, c.n2)
    ws = sent_buf(nb // 4 + GUARD)
    a = _tail_args(c, d, b, rows, inv)
    L.call("rs_dlrm_dense_tail", C.byref(a), L.ptr(ws), nb, stream())
    torch.cuda.synchronize()
    assert is_sent(ws[nb // 4:]), "workspace guard written"
    for k, buf in b.items():
        assert buf.guards_ok(), f"{k}: guard written"
    inputs_intact((b["A"], d["A"]), (b["s"], d["s"]), (b["P"], d["P"]), (b["comp2"], comp2))
    return {k: b[k].numpy() for k in TAIL_OUTS}


def tail_separate(c, d, comp2, rows, inv):
    """The same step in separate calls: rs_chain3_vec_grads, rs_chain_outer, rs_chain_rt_product
    (each twice for the bottom chain), tail_sgd's fmaf update restated on the host,
    rs_chain_aug_product twice and rs_chain3_vec_compose on the updated parameters. The
    standalone rs_chain_outer needs a 16-byte aligned P: it gets an aligned copy."""
    b = _tail_bufs(c, d, comp2)
    if c.p_off:
        b["P"] = Buf(d["P"].shape, d["P"])
    st = stream()
    nb = (2 * c.n1 + 2 * c.n2) * 4
    ws, p = sent_buf(nb // 4), Buf(c.n0)
    L.call("rs_chain3_vec_grads", b["top_k0"].ptr, L.ptr(rows), L.ptr(inv), d["n_full0"], c.n0,
           b["top_b0"].ptr, b["top_k1"].ptr, b["top_b1"].ptr, b["top_k2"].ptr, c.n1, c.n2, b["A"].ptr,
           b["s"].ptr, b["top_dk0"].ptr, b["top_db0"].ptr, b["top_dk1"].ptr, b["top_db1"].ptr,
           b["top_dk2"].ptr, b["top_db2"].ptr, p.ptr, L.ptr(ws), nb, st)
    L.call("rs_chain_outer", b["comp2"].ptr, c.b2, c.m, b["comp2"].at(c.m * c.b2), c.b2, b["P"].ptr, c.b3,
           b["dk3"].ptr, st)
    L.call("rs_chain_rt_product", b["P"].ptr, c.m, b["bot_k2"].ptr, c.b3, c.b2, b["P2"].ptr, st)
    L.call("rs_chain_outer", b["bot_k0"].ptr, c.b1, c.m, b["bot_b0"].ptr, c.b1, b["P2"].ptr, c.b2,
           b["dk2"].ptr, st)
    L.call("rs_chain_rt_product", b["P2"].ptr, c.m, b["bot_k1"].ptr, c.b2, c.b1, b["P1"].ptr, st)
    torch.cuda.synchronize()
    P1, P2 = b["P1"].numpy(), b["P2"].numpy()
    grads = [b[f"top_d{k}{i}"].numpy() for i in range(3) for k in "kb"] + \
        [P1[:c.m], P1[c.m], b["dk2"].numpy(), P2[c.m], b["dk3"].numpy(), d["P"][c.m]]
    for name, g in zip(PARAMS, grads):
        new = E.sgd_fma(b[name].numpy(), g, E.TAIL_LR)
        b[name].view.copy_(dev(new))
    _compose2(c, b, b["comp2n"])
    L.call("rs_chain_aug_product", b["comp2n"].ptr, c.b2, c.m, b["comp2n"].at(c.m * c.b2), b["bot_k2"].ptr,
           c.b2, c.b3, b["bot_b2"].ptr, b["comp3n"].ptr, st)
    nb2 = (c.n1 + 1) * 4
    L.call("rs_chain3_vec_compose", b["top_k0"].ptr, L.ptr(rows), c.n0, b["top_b0"].ptr, b["top_k1"].ptr,
           b["top_b1"].ptr, b["top_k2"].ptr, b["top_b2"].ptr, c.n1, c.n2, b["q"].ptr, b["c"].ptr,
           L.ptr(sent_buf(nb2 // 4)), nb2, st)
    torch.cuda.synchronize()
    return {k: b[k].numpy() for k in TAIL_OUTS}


def _tail_setup(c):
    d = E.tail_inputs(c)
    b = _tail_bufs(c, d, np.zeros((c.m + 1, c.b2), F32))
    _compose2(c, b, b["comp2"])
    torch.cuda.synchronize()
    return d, b["comp2"].numpy(), _i32(d["rows"]), _i32(d["inv"])


@pytest.mark.parametrize("c", E.TAIL_CASES, ids=str)
def test_dense_tail_equals_the_separate_calls(c):
    """All twelve updated parameters, every gradient and the four next-step compositions, bit
    for bit; two fused runs from fresh copies are bit-identical; the update moved every
    parameter."""
    assert E.tail_accepts(c)
    d, comp2, rows, inv = _tail_setup(c)
    fused = tail_fused(c, d, comp2, rows, inv)
    again = tail_fused(c, d, comp2, rows, inv)
    sep = tail_separate(c, d, comp2, rows, inv)
    for k in TAIL_OUTS:
        assert np.isfinite(fused[k]).all(), f"{k}: not written"
        assert same_bits(fused[k], again[k]), f"{k}: a second run differs"
        assert same_bits(fused[k], sep[k]), \
            f"{k}: {int((bits(fused[k]) != bits(sep[k])).sum())} / {fused[k].size} elements differ"
    moved = [k for k, src in zip(PARAMS, [d[f"{s}_{kb}"][i] for s in ("top", "bot") for i in range(3)
                                          for kb in "kb"]) if not same_bits(fused[k], src)]
    assert moved == PARAMS, "a parameter was not updated"
    if c.subset:  # K1 rows outside `rows` have a zero gradient and stay as they were
        outside = np.setdiff1d(np.arange(d["n_full0"]), d["rows"])
        assert not bits(fused["top_dk0"][outside]).any()
        assert same_bits(fused["top_k0"][outside], d["top_k"][0][outside])


@pytest.mark.parametrize("change", [dict(m=16), dict(b2=6)], ids=str)
def test_dense_tail_refusals(change):
    c = E.TAIL_CASES[0]
    bad = c._replace(**change)
    assert not E.tail_accepts(bad)
    d, comp2, rows, inv = _tail_setup(c)
    b = _tail_bufs(c, d, comp2)
    nb = L.lib().rs_dlrm_dense_tail_workspace_size(c.n0, c.n1, c.n2)
    ws = sent_buf(nb // 4 + GUARD)
    a = _tail_args(bad, d, b, rows, inv)
    with pytest.raises(L.RecsysError, match="rs_dlrm_dense_tail"):
        L.call("rs_dlrm_dense_tail", C.byref(a), L.ptr(ws), nb, stream())
    torch.cuda.synchronize()
    assert is_sent(ws)
    for k in TAIL_OUTS:
        if k in PARAMS:
            i, kb = int(k[-1]), k[-2]
            assert same_bits(b[k].numpy(), d[f"{k[:3]}_{kb}"][i]), f"{k} modified"
        else:
            assert b[k].untouched(), f"{k} written"
