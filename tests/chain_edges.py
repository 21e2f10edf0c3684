"""Case tables, inputs, float64 / integer restatements, restated dispatch predicates and error
bounds for the factored MLP-chain kernels of csrc/dense.hip: rs_chain_reduce,
rs_chain3_vec_grads, rs_chain3_vec_compose, rs_chain_aug_product, rs_chain_rt_product,
rs_chain_outer, rs_affine_narrow_fwd, rs_rowdot_act and the grouped rs_dlrm_dense_tail.
tests/test_chain_edges_cpu.py proves each case has the property its name claims and that the
bounds hold for the kernels' summation order replayed in fp32; tests/test_chain_edges_gpu.py
runs the cases through the kernels. NumPy only; nothing here calls a kernel.

Two kinds of input per kernel. kind "int": every operand is a small integer held in fp32 and
Σ|terms| of every output stays below 2^24, so every partial sum in any order is an integer below
2^24, no addition rounds, and the kernel's result equals the int64 evaluation bit for bit.
kind "gauss": standard normal operands, compared with float64 within a first-order summation
bound, depth·2^-24·Σ|terms|, depth read from the code (see the *_depth functions).
"""
from __future__ import annotations

import collections
import math

import numpy as np

from tests.head_edges import SIGMOID_RTOL, U32, act_bwd_f64

TWO24 = 2 ** 24
F32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def pow2_ge(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def _gauss(rng, shape):
    return rng.standard_normal(shape).astype(F32)


def draw(rng, kind, shape, lim=2):
    """Integers of [-lim, lim] (kind "int") or standard normals, fp32."""
    return _ints(rng, -lim, lim, shape) if kind == "int" else _gauss(rng, shape)


# =============================================================================================
# 1. rs_chain_reduce: A = xᵀ·G, s = Σ_b G, G = act'(y) ⊙ dy
CHUNK = 128  # kVecRows = kChainRows = kQuadRows: rows per block
KSEG = 32    # kSeg of fold_two_level

RC = collections.namedtuple("RC", "n0 nl pad B dy_off y_off g_off", defaults=(0, 0, 0))
REDUCE_SMALL_B = (1, 127, 128, 129)
REDUCE_LARGE_B = (0, 4096, 4097, 8320)
VEC_N0 = (4, 12, 512, 516, 1024)
VEC_PADS = (0, 4, 36)
QUAD_NL = (4, 12, 64, 200, 256)
OUTER_NL = (2, 3, 5, 129, 255)
NARROW_N0 = (1, 16, 17, 32)


def _reduce_cases():
    """Every kernel's widths under two of the small row counts each, in rotation; the large row
    counts (and B = 0) at the narrowest n0·nl of each kernel; nl in {8, 64} with dy, y or g_out
    alone one float past a 16-byte boundary."""
    c = []
    for i, n0 in enumerate(VEC_N0):
        for j in range(2):
            c.append(RC(n0, 1, VEC_PADS[(i + j) % 3], REDUCE_SMALL_B[(2 * i + j) % 4]))
    c += [RC(4, 1, 4 if B == 4097 else 0, B) for B in REDUCE_LARGE_B]
    for k, (nls, narrow) in enumerate(((QUAD_NL, 4), (OUTER_NL, 2))):
        for i, nl in enumerate(nls):
            for j in range(2):
                c.append(RC(NARROW_N0[(2 * i + j + k) % 4], nl, (0, 3, 1)[(i + j) % 3],
                            REDUCE_SMALL_B[(2 * i + j + 1) % 4]))
        c += [RC(1, narrow, 3 if B == 8320 else 0, B) for B in REDUCE_LARGE_B]
    for i, nl in enumerate((8, 64)):
        c += [RC(NARROW_N0[2 * i], nl, 0, 129, dy_off=1), RC(NARROW_N0[2 * i + 1], nl, 1, 128, y_off=1),
              RC(NARROW_N0[(2 * i + 3) % 4], nl, 0, 127, g_off=1)]
    return tuple(c)


REDUCE_CASES = _reduce_cases()


def reduce_accepts(n0, nl, ldx, act, B, has_y=True, x_off=0):
    """The RS_CHECK_ARGs of rs_chain_reduce restated (the workspace size apart). x_off: x's
    start in floats past a 16-byte boundary. The nl == 1 alignment rules are checked after the
    B == 0 return."""
    if not (B >= 0 and n0 >= 1 and nl >= 1 and ldx >= n0 and 0 <= act <= 2):
        return False
    if act and not has_y:
        return False
    if not ((nl == 1 and n0 <= 1024) or (nl <= 256 and n0 <= 32)):
        return False
    if B > 0 and nl == 1 and not (n0 % 4 == 0 and ldx % 4 == 0 and x_off % 4 == 0):
        return False
    return True


def reduce_regime(n0, nl, dy_off=0, y_off=0, g_off=0, has_y=True, has_g=True):
    """The dispatch of rs_chain_reduce restated → dict(kernel, n0max, cgp, P, idle):
    nl == 1: the vec kernel, cgp = the power of two >= n0/4 column groups, P = 256/cgp row
      phases, idle = the threads of the dead column groups (4·cg >= n0);
    nl % 4 == 0 and dy, y (if given), g_out (if given) on 16 bytes: the quad kernel, nl/4 column
      quads, P = 256 // (nl/4) phases, idle = 256 - P·nl/4 threads with ph >= P;
    else the outer kernel: nlp = the power of two >= nl columns, P = 256/nlp phases, idle = the
      threads with j >= nl.
    quad and outer are instantiated for N0MAX = 16 (n0 <= 16) and 32."""
    if nl == 1:
        cgp = pow2_ge(n0 // 4)
        return dict(kernel="vec", n0max=None, cgp=cgp, P=256 // cgp, idle=(cgp - n0 // 4) * (256 // cgp))
    n0max = 16 if n0 <= 16 else 32
    if nl % 4 == 0 and dy_off % 4 == 0 and (not has_y or y_off % 4 == 0) and (not has_g or g_off % 4 == 0):
        nq = nl // 4
        return dict(kernel="quad", n0max=n0max, cgp=None, P=256 // nq, idle=256 - (256 // nq) * nq)
    nlp = pow2_ge(nl)
    return dict(kernel="outer", n0max=n0max, cgp=None, P=256 // nlp, idle=(nlp - nl) * (256 // nlp))


def case_regime(c, has_g=True):
    return reduce_regime(c.n0, c.nl, c.dy_off, c.y_off, c.g_off, True, has_g)


def fold_plan(B):
    """fold_two_level restated → dict(nchunks, per, nseg, last): nchunks 128-row chunks, segments
    of per = ceil(nchunks / 32) chunks, nseg = ceil(nchunks / per) of them, the last one holding
    `last` chunks."""
    nchunks = cdiv(B, CHUNK)
    if nchunks == 0:
        return dict(nchunks=0, per=0, nseg=0, last=0)
    per = cdiv(nchunks, KSEG)
    nseg = cdiv(nchunks, per)
    return dict(nchunks=nchunks, per=per, nseg=nseg, last=nchunks - (nseg - 1) * per)


def reduce_workspace_bytes(B, n0, nl):
    """rs_chain_reduce_workspace_size restated: chunk partials + 32 segment partials + 256."""
    return (cdiv(max(B, 1), CHUNK) + KSEG) * (n0 * nl + nl) * 4 + 256


def nn_routes_fused(n0, nl, ldx, x_off=0, unit_stride=True):
    """nn.chain_reduce's predicate restated: the fused call, else rs_act_bwd_colsum + torch."""
    vec_ok = nl == 1 and n0 <= 1024 and n0 % 4 == 0 and ldx % 4 == 0 and x_off % 4 == 0
    return unit_stride and (vec_ok or (1 < nl <= 256 and n0 <= 32))


def reduce_inputs(c, act, kind):
    """x [B, n0 + pad] (the padding columns hold NaN: nobody may read them), dy [B, nl], y.
    int: g in {1, 2, 3}, column 0 of x in {1, 2, 3} (no set of dropped or doubled rows cancels
    in A[0, :] or in s), the other columns in [-3, 3]; relu's y in {0, 1, 2} with every flat
    element 5k + 1 = +0.0 and 7k + 3 = -0.0. gauss: normals, y a sigmoid / relu of normals.
    act 0: y is all NaN (unread)."""
    rng = np.random.default_rng([c.n0, c.nl, c.B, c.pad, act, kind == "int"])
    B, n0, nl = c.B, c.n0, c.nl
    x = np.full((B, n0 + c.pad), np.nan, F32)
    if kind == "int":
        x[:, :n0] = _ints(rng, -3, 3, (B, n0))
        x[:, 0] = _ints(rng, 1, 3, B)
        dy = _ints(rng, 1, 3, (B, nl))
    else:
        x[:, :n0] = _gauss(rng, (B, n0))
        dy = _gauss(rng, (B, nl))
    z = rng.standard_normal((B, nl))
    if act == 0:
        y = np.full((B, nl), np.nan, F32)
    elif act == 1:
        y = (_ints(rng, 0, 2, (B, nl)) if kind == "int" else np.maximum(z, 0.0).astype(F32))
        f = y.reshape(-1)
        f[1::5] = 0.0
        f[3::7] = -0.0
    else:
        y = (1.0 / (1.0 + np.exp(-z))).astype(F32)
    return x, dy, y


def reduce_ref(x, dy, y, act, n0):
    """float64 (exact for kind "int": every value an integer below 2^53) → (out [n0·nl + nl] =
    [A row-major; s], G [B, nl], mag = Σ_b |x·G| per output, the bound on any partial sum)."""
    G = act_bwd_f64(dy, y, act)
    x64 = x[:, :n0].astype(np.float64)
    out = np.concatenate([(x64.T @ G).reshape(-1), G.sum(0)])
    mag = np.concatenate([(np.abs(x64).T @ np.abs(G)).reshape(-1), np.abs(G).sum(0)])
    return out, G, mag


def reduce_depth(regime, B):
    """The longest chain of fp32 additions one element of `out` goes through, from the code: a
    thread adds the rows ph, ph + P, ... of its chunk: ceil(min(B, 128) / P); the P phase sums
    are added in phase order: at most P (the outer kernel starts from 0); wave w of
    fold_segments_kernel adds the chunks c0 + w, c0 + w + 4, ... of its segment: ceil(per / 4),
    and the four wave sums in order: 3; fold_chunks_kernel the same over the nseg segment
    partials: ceil(nseg / 4) + 3."""
    f = fold_plan(B)
    P = regime["P"]
    return cdiv(min(B, CHUNK), P) + P + cdiv(f["per"], 4) + 3 + cdiv(f["nseg"], 4) + 3


def reduce_bound(mag, regime, B, act):
    """|out - float64|: every term x·g is a rounded product (one more 2^-24), then `depth`
    additions whose partial sums never exceed Σ|terms|; sigmoid's g carries SIGMOID_RTOL."""
    return ((reduce_depth(regime, B) + 1) * U32 + (SIGMOID_RTOL if act == 2 else 0.0)) * mag


def fold4(rows):
    """Four waves take the rows w, w + 4, ... in order; the wave sums are added in wave order
    (fold_chunks_kernel, fold_segments_kernel), fp32."""
    w = np.zeros((4,) + rows.shape[1:], F32)
    for c in range(rows.shape[0]):
        w[c % 4] = w[c % 4] + rows[c]
    return ((w[0] + w[1]) + w[2]) + w[3]


def emulate_reduce(x, G32, n0, regime, B):
    """The kernels' summation order in NumPy fp32: rows to phases r % P within a 128-row chunk,
    each phase's rows in order, phases in order, then fold_two_level. x [B, >= n0], G32 [B, nl]
    → out [n0·nl + nl]."""
    f = fold_plan(B)
    P = regime["P"]
    nl = G32.shape[1]
    M = n0 * nl + nl
    part = np.zeros((f["nchunks"], M), F32)
    for ch in range(f["nchunks"]):
        xs, gs = x[ch * CHUNK:(ch + 1) * CHUNK, :n0], G32[ch * CHUNK:(ch + 1) * CHUNK]
        terms = np.concatenate([(xs[:, :, None] * gs[:, None, :]).reshape(len(xs), -1), gs], 1)
        acc = np.zeros((P, M), F32)
        for r in range(len(xs)):
            acc[r % P] = acc[r % P] + terms[r]
        v = acc[0].copy()
        for q in range(1, P):
            v = v + acc[q]
        part[ch] = v
    part2 = np.stack([fold4(part[s * f["per"]:(s + 1) * f["per"]]) for s in range(f["nseg"])])
    return fold4(part2)


# =============================================================================================
# 2. first-order error propagation for the weight-sized products
def _dot(M, v, ev, depth):
    """Σ_k M[..., k]·v[k] with v known within ev → (value, Σ|terms|, error bound): each product
    rounds once and each of the `depth` additions once, against partial sums within Σ|terms|;
    the operand's own error passes through |M|."""
    aM, av = np.abs(M), np.abs(v) + ev
    return M @ v, aM @ np.abs(v), (depth + 1) * U32 * (aM @ av) + aM @ ev


def _mul(a, ea, b, eb):
    """a·b, one rounding → (value, error bound)."""
    aa, ab = np.abs(a) + ea, np.abs(b) + eb
    return a * b, U32 * aa * ab + aa * eb + ab * ea


def rowdot_depth(n):
    """rowdot_wave: a lane adds its ceil(n / 64) products, then the 6-level butterfly."""
    return cdiv(n, 64) + 6


def coldot_depth(n, add=False):
    """coldot_tile: a wave adds its ceil(n / 16) products, the 16 wave sums are added in order
    (15), plus the `add` vector."""
    return cdiv(n, 16) + 15 + (1 if add else 0)


# =============================================================================================
# 3. rs_chain3_vec_grads / rs_chain3_vec_compose
C3_N0 = (1, 15, 16, 17, 100)
C3_N1 = (1, 15, 16, 17, 64, 65)
C3_N2 = (1, 63, 64, 65, 130)
C3_EXTRA = 37  # n_full0 - n0 of the subset cases
C3 = collections.namedtuple("C3", "n0 n1 n2 subset b1 b2 b3")


def _chain3_cases():
    """12 shapes: n1 cycles twice, n0 and n2 at co-prime strides; the rows mode alternates and
    the four (b1, b2) presences cycle under both modes; b3 (compose only) absent on every
    third."""
    c = []
    for i in range(12):
        bm = (i // 2 + i) % 4
        c.append(C3(C3_N0[i % 5], C3_N1[i % 6], C3_N2[(2 * i + 1) % 5], bool(i % 2),
                    bm & 1 == 0, bm & 2 == 0, i % 3 != 2))
    return tuple(c)


CHAIN3_CASES = _chain3_cases()


def chain3_inputs(c, kind):
    """kind "int": kernels and biases in [-2, 2], A in [-3, 3], s in {1, 2, 3}."""
    rng = np.random.default_rng([c.n0, c.n1, c.n2, c.subset, kind == "int", 5])
    nf = c.n0 + C3_EXTRA if c.subset else c.n0
    d = dict(n_full0=nf, K1=draw(rng, kind, (nf, c.n1)), K2=draw(rng, kind, (c.n1, c.n2)),
             K3=draw(rng, kind, c.n2), A=draw(rng, kind, c.n0, 3),
             s=(_ints(rng, 1, 3, 1) if kind == "int" else _gauss(rng, 1)),
             b1=draw(rng, kind, c.n1) if c.b1 else None, b2=draw(rng, kind, c.n2) if c.b2 else None,
             b3=draw(rng, kind, 1) if c.b3 else None, rows=None, inv=None)
    if c.subset:
        d["rows"] = rng.permutation(nf)[:c.n0].astype(np.int32)
        d["inv"] = np.full(nf, -1, np.int32)
        d["inv"][d["rows"]] = np.arange(c.n0, dtype=np.int32)
    return d


def _f64(a):
    return None if a is None else a.astype(np.float64)


def chain3_grads_ref(d):
    """The formulas above chain3_stage1 in float64 → (values, err, mag): per output of
    rs_chain3_vec_grads its value, its error bound and Σ|terms| (for kind "int" the largest
    partial sum any order can reach; mag also holds the scratch vectors q1, T2, c2, T3)."""
    K1, K2, K3, A, b1, b2 = (_f64(d[k]) for k in ("K1", "K2", "K3", "A", "b1", "b2"))
    s = float(d["s"][0])
    n0, (n1, n2) = A.size, K2.shape
    K1r = K1 if d["rows"] is None else K1[d["rows"]]
    z1, z2 = np.zeros(n1), np.zeros(n2)
    q1, m_q1, e_q1 = _dot(K2, K3, z2, rowdot_depth(n2))
    T2, m_T2, e_T2 = _dot(K1r.T, A, np.zeros(n0), coldot_depth(n0))
    if b1 is not None:
        c2, m_c2, e_c2 = _dot(K2.T, b1, z1, coldot_depth(n1, b2 is not None))
        if b2 is not None:
            c2, m_c2, e_c2 = c2 + b2, m_c2 + np.abs(b2), e_c2 + U32 * np.abs(b2)
    else:
        c2, m_c2, e_c2 = (b2.copy() if b2 is not None else z2), (np.abs(b2) if b2 is not None else z2), z2
    T3, m_T3, e_T3 = _dot(K2.T, T2, e_T2, coldot_depth(n1))
    m_T3 = np.abs(K2.T) @ m_T2
    p, m_p, e_p = _dot(K1r, q1, e_q1, rowdot_depth(n1))
    m_p = np.abs(K1r) @ m_q1
    v, e, m = {}, {}, dict(q1=m_q1, T2=m_T2, c2=m_c2, T3=m_T3, p=m_p)
    v["p"], e["p"] = p, e_p
    dk1, e_dk1 = _mul(A[:, None], 0.0, q1[None, :], e_q1[None, :])
    rows = np.arange(n0) if d["rows"] is None else d["rows"]
    v["dK1"], e["dK1"] = np.zeros_like(K1), np.zeros_like(K1)
    v["dK1"][rows], e["dK1"][rows] = dk1, e_dk1
    m["dK1"] = np.abs(A)[:, None] * m_q1[None, :]
    m2, e_m2, m_m2 = T2, e_T2, m_T2
    if b1 is not None:
        t, et = _mul(b1, 0.0, s, 0.0)
        m2, m_m2 = T2 + t, m_T2 + np.abs(t)
        e_m2 = e_T2 + et + U32 * (m_T2 + e_T2 + np.abs(t) + et)
    v["dK2"], e["dK2"] = _mul(m2[:, None], e_m2[:, None], K3[None, :], 0.0)
    m["dK2"] = m_m2[:, None] * np.abs(K3)[None, :]
    t, et = _mul(c2, e_c2, s, 0.0)
    v["dK3"] = T3 + t
    m["dK3"] = m_T3 + m_c2 * abs(s)
    e["dK3"] = e_T3 + et + U32 * (m_T3 + e_T3 + np.abs(t) + et)
    v["db1"], e["db1"] = _mul(q1, e_q1, s, 0.0)
    m["db1"] = m_q1 * abs(s)
    v["db2"], e["db2"] = _mul(K3, 0.0, s, 0.0)
    m["db2"] = np.abs(v["db2"])
    v["db3"], e["db3"], m["db3"] = np.array([s]), np.zeros(1), np.array([abs(s)])
    return v, e, m


def chain3_compose_ref(d):
    """q = K1[rows]·(K2·K3), c = b3 + K3ᵀ·b2 + (K2·K3)ᵀ·b1 → (values, err, mag). cb = K3ᵀ·b2
    (+ b3) and q1ᵀ·b1 are lane-strided sums under the butterfly (rowdot_depth), each joined by
    one more addition."""
    K1, K2, K3, b1, b2, b3 = (_f64(d[k]) for k in ("K1", "K2", "K3", "b1", "b2", "b3"))
    n1, n2 = K2.shape
    K1r = K1[:d["A"].size] if d["rows"] is None else K1[d["rows"]]
    q1, m_q1, e_q1 = _dot(K2, K3, np.zeros(n2), rowdot_depth(n2))
    q, _, e_q = _dot(K1r, q1, e_q1, rowdot_depth(n1))
    m_q = np.abs(K1r) @ m_q1
    cb, m_cb, e_cb = 0.0, 0.0, 0.0
    if b2 is not None:
        cb, m_cb, e_cb = _dot(b2, K3, np.zeros(n2), rowdot_depth(n2) + 1)
    if b3 is not None:
        cb, m_cb, e_cb = cb + b3[0], m_cb + abs(b3[0]), e_cb + U32 * (m_cb + abs(b3[0]))
    c, m_c, e_c = cb, m_cb, e_cb
    if b1 is not None:
        t, m_t, e_t = _dot(b1, q1, e_q1, rowdot_depth(n1) + 1)
        m_t = np.abs(b1) @ m_q1
        c, m_c = t + cb, m_t + m_cb
        e_c = e_t + e_cb + U32 * (m_t + m_cb + e_t + e_cb)
    v = dict(q=q, c=np.array([c], np.float64))
    return v, dict(q=e_q, c=np.array([e_c])), dict(q1=m_q1, q=m_q, c=np.array([m_c]))


def emu_rowdot(M, v):
    """rowdot_wave in fp32: out[i] = Σ_k M[i, k]·v[k], lanes stride k, then the butterfly."""
    acc = np.zeros((64, M.shape[0]), F32)
    for k in range(M.shape[1]):
        acc[k % 64] = acc[k % 64] + M[:, k] * v[k]
    return butterfly(acc)


def emu_coldot(M, v, add=None):
    """coldot_tile in fp32: out[c] = Σ_k M[k, c]·v[k], 16 waves stride k, folded in order."""
    acc = np.zeros((16, M.shape[1]), F32)
    for k in range(M.shape[0]):
        acc[k % 16] = acc[k % 16] + M[k] * v[k]
    t = acc[0]
    for j in range(1, 16):
        t = t + acc[j]
    return t if add is None else t + add


def emulate_chain3(d):
    """The three stages of rs_chain3_vec_grads and the two of rs_chain3_vec_compose in fp32, in
    the kernels' summation order → the dict of all their outputs."""
    K1, K2, K3, A, b1, b2, b3, s = (d[k] for k in ("K1", "K2", "K3", "A", "b1", "b2", "b3", "s"))
    n0 = A.size
    K1r = K1[:n0] if d["rows"] is None else K1[d["rows"]]
    q1 = emu_rowdot(K2, K3)
    T2 = emu_coldot(K1r, A)
    c2 = emu_coldot(K2, b1, b2) if b1 is not None else (b2 if b2 is not None else np.zeros_like(K3))
    T3 = emu_coldot(K2, T2)
    o = dict(p=emu_rowdot(K1r, q1), dK1=np.zeros_like(K1))
    o["dK1"][np.arange(n0) if d["rows"] is None else d["rows"]] = A[:, None] * q1[None, :]
    m2 = T2 + b1 * s[0] if b1 is not None else T2
    o.update(dK2=m2[:, None] * K3[None, :], dK3=T3 + c2 * s[0], db1=q1 * s[0], db2=K3 * s[0], db3=s.copy())
    cb = emu_rowdot(b2[None], K3)[0] if b2 is not None else F32(0)
    cb = cb + b3[0] if b3 is not None else cb
    o["q"] = o["p"]
    t = emu_rowdot(b1[None], q1)[0] if b1 is not None else F32(0)
    o["c"] = np.array([t + cb], F32)
    return o


def butterfly(v):
    """wave_sum's fixed xor butterfly over 64 lanes, fp32: [64, ...] → [...]."""
    v = v.astype(F32)
    for sh in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ sh]
    return v[0]


# =============================================================================================
# 4. rs_chain_aug_product, rs_chain_rt_product, rs_chain_outer
AUG_ROWS, AUG_LDS = 33, 16896  # kAugRows, kAugLds
AUG_M = (0, 1, 15, 16, 32)
AUG_K = (1, 16, 17, 127, 128, 129)
AUG_N = (1, 63, 64, 65, 200)
AUG = collections.namedtuple("AUG", "m k n pad cin b")


def _aug_cases():
    """k cycles twice over m and n at co-prime strides; (cin, b) presences cycle; ldm = k + 3
    on every other case; then m = 32 with k = 512: (m + 1)·k == 16896 floats, the LDS limit."""
    c = [AUG(AUG_M[i % 5], AUG_K[i % 6], AUG_N[(2 * i + 1) % 5], 3 * (i % 2),
             (i // 2 + i) % 4 & 1 == 0, (i // 2 + i) % 4 & 2 == 0) for i in range(12)]
    return tuple(c + [AUG(32, 512, 65, 0, True, True), AUG(0, 128, 64, 0, False, True)])


AUG_CASES = _aug_cases()


def aug_accepts(m, k, n, ldm):
    return 0 <= m < AUG_ROWS and k >= 1 and n >= 1 and ldm >= k and (m + 1) * k <= AUG_LDS


def aug_staging_trips(m, k):
    """Trips of aug_product_body's staging loop: 8 passes of 1024 threads each."""
    return cdiv((m + 1) * k, 8 * 1024)


def aug_unrolled_trips(k):
    """(main, tail) trips of wave 0 and of wave 15 in aug_product_body's k loop: the main loop
    takes 8 k's 16 apart while kk + 112 < k."""
    out = []
    for w in (0, 15):
        kk, main = w, 0
        while kk + 112 < k:
            kk, main = kk + 128, main + 1
        out.append((main, len(range(kk, k, 16))))
    return out


def aug_inputs(c, kind):
    """M [m, k + pad] (padding NaN), cin [k], K [k, n], b [n]."""
    rng = np.random.default_rng([c.m, c.k, c.n, c.pad, kind == "int", 6])
    M = np.full((c.m, c.k + c.pad), np.nan, F32)
    M[:, :c.k] = draw(rng, kind, (c.m, c.k))
    return dict(M=M, cin=draw(rng, kind, c.k) if c.cin else None, K=draw(rng, kind, (c.k, c.n)),
                b=draw(rng, kind, c.n) if c.b else None)


def aug_depth(k, bias):
    """A wave adds its ceil(k / 16) products; wave w + 8 is added to wave w (1), the 8 sums in
    order (7), then the bias."""
    return cdiv(k, 16) + 8 + (1 if bias else 0)


def aug_ref(d):
    """out [m + 1, n] = [M; cin]·K, + b on row m → (value, err, mag)."""
    M, K = _f64(d["M"]), _f64(d["K"])
    k = K.shape[0]
    Mt = np.vstack([M[:, :k], (_f64(d["cin"]) if d["cin"] is not None else np.zeros(k))[None]])
    out, mag = Mt @ K, np.abs(Mt) @ np.abs(K)
    if d["b"] is not None:
        out[-1] += d["b"]
        mag[-1] += np.abs(d["b"])
    return out, (aug_depth(k, d["b"] is not None) + 1) * U32 * mag, mag


def emulate_aug(d):
    """aug_product_body's order in fp32."""
    K = d["K"]
    k, n = K.shape
    Mt = np.vstack([d["M"][:, :k], (d["cin"] if d["cin"] is not None else np.zeros(k, F32))[None]])
    acc = np.zeros((16,) + (Mt.shape[0], n), F32)
    for kk in range(k):
        acc[kk % 16] = acc[kk % 16] + Mt[:, kk, None] * K[None, kk, :]
    w = acc[:8] + acc[8:]
    t = w[0]
    for j in range(1, 8):
        t = t + w[j]
    if d["b"] is not None:
        t[-1] = t[-1] + d["b"]
    return t


RT_M = (0, 1, 15, 16, 32)
RT_K = (1, 63, 64, 65, 300)
RT_N = (1, 15, 16, 17, 100)
RT_CASES = tuple((RT_M[i % 5], RT_K[(2 * i + i // 5) % 5], RT_N[(3 * i + 1) % 5]) for i in range(10))


def rt_inputs(m, k, n, kind):
    rng = np.random.default_rng([m, k, n, kind == "int", 7])
    return draw(rng, kind, (m + 1, k)), draw(rng, kind, (n, k))


def rt_ref(P, K):
    """out [m + 1, n] = P·Kᵀ → (value, err, mag): rowdot_depth(k) per output."""
    P64, K64 = _f64(P), _f64(K)
    mag = np.abs(P64) @ np.abs(K64).T
    return P64 @ K64.T, (rowdot_depth(K.shape[1]) + 1) * U32 * mag, mag


def emulate_rt(P, K):
    k = K.shape[1]
    acc = np.zeros((64, P.shape[0], K.shape[0]), F32)
    for kk in range(k):
        acc[kk % 64] = acc[kk % 64] + P[:, kk, None] * K[None, :, kk]
    return butterfly(acc)


OUT_M = (0, 1, 7, 8, 9, 32)
OUT_NA = (1, 63, 65)
OUT_NB = (4, 12, 128)
OUTER = collections.namedtuple("OUTER", "m rlast na nb pad")


def _outer_cases():
    """Every m with and without rlast (row counts 0, 1, 2, 7, 8, 9, 10, 32, 33); na, nb and the
    row stride of R rotate."""
    c = []
    for i, m in enumerate(OUT_M):
        for j, rl in enumerate((False, True)):
            c.append(OUTER(m, rl, OUT_NA[(i + j) % 3], OUT_NB[(i + 2 * j) % 3], (0, 5)[(i + j) % 2]))
    return tuple(c)


OUTER_CASES = _outer_cases()


def outer_inputs(c, kind):
    """R [m, na + pad] (padding NaN), rlast [na], P [m + 1, nb]; without rlast, row m of P is
    NaN: nobody may read it."""
    rng = np.random.default_rng([c.m, c.rlast, c.na, c.nb, kind == "int", 8])
    R = np.full((c.m, c.na + c.pad), np.nan, F32)
    R[:, :c.na] = draw(rng, kind, (c.m, c.na))
    P = draw(rng, kind, (c.m + 1, c.nb))
    if not c.rlast:
        P[c.m] = np.nan
    return R, (draw(rng, kind, c.na) if c.rlast else None), P


def outer_ref(R, rlast, P, na):
    """out [na, nb] = [R; rlast]ᵀ·P, rows added in order: depth = the row count."""
    Rt = _f64(R[:, :na])
    if rlast is not None:
        Rt = np.vstack([Rt, _f64(rlast)[None]])
    P64 = _f64(P[:Rt.shape[0]])
    mag = np.abs(Rt).T @ np.abs(P64)
    return Rt.T @ P64, (Rt.shape[0] + 1) * U32 * mag, mag


# =============================================================================================
# 5. the batch-deep forwards: rs_affine_narrow_fwd, rs_rowdot_act
# sigmoid = 1 / (1 + expf(-v)): expf within 1 ulp = 2·2^-24 (the HIP math library's stated
# accuracy), the addition within 2^-24, the IEEE division within 2^-24; the error of e = expf(-v)
# reaches y scaled by e / (1 + e) < 1. 4·2^-24 covers the sum; doubled for their compounding
SIGMOID_FWD_RTOL = 8 * U32
NARROW_ROWS = 64       # kNarrowRows
FWD_MAX_BLOCKS = 4096  # fwd_blocks' cap
FWD_N0 = (1, 15, 16, 32)
FWD_N = (4, 12, 200, 256)
FWD_B = (0, 1, 63, 64, 65)
FWD_BIG = (FWD_MAX_BLOCKS * NARROW_ROWS + 65, 1, 4)  # (B, n0, n): the second grid-stride trip
FWD = collections.namedtuple("FWD", "n0 n B padx pady act")


def _fwd_cases():
    c = []
    for i in range(10):
        c.append(FWD(FWD_N0[i % 4], FWD_N[(i + i // 4) % 4], FWD_B[i % 5], (0, 3)[i % 2],
                     (0, 4, 8)[i % 3], i % 3))
    return tuple(c)


FWD_CASES = _fwd_cases()


def narrow_trips(B):
    """(blocks, the most grid-stride trips of one block) of affine_narrow_fwd_kernel."""
    g = min(max(cdiv(B, NARROW_ROWS), 1), FWD_MAX_BLOCKS)
    return g, cdiv(cdiv(B, NARROW_ROWS), g)


def act_fwd_f64(v, act):
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-v))
    return v


def act_fwd_bound(v, ev, act):
    """relu is 1-Lipschitz, sigmoid 1/4-Lipschitz and evaluated within SIGMOID_FWD_RTOL."""
    if act == 2:
        return 0.25 * ev + SIGMOID_FWD_RTOL * act_fwd_f64(v, 2)
    return ev


def narrow_inputs(n0, n, B, padx, kind):
    """x [B, n0 + padx] (padding NaN), Qa = [Q; c] [n0 + 1, n]; Gaussian Qa scaled by
    1/sqrt(n0 + 1) so that the sigmoid is not saturated."""
    rng = np.random.default_rng([n0, n, B, padx, kind == "int", 9])
    x = np.full((B, n0 + padx), np.nan, F32)
    x[:, :n0] = draw(rng, kind, (B, n0), 3)
    Qa = draw(rng, kind, (n0 + 1, n))
    return x, (Qa if kind == "int" else (Qa / F32(math.sqrt(n0 + 1))).astype(F32))


def narrow_ref(x, Qa, act):
    """y = act(x·Q + c): k ascending from 0, then + c: depth n0 + 1 → (value, err, mag of the
    pre-activation)."""
    n0 = Qa.shape[0] - 1
    x64, Q = _f64(x[:, :n0]), _f64(Qa)
    v = x64 @ Q[:n0] + Q[n0]
    mag = np.abs(x64) @ np.abs(Q[:n0]) + np.abs(Q[n0])
    return act_fwd_f64(v, act), act_fwd_bound(v, (n0 + 2) * U32 * mag, act), mag


ROWDOT_N0 = (4, 252, 256, 260, 1024)
ROWDOT_B = (0, 1, 3, 17)
ROWDOT_CASES = tuple((ROWDOT_N0[i % 5], ROWDOT_B[(i + i // 5) % 4], (0, 4, 12)[i % 3], i % 3)
                     for i in range(10))


def rowdot_inputs(n0, B, pad, kind):
    rng = np.random.default_rng([n0, B, pad, kind == "int", 10])
    x = np.full((B, n0 + pad), np.nan, F32)
    x[:, :n0] = draw(rng, kind, (B, n0))
    q = draw(rng, kind, n0)  # Gaussian q scaled by 1/sqrt(n0): the sigmoid is not saturated
    return x, (q if kind == "int" else (q / F32(math.sqrt(n0))).astype(F32)), draw(rng, kind, 1)


def rowdot_depth_act(n0):
    """rowdot_act_kernel: a lane takes ceil(n0 / 256) float4s, each a 4-term dot (3 additions)
    added to acc (1); the butterfly (6); + c (1)."""
    return 4 * cdiv(n0, 256) + 7


def rowdot_ref(x, q, c, act):
    n0 = q.size
    x64 = _f64(x[:, :n0])
    v = x64 @ _f64(q) + float(c[0])
    mag = np.abs(x64) @ np.abs(_f64(q)) + abs(float(c[0]))
    return act_fwd_f64(v, act), act_fwd_bound(v, (rowdot_depth_act(n0) + 1) * U32 * mag, act), mag


def emulate_rowdot(x, q, c):
    """rowdot_act_kernel's order in fp32 (pre-activation)."""
    n0 = q.size
    B = x.shape[0]
    xq = np.zeros((B, 1024), F32)
    xq[:, :n0] = x[:, :n0] * q[None]
    t = xq.reshape(B, 4, 64, 4)  # [row, j, lane, element]
    acc = np.zeros((64, B), F32)
    for j in range(4):
        d = ((t[:, j, :, 0] + t[:, j, :, 1]) + t[:, j, :, 2]) + t[:, j, :, 3]
        acc = acc + d.T
    return butterfly(acc) + c[0]


# =============================================================================================
# 6. rs_dlrm_dense_tail
TAIL = collections.namedtuple("TAIL", "m b1 b2 b3 n0 n1 n2 subset p_off")
TAIL_CASES = (
    TAIL(1, 4, 68, 132, 5, 17, 65, False, 0),
    TAIL(15, 132, 4, 68, 48, 64, 1, True, 0),
    TAIL(15, 68, 132, 4, 5, 17, 65, True, 1),
    TAIL(1, 132, 68, 4, 48, 64, 1, False, 0),
)
TAIL_LR = 0.05


def tail_accepts(c):
    """The bottom-chain RS_CHECK_ARG of rs_dlrm_dense_tail restated."""
    ws = (c.b1, c.b2, c.b3)
    return 1 <= c.m < 16 and all(w >= 4 and w % 4 == 0 and (c.m + 1) * w <= AUG_LDS for w in ws)


def tail_inputs(c):
    """Gaussian parameters of both chains, the top sums A [n0], s [1] and the bottom
    P = [A; s] [m + 1, b3]."""
    rng = np.random.default_rng(list(c) + [12])
    nf = c.n0 + C3_EXTRA if c.subset else c.n0
    d = dict(n_full0=nf, rows=None, inv=None,
             top_k=[_gauss(rng, (nf, c.n1)), _gauss(rng, (c.n1, c.n2)), _gauss(rng, c.n2)],
             top_b=[_gauss(rng, c.n1), _gauss(rng, c.n2), _gauss(rng, 1)],
             bot_k=[_gauss(rng, (c.m, c.b1)), _gauss(rng, (c.b1, c.b2)), _gauss(rng, (c.b2, c.b3))],
             bot_b=[_gauss(rng, c.b1), _gauss(rng, c.b2), _gauss(rng, c.b3)],
             A=_gauss(rng, c.n0), s=_gauss(rng, 1), P=_gauss(rng, (c.m + 1, c.b3)))
    if c.subset:
        d["rows"] = rng.permutation(nf)[:c.n0].astype(np.int32)
        d["inv"] = np.full(nf, -1, np.int32)
        d["inv"][d["rows"]] = np.arange(c.n0, dtype=np.int32)
    return d


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays, exactly: the product of two fp32 is exact in float64; the
    float64 sum's rounding error is recovered (two-sum) and, where the rounded sum sits exactly
    between two fp32 values, pushes it off the tie the way the infinitely precise sum falls."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    r = s.astype(F32)
    lo = np.where(r.astype(np.float64) > s, np.nextafter(r, F32(-np.inf)), r)
    hi = np.where(r.astype(np.float64) < s, np.nextafter(r, F32(np.inf)), r)
    tie = (lo != hi) & (s - lo.astype(np.float64) == hi.astype(np.float64) - s) & (err != 0)
    return np.where(tie, np.where(err > 0, hi, lo), r).astype(F32)


def sgd_fma(p, g, lr):
    """tail_sgd: p = fmaf(-lr, g, p), lr as the float the kernel receives."""
    return fma32(np.full(g.shape, -F32(lr), F32), g, p)
