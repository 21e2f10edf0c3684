"""NumPy float32 restatement of the RS_Q8 contract (include/recsys_hip.h a-1c), written from the
contract: every operation an np.float32 element-wise operation in the stated order (np.rint is
ties-to-even; the dequantise is a multiply, then an add). The bag is the EmbeddingBag
restatement's Python loop over positions (tests/embedding_bag_ref.py) with the dequantised
element as the table element, which is what the contract says. Also the inputs the GPU tests use,
so tests/test_embedding_q8_cpu.py can prove what they claim about them.

tests/test_embedding_q8_cpu.py checks this file; tests/test_embedding_q8_gpu.py compares the
kernels with it."""
from __future__ import annotations

import numpy as np

from tests import embedding_bag_ref as B

f32 = np.float32
SUM, MEAN = B.SUM, B.MEAN
TINY = f32(2.0 ** -149)  # the smallest subnormal


def row_bytes(dim):
    return (8 + dim + 15) // 16 * 16


def narrow_ld(dim):
    """The smallest legal q_ld: a multiple of 4."""
    return (8 + dim + 3) // 4 * 4


def row_stats(table):
    """(lo, hi, scale, flagged) per row: lo = min + 0, hi = max + 0, scale = (hi - lo) / 255; a
    row with a non-finite element or an overflowing range is flagged (scale and lo then 0)."""
    x = np.asarray(table, f32)
    with np.errstate(all="ignore"):
        lo = x.min(1) + f32(0)
        hi = x.max(1) + f32(0)
        rng = hi - lo
        flagged = ~np.isfinite(x).all(1) | ~np.isfinite(rng)
        scale = rng / f32(255)
    lo = np.where(flagged, f32(0), lo).astype(f32)
    scale = np.where(flagged, f32(0), scale).astype(f32)
    return lo, hi, scale, flagged


def raw_quotient(table):
    """rint((x - lo) / scale) before the clamp (0 where scale == 0 or the row is flagged)."""
    x = np.asarray(table, f32)
    lo, _, scale, flagged = row_stats(x)
    q = np.zeros(x.shape, f32)
    live = (scale != 0) & ~flagged
    with np.errstate(all="ignore"):
        q[live] = np.rint((x[live] - lo[live, None]) / scale[live, None])
    return q


def quantize(table, q_ld=None):
    """(qtable uint8 [n, q_ld], flagged bool [n])."""
    x = np.asarray(table, f32)
    n, dim = x.shape
    q_ld = row_bytes(dim) if q_ld is None else q_ld
    lo, _, scale, flagged = row_stats(x)
    codes = np.minimum(np.maximum(raw_quotient(x), f32(0)), f32(255)).astype(np.uint8)
    q = np.zeros((n, q_ld), np.uint8)
    q[:, 0:4] = scale.view(np.uint8).reshape(n, 4)
    q[:, 4:8] = lo.view(np.uint8).reshape(n, 4)
    q[:, 8:8 + dim] = codes
    return q, flagged


def header(q):
    q = np.ascontiguousarray(q[:, :8])
    h = q.view(f32).reshape(-1, 2)
    return h[:, 0], h[:, 1]


def dequantize(q, dim):
    scale, bias = header(q)
    with np.errstate(all="ignore"):
        return (q[:, 8:8 + dim].astype(f32) * scale[:, None] + bias[:, None]).astype(f32)


def lookup(q, dim, ids, slot_offsets=None):
    """(out [n_ids, dim], flag): slot = position % n_slots; an out-of-range id reads zeros."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    table = dequantize(q, dim)
    out = np.zeros((ids.size, dim), f32)
    flag = False
    n_slots = 1 if slot_offsets is None else len(slot_offsets) - 1
    for p, i in enumerate(ids):
        lo, card = 0, q.shape[0]
        if slot_offsets is not None:
            s = p % n_slots
            lo, card = int(slot_offsets[s]), int(slot_offsets[s + 1] - slot_offsets[s])
        if 0 <= i < card:
            out[p] = table[lo + i]
        else:
            flag = True
    return out, flag


def bag_forward(q, dim, ids, n_bags, **kw):
    """tests/embedding_bag_ref.bag_forward with the dequantised element as the table element."""
    return B.bag_forward(dequantize(q, dim), ids, n_bags, **kw)


def bound(table):
    """The accuracy bound per element, float64: 0.5 scale (1 + 2^-10) + 2^-23 max|x_row| + 2^-139.
    Half a step is the rounding of the code; the 2^-10 covers the rounding of scale itself against
    a range of 255 steps ((hi - lo) / 255 is within 2^-24 relative of the exact quotient, times up
    to 255 codes) and of the quotient; 2^-23 max|x| the two roundings of code * scale + bias and
    of x - lo; 2^-139 the subnormal floor, where scale carries an absolute error of 2^-150 times
    up to 255 codes and every operation one of 2^-150."""
    x = np.asarray(table, np.float64)
    _, _, scale, _ = row_stats(table)
    return (0.5 * scale.astype(np.float64) * (1 + 2.0 ** -10))[:, None] \
        + 2.0 ** -23 * np.abs(x).max(1)[:, None] + 2.0 ** -139


# ---- inputs -------------------------------------------------------------------------------
def tie_row(dim):
    """lo = 0, hi = 255, the other elements k + 0.5: scale is exactly 1, every quotient a tie."""
    r = np.empty(dim, f32)
    for c in range(dim):
        r[c] = (c * 7) % 255 + 0.5
    r[0] = 0.0
    if dim > 1:
        r[1] = 255.0
    return r


def clamp_row(dim):
    """hi - lo = 382 * 2^-149: 382 / 255 = 1.498 rounds to a scale of one subnormal step, so the
    maximum's quotient is 382 and only the clamp makes its code 255 (dim >= 2)."""
    r = np.zeros(dim, f32)
    r[-1] = f32(382) * TINY
    if dim > 2:
        r[1:-1] = (np.arange(dim - 2) % 382).astype(f32) * TINY
    return r


def families(dim, rows=4, seed=3):
    """name -> [rows, dim] float32, every family of the contract's accuracy trial and the edge
    rows of the quantise tests; all finite with a finite range."""
    r = np.random.default_rng(seed * 1000 + dim)
    g = lambda: r.standard_normal((rows, dim))  # noqa: E731
    f = {
        "gauss": g(),
        "offset": 1000.0 + r.uniform(-0.01, 0.01, (rows, dim)),
        "small": r.uniform(-0.05, 0.05, (rows, dim)),
        "huge": g() * 1e30,
        "loguniform": np.exp(r.uniform(-80, 80, (rows, dim))) * r.choice([-1.0, 1.0], (rows, dim)),
        "three_valued": r.choice([-1.5, 0.25, 7.0], (rows, dim)),
        "two_valued": r.choice([-3.0, 11.0], (rows, dim)),
        "constant": np.repeat(r.standard_normal((rows, 1)), dim, 1),
        "zeros": np.where(r.random((rows, dim)) < 0.5, -0.0, 0.0),
        "tie": np.stack([tie_row(dim)] * rows),
        "clamp": np.stack([clamp_row(dim)] * rows),
    }
    with np.errstate(all="ignore"):
        out = {k: v.astype(f32) for k, v in f.items()}
        for e in range(-45, -35):
            out[f"subnormal{e}"] = (g() * 10.0 ** e).astype(f32)
    out["zeros"][0] = -0.0  # a row of -0 alone
    return out


def flagged_rows(dim):
    """[4, dim]: a NaN, a +inf, a -inf in an otherwise ordinary row, and a -3e38 .. 3e38 row whose
    range overflows (at dim 1 that row is a finite constant and is not flagged)."""
    r = np.random.default_rng(dim).standard_normal((4, dim)).astype(f32)
    r[0, dim // 2] = np.nan
    r[1, -1] = np.inf
    r[2, 0] = -np.inf
    r[3] = 3e38
    r[3, 0] = -3e38 if dim > 1 else 3e38
    return r


def table(dim, n_rows, flagged=True, seed=3):
    """[n_rows, dim]: the families' rows in turn; with `flagged`, flagged_rows in the first, the
    last and an inner position (as many as n_rows has room for)."""
    fam = np.concatenate(list(families(dim, seed=seed).values()))
    t = fam[np.arange(n_rows) % fam.shape[0]].copy()
    if flagged:
        bad = flagged_rows(dim)
        t[0] = bad[0]
        if n_rows > 1:
            t[-1] = bad[1]
        if n_rows > 4:
            t[n_rows // 2] = bad[2]
            t[n_rows // 2 + 1] = bad[3]
    return t


QUANT_DIMS = list(range(1, 21)) + [31, 32, 33, 64, 120, 128, 130, 136, 256, 260, 1100]
# 1100: 8 + 1100 bytes are 70 16-byte pieces, past the 64 lanes of a group (two passes); on the
# 4-byte path 256 and 260 are already past them
N_ROWS = [1, 2, 1000]
