"""Case lists, mask builders and float64 references for the edge tests of the DIEN aux-loss
kernels (csrc/dien_aux.hip) and of the valid-row products (csrc/dien_proj.hip).
tests/test_dien_rows_edges_cpu.py proves the references against brute-force loops and that every
case list reaches the path it names; tests/test_dien_rows_edges_gpu.py runs the kernels against
them. numpy and plain torch on the CPU only: nothing here touches recommender_amd.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import dien as OD

U24 = 2.0 ** -24  # the fp32 unit roundoff


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---------------------------------------------------------------------------------------------
# 1. rs_valid_rows: vr_write_kernel lists 4096-row blocks, 1024 rows per wave, 64 per ballot
VR_RS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
VR_KINDS = ("all", "none", "row0", "last", "first64", "last64", "first1024", "last1024",
            "first4096", "last4096", "random", "bytes")
VR_SENTINEL = -7


def vr_mask(kind, R, rng):
    """uint8 [R]; != 0 is a valid row. firstS / lastS: only the first / only the last row of
    every S-row stretch (a ragged last stretch has its last row at R - 1 left out: `last` has
    it). bytes: random 30 % holding 2 or 255."""
    m = np.zeros(R, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "none":
        pass
    elif kind == "row0":
        m[0] = 1
    elif kind == "last":
        m[R - 1] = 1
    elif kind.startswith("first"):
        m[::int(kind[5:])] = 1
    elif kind.startswith("last"):
        s = int(kind[4:])
        m[s - 1::s] = 1
    elif kind == "random":
        m[:] = rng.random(R) < 0.3
    elif kind == "bytes":
        m[:] = np.where(rng.random(R) < 0.3, rng.choice(np.array([2, 255], np.uint8), R), 0)
    else:
        raise ValueError(kind)
    return m


def valid_rows_ref(m):
    return np.flatnonzero(np.asarray(m).reshape(-1)).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# 2. the masked products
# (K, N) of rs_masked_proj: masked_proj_kernel<KM, NB>, KM = 16 / 36 / 64 by K, NB = ceil(N / 64)
PROJ_PAIRS = ((1, 1), (16, 65), (16, 192), (17, 64), (36, 128), (17, 129), (64, 64), (37, 65),
              (64, 192), (36, 108), (1, 129), (37, 128))
PROJ_COUNTS = (0, 1, 31, 32, 33, 127, 128, 129)  # one wave per 32 listed rows, 4 waves a block
# rs_masked_dx(_acc): masked_dx_kernel<NM>, NM = 64 / 112 / 128 / 192 by N
DX_NS = (1, 64, 65, 112, 113, 128, 129, 192)
DX_KS = (1, 36, 63, 64)
DX_COUNTS = (0, 15, 16, 17, 63, 64, 65)  # one wave per 16 listed rows, 4 waves a block
# rs_masked_wgrad: 256 threads while (K + 1)·ceil(N / 4) <= 1024, else 1024
WGRAD_PAIRS = ((1, 1), (36, 108), (36, 112), (63, 64), (64, 192), (20, 109))
WGRAD_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 8191, 8192, 8193)
WG_BLOCKS = 512  # kWgBlocks: the row chunks of a weight gradient


def proj_class(K, N):
    """(KM, NB) of the masked_proj_kernel instance rs_masked_proj launches."""
    return (16 if K <= 16 else 36 if K <= 36 else 64), (N + 63) // 64


def dx_class(N):
    """NM of the masked_dx_kernel instance."""
    return 64 if N <= 64 else 112 if N <= 112 else 128 if N <= 128 else 192


def wgrad_items(K, N):
    """Outputs (4-column groups incl. the ones row) of a wgrad block: <= 1024 → 256 threads."""
    return (K + 1) * ((N + 3) // 4)


def wgrad_per(count):
    """Listed rows per block (masked_wgrad_kernel's `per`)."""
    return ((count + WG_BLOCKS - 1) // WG_BLOCKS + 15) // 16 * 16


def dx_rs(count):
    """The R of a dx case: the count itself (every row listed), one that is no multiple of 16,
    and a multiple of 16 that is no multiple of 64."""
    r2 = count + 21
    r2 += r2 % 16 == 0
    r3 = (count + 30) // 16 * 16 + 16
    r3 += 16 * (r3 % 64 == 0)
    return tuple(r for r in (count, r2, r3) if r > 0)


def count_mask(R, count, rng, values=(1,)):
    """uint8 [R] with exactly `count` valid rows, the first and the last row among them when
    count >= 2 (so the list spans the buffer)."""
    assert 0 <= count <= R
    m = np.zeros(R, np.uint8)
    if count == R:
        rows = np.arange(R)
    elif count >= 2:
        rows = np.concatenate([[0, R - 1], 1 + rng.choice(R - 2, count - 2, replace=False)])
    else:
        rows = rng.choice(R, count, replace=False)
    m[rows] = rng.choice(np.array(values, np.uint8), len(rows))
    assert int((m != 0).sum()) == count
    return m


def proj_ref(x, W, bias, rows):
    """(y [len(rows), N] float64, bound): y = x[rows]·W + bias; the fp32 fma chain's worst case
    (n + 1)·2^-24·(Σ|x·w| + |bias|), n = K (+ 1 with a bias)."""
    x, W = np.asarray(x, np.float64)[rows], np.asarray(W, np.float64)
    y, mag, n = x @ W, np.abs(x) @ np.abs(W), W.shape[0]
    if bias is not None:
        b = np.asarray(bias, np.float64)
        y, mag, n = y + b, mag + np.abs(b), n + 1
    return y, (n + 1) * U24 * mag


def dx_ref(d, W, add, rows):
    """(dx [len(rows), K] float64, bound): dx = d[rows]·Wᵀ (+ add[rows]); n = N (+ 1)."""
    d, W = np.asarray(d, np.float64)[rows], np.asarray(W, np.float64)
    y, mag, n = d @ W.T, np.abs(d) @ np.abs(W).T, W.shape[1]
    if add is not None:
        a = np.asarray(add, np.float64)[rows]
        y, mag, n = y + a, mag + np.abs(a), n + 1
    return y, (n + 1) * U24 * mag


def shifted_rows(A, rows, shift_L):
    """A_r of rs_masked_wgrad: row r, or with shift_L > 0 row r - 1 within each length-shift_L
    sequence and 0 at its first step."""
    A = np.asarray(A, np.float64)
    if shift_L <= 0:
        return A[rows]
    out = A[np.maximum(rows - 1, 0)].copy()
    out[rows % shift_L == 0] = 0.0
    return out


def wgrad_ref(A, D, rows, shift_L=0):
    """(C [K, N], sums [N], bound C, bound sums): Σ_listed A_rᵀ·D_r and Σ_listed D_r in float64;
    the bounds with n = the listed-row count (block partials of at most n terms, then a fold)."""
    a, d = shifted_rows(A, rows, shift_L), np.asarray(D, np.float64)[rows]
    n = len(rows)
    return (a.T @ d, d.sum(0), (n + 1) * U24 * (np.abs(a).T @ np.abs(d)),
            (n + 1) * U24 * np.abs(d).sum(0))


def shift_mask(B, T, rng):
    """uint8 [B, T] for the shift_L cases: listed first steps (their A row is 0), listed rows
    whose predecessor is unlisted (it is still read) and listed rows with a listed one."""
    m = (rng.random((B, T)) < 0.4).astype(np.uint8)
    m[::2, 0] = 1
    m[1::2, 0] = 0
    m[:, 1] = 0
    m[:, 2] = 1
    m[:, 3] = 1
    return m


# ---------------------------------------------------------------------------------------------
# 3. the aux loss
AUX_LS = (2, 3, 16, 17, 18, 32, 33, 34)
AUX_BS = (1, 2, 3, 5)
AUX_KINDS = ("post", "random", "dead_tile", "only1", "only_last", "late", "bytes")
MASKED_SCALE = 8.0  # rows no valid aux row reads hold values of another scale


def aux_mask(kind, B, L, rng):
    """uint8 [B, L]; aux row t < L - 1 is valid where mask[b, t + 1] != 0. Every example has a
    valid aux row.
    post       right-padded, the last valid step at L - 1, 16, 17 (clipped to [1, L - 1]) by turn
    random     p = 1/2, one step >= 1 forced
    dead_tile  L >= 34: valid steps in 1..16 (aux tile 0) and at 33.. (tile 2), none in 17..32
    only1 / only_last   one valid aux row; step 0 valid too
    late       step 0 masked (its byte is never read), later steps valid
    bytes      random, valid steps hold 1, 2 or 255"""
    m = np.zeros((B, L), np.uint8)
    if kind == "post":
        for b in range(B):
            last = min(max((L - 1, 16, 17)[b % 3], 1), L - 1)
            m[b, :last + 1] = 1
    elif kind in ("random", "bytes", "late"):
        m[:] = rng.random((B, L)) < 0.5
        for b in range(B):
            m[b, rng.integers(1, L)] = 1
        if kind == "bytes":
            m *= rng.choice(np.array([1, 2, 255], np.uint8), (B, L))
        if kind == "late":
            m[:, 0] = 0
    elif kind == "dead_tile":
        assert L >= 34
        m[:, 0] = 1
        m[:, 1:17] = rng.random((B, 16)) < 0.5
        m[:, 33:] = rng.random((B, L - 33)) < 0.5
        m[:, 2] = 1
        m[:, 33] = 1
    elif kind == "only1":
        m[:, :2] = 1
    elif kind == "only_last":
        m[:, 0] = 1
        m[:, L - 1] = 1
    else:
        raise ValueError(kind)
    assert ((m[:, 1:] != 0).sum(1) > 0).all()
    return m


def _aux_case_list():
    cases = []
    for i, L in enumerate(AUX_LS):
        for k, kind in enumerate(AUX_KINDS):
            if kind == "dead_tile" and L < 34:
                continue
            cases.append((36, AUX_BS[(i + k) % 4], L, kind))
        for k in range(2):  # the (16, 16) instance: two kinds per L, by turn
            kind = AUX_KINDS[(2 * i + k) % len(AUX_KINDS)]
            if kind == "dead_tile" and L < 34:
                kind = "random"
            cases.append((16, AUX_BS[(i + k + 1) % 4], L, kind))
    cases += [(36, 3, 3, "all"), (36, 1, 2, "all"), (36, 5, 50, "dead_tile")]
    return tuple(cases)


# (H = E, B, L, mask kind). "all": every step valid.
AUX_CASES = _aux_case_list()


def persistent_cases(cus):
    """The loops of the persistent kernels for a device of `cus` compute units.
    backward: L = 33, every step valid: 2 live tiles per example (the third holds only hidden
    row 32, which has no aux row), B pairs of items over `cus` blocks; B = ceil(700·cus/256).
    forward: B = 2·3·cus + 3 (odd) at L = 3: ceil(B/2) rounds over 3·cus blocks.
    odd: L = 16, every step valid: one live tile per example, B = 5·cus + 1 items — the last pair
    has no second item and comes in a block's third round, after two full ones."""
    return ((36, -(-700 * cus // 256), 33, "all"), (36, 6 * cus + 3, 3, "all"),
            (36, 5 * cus + 1, 16, "all"))


def aux_live_items(mask):
    """The (tile, b) items aux_live_kernel marks live, as tile·B + b in order: the 16-row tiles
    over t < L that hold a valid aux row t <= L - 2, or every tile of an example without one."""
    m = np.asarray(mask) != 0
    B, L = m.shape
    NT = (L + 15) // 16
    cnt = m[:, 1:].sum(1)
    out = []
    for tile in range(NT):
        for b in range(B):
            rows = [t for t in range(16 * tile, min(16 * tile + 16, L - 1)) if m[b, t + 1]]
            if rows or cnt[b] == 0:
                out.append(tile * B + b)
    return out


def bwd_rounds(n_live, blocks):
    """Rounds of aux_bwd_kernel's loop per block (max, min): pairs pr = blk, blk + blocks, ..."""
    pairs = (n_live + 1) // 2
    per = [len(range(blk, pairs, blocks)) for blk in range(blocks)]
    return max(per), min(per)


def fwd_rounds(B, cus):
    """Rounds of aux_fwd_kernel's loop per block (max, min) and its grid."""
    n = (B + 1) // 2
    grid = min(n, 3 * cus)
    per = [len(range(blk, n, grid)) for blk in range(grid)]
    return max(per), min(per), grid


def fwd_tiles(L):
    return (L - 1 + 15) // 16


def bwd_tiles(L):
    return (L + 15) // 16


def aux_daux(B, rng):
    """Upstream gradients spanning 1e-3 .. 1e3 with both signs; B >= 5: one exact 0."""
    d = 10.0 ** rng.uniform(-3, 3, B) * np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    if B >= 2:
        d[0], d[1] = 1e3, -1e-3
    if B >= 5:
        d[B - 2] = 0.0
    return _f32(d)


def aux_inputs(H, B, L, kind, seed=0, mask=None):
    """hidden / pos / neg [B, L, H], the aux net's parameters in Keras layouts (W1 [2H, 80],
    W2 [80, 40], W3 [40, 1], glorot; biases 0.2·N(0, 1)), mask uint8 [B, L], daux [B]. The rows
    no valid aux row reads (hidden t with mask[t + 1] = 0 or t = L - 1; pos / neg t with
    mask[t] = 0 or t = 0) are MASKED_SCALE times larger: nothing may depend on them."""
    kinds = AUX_KINDS + ("all", "given")
    rng = np.random.default_rng([seed + 20, H, B % 1000003, L, kinds.index(kind)])
    if mask is not None:
        m = np.ascontiguousarray(mask, np.uint8)
    elif kind == "all":
        m = np.ones((B, L), np.uint8)
    else:
        m = aux_mask(kind, B, L, rng)
    v = m != 0
    read_h = np.concatenate([v[:, 1:], np.zeros((B, 1), bool)], 1)
    read_e = v.copy()
    read_e[:, 0] = False
    d = {}
    for n, read in (("hidden", read_h), ("pos", read_e), ("neg", read_e)):
        x = rng.standard_normal((B, L, H)) * 0.5
        d[n] = _f32(np.where(read[:, :, None], x, MASKED_SCALE * x))

    def glorot(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return _f32(rng.uniform(-lim, lim, (i, o)))

    d.update(W1=glorot(2 * H, 80), b1=_f32(rng.standard_normal(80) * 0.2),
             W2=glorot(80, 40), b2=_f32(rng.standard_normal(40) * 0.2),
             W3=glorot(40, 1), b3=_f32(rng.standard_normal(1) * 0.2),
             mask=m, daux=aux_daux(B, rng))
    return d


AUX_IN = ("hidden", "pos", "neg")
AUX_PARAMS = ("W1", "b1", "W2", "b2", "W3", "b3")
AUX_OUT = ("aux", "dhidden", "dpos", "dneg")


def _aux_eval(d, dtype, sl=slice(None)):
    p = {n: torch.from_numpy(d[n][sl] if n in AUX_IN else d[n]).to(dtype).requires_grad_(True)
         for n in AUX_IN + AUX_PARAMS}
    layers = [(p["W1"], p["b1"], "sigmoid"), (p["W2"], p["b2"], "sigmoid"), (p["W3"], p["b3"], None)]
    m = torch.from_numpy(d["mask"][sl] != 0)
    aux = OD.aux_loss(p["hidden"], p["pos"], p["neg"], m, layers)
    g = torch.autograd.grad(aux, list(p.values()), torch.from_numpy(d["daux"][sl]).to(dtype))
    out = dict(aux=aux.detach().numpy())
    out.update({"d" + n: t.numpy() for n, t in zip(p, g)})
    return out


def aux_eval(d, dtype):
    """oracle.dien.aux_loss and its gradients under autograd in `dtype`:
    {aux, dhidden, dpos, dneg, dW1, db1, dW2, db2, dW3, db3}."""
    return _aux_eval(d, dtype)


def aux_param_magnitude(d, chunks=None):
    """{dW1, ...}: Σ_k |g_k| in float64, g_k the contribution of example k (or, with `chunks`,
    of contiguous chunk k of the batch) to each parameter gradient."""
    B = d["mask"].shape[0]
    if chunks is None or chunks >= B:
        cuts = list(range(B + 1))
    else:
        cuts = [round(i * B / chunks) for i in range(chunks + 1)]
    mag = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        g = _aux_eval(d, torch.float64, slice(lo, hi))
        g = {"d" + n: np.abs(g["d" + n]) for n in AUX_PARAMS}
        mag = g if mag is None else {n: mag[n] + g[n] for n in mag}
    return mag


def example_scale(ref):
    """|ref| + S_b, S_b the largest |ref| of the example (axis 0) in this tensor."""
    a = np.abs(np.asarray(ref, np.float64))
    s = a.reshape(a.shape[0], -1).max(1) if a.ndim > 1 else a
    return a + s.reshape((-1,) + (1,) * (a.ndim - 1))


def worst_ratio(err, scale):
    """max err / scale; an element whose scale is 0 must have err = 0 (ratio 0, else inf)."""
    err, scale = np.asarray(err, np.float64), np.asarray(scale, np.float64)
    if err.size == 0:
        return 0.0
    r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def aux_ratios(got, ref64, mag):
    """{tensor: worst ratio of |got - ref64| under the scales of the check}: per example
    (|ref64| + S_b) for aux, dhidden, dpos, dneg; Σ_b |g_b| for the parameter gradients."""
    out = {}
    for n in AUX_OUT:
        out[n] = worst_ratio(np.abs(np.asarray(got[n], np.float64) - ref64[n]),
                             example_scale(ref64[n]))
    for n in AUX_PARAMS:
        g = np.asarray(got["d" + n], np.float64).reshape(ref64["d" + n].shape)
        out["d" + n] = worst_ratio(np.abs(g - ref64["d" + n]), mag["d" + n])
    return out


@functools.lru_cache(maxsize=None)
def aux_case(spec):
    """(inputs, float64 reference, parameter-gradient magnitudes, the fp32 control's ratios) of
    a case, computed once and shared: read only. Batches past 64 take 16 chunks for the
    magnitudes."""
    d = aux_inputs(*spec)
    r64 = aux_eval(d, torch.float64)
    mag = aux_param_magnitude(d, 16 if spec[1] > 64 else None)
    ctl = aux_ratios(aux_eval(d, torch.float32), r64, mag)
    for t in list(r64.values()) + list(mag.values()):
        t.setflags(write=False)
    return d, r64, mag, ctl


def rho32(specs):
    """The fp32 control's worst ratio pooled over the case list `specs`."""
    return max(max(aux_case(s)[3].values()) for s in specs)


def rho32_by_tensor(specs):
    """{tensor: the fp32 control's worst ratio over `specs`} — the pooled figure split by output.
    The parameter gradients of the smallest cases dominate the pooled one (pos and neg rows
    cancel inside an example, so Σ_b |g_b| is far below the terms that were rounded); split, the
    per-example outputs are held to their own, much smaller, figure."""
    names = AUX_OUT + tuple("d" + n for n in AUX_PARAMS)
    return {n: max(aux_case(s)[3][n] for s in specs) for n in names}


# the NaN pattern: example 2 of 5 has no valid aux row
def nan_case(H=36, L=18):
    m = aux_mask("random", 5, L, np.random.default_rng(3))
    m[2, 1:] = 0
    m[2, 0] = 1
    d = aux_inputs(H, 5, L, "given", seed=5, mask=m)
    d["daux"] = _f32([1.5, -0.25, 2.0, 0.0, -3.0])
    return d


# 4. the fused node: (B, L) and mask kind
FUSED_CASES = ((5, 17, "random"), (5, 17, "post"), (64, 37, "random"), (64, 37, "post"))
