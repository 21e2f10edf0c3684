"""The contract of rs_item_softmax_fwd / _bwd (include/recsys_hip.h, "Softmax cross-entropy over
item rows") restated in NumPy with the [B, M] logits materialised, in float64 (the reference) and
in float32 (the control whose error against float64, rho32, sets the tolerance), the case
generators of tests/test_item_softmax_gpu.py, and the error measures both test files share."""
import functools

import numpy as np

f32 = np.float32
TILE = 32          # streamed rows per wave tile
ROUND = 4 * TILE   # rows the four waves of a block take per round
OUT = ("loss", "lse", "dq", "dv")

B_SIZES = (1, 2, 31, 32, 33, 65)
M_SIZES = (1, 2, 31, 32, 33, 127, 128, 129, 513)
DIMS = (1, 3, 4, 63, 64, 65, 128, 160, 255, 256)
SPLITS = (1, 2, 7)


# ---- the contract --------------------------------------------------------------------------
def kept_mask(B, M, t, ids):
    """[B, M] bool: the columns row r keeps; all False for a row whose target is outside [0, M)."""
    valid = (t >= 0) & (t < M)
    tc = np.where(valid, t, 0)
    kept = np.ones((B, M), bool)
    if ids is not None:
        kept = ids[None, :] != ids[tc][:, None]
        kept[np.arange(B), tc] = True
    return kept & valid[:, None], valid, tc


def evaluate(c, dtype=np.float64):
    """{loss, lse, dq, dv} of case c = dict(q, v, targets, inv_temp, bias, ids, g) in `dtype`."""
    q, v = c["q"].astype(dtype), c["v"].astype(dtype)
    B, M = q.shape[0], v.shape[0]
    t = np.arange(B) if c.get("targets") is None else np.asarray(c["targets"], np.int64)
    kept, valid, tc = kept_mask(B, M, t, c.get("ids"))
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        z = dtype(c.get("inv_temp", 1.0)) * (q @ v.T)
        if c.get("bias") is not None:
            z = z - c["bias"].astype(dtype)[None, :]
        zk = np.where(kept, z, -np.inf)
        m = zk.max(1)  # NaN if any kept logit is NaN
        ms = np.where(np.isfinite(m), m, 0).astype(dtype)
        s = np.where(kept, np.exp(z - ms[:, None]), 0).sum(1, dtype=dtype)
        lse = np.where(np.isfinite(m), ms + np.log(s), m).astype(dtype)  # ±inf, NaN: themselves
        lse = np.where(valid, lse, np.nan)
        loss = lse - z[rows, tc]
        g = np.ones(B, dtype) if c.get("g") is None else c["g"].astype(dtype)
        p = np.where(kept, np.exp(z - lse[:, None]), 0)
        onehot = np.zeros((B, M), dtype)
        onehot[rows, tc] = 1
        coef = (g * dtype(c.get("inv_temp", 1.0)))[:, None] * (p - onehot)
        coef = np.where(valid[:, None], coef, 0).astype(dtype)
        dq = coef @ v
        dv = coef.T @ q
    return {"loss": loss.astype(dtype), "lse": lse, "dq": dq, "dv": dv}


# ---- error measures ------------------------------------------------------------------------
def row_scale(ref):
    """|ref| + the largest |ref| of the row (tests/dien_rows_edges.py example_scale), non-finite
    entries counting as 0."""
    a = np.abs(np.where(np.isfinite(ref), ref, 0.0)).astype(np.float64)
    return a + a.max(1, keepdims=True) if a.shape[1] else a


def same_pattern(got, ref):
    """NaN where the reference has NaN, the same infinity where it has one, finite elsewhere."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.isnan(got) == np.isnan(ref)).all() and
                (np.where(np.isinf(got), np.sign(got), 0) == np.where(np.isinf(ref), np.sign(ref), 0)).all())


def ratios(got, ref64):
    """{output: worst error}: absolute for loss / lse, |err| / (|ref| + row max) for dq / dv, over
    the entries where the reference is finite; an entry of scale 0 must be exact (else inf)."""
    out = {}
    for n in OUT:
        r = np.asarray(ref64[n], np.float64)
        g = np.asarray(got[n], np.float64).reshape(r.shape)
        fin = np.isfinite(r)
        with np.errstate(all="ignore"):
            err = np.where(fin, np.abs(g - r), 0.0)
        err = np.where(np.isnan(err), np.inf, err)  # a NaN where the reference is finite
        if n in ("loss", "lse"):
            out[n] = float(err.max()) if err.size else 0.0
        else:
            sc = row_scale(r)
            q = np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), np.where(err > 0, np.inf, 0.0))
            out[n] = float(q.max()) if q.size else 0.0
    return out


# ---- generators ----------------------------------------------------------------------------
def _rows(rng, n, dim):
    return (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(f32)


def _g(rng, B):
    """grad_loss of both signs over 1e-3 … 1e3."""
    g = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), B)) * rng.choice([-1.0, 1.0], B)
    if B >= 2:
        g[0], g[-1] = 1e-3, -1e3
    return g.astype(f32)


def random_case(seed, B, M, dim, targets="random", bias=True, ids="some", inv_temp=1.0, n_splits=1):
    """Random rows. targets: None (column r; needs B <= M), "identity", "reversed", "same",
    "last", "random". ids: None, "distinct", "some" (a quarter of the columns share an id with
    another), "equal" (one id), "extreme" (INT64_MIN / MAX among them)."""
    rng = np.random.default_rng(seed)
    scale = f32(3.0 / np.sqrt(inv_temp))  # logits of a few units whatever inv_temp is
    q, v = _rows(rng, B, dim) * scale, _rows(rng, M, dim) * scale
    if targets is None:
        t = None
    elif targets == "identity":
        t = np.arange(B) % M
    elif targets == "reversed":
        t = (M - 1 - np.arange(B)) % M
    elif targets == "same":
        t = np.full(B, M // 2)
    elif targets == "last":
        t = np.full(B, M - 1)
    else:
        t = rng.integers(0, M, B)
    idv = None
    if ids == "distinct":
        idv = rng.permutation(M).astype(np.int64) * 7 - 3
    elif ids == "some":
        idv = np.arange(M, dtype=np.int64)
        n = max(M // 4, 1 if M > 1 else 0)
        idv[rng.integers(0, M, n)] = idv[rng.integers(0, M, n)]
    elif ids == "equal":
        idv = np.full(M, 42, np.int64)
    elif ids == "extreme":
        idv = rng.choice(np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1],
                                  np.int64), M)
    return dict(q=q, v=v, targets=None if t is None else t.astype(np.int32), inv_temp=inv_temp,
                bias=(rng.standard_normal(M) * 2).astype(f32) if bias else None, ids=idv,
                g=_g(rng, B), n_splits=n_splits)


def dominant_case(B, M, dim, col, as_target, n_splits=1, seed=0):
    """One logit at least 30 above every other in its row: column 0 of every query is 1 and of
    every item 0, except item `col`, which holds 40; the other columns' products stay within ±1.
    as_target: every row's target is `col`; else the targets avoid it (needs M >= 2), so that
    dropping the column moves lse by 30 or more either way."""
    rng = np.random.default_rng(1000 + seed + col)
    q = rng.uniform(-1, 1, (B, dim)).astype(f32) / f32(np.sqrt(dim))
    v = rng.uniform(-1, 1, (M, dim)).astype(f32) / f32(np.sqrt(dim))
    q[:, 0], v[:, 0] = 1, 0
    v[col, 0] = 40
    if as_target:
        t = np.full(B, col)
    else:
        t = np.arange(B) % M
        t[t == col] = (col + 1) % M
    return dict(q=q, v=v, targets=t.astype(np.int32), inv_temp=1.0, bias=None, ids=None,
                g=_g(rng, B), n_splits=n_splits)


def edge_columns(M, n_splits):
    """Column 0, the last one, and both sides of every tile, wave-round and split boundary (a
    split's tiles and rounds start at its first column)."""
    per = M // n_splits
    cols = {0, M - 1}
    for sp in range(n_splits):
        lo = sp * per
        hi = M if sp == n_splits - 1 else lo + per
        for e in (lo, lo + TILE, lo + ROUND, lo + ROUND + TILE, hi):
            cols |= {e - 1, e}
    return sorted(c for c in cols if 0 <= c < M)


def duplicate_case(M, t_col, dup_col, B=5, dim=12):
    """Accidental hits: every row's target is t_col and column dup_col holds the same id; the
    duplicate is made the row's largest logit, so keeping it would move lse by 30 or more."""
    c = dominant_case(B, M, dim, dup_col, False, seed=7)
    c["targets"] = np.full(B, t_col, np.int32)
    ids = np.arange(M, dtype=np.int64) + 100
    ids[dup_col] = ids[t_col]
    c["ids"] = ids
    return c


def magnitude_case(sign, inv_temp, B=33, M=70, dim=16):
    """Logits of magnitude 1e4: one coordinate pair carries ±1e4 / inv_temp exactly, the rest is
    small noise."""
    rng = np.random.default_rng(77)
    q, v = _rows(rng, B, dim) * f32(0.1), _rows(rng, M, dim) * f32(0.1)
    q[:, 1] = 100
    v[:, 1] = f32(sign * 100.0 / inv_temp) * rng.choice([1.0, 0.5, 0.999], M).astype(f32)
    return dict(q=q, v=v, targets=rng.integers(0, M, B).astype(np.int32), inv_temp=inv_temp,
                bias=None, ids=None, g=_g(rng, B), n_splits=2)


def inf_bias_case(col=33):
    """col_bias = +inf on a column that is no row's target, and the same case with the column
    removed."""
    c = random_case(5, 33, 70, 20, targets="random", ids=None)
    c["targets"] = np.where(c["targets"] == col, col + 1, c["targets"]).astype(np.int32)
    c["bias"][col] = np.inf
    keep = np.arange(70) != col
    d = dict(c, v=c["v"][keep], bias=c["bias"][keep],
             targets=(c["targets"] - (c["targets"] > col)).astype(np.int32))
    return c, d, keep


def nan_query_case(row=3):
    c = random_case(9, 33, 70, 20)
    c["q"][row, 5] = np.nan
    return c


def zero_g_case():
    c = random_case(11, 40, 70, 24)
    c["g"][[1, 7, 33, 38]] = 0
    return c


def _build_cases():
    cs = {}
    for B in B_SIZES:
        cs[f"B{B}"] = functools.partial(random_case, 100 + B, B, 129, 20, n_splits=2)
    for M in M_SIZES:
        cs[f"M{M}"] = functools.partial(random_case, 200 + M, 33, M, 36, inv_temp=20.0)
    for dim in DIMS:
        cs[f"dim{dim}"] = functools.partial(random_case, 300 + dim, 33, 70, dim, targets=None)
    for kind in (None, "identity", "reversed", "same", "last"):
        cs[f"targets_{kind}"] = functools.partial(random_case, 400, 33, 40, 12, targets=kind)
    for kind in ("distinct", "equal", "extreme", None):
        cs[f"ids_{kind}"] = functools.partial(random_case, 500, 33, 70, 12, ids=kind)
    for t_col, dup_col in ((31, 32), (32, 31), (127, 128), (128, 127)):
        cs[f"dup_{t_col}_{dup_col}"] = functools.partial(duplicate_case, 200, t_col, dup_col)
    cs["zero_g"] = zero_g_case
    for ns in SPLITS:
        cs[f"splits{ns}"] = functools.partial(random_case, 600, 65, 513, 40, n_splits=ns)
        for as_t in (True, False):
            for col in edge_columns(300, ns):
                cs[f"dom_{ns}_{int(as_t)}_{col}"] = functools.partial(
                    dominant_case, 3, 300, 8, col, as_t, n_splits=ns)
    return cs


# name → builder; every case is finite. CASES is the pool rho32 is taken over: logits of a few
# units (and the dominant column 40 above them). MAG_CASES hold logits of 1e4, which carry a
# rounding of 1e4 · 2^-24 = 6e-4 before the softmax sees them and gradient rows whose terms of
# size g · 100 cancel: pooled with the others they would set a tolerance of order 1 on every
# gradient, so they are held to 4 × their own pooled figure (rho32(mag=True)) instead, and the
# regular cases to the much smaller one of their own pool.
CASES = _build_cases()
MAG_CASES = {f"mag_{sign}_{it}": functools.partial(magnitude_case, sign, it)
             for sign in (1, -1) for it in (1.0, 20.0)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, float64 reference, the float32 control's ratios) of a case: computed once, shared
    and read only."""
    c = (CASES[name] if name in CASES else MAG_CASES[name])()
    r64 = evaluate(c, np.float64)
    ctl = ratios(evaluate(c, np.float32), r64)
    for a in list(c.values()) + list(r64.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, r64, ctl


@functools.lru_cache(maxsize=None)
def rho32(mag=False):
    """{output: the float32 control's worst error pooled over CASES (mag: over MAG_CASES)}."""
    return {n: max(case(name)[2][n] for name in (MAG_CASES if mag else CASES)) for n in OUT}
