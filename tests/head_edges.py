"""Deterministic inputs and float64 / NumPy restatements for the MLP-head edge tests: the
activation-backward column sums of csrc/dense.hip, csrc/batchnorm.hip, csrc/loss.hip (BCE) and
csrc/metrics.hip (AUC). tests/test_head_edges_cpu.py proves each input has the property its name
claims and that the stated bounds hold for a plain fp32 reference; tests/test_head_edges_gpu.py
runs the inputs through the kernels. NumPy only at import (torch is imported where the eager
BatchNormalization fallback is sampled); nothing here calls a kernel.
"""
from __future__ import annotations

import functools
import math

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32

# =============================================================================================
# 1. activation backward + column sums (rs_act_bwd_colsum, _ld, _groups)
COL_ROWS = 512  # kColRows of csrc/dense.hip: rows per chunk

COLSUM_N = (1, 3, 4, 15, 16, 17, 60, 63, 64, 65, 68, 132)
# B = 2048 is the one row count with exactly four chunks (the last wave of fold_chunks_kernel's
# four-wave fold gets one chunk, none a second)
COLSUM_B = (1, 15, 16, 17, 511, 512, 513, 1025, 2048, 2049, 4608)


def n_chunks(B):
    return -(-B // COL_ROWS)


def _colsum_cases():
    """(N, B, act): every N with 511 or 512 rows (one chunk, ragged or full) and 513 (two, the
    second of one row), plus three of the other row counts in rotation, the act rotating with
    them: 60 cases, every N under every act, every chunk count of {1, 2, 3, 4, 5, 9} under the
    vector and the scalar kernel."""
    others = (1, 1025, 15, 2048, 16, 2049, 17, 4608)
    cases = []
    for i, N in enumerate(COLSUM_N):
        bs = [(511, 512)[i % 2], 513] + [others[(3 * i + j) % len(others)] for j in range(3)]
        for j, B in enumerate(bs):
            cases.append((N, B, (i + j) % 3))
    return tuple(cases)


COLSUM_CASES = _colsum_cases()

ESMM_BLOCKS = ((8, 12), (6, 10), (8, 11))  # column blocks of one [B, ΣN] buffer
# (n_groups, chunks per group)
GROUP_SHAPES = ((1, 1), (3, 1), (2, 3), (4, 5), (8, 1))
GROUP_N = (4, 17, 64, 100)


def colsum_inputs(N, B, act, seed=0):
    """dy Gaussian [B, N]; y a real activation output of Gaussian logits (None for act 0):
    relu's zeros are exact +0.0, and for relu every flat element 7k + 3 holds -0.0 and 5k + 1
    holds +0.0 whatever its logit was; with B >= 4, row 1 is all +0.0 and row 2 all -0.0."""
    rng = np.random.default_rng([N, B, act, seed])
    dy = rng.standard_normal((B, N)).astype(np.float32)
    if act == 0:
        return dy, None
    z = rng.standard_normal((B, N))
    if act == 1:
        y = np.maximum(z, 0.0).astype(np.float32)
        f = y.reshape(-1)
        f[1::5] = 0.0
        f[3::7] = -0.0
        if B >= 4:
            y[1] = 0.0
            y[2] = -0.0
    else:
        y = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    return dy, y


def act_bwd_f64(dy, y, act):
    """dz = act'(y)·dy in float64 on the fp32 inputs."""
    g = dy.astype(np.float64)
    if act == 1:
        return np.where(y > 0, g, 0.0)
    if act == 2:
        y64 = y.astype(np.float64)
        return g * y64 * (1.0 - y64)
    return g


# dz for sigmoid is dy·(y·(1-y)) in fp32: three roundings (1-y, the product, the product with
# dy), each within 2^-24 relative; 4·2^-24 covers their compounding
SIGMOID_RTOL = 4 * U32


def colsum_depth(nchunks):
    """The longest chain of fp32 additions that one column's db goes through, read from
    csrc/dense.hip: a thread of act_bwd_colsum_kernel adds the rows r0 + rl, r0 + rl + 16, ... of
    its 512-row chunk into acc: ceil(512 / 16) = 32 additions; the block then adds its 16 row
    lanes in order: 16; wave w of fold_chunks_kernel adds the chunks w, w + 4, ...:
    ceil(nchunks / 4); the four wave sums are added in order: 3."""
    return math.ceil(COL_ROWS / 16) + 16 + math.ceil(nchunks / 4) + 3


def colsum_db_bound(dz, nchunks):
    """|db - Σ_b dz| per column: each addition of a chain of `depth` rounds within 2^-24 of a
    partial sum that never exceeds Σ_b |dz| (first-order summation bound)."""
    return colsum_depth(nchunks) * U32 * np.abs(dz.astype(np.float64)).sum(0)


def takes_v4(N, act, dy_off=0, y_off=0, dz_off=0, ld_dy=None, ld_y=None, ld_dz=None):
    """The `v4` predicate of rs_act_bwd_colsum_ld restated: the float4 kernel runs when N is a
    multiple of 4 and every buffer the activation reads or writes starts on 16 bytes with a row
    stride that is a multiple of 4 floats. *_off: the start's offset in floats from a 16-byte
    aligned address; ld None = N."""
    def al16(off, ld):
        return (off * 4) % 16 == 0 and (N if ld is None else ld) % 4 == 0
    return N % 4 == 0 and al16(dy_off, ld_dy) and (act == 0 or (al16(y_off, ld_y) and al16(dz_off, ld_dz)))


def misaligned_lds(N):
    """(ld_dy, ld_y, ld_dz) with ld % 4 != 0 for at least dy: the scalar kernel whatever N."""
    return (N + 1 if N % 4 == 0 else N + 4 - N % 4 + 1, N + 2, N + 3)


def vector_lds(N):
    """Three different strides >= N, each a multiple of 4 (the vector kernel when N % 4 == 0)."""
    base = N + (-N) % 4
    return (base + 4, base + 8, base + 12)


# =============================================================================================
# 2. batch norm
BN_ROWS = 64  # kBnRows of csrc/batchnorm.hip
BN_C = (1, 63, 64, 65, 129)
BN_B = (2, 3, 5, 63, 64, 65, 129, 257)
BN_CASES = tuple((C, B) for C in BN_C for B in BN_B)
BN_EPS = 1e-3
COL_CONST, COL_BIG = 1, 2  # the structured columns (C >= 4); the step column is the last one
BIG_OFFSET, BIG_SCALE = 1000.0, 0.01


def bn_inputs(C, B):
    """x [B, C] ~ 3·N(0,1) + 1 with, for C >= 4, column 1 constant (2.5), column 2 =
    1000 + 0.01·N(0,1), and the last column a step: 1 on rows < 64, 5 on rows 64..127, -3 from
    row 128 on (constant inside every 64-row chunk: all its variance is between chunks).
    gamma in ±[0.5, 1.5] (every third negative), beta, dy, and moving statistics ~ N / U + 0.5."""
    rng = np.random.default_rng([C, B, 7])
    x = (3.0 * rng.standard_normal((B, C)) + 1.0).astype(np.float32)
    if C >= 4:
        x[:, COL_CONST] = 2.5
        x[:, COL_BIG] = (BIG_OFFSET + BIG_SCALE * rng.standard_normal(B)).astype(np.float32)
        r = np.arange(B)
        x[:, C - 1] = np.where(r < 64, 1.0, np.where(r < 128, 5.0, -3.0)).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    gamma[2::3] *= -1.0
    return dict(x=x, gamma=gamma, beta=rng.standard_normal(C).astype(np.float32),
                dy=rng.standard_normal((B, C)).astype(np.float32),
                mm=rng.standard_normal(C).astype(np.float32),
                mv=(rng.random(C) + 0.5).astype(np.float32))


def bn_fwd_f64(x, gamma, beta, mm, mv, momentum, training, eps=BN_EPS):
    """Keras BatchNormalization in float64 on the fp32 inputs; eps and momentum as the floats the
    kernel receives. → dict(y, mean, var, invstd, mm, mv)."""
    x64 = x.astype(np.float64)
    eps = float(np.float32(eps))
    decay = float(np.float32(1.0) - np.float32(momentum))
    mm, mv = mm.astype(np.float64), mv.astype(np.float64)
    if training:
        mean, var = x64.mean(0), x64.var(0)
        mm_new, mv_new = mm - (mm - mean) * decay, mv - (mv - var) * decay
    else:
        mean, var, mm_new, mv_new = mm, mv, mm, mv
    r = 1.0 / np.sqrt(var + eps)
    y = (x64 - mean) * r * gamma.astype(np.float64) + beta.astype(np.float64)
    return dict(y=y, mean=mean, var=var, invstd=r, mm=mm_new, mv=mv_new)


def bn_bwd(dy, x, mean, invstd, gamma, training, dtype=np.float64, perm=None):
    """rs_batch_norm_bwd's function of its own inputs (the saved mean and invstd are arguments of
    the kernel): dβ = Σ dy, dγ = Σ dy·x̂, dx = γ·r·(dy - dβ/B - x̂·dγ/B), inference dx = γ·r·dy.
    dtype float32 with a row permutation gives an fp32 sample in another summation order."""
    t = dtype
    dy, x = dy.astype(t), x.astype(t)
    m, r, g = mean.astype(t), invstd.astype(t), gamma.astype(t)
    B = x.shape[0]
    p = np.arange(B) if perm is None else perm
    xh = (x - m) * r
    dbeta = dy[p].sum(0, dtype=t)
    dgamma = (dy[p] * xh[p]).sum(0, dtype=t)
    if training:
        dx = (g * r) * ((dy - dbeta / t(B)) - xh * (dgamma / t(B)))
    else:
        dx = (g * r) * dy
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def bn_eager_samples(d, momentum, training, eps=BN_EPS):
    """Two fp32 samples of the forward: the eager fallback of BatchNormalization.forward on the
    CPU, on the input and on a row permutation of it (two summation orders).
    → [dict(y, mean, var, invstd, mm, mv)] with y in the input's row order."""
    import torch

    from recommender_amd.dien.layers import BatchNormalization

    B, C = d["x"].shape
    out = []
    for perm in (np.arange(B), np.random.default_rng(B).permutation(B)):
        bn = BatchNormalization(C, momentum=momentum, epsilon=eps, device="cpu")
        with torch.no_grad():
            bn.gamma.copy_(torch.from_numpy(d["gamma"]))
            bn.beta.copy_(torch.from_numpy(d["beta"]))
            bn.moving_mean.copy_(torch.from_numpy(d["mm"]))
            bn.moving_variance.copy_(torch.from_numpy(d["mv"]))
            x = torch.from_numpy(d["x"][perm].copy())
            y = bn(x, training=training).numpy()
            if training:
                mean, var = x.mean(0).numpy(), x.var(0, unbiased=False).numpy()
            else:
                mean, var = d["mm"], d["mv"]
        inv = np.empty_like(y)
        inv[perm] = y
        out.append(dict(y=inv, mean=mean, var=var,
                        invstd=(1.0 / np.sqrt(var + np.float32(eps))).astype(np.float32),
                        mm=bn.moving_mean.numpy().copy(), mv=bn.moving_variance.numpy().copy()))
    return out


def ulp32(v):
    """Spacing of float32 at |v| (v float64)."""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def var_one_pass_f32(x):
    """E[x²] - E[x]² in float32: what the batch-norm kernel must not compute."""
    n = np.float32(x.shape[0])
    s = x.sum(0, dtype=np.float32) / n
    return (x * x).sum(0, dtype=np.float32) / n - s * s


def var_two_pass_f32(x):
    m = x.sum(0, dtype=np.float32) / np.float32(x.shape[0])
    d = x - m
    return (d * d).sum(0, dtype=np.float32) / np.float32(x.shape[0])


# =============================================================================================
# 3. BCE
BCE_EPS = np.float32(1e-7)
BCE_HI = np.float32(1.0) - BCE_EPS  # 1 - eps in float32: 0.99999988
BCE_N = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2 ** 20, 2 ** 20 + 1, 2 ** 21 + 5)
BCE_THREADS, BCE_FWD_CAP, BCE_BWD_CAP = 256, 1024, 2048
BCE_ABS = 2.0 ** -22  # log of an argument rounded near 1
BCE_RTOL = 1e-5       # the project's rule


def bce_planted():
    """The predictions at the clip's edges and outside it, float32."""
    e, h = BCE_EPS, BCE_HI
    return np.array([0.0, 1.0, e, np.nextafter(e, np.float32(0)), h, np.nextafter(h, np.float32(2)),
                     0.5, -0.25, 1.5], np.float32)


def bce_inputs(n, soft):
    """p uniform in (0, 1) with bce_planted() spread over it (as many as fit), labels hard
    (0 / 1) or soft (0.3 at every third element, else uniform), grad_out Gaussian.
    → p, y, g, the planted positions."""
    rng = np.random.default_rng([n, int(soft), 3])
    p = rng.random(n, dtype=np.float32)
    pl = bce_planted()
    pos = (np.arange(len(pl)) * max(1, n // len(pl)))[: n] if n else np.zeros(0, np.int64)
    pos = pos[pos < n]
    p[pos] = pl[: len(pos)]
    if soft:
        y = rng.random(n, dtype=np.float32)
        y[::3] = 0.3
    else:
        y = (rng.random(n) < 0.4).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    return p, y, g, pos


def bce_f64(p, y):
    """oracle.ctr.bce in float64 with the kernel's float32 eps and clip bounds."""
    e = float(BCE_EPS)
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    pc = np.clip(p64, e, float(BCE_HI))
    with np.errstate(invalid="ignore"):
        return -(y64 * np.log(pc + e) + (1 - y64) * np.log(1 - pc + e))


def bce_grad_f64(p, y):
    """d l_i / d p_i (oracle.ctr.bce_grad without its 1/n) and the size of its two terms, which
    cancel for soft labels: → (gradient, |y/(pc+eps)| + |(1-y)/(1-pc+eps)|)."""
    e = float(BCE_EPS)
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    pc = np.clip(p64, e, float(BCE_HI))
    inside = (p64 >= e) & (p64 <= float(BCE_HI))
    a, b = y64 / (pc + e), (1 - y64) / (1 - pc + e)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(p64), np.nan, (b - a) * inside)
    return d, np.abs(a) + np.abs(b)


def bce_fwd_blocks(n):
    return min(-(-n // (BCE_THREADS * 4)), BCE_FWD_CAP)


def bce_bwd_blocks(n):
    return min(-(-n // (BCE_THREADS * 4)), BCE_BWD_CAP)


def bce_passes(n, blocks):
    """Grid-stride passes of one thread."""
    return -(-n // (blocks * BCE_THREADS))


def bce_sum_depth(n):
    """Additions on the longest chain of a reduced loss (csrc/loss.hip): a thread's passes, the
    8 levels of the block's tree, and bce_fold_kernel's walk over the block partials."""
    nb = bce_fwd_blocks(n)
    return bce_passes(n, nb) + 8 + nb


def bce_elem_tol(l64):
    return BCE_RTOL * np.abs(l64) + BCE_ABS


def bce_sum_tol(l64):
    """The per-element bound applied to the sum, plus the summation's own rounding."""
    n = l64.size
    return (BCE_RTOL * abs(l64.sum()) + BCE_ABS + bce_sum_depth(n) * U32 * np.abs(l64).sum())


# =============================================================================================
# 4. AUC
AUC_T = (2, 3, 200, 20000)
AUC_LABELS = np.array([0.0, 1.0, 0.5, -1.0, 2.0], np.float32)


def keras_thresholds(T):
    """keras.metrics.AUC.__init__, restated (recommender_amd.metrics.keras_thresholds is compared
    with it on the CPU)."""
    eps = 1e-7
    return np.array([0.0 - eps] + [(i + 1) * 1.0 / (T - 1) for i in range(T - 2)] + [1.0 + eps],
                    np.float32)


def auc_inputs(T):
    """Every interior float32 threshold, its two float32 neighbours, 0, -0.0 and 1; the labels
    cycle through {0, 1, 0.5, -1, 2}."""
    t = keras_thresholds(T)[1:-1]
    p = np.concatenate([t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2)),
                        np.array([0.0, -0.0, 1.0], np.float32)]).astype(np.float32)
    order = np.random.default_rng(T).permutation(p.size)  # no block of the grid sees one kind
    p = p[order]
    y = AUC_LABELS[np.arange(p.size) % AUC_LABELS.size]
    return p, y


def literal_tp_fp(p, y, thr, chunk=4096):
    """TP_i = Σ [y != 0][p > t_i], FP_i = Σ [y == 0][p > t_i] from the literal comparison matrix
    (oracle.metrics.keras_auc's, built over chunks of predictions so that T = 20000 fits)."""
    tp = np.zeros(thr.size, np.int64)
    fp = np.zeros(thr.size, np.int64)
    pos = y != 0
    for acc, q in ((tp, p[pos]), (fp, p[~pos])):
        for a in range(0, q.size, chunk):
            acc += np.count_nonzero(q[None, a:a + chunk] > thr[:, None], axis=1)
    return tp, fp


def buckets_from_cumulative(above, total):
    """Per-bucket counts [T + 1] from above_i = #{p > t_i} (bucket b = #{i : t_i < p}):
    bucket 0 = total - above_0, bucket b = above_{b-1} - above_b, bucket T = above_{T-1}."""
    a = np.asarray(above, np.int64)
    return np.concatenate([[total - a[0]], a[:-1] - a[1:], [a[-1]]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def auc_reference(T):
    """(p, y, neg buckets, pos buckets, ROC AUC) of auc_inputs(T), computed once."""
    p, y = auc_inputs(T)
    thr = keras_thresholds(T)
    tp, fp = literal_tp_fp(p, y, thr)
    npos = int((y != 0).sum())
    pos_b = buckets_from_cumulative(tp, npos)
    neg_b = buckets_from_cumulative(fp, p.size - npos)
    return p, y, neg_b, pos_b, roc_from_tp_fp(tp, fp, npos, p.size - npos)


def roc_from_tp_fp(tp, fp, npos, nneg):
    """The tail of oracle.metrics.keras_auc: trapezoid ROC from the cumulative counts."""
    tp, fp = tp.astype(np.float64), fp.astype(np.float64)
    fn, tn = npos - tp, nneg - fp
    recall = np.divide(tp, tp + fn, out=np.zeros_like(tp), where=(tp + fn) != 0)
    fpr = np.divide(fp, fp + tn, out=np.zeros_like(fp), where=(fp + tn) != 0)
    return float(np.sum((fpr[:-1] - fpr[1:]) * (recall[:-1] + recall[1:]) / 2.0))


def tie_heavy(T=200, n=3000):
    """Predictions drawn from 12 values only, half of them thresholds: long runs of ties."""
    rng = np.random.default_rng(T + n)
    t = keras_thresholds(T)
    vals = np.concatenate([t[[1, T // 4, T // 2, T - 2]], np.array([0, 1, .1, .25, .5, .75, .9, .33],
                                                                   np.float32)]).astype(np.float32)
    p = vals[rng.integers(0, vals.size, n)]
    y = (rng.random(n) < 0.2 + 0.6 * p).astype(np.float32)
    return p, y
