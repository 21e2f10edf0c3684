"""Shared by tests/test_pinsage_infer_{cpu,gpu}.py: the inputs of the layer-wise PinSage
inference tests, a float64 NumPy restatement of one layer (pinsage/inference/inference.py:8-41 in
the trained model's [nv, h] order) and of the head, the magnitude bounds the tolerances are
built from, and a float32 NumPy form of the kernel's arithmetic. No GPU, no torch.

Tolerances (the project's fp32 standard, 1e-5 of a magnitude bound, as oracle/check_dlrm.py):
  before the norm   |err| <= 1e-5 · M, M = Σ|x||w| + |b| of the fc_2 pre-activation, where the
                    nv columns of |x| are Σ_j (cnt_j / Σcnt) |u[nbr_j]| — the weights are convex,
                    so this also bounds every partial sum of the weighted mean. relu is
                    1-Lipschitz: the same bound after it.
  after the row norm  1e-5 · ‖M_row‖₂ / ‖z_row‖₂ per element; rows whose float64 ‖z‖ is below
                    1e-3 · ‖M_row‖ are checked for finiteness only (at most 1 % of a case).
  after the Frobenius norm  1e-5 · M / ‖z‖_F (the bound before the norm over the float64 norm).
"""
from __future__ import annotations

import numpy as np

from recommender_amd import _lib as L

T = L.RS_PINSAGE_INFER_TILE
RTOL = 1e-5
SMALL_ROW = 1e-3      # ‖z‖ < SMALL_ROW · ‖M_row‖: finiteness only
MAX_EXCLUDED = 0.01

N_ITEMS = (1, T - 1, T, T + 1, 4 * T + 1)
SHAPES = ((24, 32, 16), (16, 32, 16), (1, 1, 1), (5, 3, 7), (192, 64, 64))
KS = (1, 3, 10, 32)
NORMS = (None, "row", "frobenius")


def valid_slots(nbr, cnt, n_items):
    """Slots that carry an edge (id inside [0, n_items), count != 0) and the out-of-range ones
    (any id but -1 outside the range)."""
    inside = (nbr >= 0) & (nbr < n_items)
    return inside & (cnt != 0), (nbr != -1) & ~inside


def make_case(n, d_in, hidden, d_out, k, seed=0):
    """One layer's inputs (float32 / int32 NumPy). Neighbour rows cycle through the patterns the
    kernel must get right (row i takes pattern i % 10, as far as n and k allow):
      0 full            1 first slot empty    2 last slot empty   3 an inside slot empty
      4 entirely empty  5 self as neighbour   6 one id twice      7 a count of 512
      8 a valid id with count 0               9 ids 0 and n - 1
    The bias is positive and larger for narrow outputs, so that under relu few rows are all zero."""
    rng = np.random.default_rng([seed, n, d_in, hidden, d_out, k])
    K = hidden + d_in
    h = rng.uniform(-1, 1, (n, d_in)).astype(np.float32)
    u = np.maximum(rng.normal(0, 1, (n, hidden)), 0).astype(np.float32)  # fc_1 ends in relu
    u[rng.random((n, hidden)) < 0.1] *= -1  # and the Spark demo's fc does not
    w2 = (rng.uniform(-1, 1, (K, d_out)) / np.sqrt(K)).astype(np.float32)
    lo = 1.5 if d_out < 5 else 0.2
    b2 = rng.uniform(lo, lo + 1.0, d_out).astype(np.float32)
    nbr = rng.integers(0, n, (n, k)).astype(np.int32)
    cnt = rng.integers(1, 17, (n, k)).astype(np.int32)
    for i in range(n):
        p = i % 10
        if p == 1:
            nbr[i, 0], cnt[i, 0] = -1, 0
        elif p == 2:
            nbr[i, k - 1], cnt[i, k - 1] = -1, 0
        elif p == 3 and k >= 3:
            nbr[i, k // 2], cnt[i, k // 2] = -1, 0
        elif p == 4:
            nbr[i], cnt[i] = -1, 0
        elif p == 5:
            nbr[i, 0] = i
        elif p == 6 and k >= 2:
            nbr[i, 1] = nbr[i, 0]
        elif p == 7:
            cnt[i, k - 1] = 512  # 64 walks x 8 traversals on one item
        elif p == 8:
            cnt[i, 0] = 0
        elif p == 9:
            nbr[i, 0] = 0
            nbr[i, k - 1] = n - 1
    return dict(h=h, u=u, nbr=nbr, cnt=cnt, w2=w2, b2=b2, n=n, d_in=d_in, hidden=hidden,
                d_out=d_out, k=k)


def negative_row_case(seed=1):
    """4T + 1 items at the default sizes whose row 7 has every fc_2 pre-activation negative
    whatever its neighbours are: w2 <= 0 everywhere, u >= 0 (so nv·w2 <= 0), h[7] = +1 and a
    bias of 0.01 far below Σ|w2| over the h rows. Every other row has h <= 0 and a small u, so
    its pre-activations are positive."""
    c = make_case(4 * T + 1, 24, 32, 16, 3, seed)
    c["u"] = (np.abs(c["u"]) * 0.05).astype(np.float32)
    c["w2"] = -np.abs(c["w2"])
    c["b2"] = np.full_like(c["b2"], 0.01)
    c["h"] = -np.abs(c["h"])
    c["h"][7] = 1.0
    c["neg_row"] = 7
    return c


def weighted_mean64(u, nbr, cnt, n_items=None):
    """(nv, |nv| bound) float64: nv = Σ cnt u[nbr] / max(Σ cnt, 1) over the valid slots, and the
    same combination of |u|."""
    n, k = nbr.shape
    n_items = u.shape[0] if n_items is None else n_items
    ok, _ = valid_slots(nbr, cnt, n_items)
    u64 = u.astype(np.float64)
    w = np.where(ok, cnt, 0).astype(np.float64)
    ids = np.where(ok, nbr, 0)
    rows = u64[ids]                                   # [n, k, H]
    den = np.maximum(w.sum(1), 1.0)[:, None]
    nv = (w[:, :, None] * rows).sum(1) / den
    nv_abs = (np.abs(w)[:, :, None] * np.abs(rows)).sum(1) / den
    return nv, nv_abs


def layer_ref(h, u, nbr, cnt, w2, b2, relu, norm, u_bound=None):
    """float64 layer. Returns dict: pre (fc_2 pre-activation), z (after the optional relu),
    out (after `norm`), M (the magnitude bound of pre, elementwise), tol (elementwise tolerance
    of out) and check (rows compared by value; the others only for finiteness). u_bound: the
    magnitude bound of u's own elements when the code under test computes u itself in fp32 (fc_1);
    its weighted mean through |w2| is added to M."""
    nv, nv_abs = weighted_mean64(u, nbr, cnt, h.shape[0])
    h64, w64, b64 = h.astype(np.float64), w2.astype(np.float64), b2.astype(np.float64)
    pre = np.concatenate([nv, h64], 1) @ w64 + b64
    M = np.concatenate([nv_abs, np.abs(h64)], 1) @ np.abs(w64) + np.abs(b64)
    if u_bound is not None:
        M = M + weighted_mean64(u_bound, nbr, cnt, h.shape[0])[1] @ np.abs(w64[:u.shape[1]])
    z = np.maximum(pre, 0.0) if relu else pre
    check = np.ones(h.shape[0], bool)
    if norm == "row":
        zn = np.sqrt((z * z).sum(1))
        Mn = np.sqrt((M * M).sum(1))
        check = zn >= SMALL_ROW * Mn
        safe = np.where(zn > 0, zn, 1.0)
        out = np.where(zn[:, None] > 0, z / safe[:, None], 0.0)
        tol = np.broadcast_to((RTOL * Mn / safe)[:, None], z.shape)
    elif norm == "frobenius":
        F = np.sqrt((z * z).sum())
        out, tol = z / F, RTOL * M / F
    else:
        out, tol = z, RTOL * M
    return dict(pre=pre, z=z, out=out, M=M, tol=tol, check=check)


def layer_f32(h, u, nbr, cnt, w2, b2, relu, norm):
    """The kernel's arithmetic in float32 NumPy: the mean summed slot by slot (product rounded,
    then added), fc_2 accumulated row by row of w2 from the bias (product rounded, then added —
    one rounding more per step than the kernel's fmaf), the norms in float32."""
    f = np.float32
    n, k = nbr.shape
    ok, _ = valid_slots(nbr, cnt, n)
    acc = np.zeros((n, u.shape[1]), f)
    ws = np.zeros(n, f)
    for j in range(k):
        w = np.where(ok[:, j], cnt[:, j], 0).astype(f)
        acc = acc + w[:, None] * u[np.where(ok[:, j], nbr[:, j], 0)]
        ws = ws + w
    nv = acc / np.maximum(ws, f(1))[:, None]
    x = np.concatenate([nv, h], 1).astype(f)
    z = np.broadcast_to(b2.astype(f), (n, w2.shape[1])).copy()
    for kk in range(x.shape[1]):
        z = z + x[:, kk:kk + 1] * w2[kk].astype(f)
    if relu:
        z = np.maximum(z, f(0))
    if norm == "row":
        nrm = np.sqrt((z * z).sum(1, dtype=f))
        return np.where(nrm[:, None] > 0, z / np.where(nrm > 0, nrm, f(1))[:, None], f(0)).astype(f)
    if norm == "frobenius":
        return (z / np.sqrt((z * z).sum(dtype=f))).astype(f)
    return z


def assert_layer_close(got, ref, msg=""):
    """got (float array) against layer_ref's dict: finite everywhere, |err| <= tol on the
    checked rows, at most MAX_EXCLUDED of the rows unchecked. Returns max err / tol."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref["out"].shape, f"{msg}: shape {got.shape} != {ref['out'].shape}"
    assert np.isfinite(got).all(), f"{msg}: non-finite output"
    chk = ref["check"]
    n = chk.size
    assert (~chk).sum() <= max(MAX_EXCLUDED * n, 0), \
        f"{msg}: {(~chk).sum()} of {n} rows below the small-norm threshold (> 1 %)"
    err = np.abs(got - ref["out"])[chk]
    tol = np.asarray(ref["tol"])[chk]
    ratio = float((err / tol).max()) if err.size else 0.0
    assert ratio <= 1.0, f"{msg}: max err / tol = {ratio:.3g}"
    return ratio


def dense64(x, W, b, relu):
    """(y, M) float64: y = act(x·W + b), M = |x|·|W| + |b|."""
    x, W, b = (np.asarray(a, np.float64) for a in (x, W, b))
    y = x @ W + b
    return (np.maximum(y, 0) if relu else y), np.abs(x) @ np.abs(W) + np.abs(b)


def chain_ref(feats, nbr, cnt, convs, head, norm="row"):
    """The whole chain in float64 from the features: convs = [(W1, b1, W2, b2), ...] (relu on
    both), head = (W1, b1, W2, b2) (relu, then linear). Returns the list of stages."""
    h = np.asarray(feats, np.float64)
    stages = [h]
    for W1, b1, W2, b2 in convs:
        u, _ = dense64(h, W1, b1, True)
        h = layer_ref(h, u, nbr, cnt, np.asarray(W2, np.float64), np.asarray(b2, np.float64),
                      True, norm)["out"]
        stages.append(h)
    a, _ = dense64(h, head[0], head[1], True)
    stages.append(dense64(a, head[2], head[3], False)[0])
    return stages


def spark_convolve_loop(features, neighbors, w1, b1, w2_hn, b2):
    """inference.py:8-41 written out row by row on Python lists (float64): fc on the neighbour
    features, join on `neighbor`, multiply by the weight, group by item and sum, divide by the
    summed weight, join the item's own feature, append the pooled columns ([h, nv] order), fc,
    l2norm. features: {item: list}; neighbors: [(item, neighbor, weight)]; w2_hn has rows
    [h ; nv]. Returns {item: list} for the items the inner joins keep."""
    hidden = len(b1)
    nf = {it: (np.dot(np.array(f), w1) + b1).tolist() for it, f in features.items()}   # fc
    joined = [(it, w, nf[nb]) for it, nb, w in neighbors if nb in nf]                  # join
    sums = {}
    for it, w, f in joined:                                                            # x weight
        s = sums.setdefault(it, [0.0] * hidden + [0.0])
        for i in range(hidden):
            s[i] += f[i] * w
        s[hidden] += w                                                                 # sum(weight)
    out = {}
    for it, s in sums.items():
        if it not in features:
            continue
        pooled = [s[i] / s[hidden] for i in range(hidden)]                             # divide
        feat = list(features[it])
        for i in range(hidden):                                                        # concat
            feat.append(pooled[i])
        y = np.dot(np.array(feat), w2_hn) + b2                                         # fc
        out[it] = (y / np.linalg.norm(y)).tolist()                                     # l2norm
    return out


def hand_graph_edges(seed=3, n_users=40, n_items=57, n_edges=300, dead_items=5, dead_users=4):
    """A small bipartite rating graph with dead ends on both sides and a few hot items:
    (users, items) unique edges."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users - dead_users, n_edges)
    i = rng.integers(0, n_items - dead_items, n_edges)
    hot = rng.random(n_edges) < 0.5
    i[hot] = rng.integers(0, 8, int(hot.sum()))
    key = np.unique(u * n_items + i)
    return key // n_items, key % n_items, n_users, n_items
