"""Deterministic inputs, float64 restatements and magnitude bounds for the edge tests of
csrc/pinsage.hip: the metapath walks and the PinSAGE neighbour selection on hub, tie and
walk-shape-limit graphs, the counter wrap of the pair sampler, the exclusion set at high load,
first-appearance unique and to_block at the scan's tile edges, the weighted mean pooling, the
Frobenius normalisation in its flat and rows forms, the pair margin loss and the multi-hot mean
lookup. tests/test_pinsage_edges_cpu.py proves each input has the property its name claims and
that a plain fp32 NumPy evaluation of each float reference meets its bound with room;
tests/test_pinsage_edges_gpu.py runs the inputs through the kernels. NumPy only; nothing here
calls a kernel.

Integer kernels are compared bit for bit with oracle/pinsage.py. Float kernels are compared with
float64 under the project's bound (tests/eges_edges.py): |got - ref64| <= 1e-5 · Σ|terms|, the
magnitude sum formed in float64 per element. No case here needs a number beyond it.

Largest fp32 error / bound ratio that tests/test_pinsage_edges_cpu.py observes per kernel family
(a plain fp32 NumPy evaluation against float64, bound = 1e-5 · Σ|terms|; the test requires <= 0.25):
  weighted mean pooling   fwd 0.018    bwd 0.0117   (one edge after the other)
  Frobenius, flat         norm 0.00414 y 0.0101     dx 0.0151   (the kernel's fixed partition; Σx²
                          of the 2 097 157 elements summed one after the other is at 64.8 of the
                          bound: frob_norm_seq32)
  pair margin             scores 0.03  loss 0.0821  dh 0.0292
  multi-hot mean          out 0.0459   dtable 0.0348
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import pinsage as O
from tests.eges_edges import RTOL, bits, f32, off_by, sum_seq32, sum_tree32, within  # noqa: F401

SEED = 0x1234_5678_9ABC  # the samplers' 64-bit seed (both words non-zero)
SCAN_TILE = 4096         # csrc/sort.hip exclusive_scan_i32
RED_THREADS, RED_CHUNK = 256, 4096  # csrc/pinsage.hip kRedThreads, kRedChunk
PAIR_THREADS, MH_ROWS = 256, 32     # kPairThreads, kMhRows
STEP_WRAP = 0xFFFFFFFF


# =============================================================================================
# graphs
def small_graph_edges(seed=0, n_users=60, n_items=90, n_edges=500, dead_items=7, dead_users=5):
    """The edges of tests/test_pinsage_gpu.py small_graph → (users, items, n_users, n_items)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users - dead_users, n_edges)
    i = rng.integers(0, n_items - dead_items, n_edges)
    hot = rng.random(n_edges) < 0.5
    i[hot] = rng.integers(0, 10, int(hot.sum()))
    key = np.unique(u * n_items + i)
    return key // n_items, key % n_items, n_users, n_items


HUB_DEG = 70_000
HUB_ORD = 300  # ordinary items / users 0 .. 299 (item 0 and user 0 are the hubs)
HUB_N = HUB_ORD + HUB_DEG + 50  # the last 50 items and users have no edge: dead ends


@functools.lru_cache(maxsize=None)
def hub_graph_edges():
    """Item 0 is linked to the 70 000 users 300 .. 70 299 (each of degree 1), user 0 to the 70 000
    items 300 .. 70 299 (each of degree 1); 10 000 random edges among items / users 0 .. 299 (the
    hubs included); items and users 70 300 .. 70 349 have no edge. About 150 000 edges."""
    rng = np.random.default_rng(11)
    leaf = np.arange(HUB_ORD, HUB_ORD + HUB_DEG)
    ou = rng.integers(0, HUB_ORD, 10_000)
    oi = rng.integers(0, HUB_ORD, 10_000)
    u = np.concatenate([leaf, np.zeros(HUB_DEG, np.int64), ou])
    i = np.concatenate([np.zeros(HUB_DEG, np.int64), leaf, oi])
    key = np.unique(u * HUB_N + i)
    return key // HUB_N, key % HUB_N, HUB_N, HUB_N


def hub_seeds():
    """The hub item, items whose only user is the hub user (first, last, middle), ordinary items,
    dead items."""
    return np.array([0, 300, 301, 35_000, 70_299, 70_298] + list(range(1, 25))
                    + [70_300, 70_349, 0, 300], np.int32)


HUB_WALK = (8, 2, 0.0)             # (num_walks, T, p) for rs_metapath_walk
HUB_NEIGHBORS = (64, 2, 0.0, 10)   # (num_walks, T, p, k) for rs_pinsage_neighbors


def adjacency_draws(og, traces):
    """The adjacency index each hop of `traces` [n, 2T+1] chose, where it is determined (the
    neighbour lists of these graphs hold distinct ids, sorted): → (item_hop_idx, user_hop_idx),
    flat arrays over the hops taken from an item / from a user."""
    out = ([], [])
    for h in range(traces.shape[1] - 1):
        a, b = traces[:, h], traces[:, h + 1]
        m = (a >= 0) & (b >= 0)
        ptr, nbr = (og.u2i_indptr, og.u2i) if h & 1 else (og.i2u_indptr, og.i2u)
        for x, y in zip(a[m].tolist(), b[m].tolist()):
            lo, hi = int(ptr[x]), int(ptr[x + 1])
            out[h & 1].append(int(np.searchsorted(nbr[lo:hi], y)))
    return np.asarray(out[0]), np.asarray(out[1])


TIE_USERS, TIE_ITEMS, TIE_PER_USER = 256, 1280, 40
TIE_WALK = (64, 1, 0.0)  # C = 64 visits over a two-hop neighbourhood of about 300 items
TIE_K = (1, 10, 64, 100)
TIE_SEEDS = 97           # not a multiple of the 4 seeds a block takes at 64 walks


@functools.lru_cache(maxsize=None)
def tie_graph_edges():
    """Each of 256 users links 40 distinct items of 1280: an item has about 8 users and a two-hop
    neighbourhood of about 300 items, so 64 one-traversal walks visit most candidates once."""
    rng = np.random.default_rng(12)
    u = np.repeat(np.arange(TIE_USERS), TIE_PER_USER)
    i = np.concatenate([rng.choice(TIE_ITEMS, TIE_PER_USER, replace=False)
                        for _ in range(TIE_USERS)])
    return u, i, TIE_USERS, TIE_ITEMS


def tie_seeds():
    return np.arange(0, TIE_SEEDS * 13, 13, dtype=np.int32)


# (num_walks, T, p, k): C = 512 visits and the full LDS; half of each 64-lane group idle at T 8;
# one lane short of the group; one walk a seed (256 seeds a block); every trace stopped after its
# first hop (p = 1 saturates the stop threshold to 0xFFFFFFFF)
WALK_LIMIT_CASES = ((64, 8, 0.0, 10), (33, 8, 0.25, 5), (63, 1, 0.0, 3), (1, 8, 1.0, 4),
                    (64, 8, 1.0, 3))
LIMIT_GRAPH = dict(seed=6, n_users=200, n_items=300, n_edges=3000)


def limit_seeds():
    """All 300 items with seven -1 padding seeds mixed in: 307 seeds, no multiple of 4 or 256."""
    s = np.arange(300, dtype=np.int32)
    return np.insert(s, [0, 3, 3, 130, 255, 299, 300], -1).astype(np.int32)


def graph_edges(name):
    """(users, items, n_users, n_items) of "hub", "tie", "limit" (the 200 x 300 small_graph) and
    "pairs" (the 60 x 90 one)."""
    return {"hub": hub_graph_edges, "tie": tie_graph_edges,
            "limit": lambda: small_graph_edges(**LIMIT_GRAPH),
            "pairs": lambda: small_graph_edges(2)}[name]()


@functools.lru_cache(maxsize=None)
def oracle_graph(name):
    return O.BipartiteGraph.from_edges(*graph_edges(name))


@functools.lru_cache(maxsize=None)
def oracle_neighbors(name, num_walks, T, p, k, step=5, layer=1):
    seeds = {"hub": hub_seeds, "tie": tie_seeds, "limit": limit_seeds}[name]()
    return O.pinsage_neighbors(oracle_graph(name), seeds, num_walks, T, p, k, SEED, step, layer)


# =============================================================================================
# counter wrap
WRAP_PAIR_BASE, WRAP_BATCH = 2 ** 32 - 5, 32  # pairs 5 .. 31 have counter words 0 .. 26
AT_STEPS = (0, 7, STEP_WRAP)


# =============================================================================================
# exclusion set at high load
EXCL_N, EXCL_CAP, EXCL_WIDE = 1000, 1024, 65_536
EXCL_WALK = (8, 2, 0.0, 5)  # (num_walks, T, p, k) on the "limit" graph, seed 3, step 0, layer 0
EXCL_SEED = 3
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def pair_key(dst, src):
    return (np.asarray(dst, np.int64).astype(np.uint32).astype(np.uint64) << np.uint64(32)) \
        | np.asarray(src, np.int64).astype(np.uint32).astype(np.uint64)


def slot_of(key, mask):
    """csrc/pinsage.hip slot_of: the high word of key · 0x9E3779B97F4A7C15 (mod 2^64), masked."""
    with np.errstate(over="ignore"):
        return ((np.asarray(key, np.uint64) * _GOLD) >> np.uint64(32)).astype(np.int64) & mask


@functools.lru_cache(maxsize=None)
def excl_case():
    """→ dict(src, dst [1000] int32: the pairs handed to rs_pair_set_build (half of the edges the
    unfiltered sampler emits, ten pairs whose home slot is one of the last three of 1024, random
    fillers, (-1, ·) and (·, -1) entries, duplicates), keys (the distinct keys of the live pairs),
    seeds, unfiltered (nbr, cnt), exclude (the oracle's set of (src, dst)))."""
    rng = np.random.default_rng(13)
    og = oracle_graph("limit")
    seeds = np.arange(og.n_items, dtype=np.int32)
    nw, T, p, k = EXCL_WALK
    rn, rc = O.pinsage_neighbors(og, seeds, nw, T, p, k, EXCL_SEED, 0, 0)
    s_idx, r_idx = np.nonzero(rn >= 0)
    pick = rng.random(s_idx.size) < 0.5
    src, dst = rn[s_idx[pick], r_idx[pick]], seeds[s_idx[pick]].astype(np.int64)
    emitted = set(zip(rn[s_idx, r_idx].tolist(), seeds[s_idx].tolist()))
    # every other (src, dst) of the id space, with its home slot
    a_src, a_dst = np.divmod(np.arange(og.n_items ** 2), og.n_items)
    free = np.array([(s, d) not in emitted for s, d in zip(a_src.tolist(), a_dst.tolist())])
    a_src, a_dst = a_src[free], a_dst[free]
    home = slot_of(pair_key(a_dst, a_src), EXCL_CAP - 1)
    last = np.flatnonzero(home >= EXCL_CAP - 3)[:10]
    rest = rng.permutation(np.flatnonzero(home < EXCL_CAP - 3))[:900 - 10 - src.size]
    fill = np.concatenate([last, rest])
    src, dst = np.concatenate([src, a_src[fill]]), np.concatenate([dst, a_dst[fill]])
    assert src.size == 900
    neg_s = np.concatenate([np.full(10, -1), rng.integers(0, 300, 10)])
    neg_d = np.concatenate([rng.integers(0, 300, 10), np.full(10, -1)])
    dup = rng.integers(0, 900, EXCL_N - 900 - 20)
    o = rng.permutation(EXCL_N)
    all_s = np.concatenate([src, neg_s, src[dup]])[o].astype(np.int32)
    all_d = np.concatenate([dst, neg_d, dst[dup]])[o].astype(np.int32)
    return dict(src=all_s, dst=all_d, keys=np.unique(pair_key(dst, src)), seeds=seeds,
                unfiltered=(rn, rc), exclude=set(zip(src.tolist(), dst.tolist())))


def probe_insert(src, dst, capacity):
    """rs_pair_set_build restated one pair after the other → (table [capacity] uint64, empty =
    2^64 - 1; probes [n]: slots looked at per pair, 0 for a skipped one). The set of occupied
    slots does not depend on the order of insertion."""
    mask = capacity - 1
    empty = np.uint64(2 ** 64 - 1)
    table = np.full(capacity, empty, np.uint64)
    probes = np.zeros(len(src), np.int64)
    for n, (s, d) in enumerate(zip(np.asarray(src).tolist(), np.asarray(dst).tolist())):
        if s < 0 or d < 0:
            continue
        key = pair_key(d, s)
        h = int(slot_of(key, mask))
        c = 1
        while table[h] != empty and table[h] != key:
            h = (h + 1) & mask
            c += 1
        table[h] = key
        probes[n] = c
    return table, probes


# =============================================================================================
# rs_unique_first
UNIQUE_NODES = 5000
UNIQUE_CASES = ("n4095", "n4096", "n4097", "n8193", "all_absent", "all_equal", "wide_ids", "empty")


def unique_inputs(name):
    """→ (ids int32, n_nodes). n*: random ids in [-1, 900) with ids that appear nowhere else at
    index n - 1 and (n > 4096) at index 4096."""
    rng = np.random.default_rng([UNIQUE_CASES.index(name), 14])
    if name.startswith("n"):
        n = int(name[1:])
        ids = rng.integers(-1, 900, n).astype(np.int32)
        ids[n - 1] = 4321
        if n > SCAN_TILE:
            ids[SCAN_TILE] = 4322
        return ids, UNIQUE_NODES
    if name == "all_absent":
        return np.full(SCAN_TILE + 1, -1, np.int32), UNIQUE_NODES
    if name == "all_equal":
        return np.full(SCAN_TILE + 1, 5, np.int32), UNIQUE_NODES
    if name == "wide_ids":
        pool = np.array([0, 1, 2, 2_999_997, 2_999_998, 2_999_999, -1, 1_500_000], np.int32)
        return pool[rng.integers(0, pool.size, 5000)], 3_000_000
    return np.zeros(0, np.int32), UNIQUE_NODES


# =============================================================================================
# rs_pinsage_block through to_block
BLOCK_NODES = 8000
# (n_dst, k, kind): capacities 4095 / 4096 / 4097 around the scan tile, k 1 and 32, every slot
# empty, every slot live, one source in every destination's list, no destination
BLOCK_CASES = ((1365, 3, "mixed"), (1024, 4, "mixed"), (241, 17, "mixed"), (4097, 1, "mixed"),
               (130, 32, "mixed"), (1024, 4, "empty"), (1024, 4, "full"), (1365, 3, "hub"),
               (0, 3, "mixed"))
BLOCK_HUB = BLOCK_NODES - 1


def block_inputs(n_dst, k, kind):
    """→ (dst [n_dst], nbr [n_dst, k], cnt [n_dst, k]) int32; counts 1 .. 512 on live slots."""
    rng = np.random.default_rng([n_dst, k, ("mixed", "empty", "full", "hub").index(kind), 15])
    dst = rng.choice(BLOCK_NODES - 1, n_dst, replace=False).astype(np.int32)
    nbr = rng.integers(0, BLOCK_NODES - 1, (n_dst, k)).astype(np.int32)
    if kind in ("mixed", "hub"):
        nbr[rng.random((n_dst, k)) < 0.35] = -1
    if kind == "empty":
        nbr[:] = -1
    if kind == "hub":
        nbr[:, 0] = BLOCK_HUB
    cnt = np.where(nbr >= 0, rng.integers(1, 513, (n_dst, k)), 0).astype(np.int32)
    live = np.flatnonzero(nbr.reshape(-1) >= 0)
    if live.size:
        cnt.reshape(-1)[live[0]] = 512
        cnt.reshape(-1)[live[-1]] = 1
    return dst, nbr, cnt


# =============================================================================================
# rs_weighted_mean_agg_fwd / _bwd
AGG_DST, AGG_K = 1200, 9
AGG_DST_DEGREES = (0, 1, 3, 4, 5, 7, 8, 9)          # destination i has degree [i % 8]
AGG_SRC_DEGREES = (7, 8, 9, 15, 16, 17)             # sources AGG_DST + 1 .. + 6
AGG_H = (1, 5, 64, 70)
AGG_NODES = 20_000


@functools.lru_cache(maxsize=None)
def agg_block_inputs():
    """→ (dst, nbr, cnt). Destinations are ids 0 .. 1199 (so their local ids too); source 1200 is
    in the list of every destination that has one (1050 in-edges: the hub), sources 1201 .. 1206
    are pooled by exactly 7, 8, 9, 15, 16, 17 destinations, every other live slot holds an id of
    its own (one in-edge); the live slots of a row sit at seeded positions among its nine."""
    rng = np.random.default_rng(16)
    deg = np.array(AGG_DST_DEGREES)[np.arange(AGG_DST) % 8]
    vals = np.full((AGG_DST, AGG_K), -1, np.int64)
    fresh = AGG_DST + 1 + len(AGG_SRC_DEGREES)
    forced = np.concatenate([np.full(c, AGG_DST + 1 + j) for j, c in enumerate(AGG_SRC_DEGREES)])
    rows3 = rng.permutation(np.flatnonzero(deg >= 3))[:forced.size]
    second = dict(zip(rows3.tolist(), forced.tolist()))
    for d in range(AGG_DST):
        if deg[d] == 0:
            continue
        row = [AGG_DST]
        if d in second:
            row.append(second[d])
        while len(row) < deg[d]:
            row.append(fresh)
            fresh += 1
        vals[d, np.sort(rng.permutation(AGG_K)[:deg[d]])] = row
    assert fresh <= AGG_NODES
    cnt = np.where(vals >= 0, rng.integers(1, 513, vals.shape), 0)
    cnt[1, np.flatnonzero(vals[1] >= 0)[0]] = 512
    return np.arange(AGG_DST, dtype=np.int32), vals.astype(np.int32), cnt.astype(np.int32)


@functools.lru_cache(maxsize=None)
def agg_block():
    return O.to_block(*agg_block_inputs())


def agg_values(H, n_src):
    rng = np.random.default_rng([H, 17])
    return (rng.standard_normal((n_src, H)).astype(np.float32),
            rng.standard_normal((AGG_DST, H)).astype(np.float32))


def agg_ref(u, g, b):
    """float64: nv = Σ_e w u[src] / max(Σ w, 1) per destination, gu = Σ_e w / max(ws, 1) · g[dst]
    per source, each with its Σ|terms|; wsum (sums of integers <= 9 · 512: exact in fp32)."""
    w = b.edge_w.astype(np.float64)
    ws = np.zeros(b.n_dst)
    np.add.at(ws, b.edge_dst, w)
    den = np.maximum(ws, 1.0)
    t = w[:, None] * u.astype(np.float64)[b.edge_src] / den[b.edge_dst, None]
    nv, nv_mag = np.zeros((b.n_dst, u.shape[1])), np.zeros((b.n_dst, u.shape[1]))
    np.add.at(nv, b.edge_dst, t)
    np.add.at(nv_mag, b.edge_dst, np.abs(t))
    t = (w / den[b.edge_dst])[:, None] * g.astype(np.float64)[b.edge_dst]
    gu, gu_mag = np.zeros((b.n_src, u.shape[1])), np.zeros((b.n_src, u.shape[1]))
    np.add.at(gu, b.edge_src, t)
    np.add.at(gu_mag, b.edge_src, np.abs(t))
    return dict(nv=nv, nv_mag=nv_mag, gu=gu, gu_mag=gu_mag, wsum=ws.astype(np.float32))


def agg_f32(u, g, b):
    """The two sums in fp32, one edge after the other in CSR order."""
    H = u.shape[1]
    acc, ws = np.zeros((b.n_dst, H), np.float32), np.zeros(b.n_dst, np.float32)
    deg = np.diff(b.indptr)
    for j in range(int(deg.max(initial=0))):
        d = np.flatnonzero(deg > j)
        e = b.indptr[d] + j
        acc[d] = acc[d] + b.edge_w[e, None] * u[b.edge_src[e]]
        ws[d] = ws[d] + b.edge_w[e]
    den = np.maximum(ws, np.float32(1))
    nv = acc / den[:, None]
    gu = np.zeros((b.n_src, H), np.float32)
    tdeg = np.diff(b.t_indptr)
    for j in range(int(tdeg.max(initial=0))):
        s = np.flatnonzero(tdeg > j)
        e = b.t_edge[b.t_indptr[s] + j]
        d = b.edge_dst[e]
        gu[s] = gu[s] + (b.edge_w[e] / den[d])[:, None] * g[d]
    return nv, gu


# =============================================================================================
# Frobenius normalisation
FROB_N = (1, 4095, 4096, 4097, 1_048_576, 1_048_577, 2_097_157)  # 256 chunks, 257, 513
FROB_ROWS = ((700, 16), (257, 64))  # [capacity rows, row length]
FROB_ROWS_LIVE = ("zero", "one", "capacity", "capacity+3")


def frob_inputs(n):
    rng = np.random.default_rng([n, 18])
    return np.abs(rng.standard_normal(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def frob_ref(x, dy):
    """float64: norm, y = x / norm, dx = (dy - y Σ dy·y) / norm and dx's bound
    1e-5 · (|dy| + |y| Σ|dy·y|) / norm."""
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    norm = np.sqrt(np.sum(x * x))
    y = x / norm
    dx = (dy - y * np.sum(dy * y)) / norm
    return dict(norm=norm, y=y, dx=dx, dx_bound=RTOL * (np.abs(dy) + np.abs(y) * np.sum(np.abs(dy * y))) / norm)


def partition_sum32(a, b=None):
    """Σ a·b (b None: Σ a²) in fp32 with the fixed partition of dot_partial_kernel /
    fold_partial_kernel: per chunk of 4096, thread t sums its 16 terms t, t + 256, ... one after
    the other, a 256-wide tree folds the threads; lane j then sums the chunks j, j + 256, ... one
    after the other and a last tree folds the lanes."""
    a = f32(a).reshape(-1)
    prod = a * a if b is None else a * f32(b).reshape(-1)
    nb = -(-prod.size // RED_CHUNK)
    p = np.zeros(nb * RED_CHUNK, np.float32)
    p[:prod.size] = prod
    partial = sum_tree32(sum_seq32(p.reshape(nb, RED_CHUNK // RED_THREADS, RED_THREADS), 1), 1)
    q = np.zeros(-(-nb // RED_THREADS) * RED_THREADS, np.float32)
    q[:nb] = partial
    return sum_tree32(sum_seq32(q.reshape(-1, RED_THREADS), 0), 0)


def frob_f32(x, dy):
    """norm, y, dx in fp32 with both reductions in the kernel's partition."""
    norm = np.sqrt(partition_sum32(x))
    y = (x / norm).astype(np.float32)
    dot = partition_sum32(dy, y)
    return norm, y, ((dy - y * dot) / norm).astype(np.float32)


def frob_norm_seq32(x):
    """sqrt of Σ x² summed in fp32 one element after the other (np.cumsum keeps the order): what
    the partition is there to avoid."""
    return np.sqrt(np.cumsum(f32(x) * f32(x), dtype=np.float32)[-1])


def frob_rows_live(cap, which):
    return {"zero": 0, "one": 1, "capacity": cap, "capacity+3": cap + 3}[which]


# =============================================================================================
# rs_pair_margin_fwd / _bwd
PAIR_ROWS = 40
PAIR_R1, PAIR_R2, PAIR_R2UP = 37, 38, 39  # rows (1, 0, ..), (2, 0, ..), (nextafter(2), 0, ..)
PAIR_DELTA = 1.0
# (D, P, ld - D, padding): D 1 and the limit 64, P at the 256-pair block edges, a padded leading
# dimension, padding pairs (-1 ids) with valid / n_live ("masked") and without ("node0": they are
# pairs of node 0 with itself)
PAIR_CASES = ((1, 1, 0, "none"), (1, 257, 3, "masked"), (16, 255, 0, "node0"), (16, 256, 3, "none"),
              (63, 257, 3, "masked"), (64, 1000, 0, "masked"), (64, 256, 3, "node0"),
              (63, 1, 0, "none"), (64, 255, 3, "none"), (1, 1000, 0, "none"))
PAIR_PAD = 37  # padding pairs at the end (as many as fit below P)


def pair_inputs(D, P, ld_extra, padding):
    """→ dict(h [40, ld] fp32 with NaN in the pad columns, ps, pd, ns, nd [P] int32, valid [P]
    uint8 or None, n_live int or None). All positives point at 8 nodes. Pair 0 has
    (neg + delta) - pos exactly 0 in fp32 (rows 1, 2, 1, 1: 1 + 1 - 2), pair 1 (P >= 2) is one ulp
    of 2 below 0 (its positive row is nextafter(2))."""
    rng = np.random.default_rng([D, P, ld_extra, ("none", "masked", "node0").index(padding), 19])
    h = np.full((PAIR_ROWS, D + ld_extra), np.nan, np.float32)
    h[:, :D] = rng.standard_normal((PAIR_ROWS, D)).astype(np.float32) * np.float32(0.3)
    for r, v in ((PAIR_R1, 1.0), (PAIR_R2, 2.0), (PAIR_R2UP, np.nextafter(np.float32(2), np.float32(3)))):
        h[r, :D] = 0
        h[r, 0] = v
    ps = rng.integers(0, PAIR_R1, P).astype(np.int32)
    pd = rng.integers(0, 8, P).astype(np.int32)
    ns = ps.copy()
    nd = rng.integers(0, PAIR_R1, P).astype(np.int32)
    ps[0], pd[0], ns[0], nd[0] = PAIR_R1, PAIR_R2, PAIR_R1, PAIR_R1
    if P >= 2:
        ps[1], pd[1], ns[1], nd[1] = PAIR_R1, PAIR_R2UP, PAIR_R1, PAIR_R1
    valid, n_live = None, None
    if padding != "none":
        pad = min(PAIR_PAD, P - 2)
        for a in (ps, pd, ns, nd):
            a[P - pad:] = -1
        if padding == "masked":
            valid = np.ones(P, np.uint8)
            valid[P - pad:] = 0
            n_live = P - pad
    return dict(h=h, ps=ps, pd=pd, ns=ns, nd=nd, valid=valid, n_live=n_live)


def _pair_rows(h, D, idx, n_rows):
    """The row each endpoint reads in float64 (-1 → node 0, >= n_rows → zeros) and the node that
    takes its gradient (-1 for an endpoint out of range)."""
    idx = np.asarray(idx, np.int64)
    node = np.where(idx < 0, 0, np.where(idx >= n_rows, -1, idx))
    rows = np.where((node >= 0)[:, None], h[:, :D].astype(np.float64)[np.maximum(node, 0)], 0.0)
    return rows, node


def pair_ref(c, D, dloss=1.0, n_rows=PAIR_ROWS, delta=PAIR_DELTA):
    """float64 → dict(pos, neg, pos_mag, neg_mag (Σ_d |a b|), arg = (neg + delta) - pos, loss =
    Σ_live max(arg, 0) / n_live (its magnitude is itself), on (live and arg >= 0), dh, dh_mag
    (Σ |coef · h[other]| per node), oob)."""
    P = c["ps"].size
    (A, na), (B, nb), (Cc, nc), (E, ne) = (_pair_rows(c["h"], D, c[k], n_rows)
                                          for k in ("ps", "pd", "ns", "nd"))
    pos, neg = (A * B).sum(1), (Cc * E).sum(1)
    arg = (neg + delta) - pos
    v = np.ones(P, bool) if c["valid"] is None else c["valid"].astype(bool)
    nl = P if c["n_live"] is None else c["n_live"]
    on = v & (arg >= 0)
    coef = np.where(on, dloss / nl, 0.0)[:, None]
    dh, mag = np.zeros((n_rows, D)), np.zeros((n_rows, D))
    for node, t in ((na, -coef * B), (nb, -coef * A), (nc, coef * E), (ne, coef * Cc)):
        m = on & (node >= 0)
        np.add.at(dh, node[m], t[m])
        np.add.at(mag, node[m], np.abs(t[m]))
    return dict(pos=pos, neg=neg, pos_mag=np.abs(A * B).sum(1), neg_mag=np.abs(Cc * E).sum(1),
                arg=arg, loss=float(np.sum(np.maximum(arg, 0) * v) / nl), on=on, dh=dh, dh_mag=mag,
                oob=bool(((na < 0) | (nb < 0) | (nc < 0) | (ne < 0)).any()))


def pair_f32(c, D, dloss=1.0, n_rows=PAIR_ROWS, delta=PAIR_DELTA):
    """The same in fp32: products summed over d in order, hinges summed in pair order, each
    node's terms added in (role, pair) order."""
    P = c["ps"].size
    h32 = np.where(np.isnan(c["h"]), np.float32(0), c["h"])
    rows = [_pair_rows(h32, D, c[k], n_rows) for k in ("ps", "pd", "ns", "nd")]
    (A, na), (B, nb), (Cc, nc), (E, ne) = [(f32(r), n) for r, n in rows]
    pos, neg = sum_seq32(A * B, 1), sum_seq32(Cc * E, 1)
    arg = (neg + np.float32(delta)) - pos
    v = np.ones(P, bool) if c["valid"] is None else c["valid"].astype(bool)
    nl = np.float32(P if c["n_live"] is None else c["n_live"])
    loss = np.cumsum(np.where(v, np.maximum(arg, np.float32(0)), np.float32(0)), dtype=np.float32)[-1] / nl
    on = v & (arg >= 0)
    coef = np.where(on, np.float32(dloss) / nl, np.float32(0))[:, None]
    dh = np.zeros((n_rows, D), np.float32)
    for node, t in ((na, -coef * B), (nb, -coef * A), (nc, coef * E), (ne, coef * Cc)):
        m = on & (node >= 0)
        np.add.at(dh, node[m], t[m])
    return pos, neg, np.float32(loss), dh


# =============================================================================================
# rs_multihot_mean_fwd / _bwd
MH_ITEMS, MH_SAME_ROW = 50, 7
# (V, D, G, N): V·D at 1 and at the limit 256 both ways, D at the limit 64, G 1 / 20 / 32 (the
# limit), N around the 32-item block and past 256 blocks (8193 = 257 blocks: the fold strides)
MH_CASES = ((1, 1, 1, 1), (4, 64, 32, 31), (256, 1, 20, 32), (20, 8, 20, 33), (3, 64, 1, 8193),
            (4, 64, 20, 8193), (256, 1, 32, 33), (1, 1, 32, 8193), (20, 8, 32, 1), (3, 64, 20, 32))
MH_REJECTED = ((257, 1, 20), (1, 65, 20), (4, 8, 33))  # (V, D, G): V·D 257, D 65, G 33


def multihot_inputs(V, D, G, N):
    """→ (table [V, D], mh [50, G] int32, items [N] int64, dout [N, D]). Item 7's id row names table
    row V - 1 in all its G slots; the last example is item 7; examples 0 and 1 (N >= 2) are the same
    item."""
    rng = np.random.default_rng([V, D, G, N, 20])
    table = rng.standard_normal((V, D)).astype(np.float32)
    mh = rng.integers(0, V, (MH_ITEMS, G)).astype(np.int32)
    mh[MH_SAME_ROW] = V - 1
    items = rng.integers(0, MH_ITEMS, N).astype(np.int64)
    items[N - 1] = MH_SAME_ROW
    if N >= 3:
        items[1] = items[0]
    return table, mh, items, rng.standard_normal((N, D)).astype(np.float32)


def multihot_ref(table, mh, items, dout):
    """float64: out[n] = Σ_g table[mh[item, g]] / G, dtable[r] = Σ_n Σ_{g: id = r} dout[n] / G, an
    item outside [0, n_items) and an id outside [0, V) adding nothing; Σ|terms| of each."""
    V, D = table.shape
    G = mh.shape[1]
    ok_item = (items >= 0) & (items < mh.shape[0])
    ids = np.where(ok_item[:, None], mh[np.where(ok_item, items, 0)], -1)  # [N, G]
    ok = (ids >= 0) & (ids < V)
    t64, d64 = table.astype(np.float64), dout.astype(np.float64) / G
    out, out_mag = np.zeros((items.size, D)), np.zeros((items.size, D))
    dt, dt_mag = np.zeros((V, D)), np.zeros((V, D))
    for g in range(G):
        m = ok[:, g]
        r = ids[m, g]
        out[m] += t64[r] / G
        out_mag[m] += np.abs(t64[r]) / G
        np.add.at(dt, r, d64[m])
        np.add.at(dt_mag, r, np.abs(d64[m]))
    return dict(out=out, out_mag=out_mag, dtable=dt, dtable_mag=dt_mag,
                oob=bool((~ok).any()), ok=ok)


def multihot_f32(table, mh, items, dout):
    """The same in fp32: the forward summed over g in order, then / G; the table gradient's terms
    dout / G added one after the other."""
    V, D = table.shape
    G = mh.shape[1]
    ok_item = (items >= 0) & (items < mh.shape[0])
    ids = np.where(ok_item[:, None], mh[np.where(ok_item, items, 0)], -1)
    ok = (ids >= 0) & (ids < V)
    s = np.zeros((items.size, D), np.float32)
    gs = dout / np.float32(G)
    dt = np.zeros((V, D), np.float32)
    for g in range(G):
        m = ok[:, g]
        s[m] = s[m] + table[ids[m, g]]
        np.add.at(dt, ids[m, g], gs[m])
    return s / np.float32(G), dt
