"""Inputs and NumPy restatements for the row-sharded exchange's edge suite
(tests/test_exchange_edges_cpu.py proves their properties, tests/test_exchange_edges_gpu.py runs
the kernels of csrc/exchange.hip, csrc/sort.hip and csrc/embedding.hip against them).

Nothing here calls a kernel. The restatements are written from the contract in
include/recsys_hip.h on top of the oracle the project already trusts (oracle/sharded.py:
owner_keys; oracle/embedding.py: global_rows, sort_ids, segment_sum_tiled). Everything is integer
bookkeeping or the fixed-order fp32 fold, so every comparison is exact (floats as uint32 bits).

`World` drives W simulated ranks through a whole step with these restatements; an all-to-all of
equal blocks is the permute recv[o][r] = send[r][o].
"""
from __future__ import annotations

import numpy as np

from oracle.embedding import global_rows, segment_sum_tiled, sort_ids
from oracle.sharded import owner_keys

WAVE = 64
TILE = 32      # RS_DEDUP_TILE
GROUP = 1024   # sorted keys per group of the D = 128 walk (32 tiles)
FILL_I = 0x5A5A5A5A  # what the GPU tests prefill integer outputs with
N_SLOTS = 3

# (W, V): world 1 (key space = n_rows); key space 38 > V; uneven shards 34/33/33; production
# width; one full wave of owner threads; two waves of owner threads
GEOMETRIES = ((1, 37), (2, 37), (3, 100), (4, 130), (8, 1001), (64, 200), (65, 400))
# 5 and 70 are no multiples of the wave: with W·C = 15 one wave spans several requesters, with
# C = 70 (W >= 2) exactly two; 64 is the aligned control
CAPACITIES = (1, 5, 64, 70)
PATTERNS = ("zipf", "empty_owner_first", "empty_owner_middle", "empty_owner_last", "one_owner",
            "exact_fit", "one_over", "oob", "all_oob", "empty")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stride_of(V, W):
    return -(-V // W)


def key_space_of(V, W):
    return V if W == 1 else stride_of(V, W) * W


def shard_rows(V, W, o):
    return (V - o + W - 1) // W


def slot_offsets_of(V):
    """Three slots packed in one slab, the first of cardinality 1."""
    c1 = (V - 1) // 2
    return np.array([0, 1, 1 + c1, V], np.int64)


# =============================================================================================
# id patterns, each built by construction
def empty_owner_of(name, W):
    return {"empty_owner_first": 0, "empty_owner_middle": W // 2, "empty_owner_last": W - 1}[name]


def fit_owner(W, V, need):
    """The owner nearest the middle, from below, whose shard holds `need` rows (None: no shard
    does; owner 0's is the largest)."""
    for o in reversed(range(W // 2 + 1)):
        if shard_rows(V, W, o) >= need:
            return o
    return None


def over_of(name):
    return {"exact_fit": 0, "one_over": 1}.get(name)


def feasible(name, W, V, C, over=None):
    """A pattern that cannot exist at a geometry is left out: an empty owner needs two owners,
    an owner with C (+ over) unique rows a shard that large."""
    if name.startswith("empty_owner"):
        return W >= 2
    over = over_of(name) if over is None else over
    if over is not None:
        return fit_owner(W, V, C + over) is not None
    return True


def _pool(name, W, V, C, rng, over):
    """(rows that must each appear, rows the other positions draw from)."""
    rows = np.arange(V)
    none = np.zeros(0, np.int64)
    if name in ("zipf", "oob"):
        return none, rows
    if name.startswith("empty_owner"):
        return none, rows[rows % W != empty_owner_of(name, W)]
    if name == "one_owner":
        return none, rows[rows % W == 0]
    if over is not None:
        o = fit_owner(W, V, C + over)
        mine = rng.permutation(np.arange(o, V, W))[:C + over]
        rest = [rng.permutation(np.arange(q, V, W))[:C - 1] for q in range(W) if q != o]
        return mine, np.concatenate([mine] + rest)
    return none, none  # all_oob, empty


def _draw(pool, k, rng):
    """k heavy-tailed draws (duplicates by construction); -1 where there is nothing to draw."""
    if pool.size == 0:
        return np.full(k, -1, np.int64)
    p = rng.permutation(pool)[:60]
    return p[np.minimum((p.size * rng.random(k) ** 3).astype(np.int64), p.size - 1)]


def make_ids(name, W, V, C, seed=0, slots=False, dtype=np.int64, over=None, B=32):
    """ids [B', 3] of `dtype` (per-slot ids with `slots`, else rows of one shared table). A slot
    that holds no row of the pattern (say the one-row slot when owner 0 must stay empty) is
    filled with the id -1."""
    over = over_of(name) if over is None else over
    tag = PATTERNS.index(name) if name in PATTERNS else 99
    rng = np.random.default_rng([seed, W, V, C, tag, int(slots), over or 0])
    if name == "empty":
        return np.zeros((0, N_SLOTS), dtype)
    req, pool = _pool(name, W, V, C, rng, over)
    if slots:
        so = slot_offsets_of(V)
        per = [(req[(req >= so[s]) & (req < so[s + 1])] - so[s],
                pool[(pool >= so[s]) & (pool < so[s + 1])] - so[s]) for s in range(N_SLOTS)]
        n = max(B, max(r.size for r, _ in per))
        cols = [rng.permutation(np.concatenate([r, _draw(p, n - r.size, rng)])) for r, p in per]
        ids = np.stack(cols, 1)
        card = (so[1:] - so[:-1])[None, :].repeat(n, 0)
    else:
        n = max(B, -(-req.size // N_SLOTS))
        flat = rng.permutation(np.concatenate([req, _draw(pool, n * N_SLOTS - req.size, rng)]))
        ids = flat.reshape(n, N_SLOTS)
        card = np.full_like(ids, V)
    if name in ("oob", "all_oob"):
        hit = np.ones(ids.shape, bool) if name == "all_oob" else rng.random(ids.shape) < 0.2
        hit.reshape(-1)[:2] = True  # one of each kind at least
        kind = (np.arange(ids.size).reshape(ids.shape) % 2).astype(bool)
        ids = np.where(hit & kind, card, np.where(hit, -1, ids))
    return ids.astype(dtype)


def spill_world_ids(W, V, C, slots=False, dtype=np.int64):
    """Per-rank ids for a spill round: rank 0 has excess 0, rank 1 excess 1 (below C2), rank 2
    excess 3 (= C2 = 3), every further rank excess 0."""
    ex = [0, 1, 3] + [0] * (W - 3)
    return [make_ids("exact_fit", W, V, C, seed=10 + r, slots=slots, dtype=dtype, over=ex[r])
            for r in range(W)], ex


# =============================================================================================
# restatements
def sort_sharded(ids, V, W, slot_offsets=None):
    """rs_sort_ids_sharded: (sorted owner-major keys uint32, positions int32). OOB ids follow
    every valid key, grouped by slot, in position order; their key is the key space."""
    rows = global_rows(ids, V, slot_offsets)
    keys, _, ks = owner_keys(rows, V, W)
    n_slots = 1 if slot_offsets is None else np.asarray(slot_offsets).size - 1
    slot = np.arange(rows.size) % n_slots
    k = np.where(rows < 0, ks + slot, keys).astype(np.int64)
    pos = np.argsort(k, kind="stable")
    return np.minimum(k[pos], ks).astype(np.uint32), pos.astype(np.int32)


def unique_inverse(sk, pos, V, W):
    """rs_unique_inverse: uniq keys, inverse (-1 for OOB), n_unique, owner_counts and the
    exclusive scan of the head flags (the workspace head)."""
    sk = np.asarray(sk).astype(np.int64)
    stride, ks = stride_of(V, W), key_space_of(V, W)
    valid = sk < ks
    head = valid.copy()
    head[1:] &= sk[1:] != sk[:-1]
    excl = np.cumsum(head) - head
    uniq = sk[head]
    inverse = np.full(sk.size, -1, np.int32)
    inverse[np.asarray(pos)] = np.where(valid, excl + head - 1, -1)
    return dict(uniq=uniq.astype(np.uint32), inverse=inverse, n_unique=int(uniq.size),
                owner_counts=np.bincount(uniq // stride, minlength=W).astype(np.int32),
                seg_excl=excl.astype(np.int32))


def _dealt(uniq, counts, W, stride, mut=""):
    """(owner, rank among the owner's unique rows, owner-local row) of every unique key."""
    uniq = np.asarray(uniq).astype(np.int64)
    counts = np.asarray(counts).astype(np.int64)
    ostart = np.cumsum(counts) - counts
    o = uniq % W if mut == "owner_mod" else uniq // stride
    return o, np.arange(uniq.size) - ostart[o], uniq - o * stride


def _by_inverse(inverse, slot_of):
    """Each position's slot: that of its unique row, -1 for an OOB id."""
    inverse = np.asarray(inverse)
    if not slot_of.size:
        return np.full(inverse.size, -1, np.int32)
    return np.where(inverse >= 0, slot_of[np.maximum(inverse, 0)], -1).astype(np.int32)


def pack(uniq, counts, W, stride, C, inverse, mut=""):
    """rs_exchange_pack + rs_exchange_excess. `mut` names a deliberately wrong variant (the
    mutation checks): "le" takes j <= C for j < C, "owner_mod" key % W for key // stride."""
    o, j, local = _dealt(uniq, counts, W, stride, mut)
    fits = (j <= C) if mut == "le" else (j < C)
    slot_of = np.where(fits, o * C + j, -1).astype(np.int32)
    send_ids = np.full(W * C, -1, np.int32)
    send_ids[slot_of[fits]] = local[fits]
    inverse_slot = _by_inverse(inverse, slot_of)
    return dict(send_ids=send_ids, slot_of=slot_of, inverse_slot=inverse_slot,
                overflow=int((~fits).any()), excess=excess(counts, C))


def excess(counts, C):
    """rs_exchange_excess: max_o max(0, counts[o] - C)."""
    return int(max(0, (np.asarray(counts).astype(np.int64) - C).max()))


def pack_spill(uniq, counts, W, stride, C, C2, inverse, slot_of, mut=""):
    """rs_exchange_pack_spill: the rows past the capacity take slots W·C + o·C2 + (j - C); rows
    within the capacity keep their slots, rows past C + C2 keep -1 and raise the overflow.
    mut "spill_base": the slot base o·C for W·C + o·C2."""
    o, j, local = _dealt(uniq, counts, W, stride)
    j = j - C
    sel = (j >= 0) & (j < C2)
    slot_of = np.asarray(slot_of).copy()
    base = o * C if mut == "spill_base" else W * C + o * C2
    slot_of[sel] = (base + j)[sel]
    spill_ids = np.full(W * C2, -1, np.int32)
    spill_ids[(o * C2 + j)[sel]] = local[sel]
    inverse_slot = _by_inverse(inverse, slot_of)
    return dict(spill_ids=spill_ids, slot_of=slot_of, inverse_slot=inverse_slot,
                overflow=int((j >= C2).any()))


def gather_padded(shard, n_rows, ids, dim):
    """rs_gather_rows_padded: out[i] = shard[ids[i]], a zero row for padding / out of range."""
    ids = np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < n_rows)
    out = np.zeros((ids.size, dim), np.float32)
    out[ok] = shard[ids[ok]]
    return out


def mark(ids, stamp, n_rows, seq):
    """rs_exchange_mark: stamp[row] = seq for every requested row in range."""
    ids = np.asarray(ids).astype(np.int64)
    out = np.asarray(stamp).copy()
    out[ids[(ids >= 0) & (ids < n_rows)]] = seq
    return out


def classify(recv_ids, W, C, stamp, n_rows, pred):
    """rs_exchange_classify: per requester, the sorted (row, slot) pairs whose row carries the
    stamp `pred`, and their count. The list order is not part of the contract."""
    ids = np.asarray(recv_ids).astype(np.int64).reshape(W, C)
    ok = (ids >= 0) & (ids < n_rows)
    hit = ok & (np.asarray(stamp)[np.where(ok, ids, 0)] == pred)
    pairs = [sorted((int(ids[r, s]), int(s)) for s in np.flatnonzero(hit[r])) for r in range(W)]
    return pairs, np.array([len(p) for p in pairs], np.int32)


def scatter_late(recv_rows, recv_slot, W, C, C_late, rows):
    """rs_exchange_scatter_late: rows[o·C + recv_slot[o·C + k]] = recv_rows[o·C_late + k] for
    k < C_late, slot -1 skipped; every other row of `rows` stays."""
    out = np.asarray(rows).copy()
    for o in range(W):
        for k in range(C_late):
            j = int(recv_slot[o * C + k])
            if j >= 0:
                out[o * C + j] = recv_rows[o * C_late + k]
    return out


def dedup_mapped(sk, pos, grad, row_scale, scale_group, key_lo, key_hi, seg_map, n_rows,
                 uniq_rows, uniq_grad):
    """rs_embedding_dedup_grad_mapped_range, written into the given buffers: for every segment
    s (numbered over the whole key space) whose key is in [key_lo, key_hi), uniq_rows[s] = the
    key and uniq_grad[seg_map[s]] (row s without a map; skipped where the map is < 0) = the
    tiled fold of row_scale[p // scale_group] * grad[p] (one fp32 multiply) over its positions.
    The tiles are those of the whole sorted array, so ranges emit what one call does."""
    grad = np.asarray(grad, np.float32)
    if row_scale is not None:
        rs = np.asarray(row_scale, np.float32)[np.arange(grad.shape[0]) // scale_group]
        grad = (rs[:, None] * grad).astype(np.float32)
    uk, ug = segment_sum_tiled(sk, pos, grad, n_rows)
    uk = uk.astype(np.int64)
    for s in np.flatnonzero((uk >= key_lo) & (uk < key_hi)):
        uniq_rows[s] = uk[s]
        dst = s if seg_map is None else int(seg_map[s])
        if dst >= 0:
            uniq_grad[dst] = ug[s]


# =============================================================================================
# comparisons shared by the CPU mutation checks and the GPU tests
def same(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    if want.dtype.kind == "f":
        got, want = bits(got), bits(want)
    bad = got != want
    assert not bad.any(), (f"{msg}: {int(bad.sum())} / {bad.size} differ; first at "
                           f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} != {want[bad][0]!r}")


def compare_pack(got, want, msg=""):
    U = want["slot_of"].size
    same(got["send_ids"], want["send_ids"], f"{msg} send_ids")
    same(np.asarray(got["slot_of"])[:U], want["slot_of"], f"{msg} slot_of[:U]")
    same(got["inverse_slot"], want["inverse_slot"], f"{msg} inverse_slot")
    assert int(got["overflow"]) == want["overflow"], f"{msg} overflow flag"
    assert int(got["excess"]) == want["excess"], f"{msg} excess"


def compare_spill(got, want, msg=""):
    U = want["slot_of"].size
    same(got["spill_ids"], want["spill_ids"], f"{msg} spill_ids")
    same(np.asarray(got["slot_of"])[:U], want["slot_of"], f"{msg} slot_of[:U]")
    same(got["inverse_slot"], want["inverse_slot"], f"{msg} inverse_slot")
    assert int(got["overflow"]) == want["overflow"], f"{msg} overflow flag"


def check_lookup(world, fw, per_rank_ids, table, msg=""):
    """Every position reads table[global row] (a zero row / slot -1 where the id is OOB) and every
    padding slot holds the id -1 and a zero row."""
    W, C, C2 = world.W, world.C, fw["C2"]
    for r, ids in enumerate(per_rank_ids):
        rows = global_rows(ids, world.V, world.slot_offsets)
        want = np.zeros((rows.size, table.shape[1]), np.float32)
        want[rows >= 0] = table[rows[rows >= 0]]
        same(fw["lookup"][r], want, f"{msg} rank {r} lookup")
        assert ((fw["inv_slot"][r] < 0) == (rows < 0)).all(), f"{msg} rank {r}: slot -1 iff OOB"
        sent = np.concatenate([fw["send_ids"][r], fw["spill_ids"][r]])
        used = np.zeros(W * (C + C2), bool)
        used[fw["inv_slot"][r][rows >= 0]] = True
        assert ((sent >= 0) == used).all(), f"{msg} rank {r}: a slot is live iff a position reads it"
        assert not fw["rows"][r][~used].any(), f"{msg} rank {r}: a padding slot's row is not zero"


# =============================================================================================
def permute(send, c):
    """The all-to-all of equal blocks of c entries: recv[o] = [send[r][o·c:(o+1)·c] for r]."""
    W = len(send)
    return [np.concatenate([send[r][o * c:(o + 1) * c] for r in range(W)]) for o in range(W)]


class World:
    """W simulated ranks of the row-sharded slab over one [V, D] table, every stage one of the
    restatements above."""

    def __init__(self, W, V, C, table, slot_offsets=None, mut=""):
        self.W, self.V, self.C, self.D = W, V, C, table.shape[1]
        self.stride, self.key_space = stride_of(V, W), key_space_of(V, W)
        self.slot_offsets = slot_offsets
        self.shards = [np.ascontiguousarray(table[o::W]) for o in range(W)]
        self.mut = mut

    def full_table(self):
        out = np.empty((self.V, self.D), np.float32)
        for o in range(self.W):
            out[o::self.W] = self.shards[o]
        return out

    def forward(self, per_rank_ids):
        W, V, C, D = self.W, self.V, self.C, self.D
        sk, pos, un, pk = [], [], [], []
        for ids in per_rank_ids:
            k, p = sort_sharded(ids, V, W, self.slot_offsets)
            u = unique_inverse(k, p, V, W)
            sk.append(k), pos.append(p), un.append(u)
            pk.append(pack(u["uniq"], u["owner_counts"], W, self.stride, C, u["inverse"],
                           self.mut))
        C2 = max(p["excess"] for p in pk)  # the all-reduce (MAX)
        slot_of = [p["slot_of"] for p in pk]
        inv_slot = [p["inverse_slot"] for p in pk]
        send_ids = [p["send_ids"] for p in pk]
        spill_ids = [np.zeros(0, np.int32)] * W
        if C2:
            sp = [pack_spill(u["uniq"], u["owner_counts"], W, self.stride, C, C2, u["inverse"],
                             s, self.mut) for u, s in zip(un, slot_of)]
            slot_of = [s["slot_of"] for s in sp]
            inv_slot = [s["inverse_slot"] for s in sp]
            spill_ids = [s["spill_ids"] for s in sp]
        recv_ids, recv_spill = permute(send_ids, C), permute(spill_ids, C2)
        serve = lambda o, ids: gather_padded(self.shards[o], self.shards[o].shape[0], ids, D)
        rows_c = permute([serve(o, recv_ids[o]) for o in range(W)], C)
        rows_s = permute([serve(o, recv_spill[o]) for o in range(W)], C2)
        rows = [np.concatenate([a, b]) for a, b in zip(rows_c, rows_s)]
        lookup = []
        for r in range(W):
            out = np.zeros((inv_slot[r].size, D), np.float32)
            ok = inv_slot[r] >= 0
            out[ok] = rows[r][inv_slot[r][ok]]
            lookup.append(out)
        return dict(sk=sk, pos=pos, unique=un, slot_of=slot_of, inv_slot=inv_slot,
                    send_ids=send_ids, spill_ids=spill_ids, recv_ids=recv_ids,
                    recv_spill=recv_spill, rows=rows, lookup=lookup, C2=C2)

    def send_blocks(self, fw, per_rank_grads, row_scale=None, scale_group=1):
        """Each rank's [W·(C + C2), D] gradient send block; padding slots stay NaN."""
        out = []
        for r, g in enumerate(per_rank_grads):
            n = fw["sk"][r].size
            send = np.full((self.W * (self.C + fw["C2"]), self.D), np.nan, np.float32)
            if n:
                dedup_mapped(fw["sk"][r], fw["pos"][r], g, None if row_scale is None else
                             row_scale[r], scale_group, 0, self.key_space, fw["slot_of"][r],
                             self.key_space, np.zeros(n, np.int64), send)
            out.append(send)
        return out

    def received(self, fw, send):
        """Per owner: (local rows, gradient rows), source-rank-major [W, C + C2] with each
        source's capacity block before its spill block."""
        W, C, C2, D = self.W, self.C, fw["C2"], self.D
        gc = permute([s[:W * C] for s in send], C)
        gs = permute([s[W * C:] for s in send], C2)
        out = []
        for o in range(W):
            ids = np.concatenate([fw["recv_ids"][o].reshape(W, C),
                                  fw["recv_spill"][o].reshape(W, C2)], 1).reshape(-1)
            g = np.concatenate([gc[o].reshape(W, C, D), gs[o].reshape(W, C2, D)], 1)
            out.append((ids, g.reshape(-1, D)))
        return out

    def backward(self, fw, per_rank_grads, lr, global_grads=False):
        """The owners' folded gradients (rows of each rank's local mean scaled by float32(1/W)
        before the fold, as oracle.sharded.sharded_owner_grads) and the SGD apply with lr/W
        (oracle.sharded.sharded_sgd_step), the padding slots left out."""
        W, D = self.W, self.D
        recv = self.received(fw, self.send_blocks(fw, per_rank_grads))
        lr_w = (np.float32(float(np.float32(lr)) / W) if W > 1 and not global_grads
                else np.float32(lr))
        owner_grads = []
        for o, (ids, g) in enumerate(recv):
            n_rows = self.shards[o].shape[0]
            if not (ids >= 0).any():
                owner_grads.append((np.zeros(0, np.int64), np.zeros((0, D), np.float32)))
                continue
            sr, sp, _ = sort_ids(ids, n_rows)
            scaled = g * np.float32(1.0 / W) if W > 1 else g
            ur, ug = segment_sum_tiled(sr, sp, scaled, n_rows)
            owner_grads.append((ur.astype(np.int64), ug))
            ur, ug = segment_sum_tiled(sr, sp, g, n_rows)
            ur = ur.astype(np.int64)
            self.shards[o] = self.shards[o].copy()
            self.shards[o][ur] = self.shards[o][ur] - lr_w * ug
        return owner_grads


# =============================================================================================
# ranged-dedup inputs
DEDUP_V, DEDUP_N, DEDUP_D, DEDUP_GROUP = 600, 2100, 128, 3
DEDUP_BELOW = (0, 1024, 1041, 1056, 2100)  # positions with key < K
DEDUP_WORLDS = (2, 3, 4)
CROSS = dict(below=1070, run_lo=(1050, 1070), run_hi=(1070, 1095))  # see dedup_input


def dedup_boundary(W):
    """K = (W // 2)·stride: the first key of the second owner half."""
    return (W // 2) * stride_of(DEDUP_V, W)


def dedup_input(W, below, cross=False, seed=0):
    """2100 keys of the world-W key space over 600 rows, `below` of them under K, sorted stably,
    with gradient rows, a row scale per group of 3 positions and a segment map with holes.
    Heavy duplicates: runs cross tiles and the 1024-key groups. With 0 < below < 2100 a few OOB
    sentinels end the array. cross: below = 1070 with key K - 1 at sorted positions [1050, 1070)
    (a run over the tile boundary 1056 that ends where K begins, mid-tile) and key K at
    [1070, 1095) (over the boundary 1088)."""
    rng = np.random.default_rng([seed, W, below, int(cross)])
    ks, K = key_space_of(DEDUP_V, W), dedup_boundary(W)
    n = DEDUP_N
    n_sent = 5 if 0 < below < n else 0

    def draws(lo, hi, k):
        pool = rng.permutation(np.arange(lo, hi))[:40]
        return pool[np.minimum((pool.size * rng.random(k) ** 2).astype(np.int64), pool.size - 1)]

    if cross:
        below = CROSS["below"]
        a, b = CROSS["run_lo"], CROSS["run_hi"]
        keys = np.concatenate([draws(0, K - 1, a[0]), np.full(a[1] - a[0], K - 1),
                               np.full(b[1] - b[0], K),
                               draws(K + 1, ks, n - b[1] - n_sent), np.full(n_sent, ks)])
    else:
        keys = np.concatenate([draws(0, K, below), draws(K, ks, n - below - n_sent),
                               np.full(n_sent, ks)])
    keys = rng.permutation(keys).astype(np.int64)
    pos = np.argsort(keys, kind="stable")
    sk = keys[pos]
    n_unique = np.unique(sk[sk < ks]).size
    seg_map = rng.permutation(n_unique + 8)[:n_unique].astype(np.int32)
    seg_map[rng.random(n_unique) < 0.15] = -1
    seg_map[0] = -1
    return dict(W=W, K=K, key_space=ks, below=below, sk=sk.astype(np.uint32),
                pos=pos.astype(np.int32), n_unique=n_unique, seg_map=seg_map,
                grad=rng.standard_normal((n, DEDUP_D)).astype(np.float32),
                row_scale=rng.standard_normal(n // DEDUP_GROUP).astype(np.float32))


DEDUP_CASES = [(W, b, False) for W in DEDUP_WORLDS for b in DEDUP_BELOW] + \
              [(W, CROSS["below"], True) for W in DEDUP_WORLDS]


def dedup_ref(inp, scaled, mapped, key_lo=0, key_hi=None, width=None):
    """(uniq_rows, uniq_grad) buffers as the call leaves them, prefilled FILL_I / NaN."""
    D = inp["grad"].shape[1] if width is None else width
    grad = inp["grad"][:, :D]
    rows = np.full(DEDUP_N, FILL_I, np.int64)
    out = np.full((inp["n_unique"] + 8, D), np.nan, np.float32)
    dedup_mapped(inp["sk"], inp["pos"], grad, inp["row_scale"] if scaled else None, DEDUP_GROUP,
                 key_lo, inp["key_space"] if key_hi is None else key_hi,
                 inp["seg_map"] if mapped else None, inp["key_space"], rows, out)
    return rows, out
