"""The inputs of tests/test_exchange_edges_gpu.py have the property their name claims, the
restatements of tests/exchange_edges.py driven as W simulated ranks agree with the oracle the
project already trusts (table lookup; oracle.sharded.sharded_sgd_step and sharded_owner_grads,
bit for bit), and three deliberately wrong restatements are caught by the comparisons the GPU
file makes — all without a GPU."""
import numpy as np
import pytest

from oracle.embedding import global_rows, segment_sum_tiled
from oracle.sharded import owner_keys, sharded_owner_grads, sharded_sgd_step
from tests import exchange_edges as E

D = 8
LR = 0.05


def cases(names=E.PATTERNS):
    return [(W, V, C, n) for W, V in E.GEOMETRIES for C in E.CAPACITIES for n in names
            if E.feasible(n, W, V, C)]


def unique_of(ids, W, V, slots):
    so = E.slot_offsets_of(V) if slots else None
    sk, pos = E.sort_sharded(ids, V, W, so)
    return E.unique_inverse(sk, pos, V, W), sk, pos


# =============================================================================================
# named properties
def test_geometries_and_capacities_reach_what_they_claim():
    g = {W: V for W, V in E.GEOMETRIES}
    assert E.key_space_of(37, 1) == 37 and E.key_space_of(37, 2) == 38 > 37
    assert E.stride_of(100, 3) == 34 and [E.shard_rows(100, 3, o) for o in range(3)] == [34, 33, 33]
    assert 8 in g and g[8] == 1001
    # owner_counts_kernel runs 64·ceil(W/64) threads: one wave at 64, two at 65
    assert -(-64 // E.WAVE) == 1 and -(-65 // E.WAVE) == 2 and {64, 65} <= set(g)
    for W, V in E.GEOMETRIES:
        assert sum(E.shard_rows(V, W, o) for o in range(W)) == V
    assert {C % E.WAVE == 0 for C in E.CAPACITIES} == {True, False}
    assert 64 in E.CAPACITIES and 5 % E.WAVE and 70 % E.WAVE
    # W·C = 15: one wave spans all three requesters
    assert 3 * 5 == 15 < E.WAVE
    # C = 70, W >= 2: every wave of the W·C slots spans at most two requesters, and some wave
    # spans exactly two
    for W in (2, 3, 4, 8):
        spans = [len({i // 70 for i in range(w, min(w + E.WAVE, W * 70))})
                 for w in range(0, W * 70, E.WAVE)]
        assert max(spans) == 2
    # every capacity meets exact_fit and one_over at some geometry, every geometry at some capacity
    for C in E.CAPACITIES:
        assert any(E.feasible("one_over", W, V, C) for W, V in E.GEOMETRIES)
    for W, V in E.GEOMETRIES:
        assert any(E.feasible("one_over", W, V, C) for C in E.CAPACITIES)
    assert E.feasible("one_over", 8, 1001, 70) and E.feasible("one_over", 65, 400, 5)


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("W,V,C,name", cases())
def test_pattern_has_its_property(W, V, C, name, slots):
    ids = E.make_ids(name, W, V, C, slots=slots)
    i32 = E.make_ids(name, W, V, C, slots=slots, dtype=np.int32)
    assert ids.dtype == np.int64 and i32.dtype == np.int32 and (ids == i32).all()
    assert ids.ndim == 2 and ids.shape[1] == E.N_SLOTS
    so = E.slot_offsets_of(V) if slots else None
    assert so is None or (so[1] - so[0] == 1 and so[-1] == V)
    rows = global_rows(ids, V, so)
    u, sk, pos = unique_of(ids, W, V, slots)
    counts = u["owner_counts"]
    p = E.pack(u["uniq"], counts, W, E.stride_of(V, W), C, u["inverse"])
    assert counts.sum() == u["n_unique"] == np.unique(rows[rows >= 0]).size
    if name == "zipf":
        # heavy duplicates: a third of the positions repeat a row, one row is read many times
        assert (rows >= 0).all() and u["n_unique"] <= rows.size * 2 // 3
        assert np.bincount(rows).max() >= 6
    elif name.startswith("empty_owner"):
        o = E.empty_owner_of(name, W)
        assert counts[o] == 0 and u["n_unique"] > 0
        assert (p["send_ids"][o * C:(o + 1) * C] == -1).all()
    elif name == "one_owner":
        assert counts[0] == u["n_unique"] > 0 and not counts[1:].any()
    elif name == "exact_fit":
        assert (counts == C).sum() == 1 and counts.max() == C
        assert p["excess"] == 0 and p["overflow"] == 0 and (p["slot_of"] >= 0).all()
    elif name == "one_over":
        assert (counts == C + 1).sum() == 1 and counts.max() == C + 1
        assert p["excess"] == 1 and p["overflow"] == 1 and (p["slot_of"] == -1).sum() == 1
    elif name == "oob":
        card = np.diff(so)[np.arange(ids.size) % E.N_SLOTS] if slots else V
        flat = ids.reshape(-1)
        assert (flat == -1).any() and (flat == card).any() and (rows >= 0).any()
        assert ((rows < 0) == ((flat == -1) | (flat == card))).all()
    elif name == "all_oob":
        assert ids.size and (rows < 0).all() and u["n_unique"] == 0 and not counts.any()
        assert (u["inverse"] == -1).all() and (p["send_ids"] == -1).all()
    elif name == "empty":
        assert ids.size == 0 and u["n_unique"] == 0
    # the sentinel is the key space, the padding keys of a key space larger than V never occur
    ks = E.key_space_of(V, W)
    assert (sk[rows[pos] < 0] == ks).all() and (sk[rows[pos] >= 0] < ks).all()
    real = owner_keys(np.arange(V), V, W)[0]
    assert np.isin(u["uniq"], real).all() and ks >= V


@pytest.mark.parametrize("W,V,C", [(3, 100, 5), (4, 130, 5), (8, 1001, 64), (8, 1001, 70),
                                   (3, 100, 1)])
def test_spill_inputs_have_their_excesses(W, V, C):
    per_rank, ex = E.spill_world_ids(W, V, C)
    assert ex[:3] == [0, 1, 3] and max(ex) == 3
    for r, ids in enumerate(per_rank):
        u, _, _ = unique_of(ids, W, V, False)
        assert E.excess(u["owner_counts"], C) == ex[r]
    assert 0 < ex[1] < max(ex)  # rank 1's spill block holds padding


# =============================================================================================
# the simulated world against the oracle
def run_world(W, V, C, per_rank_ids, slots, seed=0, backward=True):
    rng = np.random.default_rng([seed, W, V, C])
    table = rng.standard_normal((V, D)).astype(np.float32)
    so = E.slot_offsets_of(V) if slots else None
    world = E.World(W, V, C, table, so)
    fw = world.forward(per_rank_ids)
    E.check_lookup(world, fw, per_rank_ids, table)
    if not backward:
        return fw
    grads = [rng.standard_normal((i.size, D)).astype(np.float32) for i in per_rank_ids]
    got = world.backward(fw, grads, LR)
    want = sharded_owner_grads(per_rank_ids, grads, W, V, so)
    for o in range(W):
        E.same(got[o][0], want[o][0], f"owner {o} rows")
        E.same(got[o][1], want[o][1], f"owner {o} folded grads")
    E.same(world.full_table(), sharded_sgd_step(table, per_rank_ids, grads, LR, W, so),
           "table after the SGD apply")
    return fw


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("C", E.CAPACITIES)
@pytest.mark.parametrize("W,V", E.GEOMETRIES)
def test_world_lookup_and_backward_equal_the_oracle(W, V, C, slots):
    spilled = 0
    for name in E.PATTERNS:
        if not E.feasible(name, W, V, C):
            continue
        # rank 0 carries the named pattern; the others vary it, so ranks differ (and the empty
        # batch meets non-empty ones)
        other = "zipf" if name in ("empty", "all_oob") else name
        # (of a wide world's ranks, eight carry a batch and the rest the empty one)
        per_rank = [E.make_ids(name if r == 0 else other if r < 8 else "empty", W, V, C, seed=r,
                               slots=slots, dtype=np.int32 if r % 2 else np.int64)
                    for r in range(W)]
        # the oracle's step costs W² Python loops: a wide world takes it on four patterns
        back = W < 64 or name in ("zipf", "one_over", "oob", "empty")
        spilled += run_world(W, V, C, per_rank, slots, backward=back)["C2"] > 0
    for name in ("empty", "all_oob"):  # every rank at once
        fw = run_world(W, V, C, [E.make_ids(name, W, V, C, seed=r, slots=slots)
                                 for r in range(W)], slots, backward=W < 64)
        assert fw["C2"] == 0 and all((s == -1).all() for s in fw["send_ids"])
    if E.feasible("one_over", W, V, C):
        assert spilled  # the spill round was reached


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("W,V,C", [(3, 100, 5), (4, 130, 5), (8, 1001, 64), (8, 1001, 70)])
def test_world_spill_round(W, V, C, slots):
    per_rank, ex = E.spill_world_ids(W, V, C, slots)
    fw = run_world(W, V, C, per_rank, slots)
    assert fw["C2"] == 3
    for r in range(W):
        assert (fw["spill_ids"][r] >= 0).sum() == ex[r]  # the rest of the block is padding
        assert (fw["slot_of"][r] >= 0).all()


# =============================================================================================
# ranged-dedup inputs
@pytest.mark.parametrize("W,below,cross", E.DEDUP_CASES)
def test_dedup_input_boundaries(W, below, cross):
    inp = E.dedup_input(W, below, cross)
    sk, K = inp["sk"].astype(np.int64), inp["K"]
    assert sk.size == E.DEDUP_N == 2100 > 2 * E.GROUP and (np.diff(sk) >= 0).all()
    assert K == (W // 2) * E.stride_of(E.DEDUP_V, W) and 0 < K < inp["key_space"]
    b = int((sk < K).sum())
    assert b == inp["below"] and (cross or b == below)
    assert (inp["seg_map"] == -1).any() and (inp["seg_map"] >= 0).any()
    live = inp["seg_map"][inp["seg_map"] >= 0]
    assert np.unique(live).size == live.size and live.max() < inp["n_unique"] + 8
    if cross:
        lo, hi = E.CROSS["run_lo"], E.CROSS["run_hi"]
        assert (sk[lo[0]:lo[1]] == K - 1).all() and sk[lo[0] - 1] < K - 1
        assert lo[0] < 1056 < lo[1] and 1056 % E.TILE == 0 and lo[1] % E.TILE  # K mid-tile
        assert (sk[hi[0]:hi[1]] == K).all() and sk[hi[1]] > K and hi[0] < 1088 < hi[1]
    else:
        assert {0: b == 0, 1024: b % E.GROUP == 0, 1041: b % E.TILE != 0,
                1056: b % E.TILE == 0 and b % E.GROUP != 0, 2100: b == sk.size}[below]
        if 0 < b < sk.size:
            assert (sk == inp["key_space"]).sum() == 5
        else:
            assert (sk < inp["key_space"]).all()  # a half with no key at all
    # runs cross tiles and groups
    heads = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[heads[1:], sk.size] - 1
    assert (heads // E.TILE != ends // E.TILE).any()
    if 0 < b < sk.size:
        assert (heads // E.GROUP != ends // E.GROUP).any()


@pytest.mark.parametrize("W,below,cross", E.DEDUP_CASES)
def test_dedup_ranges_emit_what_one_call_does(W, below, cross):
    inp = E.dedup_input(W, below, cross)
    K, ks = inp["K"], inp["key_space"]
    for scaled in (False, True):
        rows, out = E.dedup_ref(inp, scaled, True)
        r2 = np.full(E.DEDUP_N, E.FILL_I, np.int64)
        o2 = np.full_like(out, np.nan)
        sc = inp["row_scale"] if scaled else None
        for lo, hi in ((0, K), (K, ks)):
            E.dedup_mapped(inp["sk"], inp["pos"], inp["grad"], sc, E.DEDUP_GROUP, lo, hi,
                           inp["seg_map"], ks, r2, o2)
        E.same(r2, rows, "uniq_rows")
        E.same(o2, out, "uniq_grad")
        # unmapped, it is the oracle's fold; rows of the map's holes and the spare rows stay NaN
        g = inp["grad"] if not scaled else \
            (inp["row_scale"][np.arange(E.DEDUP_N) // E.DEDUP_GROUP, None] * inp["grad"])
        uk, ug = segment_sum_tiled(inp["sk"], inp["pos"], g.astype(np.float32), ks)
        live = inp["seg_map"] >= 0
        E.same(out[inp["seg_map"][live]], ug[live], "mapped rows")
        assert np.isnan(out).all(1).sum() == out.shape[0] - live.sum()
        E.same(rows[:inp["n_unique"]], uk.astype(np.int64), "keys")
        assert (rows[inp["n_unique"]:] == E.FILL_I).all()
    if below in (0, 2100):  # a range holding no key writes nothing
        lo, hi = ((0, K) if below == 0 else (K, ks))
        rows, out = E.dedup_ref(inp, False, True, lo, hi)
        assert (rows == E.FILL_I).all() and np.isnan(out).all()


# =============================================================================================
# the rows-ahead restatements close the loop: early rows + late rows = a fresh gather
@pytest.mark.parametrize("W,C", [(3, 5), (2, 70), (4, 64)])
def test_mark_classify_scatter_late_round_trip(W, C):
    rng = np.random.default_rng([W, C])
    n_rows, dim = 50, 4
    before = rng.standard_normal((n_rows, dim)).astype(np.float32)
    after = before.copy()
    cur = rng.integers(-1, n_rows, W * C).astype(np.int32)
    nxt = rng.integers(-1, n_rows + 2, W * C).astype(np.int32)  # n_rows, n_rows + 1: out of range
    touched = cur[cur >= 0]
    after[touched] += 1.0
    stamp = E.mark(cur, np.zeros(n_rows, np.int32), n_rows, 7)
    assert set(np.flatnonzero(stamp == 7)) == set(touched.tolist())
    pairs, cnt = E.classify(nxt, W, C, stamp, n_rows, 7)
    CL = int(cnt.max())
    late_rows = np.full((W, C), -1, np.int32)
    late_slot = np.full((W, C), -1, np.int32)
    for r in range(W):
        for k, (row, s) in enumerate(pairs[r]):
            late_rows[r, k], late_slot[r, k] = row, s
            assert nxt[r * C + s] == row and 0 <= row < n_rows
    early = E.gather_padded(before, n_rows, nxt, dim)
    recv = E.gather_padded(after, n_rows, late_rows[:, :CL].reshape(-1), dim)
    got = E.scatter_late(recv, late_slot.reshape(-1), W, C, CL, early)
    E.same(got, E.gather_padded(after, n_rows, nxt, dim), "early + late rows")


# =============================================================================================
# mutations: each wrong restatement is caught by a comparison the GPU file makes
def _pack_inputs(name, W, V, C):
    ids = E.make_ids(name, W, V, C)
    u, _, _ = unique_of(ids, W, V, False)
    return u, (u["uniq"], u["owner_counts"], W, E.stride_of(V, W), C, u["inverse"])


def test_mutation_j_le_capacity_is_caught():
    for name in ("exact_fit", "one_over"):
        u, args = _pack_inputs(name, 3, 100, 5)
        assert E.fit_owner(3, 100, 6) == 1  # the wrong slot lands in the next owner's block
        want = E.pack(*args)
        if name == "exact_fit":  # no row at j == C: the mutant cannot show
            E.compare_pack(E.pack(*args, mut="le"), want)
        else:
            with pytest.raises(AssertionError):
                E.compare_pack(E.pack(*args, mut="le"), want)


def test_mutation_owner_by_modulo_is_caught():
    u, args = _pack_inputs("zipf", 4, 130, 64)
    assert u["n_unique"] <= 4 * 64
    with pytest.raises(AssertionError):
        E.compare_pack(E.pack(*args, mut="owner_mod"), E.pack(*args))
    # and by the lookup of the simulated world
    table = np.random.default_rng(0).standard_normal((130, D)).astype(np.float32)
    per_rank = [E.make_ids("zipf", 4, 130, 64, seed=r) for r in range(4)]
    world = E.World(4, 130, 64, table, mut="owner_mod")
    with pytest.raises(AssertionError):
        E.check_lookup(world, world.forward(per_rank), per_rank, table)


def test_mutation_spill_slot_base_is_caught():
    W, V, C, C2 = 3, 100, 5, 3
    per_rank, ex = E.spill_world_ids(W, V, C)
    u, _, _ = unique_of(per_rank[2], W, V, False)
    args = (u["uniq"], u["owner_counts"], W, E.stride_of(V, W), C)
    p = E.pack(*args, u["inverse"])
    want = E.pack_spill(*args, C2, u["inverse"], p["slot_of"])
    with pytest.raises(AssertionError):
        E.compare_spill(E.pack_spill(*args, C2, u["inverse"], p["slot_of"], mut="spill_base"), want)
    table = np.random.default_rng(0).standard_normal((V, D)).astype(np.float32)
    world = E.World(W, V, C, table, mut="spill_base")
    with pytest.raises(AssertionError):
        E.check_lookup(world, world.forward(per_rank), per_rank, table)
