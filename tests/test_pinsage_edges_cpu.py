"""The inputs of tests/test_pinsage_edges_gpu.py have the property their name claims (degrees, tie
counts, probe chains, scan-tile positions, an exact-zero hinge: checked on the data), the float64
restatements of tests/pinsage_edges.py agree with torch float64 autograd, and a plain fp32 NumPy
evaluation of each float reference meets the bound 1e-5 · Σ|terms| at a quarter of it — all without
a GPU. The last test prints the largest fp32 error / bound ratio seen per kernel family (the
figures in the docstring of tests/pinsage_edges.py)."""
import numpy as np
import pytest
import torch

from oracle import pinsage as O
from tests import pinsage_edges as P

QUARTER = 0.25
RATIOS: dict = {}


def room(got, ref, bound, family, msg):
    """fp32 `got` within a quarter of `bound` of `ref`; the ratio to the full bound is recorded."""
    q = P.off_by(got, ref, bound)
    RATIOS[family] = max(RATIOS.get(family, 0.0), q)
    print(f"  {msg}: fp32 err / bound {q:.3g}")
    assert q <= QUARTER, f"{msg}: fp32 evaluation at {q:.3g} of the bound"


# =============================================================================================
# graphs
def test_hub_graph_has_its_degrees_and_draws_past_2_16():
    u, i, nu, ni = P.hub_graph_edges()
    og = P.oracle_graph("hub")
    ideg, udeg = np.diff(og.i2u_indptr), np.diff(og.u2i_indptr)
    assert 140_000 <= u.size <= 160_000
    assert ideg[0] >= P.HUB_DEG and udeg[0] >= P.HUB_DEG
    assert np.unique(og.i2u[:ideg[0]]).size == ideg[0] and np.unique(og.u2i[:udeg[0]]).size == udeg[0]
    assert ideg[1:].max() < 200 and udeg[1:].max() < 200   # everything else is ordinary
    assert (ideg[P.HUB_ORD:P.HUB_ORD + P.HUB_DEG] == 1).all()
    assert (ideg[-50:] == 0).all() and (udeg[-50:] == 0).all()  # dead ends on both sides
    seeds = P.hub_seeds()
    assert 0 in seeds and (ideg[seeds] == 0).any() and (og.i2u[og.i2u_indptr[seeds[1:6]]] == 0).all()
    nw, T, p = P.HUB_WALK
    tr = O.metapath_walk(og, seeds, nw, T, p, P.SEED, 7, 0)
    from_item, from_user = P.adjacency_draws(og, tr)
    # bounded(r, deg) with deg > 2^16: the high half of the product decides these
    assert from_item.max() >= 65_536 and from_user.max() >= 65_536
    assert (tr[np.repeat(ideg[seeds] == 0, nw), 1:] == -1).all()
    rn, rc = P.oracle_neighbors("hub", *P.HUB_NEIGHBORS)
    assert (rn[ideg[seeds] == 0] == -1).all()
    # the neighbour walks too draw past 2^16 on both sides; a seed behind the hub user has ten
    # candidates, the hub item mostly returns to itself (its users have no other item)
    nw, T, p, _ = P.HUB_NEIGHBORS
    from_item, from_user = P.adjacency_draws(og, O.metapath_walk(og, seeds, nw, T, p, P.SEED, 5, 1))
    assert from_item.max() >= 65_536 and from_user.max() >= 65_536
    assert (rn[1] >= P.HUB_ORD).all() and rn[0, 0] == 0


def test_tie_graph_ties_at_the_cut():
    og = P.oracle_graph("tie")
    assert (np.diff(og.u2i_indptr) == P.TIE_PER_USER).all()
    nw, T, p = P.TIE_WALK
    assert P.TIE_SEEDS % (256 // nw) != 0
    rn, rc = P.oracle_neighbors("tie", nw, T, p, 100)
    distinct = (rn >= 0).sum(1)
    assert distinct.max() <= nw * T and np.median(distinct) >= 50   # most visited once
    for k in (1, 10):
        tie = (rc[:, k - 1] == rc[:, k]) & (rc[:, k] > 0)
        print(f"  k {k}: {int(tie.sum())} / {tie.size} seeds tie on count at the cut")
        assert tie.mean() > 0.5
        # and the id order decides: within a tie run the ids ascend
        assert (rn[tie, k - 1] < rn[tie, k]).all()
    for k in (64, 100):
        assert (distinct < k).mean() > 0.9  # trailing slots -1 / 0
    assert (rn[:, 64:] == -1).all() and (rc[:, 64:] == 0).all()


def test_walk_limit_cases_reach_the_limits():
    cs = P.WALK_LIMIT_CASES
    assert max(nw * T for nw, T, _, _ in cs) == 512 and {T for _, T, _, _ in cs} == {1, 8}
    assert {nw for nw, _, _, _ in cs} == {1, 33, 63, 64}
    assert O.stop_threshold(1.0) == 0xFFFFFFFF and O.stop_threshold(0.0) == 0
    seeds = P.limit_seeds()
    assert (seeds == -1).sum() == 7 and np.array_equal(seeds[seeds >= 0], np.arange(300))
    for nw, T, p, k in cs:
        wshift = int(np.ceil(np.log2(nw))) if nw > 1 else 0
        assert seeds.size % (256 >> wshift) != 0
        rn, rc = P.oracle_neighbors("limit", nw, T, p, k)
        assert (rn[seeds == -1] == -1).all() and (rc[seeds == -1] == 0).all()
        # p = 1: the stop draw after the first hop (item -> user) is below 0xFFFFFFFF, so every
        # trace ends on the user and no item is ever visited: k empty slots for every seed
        assert (rn >= 0).any() != (p == 1.0)
    rn, rc = P.oracle_neighbors("limit", 64, 8, 0.0, 10)
    assert rc.sum(1).max() > 64 and (rn[:, -1] >= 0).any()


def test_pair_counter_wraps_by_design():
    og = P.oracle_graph("pairs")
    gi = (P.WRAP_PAIR_BASE + np.arange(P.WRAP_BATCH)) & 0xFFFFFFFF
    assert gi[4] == 0xFFFFFFFF and gi[5] == 0 and P.WRAP_PAIR_BASE + P.WRAP_BATCH > 2 ** 32
    whole = O.item_pairs(og, P.WRAP_PAIR_BASE, P.WRAP_BATCH, 4, P.STEP_WRAP)
    head = O.item_pairs(og, P.WRAP_PAIR_BASE, 5, 4, P.STEP_WRAP)
    tail = O.item_pairs(og, 0, P.WRAP_BATCH - 5, 4, P.STEP_WRAP)
    for w, a, b in zip(whole, head, tail):
        assert np.array_equal(w, np.concatenate([a, b])) and w.size > 0
    other = O.item_pairs(og, P.WRAP_PAIR_BASE, P.WRAP_BATCH, 4, 0)
    assert not np.array_equal(whole[0], other[0])  # the step word matters


# =============================================================================================
# exclusion set
def test_exclusion_pairs_chain_wrap_and_occupied_homes():
    c = P.excl_case()
    assert c["src"].size == c["dst"].size == P.EXCL_N
    skipped = (c["src"] < 0) | (c["dst"] < 0)
    assert ((c["src"] < 0) & (c["dst"] >= 0)).any() and ((c["dst"] < 0) & (c["src"] >= 0)).any()
    live_keys = P.pair_key(c["dst"][~skipped], c["src"][~skipped])
    assert np.array_equal(np.unique(live_keys), c["keys"])
    assert 850 <= c["keys"].size < live_keys.size   # duplicates; load >= 0.83 of 1024 slots
    table, probes = P.probe_insert(c["src"], c["dst"], P.EXCL_CAP)
    occupied = table != np.uint64(2 ** 64 - 1)
    assert occupied.sum() == c["keys"].size and (probes[skipped] == 0).all()
    print(f"  load {occupied.mean():.3f}, longest probe chain {probes.max()}")
    assert probes.max() >= 8
    stored = np.flatnonzero(occupied)
    home = P.slot_of(table[stored], P.EXCL_CAP - 1)
    wrapped = stored < home    # stored before its home slot: the chain ran past the table's end
    assert wrapped.any() and occupied[P.EXCL_CAP - 1] and occupied[0]
    # the occupied set does not depend on the order of insertion
    t2, _ = P.probe_insert(c["src"][::-1], c["dst"][::-1], P.EXCL_CAP)
    assert np.array_equal(t2 != np.uint64(2 ** 64 - 1), occupied)
    # the sampler's look-ups: pairs in the set, and absent pairs whose home slot is taken
    rn, _ = c["unfiltered"]
    s_idx, r_idx = np.nonzero(rn >= 0)
    look = P.pair_key(c["seeds"][s_idx], rn[s_idx, r_idx])
    present = np.isin(look, c["keys"])
    assert present.sum() > 300 and (~present).sum() > 300
    assert occupied[P.slot_of(look[~present], P.EXCL_CAP - 1)].sum() > 100
    # at the wide capacity nothing of this happens: load 0.014
    _, wide = P.probe_insert(c["src"], c["dst"], P.EXCL_WIDE)
    assert wide.max() <= 3
    nw, T, p, k = P.EXCL_WALK
    en, _ = O.pinsage_neighbors(P.oracle_graph("limit"), c["seeds"], nw, T, p, k, P.EXCL_SEED, 0, 0,
                                exclude=c["exclude"])
    assert (en == -1).sum() - (rn == -1).sum() == present.sum()


# =============================================================================================
# unique / block
def test_unique_inputs_sit_on_the_scan_tile():
    assert {P.unique_inputs(n)[0].size for n in P.UNIQUE_CASES if n.startswith("n")} == \
        {P.SCAN_TILE - 1, P.SCAN_TILE, P.SCAN_TILE + 1, 2 * P.SCAN_TILE + 1}
    for name in P.UNIQUE_CASES:
        ids, n_nodes = P.unique_inputs(name)
        uniq, local = O.unique_first(ids)
        assert ids.max(initial=-1) < n_nodes
        if name.startswith("n"):
            n = ids.size
            assert local[n - 1] == uniq.size - 1 and (ids[:n - 1] != ids[n - 1]).all()
            if n > P.SCAN_TILE:
                assert (ids[:P.SCAN_TILE] != ids[P.SCAN_TILE]).all()
            assert (ids == -1).any() and uniq.size < n
    assert O.unique_first(P.unique_inputs("all_absent")[0])[0].size == 0
    assert O.unique_first(P.unique_inputs("all_equal")[0])[0].tolist() == [5]
    ids, n_nodes = P.unique_inputs("wide_ids")
    assert n_nodes == 3_000_000 and {0, n_nodes - 1} <= set(ids.tolist())
    assert P.unique_inputs("empty")[0].size == 0


def test_block_cases_cover_tile_edges_and_degenerate_blocks():
    caps = {n * k for n, k, _ in P.BLOCK_CASES}
    assert {4095, 4096, 4097, 0} <= caps and {1, 32} <= {k for _, k, _ in P.BLOCK_CASES}
    for n_dst, k, kind in P.BLOCK_CASES:
        dst, nbr, cnt = P.block_inputs(n_dst, k, kind)
        b = O.to_block(dst, nbr, cnt)
        assert ((cnt > 0) == (nbr >= 0)).all() and cnt.max(initial=0) <= 512
        if kind == "empty":
            assert b.edge_src.size == 0 and not b.indptr.any() and not b.t_indptr.any()
        if kind == "full":
            assert b.edge_src.size == n_dst * k
        if kind == "hub":
            tdeg = np.diff(b.t_indptr)
            assert tdeg.max() == n_dst and b.src_nodes[np.argmax(tdeg)] == P.BLOCK_HUB
            assert (tdeg[:n_dst] == 0).sum() > n_dst // 2  # the destinations' own rows: mostly unused
        if kind == "mixed" and n_dst:
            assert cnt.max() == 512 and 0 < b.edge_src.size < n_dst * k


# =============================================================================================
# weighted mean pooling
def test_agg_block_has_its_degrees():
    b = P.agg_block()
    deg, tdeg = np.diff(b.indptr), np.diff(b.t_indptr)
    assert set(deg.tolist()) == set(P.AGG_DST_DEGREES)   # 4-at-a-time loop: 0, 1 and 2 passes, tails 0..3
    assert set(tdeg.tolist()) == {0, 1} | set(P.AGG_SRC_DEGREES) | {int(tdeg.max())}
    assert tdeg.max() >= 1000 and tdeg[P.AGG_DST] == tdeg.max()   # the hub: 131 passes of 8 and a tail
    assert (tdeg[:P.AGG_DST] == 0).all() and b.edge_w.max() == 512
    assert b.n_dst * P.AGG_K > P.SCAN_TILE


@pytest.mark.parametrize("H", P.AGG_H)
def test_agg_fp32_reference_within_bound(H):
    b = P.agg_block()
    u, g = P.agg_values(H, b.n_src)
    r = P.agg_ref(u, g, b)
    nv, gu = P.agg_f32(u, g, b)
    room(nv, r["nv"], P.RTOL * r["nv_mag"], "agg fwd", f"agg H {H} nv")
    room(gu, r["gu"], P.RTOL * r["gu_mag"], "agg bwd", f"agg H {H} gu")
    assert not r["nv"][np.diff(b.indptr) == 0].any() and (r["wsum"][np.diff(b.indptr) == 0] == 0).all()


def test_agg_ref_equals_torch_float64_autograd():
    b = P.agg_block()
    u, g = P.agg_values(5, b.n_src)
    r = P.agg_ref(u, g, b)
    ut = torch.from_numpy(u).double().requires_grad_()
    src, dst = torch.from_numpy(b.edge_src), torch.from_numpy(b.edge_dst)
    w = torch.from_numpy(b.edge_w).double()
    vs = torch.zeros(b.n_dst, 5, dtype=torch.float64).index_add(0, dst, ut[src] * w[:, None])
    ws = torch.zeros(b.n_dst, dtype=torch.float64).index_add(0, dst, w)
    nv = vs / torch.clamp(ws, min=1)[:, None]
    nv.backward(torch.from_numpy(g).double())
    assert P.off_by(nv.detach().numpy(), r["nv"], 1e-12 * r["nv_mag"]) <= 1
    assert P.off_by(ut.grad.numpy(), r["gu"], 1e-12 * r["gu_mag"]) <= 1


# =============================================================================================
# Frobenius
def test_frobenius_sizes_reach_the_fold_loop():
    nb = [-(-n // P.RED_CHUNK) for n in P.FROB_N]
    assert nb == [1, 1, 1, 2, 256, 257, 513]  # the fold's i += 256 loop: 1, 2 and 3 passes
    ones = np.ones(1_048_576, np.float32)
    assert P.partition_sum32(ones) == 1024.0 ** 2 and P.partition_sum32(ones[:4096]) == 64.0 ** 2
    assert np.float32(1) / np.float32(1024) == 2.0 ** -10


@pytest.mark.parametrize("n", P.FROB_N)
def test_frobenius_fp32_partition_within_bound(n):
    x, dy = P.frob_inputs(n)
    r = P.frob_ref(x, dy)
    norm, y, dx = P.frob_f32(x, dy)
    room(norm, r["norm"], P.RTOL * r["norm"], "frob norm", f"frob n {n} norm")
    room(y, r["y"], P.RTOL * r["y"], "frob y", f"frob n {n} y")
    room(dx, r["dx"], r["dx_bound"], "frob dx", f"frob n {n} dx")
    if n == max(P.FROB_N):
        q = P.off_by(P.frob_norm_seq32(x), r["norm"], P.RTOL * r["norm"])
        print(f"  frob n {n} norm, sequential fp32 sum: err / bound {q:.3g}")
        RATIOS["frob norm, sequential"] = q
        assert q > 1  # why the kernel sums in a fixed two-level partition


def test_frobenius_ref_equals_torch_float64_autograd():
    x, dy = P.frob_inputs(4097)
    r = P.frob_ref(x, dy)
    xt = torch.from_numpy(x).double().requires_grad_()
    y = xt / torch.norm(xt)
    y.backward(torch.from_numpy(dy).double())
    assert np.abs(y.detach().numpy() - r["y"]).max() <= 1e-14
    assert P.off_by(xt.grad.numpy(), r["dx"], 1e-7 * r["dx_bound"]) <= 1


def test_frobenius_all_zero_reference_is_nan():
    """What the reference x / torch.norm(x) gives for an all-zero x: NaN everywhere. The GPU test
    pins parity with this; it is not a wish."""
    x = torch.zeros(5, 4)
    assert torch.isnan(x / torch.norm(x)).all()
    assert [P.frob_rows_live(700, w) for w in P.FROB_ROWS_LIVE] == [0, 1, 700, 703]


# =============================================================================================
# pair margin
def test_pair_cases_cover_the_lists():
    c = P.PAIR_CASES
    assert {x[0] for x in c} == {1, 16, 63, 64} and {x[1] for x in c} == {1, 255, 256, 257, 1000}
    assert {x[2] for x in c} == {0, 3} and {x[3] for x in c} == {"none", "masked", "node0"}
    for D in (1, 64):
        assert {x[2] for x in c if x[0] == D} == {0, 3}


@pytest.mark.parametrize("D,npairs,ld_extra,padding", P.PAIR_CASES)
def test_pair_inputs_and_fp32_reference(D, npairs, ld_extra, padding):
    c = P.pair_inputs(D, npairs, ld_extra, padding)
    r = P.pair_ref(c, D)
    pos, neg, loss, dh = P.pair_f32(c, D)
    assert c["h"].shape == (P.PAIR_ROWS, D + ld_extra) and np.isnan(c["h"][:, D:]).all()
    assert not np.isnan(c["h"][:, :D]).any() and not r["oob"]
    # the hinge exactly at 0, in fp32 as in float64: it carries gradient (>= 0)
    arg32 = (neg + np.float32(P.PAIR_DELTA)) - pos
    assert arg32[0] == 0.0 and r["arg"][0] == 0.0 and r["on"][0]
    g = 1.0 / (npairs if c["n_live"] is None else c["n_live"])
    assert r["dh"][P.PAIR_R2, 0] == -g and not r["dh"][P.PAIR_R2, 1:].any()
    if npairs >= 2:  # one ulp of 2 below 0: no gradient
        assert arg32[1] == -(2.0 ** -22) and r["arg"][1] == -(2.0 ** -22) and not r["on"][1]
        assert not r["dh"][P.PAIR_R2UP].any()
        assert (c["pd"][2:][c["pd"][2:] >= 0] < 8).all()  # all positives onto 8 nodes
    live = np.arange(npairs) >= 2
    if padding != "none":
        assert (c["ps"][-1], c["pd"][-1], c["ns"][-1], c["nd"][-1]) == (-1, -1, -1, -1)
        assert (c["valid"] is None) == (padding == "node0")
        if padding == "masked":
            assert c["n_live"] == c["valid"].sum() < npairs and not r["on"][c["valid"] == 0].any()
        else:
            assert r["on"][-1] and abs(r["arg"][-1] - 1.0) < 1e-12 and arg32[-1] == 1.0   # node 0 with itself: the hinge is delta
    # no other hinge is near 0: the float64 and the fp32 evaluation agree on who carries gradient
    assert (np.abs(r["arg"][live]) > 1e-3).all() and np.array_equal(arg32 >= 0, r["arg"] >= 0)
    room(pos, r["pos"], P.RTOL * r["pos_mag"], "pair scores", f"pair D {D} P {npairs} pos")
    room(neg, r["neg"], P.RTOL * r["neg_mag"], "pair scores", f"pair D {D} P {npairs} neg")
    room(loss, r["loss"], P.RTOL * r["loss"], "pair loss", f"pair D {D} P {npairs} loss")
    room(dh, r["dh"], P.RTOL * r["dh_mag"], "pair dh", f"pair D {D} P {npairs} dh")


@pytest.mark.parametrize("case", [P.PAIR_CASES[4], P.PAIR_CASES[6]])
def test_pair_ref_equals_torch_float64_autograd(case):
    from recommender_amd.pinsage.model import margin_loss

    D = case[0]
    c = P.pair_inputs(*case)
    r = P.pair_ref(c, D)
    h = torch.from_numpy(c["h"][:, :D].copy()).double().requires_grad_()

    def score(a, b):
        a, b = (torch.from_numpy(c[k].astype(np.int64)).clamp_min(0) for k in (a, b))
        return (h[a] * h[b]).sum(-1)

    valid = None if c["valid"] is None else torch.from_numpy(c["valid"]).bool()
    nl = None if c["n_live"] is None else torch.tensor([c["n_live"]], dtype=torch.int32)
    loss = margin_loss(score("ps", "pd"), score("ns", "nd"), P.PAIR_DELTA, valid, nl)
    loss.backward()
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-13 * r["loss"]
    assert P.off_by(h.grad.numpy(), r["dh"], 1e-12 * r["dh_mag"] + 1e-300) <= 1


def test_pair_all_invalid_reference_is_nan():
    """What margin_loss gives when no pair is live (n_live = 0): the loss 0 / 0 = NaN, and its
    backward hands every node that an active hinge touches 0 · inf = NaN; the GPU test asserts the
    kernels give the same."""
    from recommender_amd.pinsage.model import margin_loss

    c = P.pair_inputs(16, 255, 0, "none")
    h = torch.from_numpy(c["h"]).requires_grad_()
    pad = torch.full((255,), -1, dtype=torch.int64).clamp_min(0)
    s = (h[pad] * h[pad]).sum(-1)
    loss = margin_loss(s, s, 1.0, torch.zeros(255, dtype=torch.bool), torch.zeros(1, dtype=torch.int32))
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(h.grad[0]).all() and not h.grad[1:].any()


# =============================================================================================
# multi-hot mean
def test_multihot_cases_cover_the_lists():
    c = P.MH_CASES
    assert {(V, D) for V, D, _, _ in c} == {(1, 1), (4, 64), (256, 1), (20, 8), (3, 64)}
    assert {G for _, _, G, _ in c} == {1, 20, 32} and {N for _, _, _, N in c} == {1, 31, 32, 33, 8193}
    assert max(V * D for V, D, _, _ in c) == 256 and -(-8193 // P.MH_ROWS) == 257
    assert [(V * D > 256, D > 64, G > 32) for V, D, G in P.MH_REJECTED] == \
        [(True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.parametrize("V,D,G,N", P.MH_CASES)
def test_multihot_inputs_and_fp32_reference(V, D, G, N):
    table, mh, items, dout = P.multihot_inputs(V, D, G, N)
    r = P.multihot_ref(table, mh, items, dout)
    assert not r["oob"] and (mh[P.MH_SAME_ROW] == V - 1).all() and items[-1] == P.MH_SAME_ROW
    if N >= 3:
        assert items[0] == items[1]
    if N > P.MH_ITEMS:
        assert np.unique(items).size < N   # repeated items
    out, dt = P.multihot_f32(table, mh, items, dout)
    room(out, r["out"], P.RTOL * r["out_mag"], "multihot out", f"multihot V {V} D {D} G {G} N {N} out")
    room(dt, r["dtable"], P.RTOL * r["dtable_mag"], "multihot dtable",
         f"multihot V {V} D {D} G {G} N {N} dtable")
    # out of range: an item and an id add nothing, everything else is unchanged
    bad_items, bad_mh = items.copy(), mh.copy()
    bad_items[0] = P.MH_ITEMS + 3
    bad_mh[P.MH_SAME_ROW, G - 1] = V
    rb = P.multihot_ref(table, bad_mh, bad_items, dout)
    assert rb["oob"] and not rb["out"][0].any()
    keep = (bad_items != P.MH_SAME_ROW) & (np.arange(N) != 0)
    assert np.array_equal(rb["out"][keep], r["out"][keep])


def test_multihot_ref_equals_torch_float64_autograd():
    table, mh, items, dout = P.multihot_inputs(20, 8, 20, 33)
    r = P.multihot_ref(table, mh, items, dout)
    t = torch.from_numpy(table).double().requires_grad_()
    out = t[torch.from_numpy(mh.astype(np.int64))[torch.from_numpy(items)]].mean(1)
    out.backward(torch.from_numpy(dout).double())
    assert P.off_by(out.detach().numpy(), r["out"], 1e-12 * r["out_mag"]) <= 1
    assert P.off_by(t.grad.numpy(), r["dtable"], 1e-12 * r["dtable_mag"]) <= 1


def test_zz_print_largest_fp32_ratios():
    """Prints what the docstring of tests/pinsage_edges.py records (run the whole file with -s)."""
    for k in sorted(RATIOS):
        print(f"  {k}: largest fp32 err / bound {RATIOS[k]:.3g}")
