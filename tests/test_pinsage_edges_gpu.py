"""The kernels of csrc/pinsage.hip at their edges: walks and neighbour selection on hub, tie and
walk-shape-limit graphs, counter and step wrap, the exclusion set at high load, first-appearance
unique and to_block at the scan's tile edges, the weighted mean pooling, the Frobenius
normalisation, the pair margin loss and the multi-hot mean lookup. Inputs, float64 restatements
and bounds come from tests/pinsage_edges.py, whose properties tests/test_pinsage_edges_cpu.py
proves.

Integer results are compared bit for bit with oracle/pinsage.py. Float results are compared with
float64 under |got - ref64| <= 1e-5 · Σ|terms|; every float call runs twice and must give the
same bits. The float kernels are called through the C ABI (L.call) with every output prefilled
with a NaN bit pattern (SENT) and a tail behind it that must come back unchanged.
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import pinsage as O
from recommender_amd import _lib as L
from recommender_amd.pinsage import PinSageSampler
from recommender_amd.pinsage.graph import HeteroGraph, PairGraph
from tests import pinsage_edges as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC12345    # a quiet NaN with a payload no kernel produces
SENT_I = -0x5A5A5A5  # an id no sampler produces
TAIL = 8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent_buf(n):
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENT)
    return t


def is_sent(t):
    return bool((t.view(torch.int32) == SENT).all())


def stream():
    return L.stream_ptr(torch.device(DEV))


def same_bits(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    bad = P.bits(got) != P.bits(want)
    assert not bad.any(), (f"{msg}: {int(bad.sum())} / {bad.size} elements differ in bits; first at "
                           f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} != {want[bad][0]!r}")


def same_ints(got, want, msg):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_array_equal(got, np.asarray(want), err_msg=msg)


def twice(run, *args, **kw):
    """run(...) twice → the first result (a dict of arrays), after checking the second has its bits."""
    a, b = run(*args, **kw), run(*args, **kw)
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float32:
            same_bits(b[k], a[k], f"{k}, the same call again")
        else:
            assert np.array_equal(a[k], b[k]), f"{k}, the same call again"
    return a


@functools.lru_cache(maxsize=None)
def graph(name):
    u, i, nu, ni = P.graph_edges(name)
    return HeteroGraph(u, i, nu, ni, device=DEV)


def sampler(name, num_walks, T, p, k, seed=P.SEED):
    g = graph(name)
    return PinSageSampler(g, g.itype, g.utype, 2, T, num_walks, p, k, seed=seed)


def stub_sampler(n_items, k=3):
    """A sampler for unique_first / to_block alone: they read the graph's device and id space."""
    g = types.SimpleNamespace(device=torch.device(DEV, torch.cuda.current_device()), n_items=n_items)
    return PinSageSampler(g, "movie", "user", 2, 2, 4, 0.0, k)


def run_walk(name, seeds, num_walks, T, p, step, layer):
    g, s = graph(name), dev(seeds)
    tr = torch.full((seeds.size * num_walks, 2 * T + 1), SENT_I, dtype=torch.int32, device=DEV)
    L.call("rs_metapath_walk", *(L.ptr(t) for t in g.csr_args()), L.ptr(s), seeds.size,
           num_walks, T, p, P.SEED, step, layer, L.ptr(tr), stream())
    return tr.cpu().numpy()


def step_word(step):
    """[1] int32 device word holding the 32-bit step."""
    return torch.tensor([step - 2 ** 32 if step >= 2 ** 31 else step], dtype=torch.int32, device=DEV)


def neighbors_at(name, seeds, num_walks, T, p, k, step, layer, seed=P.SEED):
    g, s, word = graph(name), dev(seeds), step_word(step)  # named: alive until the call is queued
    n = seeds.size
    nbr = torch.full((n, k), SENT_I, dtype=torch.int32, device=DEV)
    cnt = torch.full((n, k), SENT_I, dtype=torch.int32, device=DEV)
    L.call("rs_pinsage_neighbors_at", *(L.ptr(t) for t in g.csr_args()), L.ptr(s), n,
           num_walks, T, p, seed, L.ptr(word), layer, k, None, 0, L.ptr(nbr), L.ptr(cnt), stream())
    return nbr.cpu().numpy(), cnt.cpu().numpy()


# =============================================================================================
# walks and neighbours
def test_graphs_match_oracle_csr():
    for name in ("hub", "tie", "limit", "pairs"):
        g, og = graph(name), P.oracle_graph(name)
        for a, b in zip(g.csr_args(), (og.i2u_indptr, og.i2u, og.u2i_indptr, og.u2i)):
            same_ints(a, b, name)


def test_hub_graph_walks_and_neighbors_bit_exact():
    """hop() on large degrees: bounded(r, deg) with deg = 70 000 > 2^16 on the item side and on the
    user side (the CPU file shows draws with adjacency index >= 65 536 on both), from the hub
    item, items behind the hub user, ordinary and dead items."""
    og, seeds = P.oracle_graph("hub"), P.hub_seeds()
    nw, T, p = P.HUB_WALK
    same_ints(run_walk("hub", seeds, nw, T, p, 7, 0), O.metapath_walk(og, seeds, nw, T, p, P.SEED, 7, 0),
              "hub walks")
    nw, T, p, k = P.HUB_NEIGHBORS
    nbr, cnt = sampler("hub", nw, T, p, k).neighbors(dev(seeds), layer=1, step=5)
    rn, rc = P.oracle_neighbors("hub", nw, T, p, k)
    same_ints(nbr, rn, "hub neighbours")
    same_ints(cnt, rc, "hub counts")


@pytest.mark.parametrize("k", P.TIE_K)
def test_tie_graph_selection_bit_exact(k):
    """neighbors_kernel's (count desc, id asc) selection loop as the deciding code: 64 visits over
    about 300 candidates, most visited once, so the k-th and (k+1)-th tie on count for most seeds
    (k 1, 10); k 64 and 100 exceed the distinct candidates: trailing slots -1 / 0."""
    nw, T, p = P.TIE_WALK
    nbr, cnt = sampler("tie", nw, T, p, k).neighbors(dev(P.tie_seeds()), layer=1, step=5)
    rn, rc = P.oracle_neighbors("tie", nw, T, p, k)
    same_ints(nbr, rn, f"tie k {k} neighbours")
    same_ints(cnt, rc, f"tie k {k} counts")


@pytest.mark.parametrize("num_walks,T,p,k", P.WALK_LIMIT_CASES)
def test_walk_shape_limits_bit_exact(num_walks, T, p, k):
    """neighbors_kernel at its limits: C = num_walks · T = 512 visits (the O(C^2) count, 2·256·T
    ints of dynamic LDS), T = 8, num_walks 33 (half of each 64-lane group idle) and 63, one walk a
    seed, p = 1.0 (stop threshold saturated to 0xFFFFFFFF: nothing is visited); 307 seeds (no
    multiple of the seeds a block takes) with -1 padding seeds mixed in: k empty slots each."""
    seeds = P.limit_seeds()
    nbr, cnt = sampler("limit", num_walks, T, p, k).neighbors(dev(seeds), layer=1, step=5)
    rn, rc = P.oracle_neighbors("limit", num_walks, T, p, k)
    same_ints(nbr, rn, "neighbours")
    same_ints(cnt, rc, "counts")
    tr = run_walk("limit", seeds[:40], num_walks, T, p, 5, 1)
    same_ints(tr, O.metapath_walk(P.oracle_graph("limit"), seeds[:40], num_walks, T, p, P.SEED, 5, 1),
              "walks")


def test_walk_shapes_past_the_limits_are_rejected():
    g = graph("limit")
    for nw, T in ((65, 2), (4, 9), (0, 2), (4, 0)):
        with pytest.raises(ValueError):
            PinSageSampler(g, g.itype, g.utype, 2, T, nw, 0.0, 3)
        seeds = dev(np.arange(4, dtype=np.int32))
        out = torch.full((4, 3), SENT_I, dtype=torch.int32, device=DEV)
        with pytest.raises(L.RecsysError):
            L.call("rs_pinsage_neighbors", *(L.ptr(t) for t in g.csr_args()), L.ptr(seeds), 4, nw, T,
                   0.0, 4, 0, 0, 3, None, 0, L.ptr(out), L.ptr(out), stream())
        assert bool((out == SENT_I).all())


# =============================================================================================
# counter and step wrap
def test_pair_counter_and_step_wrap_bit_exact():
    """The counter word (uint32)(pair_base + i) crossing 2^32 inside one batch (pair_base 2^32 - 5,
    batch 32) and step 0xFFFFFFFF, for pairs, walks and neighbours."""
    from recommender_amd.pinsage.sampler import item_pairs

    og = P.oracle_graph("pairs")
    for step in (P.STEP_WRAP, 3):
        got = item_pairs(graph("pairs"), P.WRAP_BATCH, 4, step, P.WRAP_PAIR_BASE)
        for a, b in zip(got, O.item_pairs(og, P.WRAP_PAIR_BASE, P.WRAP_BATCH, 4, step)):
            same_ints(a, b, f"pairs at step {step:#x}")
    seeds = np.arange(og.n_items, dtype=np.int32)
    same_ints(run_walk("pairs", seeds, 5, 2, 0.2, P.STEP_WRAP, 1),
              O.metapath_walk(og, seeds, 5, 2, 0.2, P.SEED, P.STEP_WRAP, 1), "walks at the last step")
    nbr, cnt = sampler("pairs", 7, 3, 0.2, 4).neighbors(dev(seeds), layer=1, step=P.STEP_WRAP)
    rn, rc = O.pinsage_neighbors(og, seeds, 7, 3, 0.2, 4, P.SEED, P.STEP_WRAP, 1)
    same_ints(nbr, rn, "neighbours at the last step")
    same_ints(cnt, rc, "counts at the last step")


@pytest.mark.parametrize("batch", [P.SCAN_TILE - 1, P.SCAN_TILE, P.SCAN_TILE + 1])
def test_item_pairs_at_the_scan_tile(batch):
    """rs_item_pairs' compaction offsets from exclusive_scan_i32 with the batch at the scan's
    4096-element tile: 4095, 4096, 4097 pairs, some dropped (dead-end heads) on both sides of it."""
    from recommender_amd.pinsage.sampler import item_pairs

    got = item_pairs(graph("pairs"), batch, 4, 3, 100)
    ref = O.item_pairs(P.oracle_graph("pairs"), 100, batch, 4, 3)
    assert 0 < ref[0].size < batch
    for a, b in zip(got, ref):
        same_ints(a, b, f"pairs, batch {batch}")


@pytest.mark.parametrize("step", P.AT_STEPS)
def test_device_step_entry_points_equal_host_step(step):
    """rs_item_pairs_at and rs_pinsage_neighbors_at (the step read from a device word) against
    the host-step calls and the oracle, at steps 0, 7 and 0xFFFFFFFF."""
    og = P.oracle_graph("pairs")
    host, at = sampler("pairs", 7, 3, 0.2, 4), sampler("pairs", 7, 3, 0.2, 4)
    a = host.sample_pairs_static(48, 4, step, 11)
    word = step_word(step)
    b = at.sample_pairs_static(48, 4, 12345, 11, step_dev=word)
    rh, rp, rn = O.item_pairs(og, 11, 48, 4, step)
    assert int(a[3]) == int(b[3]) == rh.size
    for x, y, r in zip(a[:3], b[:3], (rh, rp, rn)):
        same_ints(y, x.cpu().numpy(), "device step vs host step")
        same_ints(x[:rh.size], r, "pairs")
        assert bool((x[rh.size:] == -1).all())
    seeds = np.arange(og.n_items, dtype=np.int32)
    nbr, cnt = host.neighbors(dev(seeds), layer=1, step=step)
    nbr_at, cnt_at = neighbors_at("pairs", seeds, 7, 3, 0.2, 4, step, 1)
    rn, rc = O.pinsage_neighbors(og, seeds, 7, 3, 0.2, 4, P.SEED, step, 1)
    same_ints(nbr_at, nbr.cpu().numpy(), "device step vs host step neighbours")
    same_ints(cnt_at, cnt.cpu().numpy(), "device step vs host step counts")
    same_ints(nbr, rn, "neighbours")
    same_ints(cnt, rc, "counts")


# =============================================================================================
# exclusion set
def build_pair_set(src, dst, capacity):
    s, d = dev(src), dev(dst)
    table = torch.full((capacity,), -1, dtype=torch.int64, device=DEV)
    L.call("rs_pair_set_build", L.ptr(s), L.ptr(d), src.size, L.ptr(table), capacity, stream())
    return table


def test_exclusion_set_at_high_load():
    """pair_set_build_kernel / pair_set_has at load 0.88 (1000 pairs with duplicates and skipped
    (-1, ·), (·, -1) entries into 1024 slots): probe chains past 8, a chain that wraps from the
    last slot to slot 0, look-ups of absent pairs whose home slot is taken. The table holds the
    expected keys in the expected slots' set; the neighbours equal the oracle's exclude= result
    and the result with capacity 65 536."""
    c = P.excl_case()
    table = build_pair_set(c["src"], c["dst"], P.EXCL_CAP)
    wide = build_pair_set(c["src"], c["dst"], P.EXCL_WIDE)
    got = table.cpu().numpy().view(np.uint64)
    empty = np.uint64(2 ** 64 - 1)
    want, _ = P.probe_insert(c["src"], c["dst"], P.EXCL_CAP)
    assert np.array_equal(np.sort(got[got != empty]), c["keys"]), "the table's keys"
    assert np.array_equal(got != empty, want != empty), "the occupied slots"
    nw, T, p, k = P.EXCL_WALK
    smp = sampler("limit", nw, T, p, k, seed=P.EXCL_SEED)
    seeds = dev(c["seeds"])
    en, ec = O.pinsage_neighbors(P.oracle_graph("limit"), c["seeds"], nw, T, p, k, P.EXCL_SEED, 0, 0,
                                 exclude=c["exclude"])
    for t, cap in ((table, P.EXCL_CAP), (wide, P.EXCL_WIDE)):
        nbr, cnt = smp.neighbors(seeds, layer=0, excl=(t, cap), step=0)
        same_ints(nbr, en, f"neighbours, capacity {cap}")
        same_ints(cnt, ec, f"counts, capacity {cap}")
    nbr, cnt = smp.neighbors(seeds, layer=0, step=0)
    same_ints(nbr, c["unfiltered"][0], "neighbours without the set")


def test_pair_set_capacities_rejected():
    """capacity == n and a capacity that is no power of two are rejected; the table is untouched."""
    c = P.excl_case()
    src, dst = dev(np.resize(c["src"], 1024)), dev(np.resize(c["dst"], 1024))
    for n, cap in ((1024, 1024), (1000, 1000), (1000, 1536)):
        table = torch.full((2048,), -1, dtype=torch.int64, device=DEV)
        with pytest.raises(L.RecsysError):
            L.call("rs_pair_set_build", L.ptr(src), L.ptr(dst), n, L.ptr(table), cap, stream())
        assert bool((table == -1).all())


# =============================================================================================
# unique / block
@pytest.mark.parametrize("name", P.UNIQUE_CASES)
def test_unique_first_edges(name):
    """rs_unique_first's positions from exclusive_scan_i32 at its 4096-element tile: n 4095, 4096,
    4097, 8193 with first appearances at index n - 1 and at 4096; all ids -1 (count 0), all ids
    equal, ids at both ends of a 3 000 000-node space, n = 0."""
    ids, n_nodes = P.unique_inputs(name)
    smp = stub_sampler(n_nodes)
    uniq, local, nu = smp.unique_first(dev(ids), n_nodes)
    ru, rl = O.unique_first(ids)
    assert int(nu.item()) == ru.size
    same_ints(uniq[:ru.size], ru, "uniq")
    same_ints(local, rl, "local")
    assert int(smp.err_flag.item()) == 0


def check_block(b, rb):
    E = int(b.n_edges.item())
    assert b.n_dst == rb.n_dst and b.n_src == rb.n_src and E == rb.edge_src.size
    same_ints(b.src_nodes, rb.src_nodes, "src_nodes")
    same_ints(b.indptr, rb.indptr, "indptr")
    same_ints(b.edge_src[:E], rb.edge_src, "edge_src")
    same_ints(b.edge_dst[:E], rb.edge_dst, "edge_dst")
    same_ints(b.edge_w[:E], rb.edge_w, "edge_w")
    same_ints(b.t_indptr, rb.t_indptr, "t_indptr")
    same_ints(b.t_edge[:E], rb.t_edge, "t_edge")


def device_block(dst, nbr, cnt, n_items):
    return stub_sampler(n_items, nbr.shape[1]).to_block(dev(dst), dev(nbr), dev(cnt))


@pytest.mark.parametrize("n_dst,k,kind", P.BLOCK_CASES)
def test_block_edges(n_dst, k, kind):
    """rs_pinsage_block through to_block: capacity n_dst · k at 4095 / 4096 / 4097 (the scan tile
    under epos), k 1 and 32, every slot -1 (n_edges 0, indptr and t_indptr all 0), every slot
    live, a source in every destination's list (one transpose row of n_dst edges, the
    destinations' own rows mostly unused), counts up to 512, n_dst = 0."""
    dst, nbr, cnt = P.block_inputs(n_dst, k, kind)
    check_block(device_block(dst, nbr, cnt, P.BLOCK_NODES), O.to_block(dst, nbr, cnt))


# =============================================================================================
# weighted mean pooling
@functools.lru_cache(maxsize=None)
def agg_device_block():
    return device_block(*P.agg_block_inputs(), P.AGG_NODES)


def run_agg(b, u, g):
    H = u.shape[1]
    ut, gt = dev(u), dev(g)
    nv, ws, gu = sent_buf(b.n_dst * H + TAIL), sent_buf(b.n_dst + TAIL), sent_buf(b.n_src * H + TAIL)
    L.call("rs_weighted_mean_agg_fwd", L.ptr(ut), b.n_src, H, L.ptr(b.indptr), L.ptr(b.edge_src),
           L.ptr(b.edge_w), b.n_dst, L.ptr(nv), L.ptr(ws), stream())
    L.call("rs_weighted_mean_agg_bwd", L.ptr(gt), H, L.ptr(b.t_indptr), L.ptr(b.t_edge),
           L.ptr(b.edge_dst), L.ptr(b.edge_w), L.ptr(ws), b.n_src, L.ptr(gu), stream())
    torch.cuda.synchronize()
    assert is_sent(nv[b.n_dst * H:]) and is_sent(ws[b.n_dst:]) and is_sent(gu[b.n_src * H:]), \
        "an output was written past its end"
    return dict(nv=nv[:b.n_dst * H].view(b.n_dst, H).cpu().numpy(), wsum=ws[:b.n_dst].cpu().numpy(),
                gu=gu[:b.n_src * H].view(b.n_src, H).cpu().numpy())


@pytest.mark.parametrize("H", P.AGG_H)
def test_weighted_mean_agg_edges(H):
    """agg_fwd_kernel's 4-at-a-time edge loop (destination in-degrees 0, 1, 3, 4, 5, 7, 8, 9: no,
    one and two passes with every tail) and agg_bwd_kernel's 8-at-a-time loop (source in-degrees
    0, 1, 7, 8, 9, 15, 16, 17 and a hub of 1050), H 1, 5, 64, 70, weights up to 512; a destination
    without in-edges gives exact zeros and wsum 0."""
    b, rb = agg_device_block(), P.agg_block()
    check_block(b, rb)
    u, g = P.agg_values(H, rb.n_src)
    r = P.agg_ref(u, g, rb)
    got = twice(run_agg, b, u, g)
    P.within(got["nv"], r["nv"], P.RTOL * r["nv_mag"], f"agg H {H} nv")
    P.within(got["gu"], r["gu"], P.RTOL * r["gu_mag"], f"agg H {H} gu")
    same_bits(got["wsum"], r["wsum"], "wsum (sums of integers)")
    none = np.diff(rb.indptr) == 0
    assert none.any() and not P.bits(got["nv"][none]).any() and not P.bits(got["wsum"][none]).any()
    assert not P.bits(got["gu"][:rb.n_dst]).any()  # the destinations' own rows: no in-edge


# =============================================================================================
# Frobenius
def run_frob(x, dy, n_rows=None):
    """The flat entry points on 1-D x / dy, or (n_rows given) the rows form on 2-D ones."""
    xt, dyt = dev(x), dev(dy)
    n = x.size
    y, dx, norm = sent_buf(n + TAIL), sent_buf(n + TAIL), sent_buf(1 + TAIL)
    ws = L.scratch(L.lib().rs_frobenius_workspace_size(n), xt.device)
    if n_rows is None:
        L.call("rs_frobenius_normalize_fwd", L.ptr(xt), n, L.ptr(y), L.ptr(norm), L.ptr(ws), ws.numel(),
               stream())
        L.call("rs_frobenius_normalize_bwd", L.ptr(dyt), L.ptr(y), L.ptr(norm), n, L.ptr(dx), L.ptr(ws),
               ws.numel(), stream())
    else:
        live = torch.tensor([n_rows], dtype=torch.int32, device=DEV)
        L.call("rs_frobenius_normalize_rows_fwd", L.ptr(xt), x.shape[0], x.shape[1], L.ptr(live),
               L.ptr(y), L.ptr(norm), L.ptr(ws), ws.numel(), stream())
        L.call("rs_frobenius_normalize_rows_bwd", L.ptr(dyt), L.ptr(y), L.ptr(norm), x.shape[0],
               x.shape[1], L.ptr(live), L.ptr(dx), L.ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    assert is_sent(y[n:]) and is_sent(dx[n:]) and is_sent(norm[1:]), "an output was written past its end"
    return dict(y=y[:n].cpu().numpy().reshape(x.shape), dx=dx[:n].cpu().numpy().reshape(x.shape),
                norm=norm[:1].cpu().numpy())


@pytest.mark.parametrize("n", P.FROB_N)
def test_frobenius_flat_edges(n):
    """dot_partial_kernel / fold_partial_kernel at the 4096-element chunk edge (n 4095, 4096, 4097)
    and with 256, 257 and 513 chunks (n 1 048 576, 1 048 577, 2 097 157: the fold's i += 256 loop
    runs once, twice, three times); norm and y within 1e-5 relative of float64, dx within
    1e-5 · (|dy| + |y| Σ|dy·y|) / norm."""
    x, dy = P.frob_inputs(n)
    r = P.frob_ref(x, dy)
    got = twice(run_frob, x, dy)
    P.within(got["norm"], [r["norm"]], P.RTOL * r["norm"], f"frob n {n} norm")
    P.within(got["y"], r["y"], P.RTOL * r["y"], f"frob n {n} y")
    P.within(got["dx"], r["dx"], r["dx_bound"], f"frob n {n} dx")


@pytest.mark.parametrize("n,norm", [(4096, 64.0), (1_048_576, 1024.0)])
def test_frobenius_known_answers(n, norm):
    """x ≡ 1: every partial sum is an integer below 2^24, so norm is sqrt(n) and y is 1 / sqrt(n)
    exactly; a dropped or double-counted chunk changes them."""
    x = np.ones(n, np.float32)
    got = run_frob(x, x)
    same_bits(got["norm"], np.array([norm], np.float32), "norm")
    same_bits(got["y"], np.full(n, 1.0 / norm, np.float32), "y")


@pytest.mark.parametrize("which", P.FROB_ROWS_LIVE)
@pytest.mark.parametrize("cap,row_len", P.FROB_ROWS)
def test_frobenius_rows_edges(cap, row_len, which):
    """The rows form's live_len at n_rows 0, 1, the capacity and past it (clamped): padding rows of
    x and dy hold NaN, none reaches norm, y or dx; padding outputs are exactly 0; the live part
    equals the flat call bit for bit; n_rows 0 gives all-zero y and dx."""
    n_rows = P.frob_rows_live(cap, which)
    m = min(n_rows, cap)
    x, dy = (a.reshape(cap, row_len).copy() for a in P.frob_inputs(cap * row_len))
    x[m:], dy[m:] = np.nan, np.nan
    got = twice(run_frob, x, dy, n_rows=n_rows)
    assert not P.bits(got["y"][m:]).any() and not P.bits(got["dx"][m:]).any(), "padding rows not +0"
    for k in ("y", "dx", "norm"):
        assert not np.isnan(got[k]).any(), f"a NaN of the padding reached {k}"
    if m == 0:
        assert not P.bits(got["norm"]).any()
        return
    flat = run_frob(x[:m].reshape(-1), dy[:m].reshape(-1))
    same_bits(got["norm"], flat["norm"], "norm vs the flat call")
    same_bits(got["y"][:m].reshape(-1), flat["y"], "y vs the flat call")
    same_bits(got["dx"][:m].reshape(-1), flat["dx"], "dx vs the flat call")


def test_frobenius_all_zero_live_rows_match_the_reference():
    """All-zero live rows: norm 0 and y = 0 / 0 = NaN on the live rows, which is what the reference
    x / torch.norm(x) gives. This pins parity with the reference, not a wish; padding stays 0."""
    cap, row_len, m = 257, 64, 200
    x = np.zeros((cap, row_len), np.float32)
    x[m:] = np.nan
    got = run_frob(x, np.ones_like(x), n_rows=m)
    xt = torch.zeros(m, row_len, device=DEV)
    ref = (xt / torch.norm(xt)).cpu().numpy()
    assert np.isnan(ref).all() and np.array_equal(np.isnan(got["y"][:m]), np.isnan(ref))
    assert not P.bits(got["norm"]).any() and not P.bits(got["y"][m:]).any()


# =============================================================================================
# pair margin
def run_pair(c, D, dloss=0.5, n_rows=P.PAIR_ROWS):
    h = dev(c["h"])
    npairs = c["ps"].size
    idx = [dev(c[k]) for k in ("ps", "pd", "ns", "nd")]
    valid = None if c["valid"] is None else dev(c["valid"])
    n_live = None if c["n_live"] is None else torch.tensor([c["n_live"]], dtype=torch.int32, device=DEV)
    pos, neg = sent_buf(npairs + TAIL), sent_buf(npairs + TAIL)
    loss, dh = sent_buf(1 + TAIL), sent_buf(n_rows * D + TAIL)
    flag = torch.tensor([0, SENT_I], dtype=torch.int32, device=DEV)
    wf = L.scratch(L.lib().rs_pair_margin_workspace_size(npairs), h.device)
    wb = L.scratch(L.lib().rs_pair_margin_bwd_workspace_size(npairs, D), h.device)
    dl = torch.tensor([dloss], dtype=torch.float32, device=DEV)
    L.call("rs_pair_margin_fwd", L.ptr(h), h.shape[1], D, n_rows, *(L.ptr(t) for t in idx), npairs,
           P.PAIR_DELTA, L.ptr(valid), L.ptr(n_live), L.ptr(pos), L.ptr(neg), L.ptr(loss),
           L.ptr(flag), L.ptr(wf), wf.numel(), stream())
    L.call("rs_pair_margin_bwd", L.ptr(h), h.shape[1], D, n_rows, *(L.ptr(t) for t in idx), npairs,
           P.PAIR_DELTA, L.ptr(valid), L.ptr(n_live), L.ptr(pos), L.ptr(neg), L.ptr(dl), L.ptr(dh),
           L.ptr(flag), L.ptr(wb), wb.numel(), stream())
    torch.cuda.synchronize()
    assert is_sent(pos[npairs:]) and is_sent(neg[npairs:]) and is_sent(loss[1:]) and \
        is_sent(dh[n_rows * D:]), "an output was written past its end"
    assert int(flag[1]) == SENT_I, "the word behind the error flag was written"
    return dict(pos=pos[:npairs].cpu().numpy(), neg=neg[:npairs].cpu().numpy(),
                loss=loss[:1].cpu().numpy(), dh=dh[:n_rows * D].view(n_rows, D).cpu().numpy(),
                flag=np.array(int(flag[0])))


def check_pair(got, r, msg):
    P.within(got["pos"], r["pos"], P.RTOL * r["pos_mag"], f"{msg} pos")
    P.within(got["neg"], r["neg"], P.RTOL * r["neg_mag"], f"{msg} neg")
    P.within(got["loss"], [r["loss"]], P.RTOL * r["loss"], f"{msg} loss")
    P.within(got["dh"], r["dh"], P.RTOL * r["dh_mag"], f"{msg} dh")


@pytest.mark.parametrize("D,npairs,ld_extra,padding", P.PAIR_CASES)
def test_pair_margin_edges(D, npairs, ld_extra, padding):
    """rs_pair_margin_fwd / _bwd through the C ABI: D 1, 16, 63 and the limit 64; P 1, 255, 256,
    257, 1000 (the 256-pair block edge); ld = D and D + 3 with NaN in the pad columns; all
    positives onto 8 nodes; padding pairs with and without valid / n_live. Pair 0's
    (neg + delta) - pos is exactly 0 in fp32 and must carry gradient (the backward's >= 0 rule);
    pair 1 is one ulp below 0 and must carry none."""
    c = P.pair_inputs(D, npairs, ld_extra, padding)
    r = P.pair_ref(c, D, dloss=0.5)
    got = twice(run_pair, c, D)
    assert int(got["flag"]) == 0
    check_pair(got, r, f"pair D {D} P {npairs} ld+{ld_extra} {padding}")
    g = np.float32(0.5) / np.float32(npairs if c["n_live"] is None else c["n_live"])
    same_bits(got["dh"][P.PAIR_R2, :1], np.array([-g], np.float32), "the hinge exactly at 0 carries -g")
    if npairs >= 2:
        assert not got["dh"][P.PAIR_R2UP].any(), "the hinge one ulp below 0 carries gradient"


def test_pair_margin_without_a_live_pair_matches_margin_loss():
    """All pairs invalid, n_live 0: the loss and the gradient equal what margin_loss over
    item2item_scorer gives for the same inputs: the loss 0 / 0 = NaN, and node 0 (which every
    padding pair scores, with an active hinge of delta) takes 0 · inf = NaN, every other row 0.
    This pins parity with the reference path, not a wish."""
    from recommender_amd.pinsage.model import item2item_scorer, margin_loss

    D, npairs = 16, 255
    c = P.pair_inputs(D, npairs, 0, "none")
    for k in ("ps", "pd", "ns", "nd"):
        c[k][:] = -1
    c["valid"], c["n_live"] = np.zeros(npairs, np.uint8), 0
    got = run_pair(c, D, dloss=1.0)
    h = dev(c["h"]).requires_grad_()
    pad = dev(c["ps"])
    valid, nv = torch.zeros(npairs, dtype=torch.bool, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    pg, ng = (PairGraph(pad, pad, torch.arange(P.PAIR_ROWS, device=DEV), valid, nv) for _ in range(2))
    ref = margin_loss(item2item_scorer(pg, h), item2item_scorer(ng, h), P.PAIR_DELTA, valid, nv)
    ref.backward()
    ref_dh = h.grad.cpu().numpy()
    print(f"  loss got {got['loss'][0]!r} ref {float(ref.detach())!r}; dh[0, 0] got {got['dh'][0, 0]!r} "
          f"ref {ref_dh[0, 0]!r}; dh[1:] any got {bool(got['dh'][1:].any())} ref {bool(ref_dh[1:].any())}")
    assert np.isnan(got["loss"][0]) and np.isnan(float(ref.detach()))
    assert np.array_equal(np.isnan(got["dh"]), np.isnan(ref_dh)), "NaN rows differ from margin_loss's"
    assert np.array_equal(np.nan_to_num(got["dh"]), np.nan_to_num(ref_dh))


def test_pair_margin_rejects_d_65():
    c = P.pair_inputs(64, 255, 3, "none")
    with pytest.raises(L.RecsysError):
        run_pair(c, 65)


def test_pair_margin_endpoint_out_of_range():
    """An endpoint >= n_rows reads a zero row, takes no gradient and flags RS_ERRBIT_OOB; the other
    pairs' scores keep their bits."""
    D, npairs = 16, 257
    c = P.pair_inputs(D, npairs, 3, "none")
    clean = run_pair(c, D)
    c["nd"][9] = P.PAIR_ROWS + 5
    got = twice(run_pair, c, D)
    r = P.pair_ref(c, D, dloss=0.5)
    assert r["oob"] and int(got["flag"]) & L.RS_ERRBIT_OOB and int(clean["flag"]) == 0
    keep = np.arange(npairs) != 9
    same_bits(got["pos"], clean["pos"], "pos")
    same_bits(got["neg"][keep], clean["neg"][keep], "neg of the other pairs")
    assert P.bits(got["neg"][9:10])[0] == 0, "the score of the zero row is not +0"
    check_pair(got, r, "pair with an endpoint out of range")


# =============================================================================================
# multi-hot mean
def run_multihot(table, mh, items, dout):
    V, D = table.shape
    G, N = mh.shape[1], items.size
    t, m, it, do = dev(table), dev(mh), dev(items), dev(dout)
    out, dt = sent_buf(N * D + TAIL), sent_buf(V * D + TAIL)
    flag = torch.tensor([0, SENT_I], dtype=torch.int32, device=DEV)
    L.call("rs_multihot_mean_fwd", L.ptr(t), V, D, L.ptr(m), G, mh.shape[0], L.ptr(it), N, L.ptr(out),
           L.ptr(flag), stream())
    ws = L.scratch(L.lib().rs_multihot_mean_bwd_workspace_size(N, V, D), t.device)
    L.call("rs_multihot_mean_bwd", L.ptr(m), G, mh.shape[0], L.ptr(it), N, L.ptr(do), V, D, L.ptr(dt),
           L.ptr(flag), L.ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    assert is_sent(out[N * D:]) and is_sent(dt[V * D:]), "an output was written past its end"
    assert int(flag[1]) == SENT_I, "the word behind the error flag was written"
    return dict(out=out[:N * D].view(N, D).cpu().numpy(), dtable=dt[:V * D].view(V, D).cpu().numpy(),
                flag=np.array(int(flag[0])))


def check_multihot(got, r, msg):
    P.within(got["out"], r["out"], P.RTOL * r["out_mag"], f"{msg} out")
    P.within(got["dtable"], r["dtable"], P.RTOL * r["dtable_mag"], f"{msg} dtable")


@pytest.mark.parametrize("V,D,G,N", P.MH_CASES)
def test_multihot_mean_edges(V, D, G, N):
    """rs_multihot_mean_fwd / _bwd at V·D 1 and 256 (both ways), D 64, G 1, 20 and the limit 32,
    N 1, 31, 32, 33 (the 32-item block) and 8193 (257 partial blocks: the strided loop of
    multihot_mean_bwd_fold_kernel); repeated items, an id row naming one table row G times."""
    table, mh, items, dout = P.multihot_inputs(V, D, G, N)
    got = twice(run_multihot, table, mh, items, dout)
    assert int(got["flag"]) == 0
    check_multihot(got, P.multihot_ref(table, mh, items, dout), f"multihot V {V} D {D} G {G} N {N}")


@pytest.mark.parametrize("V,D,G,N", [P.MH_CASES[3], P.MH_CASES[5]])
@pytest.mark.parametrize("what", ["item_high", "item_negative", "id_high", "id_negative"])
def test_multihot_mean_out_of_range(V, D, G, N, what):
    """An item outside [0, n_items) and an id outside [0, V): zero contribution, RS_ERRBIT_OOB,
    every other output row unchanged in bits."""
    table, mh, items, dout = P.multihot_inputs(V, D, G, N)
    clean = run_multihot(table, mh, items, dout)
    if what.startswith("item"):
        items[0] = P.MH_ITEMS + 3 if what == "item_high" else -1
        touched = np.arange(N) == 0
    else:
        mh[P.MH_SAME_ROW, G - 1] = V if what == "id_high" else -1
        touched = items == P.MH_SAME_ROW
    got = twice(run_multihot, table, mh, items, dout)
    r = P.multihot_ref(table, mh, items, dout)
    assert r["oob"] and int(got["flag"]) & L.RS_ERRBIT_OOB and int(clean["flag"]) == 0
    same_bits(got["out"][~touched], clean["out"][~touched], "the other rows")
    if what.startswith("item"):
        assert not P.bits(got["out"][0]).any(), "the row of the item out of range is not +0"
    check_multihot(got, r, f"multihot {what}")


@pytest.mark.parametrize("V,D,G", P.MH_REJECTED)
def test_multihot_mean_bwd_rejects_past_the_limits(V, D, G):
    mh = dev(np.zeros((P.MH_ITEMS, G), np.int32))
    items, dout = dev(np.zeros(4, np.int64)), dev(np.zeros((4, D), np.float32))
    dt = sent_buf(V * D)
    ws = L.scratch(1 << 20, mh.device)
    with pytest.raises(L.RecsysError):
        L.call("rs_multihot_mean_bwd", L.ptr(mh), G, P.MH_ITEMS, L.ptr(items), 4, L.ptr(dout), V, D,
               L.ptr(dt), None, L.ptr(ws), ws.numel(), stream())
    assert is_sent(dt)
