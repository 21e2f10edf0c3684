"""The inputs of tests/test_eges_edges_gpu.py have the property their name claims, the float64
restatements of tests/eges_edges.py agree with torch float64 autograd, a plain fp32 NumPy
evaluation (in two summation orders) meets every bound at a quarter of the tolerance, and three
deliberately wrong references are caught — all without a GPU."""
import numpy as np
import pytest
import torch

from oracle import eges as O
from oracle.pinsage import draw
from tests import eges_edges as E

QUARTER = 0.25


# =============================================================================================
# 1. match logits
def test_match_cases_cover_the_lists():
    c = E.MATCH_CASES
    assert 18 <= len(c) <= 24
    assert {x[0] for x in c} == set(E.MATCH_D) and {x[2] for x in c} == set(E.MATCH_B)
    assert {(x[1], x[3]) for x in c} == {(m, i) for m in E.MATCH_M for i in (False, True)}
    for D in E.MATCH_D:
        assert {x[4] for x in c if x[0] == D} == set(E.MATCH_KINDS)
    # the lane-stride loop: zero, one and two full passes, and ragged ones
    assert {-(-D // E.WAVE) for D in E.MATCH_D} == {1, 2, 3} and 64 in E.MATCH_D and 128 in E.MATCH_D
    # an empty wave in the last block for every B but 4
    assert {B % E.WAVES_PER_BLOCK for B in E.MATCH_B} == {0, 1, 3}


@pytest.mark.parametrize("D,M,B,id64,kind", E.MATCH_CASES)
def test_match_inputs_and_fp32_reference(D, M, B, id64, kind):
    table, ids, hidden, g = E.match_inputs(D, M, B, kind)
    r = E.match_ref(table, ids, hidden, g)
    assert r["valid"].all() and ids.shape == (B, M)
    if kind == "cancel":
        # the bound is what is tested, not |ref|: the terms cancel (exactly, for even D)
        if D % 2 == 0:
            assert np.abs(r["logits"]).max() <= 1e-12 * r["logits_mag"].max()
        elif D > 1:
            assert (np.abs(r["logits"]) < (1.5 / (D // 2 + 1)) * r["logits_mag"]).all() or D <= 3
        assert (r["logits_mag"] > 0).all()
    if kind == "same_row":
        assert (ids[B - 1] == ids[B - 1, 0]).all()
    for order in E.SUMS32:
        lg, gh = E.match_f32(table, ids, hidden, g, order)
        E.within(lg, r["logits"], E.RTOL * r["logits_mag"], f"{order} logits", QUARTER)
        E.within(gh, r["grad_hidden"], E.RTOL * r["grad_hidden_mag"], f"{order} grad_hidden", QUARTER)


@pytest.mark.parametrize("D,M,B,id64,kind", [c for c in E.MATCH_CASES if c[4] == "gauss"])
def test_match_ref_equals_torch_float64_autograd(D, M, B, id64, kind):
    table, ids, hidden, g = E.match_inputs(D, M, B, kind)
    r = E.match_ref(table, ids, hidden, g)
    w = torch.from_numpy(table).double().requires_grad_()
    h = torch.from_numpy(hidden).double().requires_grad_()
    rows = w[torch.from_numpy(ids)]
    rows.retain_grad()
    out = torch.einsum("bmd,bd->bm", rows, h)
    out.backward(torch.from_numpy(g).double())
    assert np.abs(out.detach().numpy() - r["logits"]).max() <= 1e-13 * r["logits_mag"].max()
    assert np.abs(h.grad.numpy() - r["grad_hidden"]).max() <= 1e-13 * r["grad_hidden_mag"].max()
    # grad_rows is the one fp32 product g·h: the float64 product rounded once
    assert np.array_equal(E.bits(r["grad_rows32"]), E.bits(rows.grad.numpy().astype(np.float32)))


def test_oob_values():
    vals = dict((n, (v, w)) for n, v, w in E.oob_values())
    assert vals["minus_one"][0] == -1 and vals["n_rows"][0] == E.MATCH_ROWS
    v = np.array([vals["2^32+1"][0], vals["int64_min"][0]], np.int64)
    assert v[0] == 2 ** 32 + 1 and v[1] == np.iinfo(np.int64).min
    # their low 32-bit words are valid rows: a kernel that truncated would read rows 1 and 0
    assert (v.view(np.uint32)[::2] == [1, 0]).all()
    assert not vals["minus_one"][1] and not vals["n_rows"][1]
    table, ids, hidden, g = E.match_inputs(65, 6, 5, "gauss")
    assert np.abs(table[:2] @ hidden.T).min() > 0  # an aliased read gives a non-zero logit
    for _, (val, _) in vals.items():
        bad = ids.copy()
        bad[2, 3] = val
        r, good = E.match_ref(table, bad, hidden, g), E.match_ref(table, ids, hidden, g)
        assert r["logits"][2, 3] == 0.0 and not r["valid"][2, 3] and r["valid"].sum() == ids.size - 1
        mask = np.ones_like(ids, bool)
        mask[2, 3] = False
        assert np.array_equal(r["logits"][mask], good["logits"][mask])
        assert np.array_equal(r["grad_hidden"][[0, 1, 3, 4]], good["grad_hidden"][[0, 1, 3, 4]])
        assert not np.array_equal(r["grad_hidden"][2], good["grad_hidden"][2])


# =============================================================================================
# 2. side pooling
def test_pool_cases_cover_the_lists():
    for cases, ds in ((E.POOL_SCALAR_CASES, E.POOL_SCALAR_D), (E.POOL_VECTOR_CASES, E.POOL_VECTOR_D)):
        for D in ds:
            mine = [c for c in cases if c[0] == D]
            assert {c[3] for c in mine} == set(E.POOL_MODES)
            assert {c[1] for c in mine} == set(E.POOL_B) and {c[2] for c in mine} == set(E.POOL_S)
        for mode in E.POOL_MODES:  # every mode meets an odd batch (an empty upper half-wave)
            assert any(c[1] % 2 == 1 and c[1] > 1 for c in cases if c[3] == mode)
    assert all(D % 4 == 0 and D <= 128 for D in E.POOL_VECTOR_D)
    assert all(D % 4 != 0 or D > 128 for D in E.POOL_SCALAR_D)
    assert max(E.POOL_S) == E.MAX_SIDE


def test_pool_routing_contract():
    for D in E.POOL_VECTOR_D:
        for layout in E.LAYOUTS:
            sb, ss, n = E.layout_strides(layout, 7, 3, D)
            assert E.pool_route(D, 3, sb, ss) == "vector"
            assert n >= 6 * sb + 2 * ss + D
        assert E.pool_route(D, 3, 3 * D, D, offsets=(1, 0)) == "scalar"   # one float off, dense
        assert E.pool_route(D, 3, 3 * D + 8, D + 4, offsets=(1, 0)) == "rejected"
        assert E.pool_route(D, 3, 3 * D + 6, D + 2) == "rejected"         # strides not 4k
    for D in E.POOL_SCALAR_D:
        assert E.pool_route(D, 3, 3 * D, D) == "scalar"
        sb, ss, _ = E.layout_strides("padded", 7, 3, D)
        assert E.pool_route(D, 3, sb, ss) == "rejected"
        if 7 > 1:
            sb, ss, _ = E.layout_strides("ebh", 7, 3, D)
            assert E.pool_route(D, 3, sb, ss) == "rejected"
    # padded: ss = D + 4, sb = S·ss + 8
    assert E.layout_strides("padded", 2, 3, 8) == (3 * 12 + 8, 12, 2 * 44)


@pytest.mark.parametrize("S", E.POOL_S)
def test_logit_sets_have_their_property_in_fp32(S):
    B = 9
    rng = np.random.default_rng(S)
    r = np.arange(B)
    w = E.pool_logits("equal", B, S, rng)
    a = E.softmax32(w)
    assert (w == w[:, :1]).all() and (a == a[:, :1]).all()
    assert np.abs(a.astype(np.float64) - 1.0 / S).max() <= 2 * E.U32 * S / S
    w = E.pool_logits("spread60", B, S, rng)
    a = E.softmax32(w)
    assert (a[r, (r + 1) % S] == 1.0).all(), "the +60 weight does not saturate"
    assert a.sum() == B and ((a == 0) | (a == 1)).all(), "a -60 weight does not underflow to 0"
    assert np.float32(np.exp(np.float32(-120.0))) == 0.0
    w = E.pool_logits("offset1e4", B, S, rng)
    assert (w > 9990).all() and (S == 1 or (np.ptp(w, 1) > 0).all())
    assert np.isfinite(E.softmax32(w)).all()
    assert np.isnan(E.softmax32(w, subtract_max=False)).all(), "finite without the max subtraction"
    w = E.pool_logits("neg1e30", B, S, rng)
    a = E.softmax32(w)
    assert np.isfinite(a).all()
    if S >= 2:
        assert (w[r, r % S] == E.NEG_BIG).all() and (a[r, r % S] == 0.0).all()
        assert ((w == E.NEG_BIG).sum(1) == 1).all()
        assert (E.softmax64(w)[r, r % S] == 0.0).all()
    else:
        assert (a == 1.0).all()
    w = E.pool_logits("gauss", B, S, rng)
    assert S == 1 or (E.softmax32(w) > 0).all()


SOFTMAX_CASES = [c for c in E.POOL_SCALAR_CASES + E.POOL_VECTOR_CASES if c[3] != "mean"]


@pytest.mark.parametrize("D,B,S,mode", SOFTMAX_CASES)
def test_pool_fp32_reference_meets_the_bounds_at_a_quarter(D, B, S, mode):
    side, wl, g = E.pool_inputs(D, B, S, mode)
    fwd = E.pool_fwd_ref(side, wl)
    bwd = E.pool_bwd_ref(side, fwd["attn32"], g)
    assert np.isfinite(fwd["hidden"]).all() and np.isfinite(bwd["grad_w"]).all()
    for order in E.SUMS32:
        s = E.pool_f32(side, wl, g, order, attn32=fwd["attn32"])
        E.pool_check_fwd(s["attn"], s["hidden"], fwd, f"{order}", QUARTER)
        E.pool_check_bwd(s["grad_side"], s["grad_w"], bwd, f"{order}", QUARTER)
    if mode == "neg1e30" and S >= 2:
        r = np.arange(B)
        assert (fwd["attn32"][r, r % S] == 0).all() and (bwd["grad_w"][r, r % S] == 0).all()
        assert (bwd["grad_side"][r, r % S] == 0).all()


@pytest.mark.parametrize("D,B,S,mode", [c for c in SOFTMAX_CASES if c[3] == "gauss"] +
                         [c for c in E.POOL_SCALAR_CASES + E.POOL_VECTOR_CASES if c[3] == "mean"])
def test_pool_ref_equals_torch_float64_autograd(D, B, S, mode):
    side, wl, g = E.pool_inputs(D, B, S, mode)
    x = torch.from_numpy(side).double().requires_grad_()
    gt = torch.from_numpy(g).double()
    fwd = E.pool_fwd_ref(side, wl)
    if mode == "mean":
        out = x.sum(1) / S
        out.backward(gt)
        bwd = E.pool_bwd_ref(side, None, g)
        mag = np.abs(side.astype(np.float64)).sum(1) / S
        # the fp32 evaluation the kernels are held to, bit for bit, is itself within S + 1
        # roundings of float64
        assert (np.abs(fwd["hidden32"] - out.detach().numpy()) <= (S + 1) * E.U32 * mag).all()
        assert (np.abs(bwd["grad_side32"] - x.grad.numpy()) <= E.U32 * np.abs(x.grad.numpy())).all()
        return
    w = torch.from_numpy(wl).double().requires_grad_()
    a = torch.softmax(w, -1)
    out = torch.einsum("bs,bsd->bd", a, x)
    out.backward(gt)
    assert np.abs(a.detach().numpy() - fwd["attn"]).max() <= 1e-15
    assert (np.abs(out.detach().numpy() - fwd["hidden"]) <= 1e-13 * fwd["hidden_mag"] + 1e-300).all()
    # the backward restatement takes the float32 weights (the kernel's input): 2^-24 apart
    bwd = E.pool_bwd_ref(side, fwd["attn32"], g)
    assert (np.abs(x.grad.numpy() - bwd["grad_side"]) <= 2 * E.U32 * bwd["grad_side_mag"]).all()
    assert (np.abs(w.grad.numpy() - bwd["grad_w"]) <= 4 * E.U32 * bwd["grad_w_mag"]).all()


def _caught(**wrong):
    """The softmax cases whose bounds the deliberately wrong fp32 evaluation misses."""
    hits = []
    for D, B, S, mode in SOFTMAX_CASES:
        side, wl, g = E.pool_inputs(D, B, S, mode)
        fwd = E.pool_fwd_ref(side, wl)
        s = E.pool_f32(side, wl, g, "sequential", attn32=fwd["attn32"], **wrong)
        q = max(E.off_by(s["attn"], fwd["attn"], E.attn_bound(fwd["attn"])),
                E.off_by(s["hidden"], fwd["hidden"], E.hidden_bound(fwd)))
        if q > 1.0:
            hits.append((D, B, S, mode))
    return hits


def test_wrong_references_are_caught():
    no_max = _caught(subtract_max=False)
    assert {c[3] for c in no_max} >= {"offset1e4"}, "a softmax without max subtraction passes"
    assert all(c in no_max for c in SOFTMAX_CASES if c[3] == "offset1e4")
    shifted = _caught(shift=1)
    assert any(c[3] == "gauss" for c in shifted), "weights shifted by one side pass"
    assert all(c in shifted for c in SOFTMAX_CASES if c[3] in ("gauss", "spread60") and c[2] > 1)
    odd = _caught(off_by_one=True)
    assert odd and all(c[1] % 2 == 1 and c[1] > 1 for c in odd), "an index off by one passes"
    assert {c for c in SOFTMAX_CASES if c[1] in (3, 7, 9) and c[3] == "gauss"} <= set(odd)
    assert _caught() == []


def test_multi_cases_and_bias_inputs():
    c = E.MULTI_CASES
    assert len(c) == 9
    for k, vals in enumerate((E.MULTI_T, E.MULTI_E, E.MULTI_H, E.MULTI_B)):
        assert {x[k] for x in c} == set(vals)
    assert max(E.MULTI_T) == E.MAX_TASKS and max(E.MULTI_E) == E.MAX_SIDE
    assert all(H % 4 == 0 and H <= 128 for H in E.MULTI_H)
    for T, Ex, H, B, kind in c:
        z, wl, g, bias = E.multi_inputs(T, Ex, H, B, kind, with_bias=True)
        assert z.shape == (B, Ex, H) and wl.shape == (T, B, Ex) and g.shape == (T, B, H)
        pre = (z + bias[None]).astype(np.float32)
        y = E.relu_bias32(z, bias)
        assert (pre[::2, ::2, 0] == 0).all() and (pre == 0).sum() >= (B + 1) // 2
        assert (z < 0).any() and (pre < 0).any() and (y[pre < 0] == 0).all()
        assert not np.signbit(y).any() and np.array_equal(y[pre > 0], pre[pre > 0])


def test_hidden_bound_floor_is_needed_only_under_float32_range():
    """relu rows under a saturated softmax: where the weight-1 side holds an exact 0, float64
    gives Σ of 8e-53-weighted values, any float32 evaluation 0: the relative bound alone (0 there
    to 1e-57) cannot hold, ATTN_FLOOR · Σ|x_s| can, and is below 1e-33 everywhere."""
    z, wl, g, b = E.multi_inputs(1, 16, 128, 7, "spread60", with_bias=True)
    side = E.relu_bias32(z, b)
    fwd = E.pool_fwd_ref(side, wl[0])
    s = E.pool_f32(side, wl[0], g[0], "sequential")
    tiny = (fwd["hidden"] > 0) & (fwd["hidden"] < 1e-45)
    assert tiny.any() and (s["hidden"][tiny] == 0).all()
    assert E.off_by(s["hidden"], fwd["hidden"], E.RTOL * fwd["hidden_mag"]) > 1e3
    E.within(s["hidden"], fwd["hidden"], E.hidden_bound(fwd), "hidden with the floor", QUARTER)
    assert (E.ATTN_FLOOR * fwd["side_abs_sum"]).max() < 1e-33
    assert (E.ATTN_FLOOR * fwd["side_abs_sum"] < 1e-25 * E.RTOL * fwd["hidden_mag"])[~tiny & (fwd["hidden"] > 0)].all()


def test_multi_grad_side_reference():
    T, Ex, H, B, kind = 4, 8, 80, 7, "gauss"
    side, wl, g, _ = E.multi_inputs(T, Ex, H, B, kind)
    x = torch.from_numpy(side).double().requires_grad_()
    total = 0
    a32 = []
    for t in range(T):
        a = torch.softmax(torch.from_numpy(wl[t]).double(), -1)
        total = total + (torch.einsum("bs,bsd->bd", a, x) * torch.from_numpy(g[t]).double()).sum()
        a32.append(E.pool_fwd_ref(side, wl[t])["attn32"])
    total.backward()
    ref, mag = E.multi_grad_side_ref(a32, list(g))
    assert (np.abs(x.grad.numpy() - ref) <= 2 * E.U32 * mag).all()
    E.within(E.multi_grad_side_sum32(a32, list(g)), ref, E.RTOL * mag, "task-ordered fp32 sum", QUARTER)


# =============================================================================================
# 3. pair sampler
@pytest.mark.parametrize("n_nodes", E.GRAPH_NODES)
def test_edge_graph_has_every_feature(n_nodes):
    g = indptr, indices, w = E.edge_graph(n_nodes)
    deg = np.diff(indptr)
    assert indptr[0] == 0 and indptr[-1] == indices.size == w.size and len(indptr) == n_nodes + 1
    assert ((indices >= 0) & (indices < n_nodes)).all() and (w >= 0).all()

    def ws(v):
        return w[indptr[v]:indptr[v + 1]]

    assert deg[E.N_OOV] == 0 and deg[E.N_EDGELESS] == 0
    assert deg[E.N_ALLZERO] == 3 and not ws(E.N_ALLZERO).any()
    assert ws(E.N_ZERO_FIRST)[0] == 0 and ws(E.N_ZERO_FIRST)[1:].all()
    assert ws(E.N_ZERO_LAST)[-1] == 0 and ws(E.N_ZERO_LAST)[:-1].all()
    assert ws(E.N_ZERO_MID)[1] == 0 and ws(E.N_ZERO_MID)[0] > 0 and ws(E.N_ZERO_MID)[2] > 0
    assert deg[E.N_SINGLE] == 1 and ws(E.N_SINGLE)[0] > 0
    assert E.N_SELF in indices[indptr[E.N_SELF]:indptr[E.N_SELF + 1]]
    assert deg[E.N_HUB] >= 1000 and (ws(E.N_HUB) == 0).sum() >= 100 and (ws(E.N_HUB) > 0).sum() >= 800
    x = ws(E.N_EXTREME)
    tiny = np.finfo(np.float32).tiny
    assert 0 < x[0] < tiny and x[1] == np.float32(1e30) and x[2] == np.float32(1e-3)
    assert (ws(E.N_DENORM) > 0).all() and (ws(E.N_DENORM) < tiny).all()
    assert (n_nodes < 256) == (n_nodes == E.GRAPH_NODES[0]) and max(E.GRAPH_NODES) > 256
    # no edge of positive weight leads to node 0: a step along a weight-0 edge shows as a 0
    assert not (w[indices == E.N_OOV] > 0).any() and (indices == E.N_OOV).sum() > 300
    for v in (E.N_OOV, E.N_EDGELESS, E.N_ALLZERO):
        assert E.dead_end(g, v)
    assert not any(E.dead_end(g, v) for v in range(n_nodes) if v not in (0, 2, 3))
    # the float64 prefix: plateaus at the weight-0 edges, the 1e-3 absorbed behind the 1e30
    cum = O.weight_prefix(indptr, w)
    hub = cum[indptr[1]:indptr[2]]
    assert (np.diff(hub) == 0).sum() >= 100 and (np.diff(hub) >= 0).all()
    ext = cum[indptr[E.N_EXTREME]:indptr[E.N_EXTREME + 1]]
    assert ext[0] > 0 and ext[1] == ext[2] == float(np.float32(1e30))


@pytest.mark.parametrize("n_nodes", E.GRAPH_NODES)
def test_oracle_walks_have_the_properties_and_reach_the_special_nodes(n_nodes):
    g = indptr, indices, w = E.edge_graph(n_nodes)
    cum = O.weight_prefix(indptr, w)
    tr = O.weighted_walks(indptr, indices, cum, 2, E.WALK_BASE, 257, 12, E.SEED, E.STEP)
    assert (tr[:, 0] == 1).all()  # n_items = 2: every walk starts at the hub
    E.check_walks(g, tr, 2)
    seen = set(np.unique(tr).tolist())
    assert {-1, E.N_EDGELESS, E.N_ALLZERO, E.N_ZERO_FIRST, E.N_ZERO_LAST, E.N_ZERO_MID, E.N_SINGLE,
            E.N_SELF, E.N_EXTREME, E.N_DENORM} <= seen and E.N_OOV not in seen
    steps = set(zip(tr[:, :-1].reshape(-1).tolist(), tr[:, 1:].reshape(-1).tolist()))
    assert (E.N_SELF, E.N_SELF) in steps and (E.N_EXTREME, 12) in steps
    assert (tr[:, 2] == 1).any()  # a hub step that is not the first draw of its walk
    # the check itself catches a step along a weight-0 edge and a walk past its dead end
    bad = tr.copy()
    bad[0, 1] = 0
    with pytest.raises(AssertionError):
        E.check_walks(g, bad, 2)
    bad = tr.copy()
    i, j = np.argwhere(tr == -1)[0]
    bad[i, j] = 1
    with pytest.raises(AssertionError):
        E.check_walks(g, bad, 2)


def test_skipgram_cases():
    names = {c[0]: c for c in E.SKIPGRAM_CASES}
    # a trace's slot count is even whatever (len, window): n_traces · slots is never 4097
    assert all(E.skipgram_slots(ln, wd) % 2 == 0 for ln in range(1, 24) for wd in range(1, 24))
    slots = {n: c[1] * E.skipgram_slots(c[2], c[3]) for n, c in names.items()}
    assert slots["len1"] == 0 and slots["no_traces"] == 0
    assert slots["tile_minus_2"] == E.SCAN_TILE - 2 and slots["tile_exact"] == E.SCAN_TILE
    assert slots["tile_plus_2"] == E.SCAN_TILE + 2 == slots["tile_plus_2_of_6"]
    assert slots["two_tiles_valid"] == 2 * E.SCAN_TILE + 2
    assert names["window_ge_len"][3] == names["window_ge_len"][2] and names["window_gt_len"][3] > names["window_gt_len"][2]
    assert names["window1"][3] == 1
    for name, n, ln, wd, fill in E.SKIPGRAM_CASES:
        tr = E.skipgram_traces(n, ln, fill)
        t, c = E.skipgram_ref(tr, wd)
        ot, oc = O.skipgram_pairs(tr, wd)
        assert np.array_equal(t, ot) and np.array_equal(c, oc), name
        assert (t > 0).all() and (c > 0).all() and t.size <= slots[name]
        if fill == "valid":
            assert t.size == slots[name]
        if fill == "dead":
            assert t.size == 0
    tr = E.skipgram_traces(15, 6, "holes")
    assert tr[9, 0] == -1 and tr[10, -1] == 0 and tr[11, 3] == -1  # 0 and -1 swapped
    assert tr[3, 0] == 0 and tr[4, -1] == -1 and tr[5, 3] == 0 and (tr[0, 3:] == -1).all()
    assert (tr[1] == -1).all() and (tr[2] > 0).all() and (tr[8] > 0).all()
    assert (tr[3, 1:] > 0).all() and (tr[4, :-1] > 0).all() and (tr[0, :3] > 0).all()
    # pairs on both sides of the tile edge survive in the tile cases (the scan carries a count)
    for name in ("tile_exact", "tile_plus_2", "tile_plus_2_of_6"):
        _, n, ln, wd, fill = names[name]
        tr = E.skipgram_traces(n, ln, fill)
        per = E.skipgram_slots(ln, wd)
        first_of_tile2 = E.SCAN_TILE // per
        assert E.skipgram_ref(tr[:first_of_tile2], wd)[0].size > 0
        if n > first_of_tile2:
            assert E.skipgram_ref(tr[first_of_tile2:], wd)[0].size > 0


def test_negative_cases_and_tables():
    assert {(r, s) for r, s, _ in E.NEG_CASES} == {(1, 1), (2, 1), (2, 2), (20, 20), (300, 5),
                                                  (E.BIG_RANGE, 5)}
    assert {n for r, _, n in E.NEG_CASES if r != E.BIG_RANGE} == {1, 255, 257}
    assert all(n <= 64 for r, _, n in E.NEG_CASES if r == E.BIG_RANGE)
    assert E.NEG_PAIR_BASE > 2 ** 31
    for r in (1, 2, 20, 300, E.BIG_RANGE):
        cdf = E.log_uniform_cdf(r)
        assert np.array_equal(cdf, O.log_uniform_cdf(r)) and cdf[-1] == 0xFFFFFFFF
        assert (np.diff(cdf.astype(np.int64)) > 0).all()
    # the float inverse-CDF guess exp2(r · log2(range + 1) / 2^32) - 1 misses the answer on the
    # large table for a few draws in a hundred (the walk along the table then has work to do);
    # on the 300-class table of the existing tests it all but never does
    r = np.linspace(0, 2 ** 32 - 1, 200001).astype(np.uint64).astype(np.uint32)
    miss = {}
    for rng_max in (300, E.BIG_RANGE):
        l2r = np.float32(np.log2(np.float32(rng_max) + np.float32(1))) * np.float32(2.0 ** -32)
        guess = np.clip(np.exp2(r.astype(np.float32) * l2r).astype(np.int64) - 1, 0, rng_max - 1)
        exact = np.minimum(np.searchsorted(E.log_uniform_cdf(rng_max), r, side="right"), rng_max - 1)
        miss[rng_max] = float((guess != exact).mean())
    assert miss[E.BIG_RANGE] > 0.01 and miss[300] < 1e-3, miss
    # the skewed tables put the answer hundreds of classes from the guess, on a known side
    l2r = np.float32(np.log2(np.float32(E.SKEW_RANGE + 1))) * np.float32(2.0 ** -32)
    guess = np.clip(np.exp2(r.astype(np.float32) * l2r).astype(np.int64) - 1, 0, E.SKEW_RANGE - 1)
    for kind, sign in (("down", 1), ("up", -1)):
        cdf = E.skewed_cdf(kind)
        assert cdf.size == E.SKEW_RANGE and (np.diff(cdf.astype(np.int64)) >= 0).all()
        exact = np.minimum(np.searchsorted(cdf, r, side="right"), E.SKEW_RANGE - 1)
        gap = sign * (guess - exact)
        assert (gap >= 0).all() and (gap > 100).mean() > 0.3 and gap.max() > 900, kind
    # (all draws but 0xFFFFFFFF itself, which no entry exceeds)
    assert np.unique(np.searchsorted(E.skewed_cdf("down"), r[:-1], side="right")).tolist() == list(range(31))
    assert (np.searchsorted(E.skewed_cdf("up"), r[r >= 2 ** 31], side="right") == E.SKEW_RANGE).all()
    out = O.log_uniform_sample(E.log_uniform_cdf(20), E.NEG_PAIR_BASE, 3, 20, E.SEED, E.STEP)
    E.check_negatives(out, 20, 20)
    # the all-pairs-at-once restatement equals the oracle
    for rng_max, ns, n in ((20, 20, 9), (300, 5, 33), (2, 2, 17), (1, 1, 5), (E.BIG_RANGE, 5, 8)):
        cdf = E.log_uniform_cdf(rng_max)
        assert np.array_equal(E.log_uniform_ref(cdf, E.NEG_PAIR_BASE, n, ns, E.SEED, E.STEP),
                              O.log_uniform_sample(cdf, E.NEG_PAIR_BASE, n, ns, E.SEED, E.STEP))
    with pytest.raises(AssertionError):
        E.check_negatives(np.array([[1, 1]]), 4, 2)
    with pytest.raises(AssertionError):
        E.check_negatives(np.array([[1, 4]]), 4, 2)


def test_retry_table_never_draws_the_last_word():
    """With a table of 0xFFFFFFFF only class 0 is drawable unless a draw is 0xFFFFFFFF itself:
    none of the 4096 · num_sampled draws of any of the pairs is."""
    p = np.repeat(np.arange(E.RETRY_PAIRS), E.RETRY_DRAWS)
    d = np.tile(np.arange(E.RETRY_DRAWS), E.RETRY_PAIRS)
    r = draw(E.SEED, O.PURPOSE_NEG, E.NEG_PAIR_BASE + p, 0, E.STEP, d)
    assert r.size == E.RETRY_PAIRS * E.RETRY_DRAWS and (r != 0xFFFFFFFF).all()
