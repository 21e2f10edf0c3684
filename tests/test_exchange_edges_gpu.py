"""The row-sharded slab's kernels at their capacity, owner and wave edges, one process, one GPU
context: csrc/exchange.hip (pack, excess, spill pack, padded gather, mark, classify, late
scatter), csrc/sort.hip (sharded sort, unique / inverse) and csrc/embedding.hip (the mapped and
ranged dedup). Inputs, NumPy restatements and comparisons come from tests/exchange_edges.py,
whose properties tests/test_exchange_edges_cpu.py proves.

The C ABI is called directly (L.call). Every output is prefilled — integers with 0x5A5A5A5A,
floats with NaN — and has a tail behind it: what the header promises must be written, the rest
must come back unchanged. Integers are compared exactly, floats as uint32 bits. An all-to-all of
equal blocks is a tensor permute, recv[o][r] = send[r][o].
"""
import numpy as np
import pytest
import torch

from oracle.embedding import sort_ids
from oracle.sharded import sharded_sgd_step
from recommender_amd import _lib as L
from recommender_amd.optim import SortedIds
from tests import exchange_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = E.FILL_I
TAIL = 8
I32_MIN = -2 ** 31


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def ibuf(n):
    return torch.full((int(n) + TAIL,), FILL, dtype=torch.int32, device=DEV)


def fbuf(n, d):
    return torch.full((int(n) + TAIL, d), float("nan"), dtype=torch.float32, device=DEV)


def stream():
    return L.stream_ptr(torch.device(DEV))


def untouched(t, start, msg):
    """The entries of a prefilled buffer from `start` on still hold the fill."""
    rest = t[start:]
    ok = torch.isnan(rest).all() if t.dtype.is_floating_point else (rest == FILL).all()
    assert bool(ok), f"{msg}: written past what the header promises"


def same_f(got, want, msg):
    """Bit equality where NaN (the fill) must sit exactly where the reference has it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    assert (np.isnan(got) == np.isnan(want)).all(), f"{msg}: the written elements differ"
    E.same(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0), msg)


def so_of(V, slots):
    return E.slot_offsets_of(V) if slots else None


# =============================================================================================
# the entry points, each on prefilled buffers
def k_sort(ids, V, W, so):
    """rs_sort_ids_sharded → (keys, pos, n_unique) tensors with tails."""
    t = dev(ids)
    n = t.numel()
    sot = None if so is None else dev(so)
    keys, pos, nu = ibuf(n), ibuf(n), ibuf(1)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = L.scratch(L.lib().rs_sort_ids_workspace_size(n), DEV)
    L.call("rs_sort_ids_sharded", L.ptr(t), L.id_dtype_code(t), n, L.ptr(sot),
           1 if so is None else E.N_SLOTS, V, W, L.ptr(keys), L.ptr(pos), L.ptr(nu), L.ptr(err),
           L.ptr(ws), ws.numel(), stream())
    return keys, pos, nu, err


def k_unique(keys, pos, n, V, W, with_counts=True):
    """rs_unique_inverse → dict of tensors with tails; ws is the workspace (int32 view)."""
    uniq, inv, nu = ibuf(n), ibuf(n), ibuf(1)
    counts = ibuf(W) if with_counts else None
    ws = L.scratch(L.lib().rs_unique_inverse_workspace_size(n), DEV)
    ws.fill_(0x5A)
    L.call("rs_unique_inverse", L.ptr(keys), L.ptr(pos), n, V, W, L.ptr(uniq), L.ptr(inv),
           L.ptr(nu), L.ptr(counts), L.ptr(ws), ws.numel(), stream())
    return dict(uniq=uniq, inverse=inv, n_unique=nu, owner_counts=counts, ws=ws)


def check_unique(got, want, n, W, msg):
    U = want["n_unique"]
    assert host(got["n_unique"]).tolist() == [U] + [FILL] * TAIL, f"{msg} n_unique"
    E.same(host(got["uniq"][:U]), want["uniq"].astype(np.int32), f"{msg} uniq keys")
    untouched(got["uniq"], U, f"{msg} uniq keys")
    E.same(host(got["inverse"][:n]), want["inverse"], f"{msg} inverse")
    untouched(got["inverse"], n, f"{msg} inverse")
    if got["owner_counts"] is not None:
        E.same(host(got["owner_counts"][:W]), want["owner_counts"], f"{msg} owner_counts")
        untouched(got["owner_counts"], W, f"{msg} owner_counts")
    if n:  # the workspace head: the segment index of every sorted key
        head = got["ws"][:4 * n].view(torch.int32)
        E.same(host(head), want["seg_excl"], f"{msg} workspace head")


def k_pack(u, W, stride, C, n):
    """rs_exchange_pack + rs_exchange_excess on uploaded unique / inverse arrays."""
    uniq, inv = ibuf(n), dev(u["inverse"])  # [n_ids] as the callers size it; U keys are read
    uniq[:u["n_unique"]] = dev(u["uniq"].astype(np.int32))
    nu = torch.tensor([u["n_unique"]], dtype=torch.int32, device=DEV)
    counts = dev(u["owner_counts"])
    send, slot_of, inv_slot = ibuf(W * C), ibuf(max(n, 1)), ibuf(max(n, 1))
    over = torch.tensor([0] + [FILL] * TAIL, dtype=torch.int32, device=DEV)
    exc = torch.full((1 + TAIL,), FILL, dtype=torch.int64, device=DEV)
    L.call("rs_exchange_pack", L.ptr(uniq), L.ptr(nu), L.ptr(counts), W, stride, C, L.ptr(inv), n,
           L.ptr(send), L.ptr(slot_of), L.ptr(inv_slot), L.ptr(over), stream())
    L.call("rs_exchange_excess", L.ptr(counts), W, C, L.ptr(exc), stream())
    return dict(send_ids=send, slot_of=slot_of, inverse_slot=inv_slot, overflow=over, excess=exc,
                dev=(uniq, nu, counts, inv))


def check_pack(got, want, u, W, C, n, msg):
    U = u["n_unique"]
    E.compare_pack(dict(send_ids=host(got["send_ids"][:W * C]), slot_of=host(got["slot_of"]),
                        inverse_slot=host(got["inverse_slot"][:n]),
                        overflow=int(got["overflow"][0]), excess=int(got["excess"][0])),
                   want, msg)
    untouched(got["send_ids"], W * C, f"{msg} send_ids")
    untouched(got["slot_of"], U, f"{msg} slot_of")
    untouched(got["inverse_slot"], n, f"{msg} inverse_slot")
    untouched(got["overflow"], 1, f"{msg} overflow")
    assert (host(got["excess"][1:]) == FILL).all(), f"{msg} excess"


def k_gather(shard, n_rows, dim, ids):
    n = ids.numel()
    out = fbuf(n, dim).view(-1)[:n * dim + TAIL]
    L.call("rs_gather_rows_padded", L.ptr(shard), n_rows, dim, L.ptr(ids), n, L.ptr(out), stream())
    untouched(out, n * dim, "gather")
    return out[:n * dim].view(n, dim)


def permute(send, c):
    """recv[o] = the blocks of c rows every rank r sent owner o, r-major."""
    W = len(send)
    return [torch.cat([send[r][o * c:(o + 1) * c] for r in range(W)]) for o in range(W)]


# =============================================================================================
# 1. sort, unique, inverse
@pytest.mark.parametrize("W,V", E.GEOMETRIES)
def test_sort_unique_inverse(W, V):
    C = 5 if E.feasible("one_over", W, V, 5) else 1
    i = 0
    for name in E.PATTERNS:
        if not E.feasible(name, W, V, C):
            continue
        for slots in (False, True):
            for dtype in (np.int32, np.int64):
                msg = f"{name} slots={slots} {np.dtype(dtype).name}"
                ids = E.make_ids(name, W, V, C, slots=slots, dtype=dtype)
                so, n = so_of(V, slots), ids.size
                sk, sp = E.sort_sharded(ids, V, W, so)
                want = E.unique_inverse(sk, sp, V, W)
                keys, pos, nu, err = k_sort(ids, V, W, so)
                E.same(host(keys[:n]), sk.astype(np.int32), f"{msg} sorted keys")
                E.same(host(pos[:n]), sp, f"{msg} sorted pos")
                untouched(keys, n, f"{msg} keys")
                untouched(pos, n, f"{msg} pos")
                assert host(nu).tolist() == [want["n_unique"]] + [FILL] * TAIL, f"{msg} count"
                assert bool(int(err[0]) & L.RS_ERRBIT_OOB) == bool((sk == E.key_space_of(V, W)).any())
                i += 1
                got = k_unique(keys, pos, n, V, W, with_counts=bool(i % 3))  # NULL counts accepted
                check_unique(got, want, n, W, msg)


# =============================================================================================
# 2. pack and excess
@pytest.mark.parametrize("W,V", E.GEOMETRIES)
def test_pack_and_excess(W, V):
    stride = E.stride_of(V, W)
    for C in E.CAPACITIES:
        for name in E.PATTERNS:
            if not E.feasible(name, W, V, C):
                continue
            for slots in (False, True):
                msg = f"C={C} {name} slots={slots}"
                ids = E.make_ids(name, W, V, C, slots=slots)
                n = ids.size
                u = E.unique_inverse(*E.sort_sharded(ids, V, W, so_of(V, slots)), V, W)
                want = E.pack(u["uniq"], u["owner_counts"], W, stride, C, u["inverse"])
                got = k_pack(u, W, stride, C, n)
                torch.cuda.synchronize()
                check_pack(got, want, u, W, C, n, msg)
                if name == "one_over":
                    assert want["excess"] == 1 and (host(got["slot_of"][:u["n_unique"]]) == -1).sum() == 1
                # capacity 0: the largest count (the late round's size in recommender_amd/sharded.py)
                mx = torch.full((2,), FILL, dtype=torch.int64, device=DEV)
                L.call("rs_exchange_excess", L.ptr(got["dev"][2]), W, 0, L.ptr(mx), stream())
                assert host(mx).tolist() == [int(u["owner_counts"].max()), FILL], f"{msg} excess at 0"


# =============================================================================================
# 3. spill pack
def k_spill(p, W, stride, C, C2, n, overflow):
    uniq, nu, counts, inv = p["dev"]
    spill = ibuf(W * C2)
    L.call("rs_exchange_pack_spill", L.ptr(uniq), L.ptr(nu), L.ptr(counts), W, stride, C, C2,
           L.ptr(inv), n, L.ptr(spill), L.ptr(p["slot_of"]), L.ptr(p["inverse_slot"]),
           L.ptr(overflow), stream())
    return spill


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("W,V,C", [(3, 100, 5), (4, 130, 5), (8, 1001, 64), (8, 1001, 70), (3, 100, 1)])
def test_spill_pack(W, V, C, slots):
    stride = E.stride_of(V, W)
    per_rank, ex = E.spill_world_ids(W, V, C, slots)
    # (rank, C2, overflow pointer): the three ranks at the all-reduced C2 = 3 (excess 0: all
    # padding; 1: padding behind one row; 3: full), then C2 one below rank 2's excess
    for r, C2, with_flag in [(0, 3, True), (1, 3, True), (2, 3, True), (2, 2, True), (2, 2, False),
                             (1, 3, False)]:
        msg = f"rank {r} C2={C2} flag={with_flag}"
        ids = per_rank[r]
        n = ids.size
        u = E.unique_inverse(*E.sort_sharded(ids, V, W, so_of(V, slots)), V, W)
        U = u["n_unique"]
        args = (u["uniq"], u["owner_counts"], W, stride, C)
        p_want = E.pack(*args, u["inverse"])
        want = E.pack_spill(*args, C2, u["inverse"], p_want["slot_of"])
        assert want["overflow"] == int(ex[r] > C2)
        p = k_pack(u, W, stride, C, n)
        flag = torch.tensor([0] + [FILL] * TAIL, dtype=torch.int32, device=DEV)
        spill = k_spill(p, W, stride, C, C2, n, flag if with_flag else None)
        torch.cuda.synchronize()
        got = dict(spill_ids=host(spill[:W * C2]), slot_of=host(p["slot_of"]),
                   inverse_slot=host(p["inverse_slot"][:n]),
                   overflow=int(flag[0]) if with_flag else want["overflow"])
        E.compare_spill(got, want, msg)
        untouched(spill, W * C2, f"{msg} spill_ids")
        untouched(p["slot_of"], U, f"{msg} slot_of")
        untouched(p["inverse_slot"], n, f"{msg} inverse_slot")
        assert host(flag).tolist() == [want["overflow"] if with_flag else 0] + [FILL] * TAIL
        # the rows within the capacity keep the slots rs_exchange_pack gave them
        kept = p_want["slot_of"] >= 0
        E.same(host(p["slot_of"][:U])[kept], p_want["slot_of"][kept], f"{msg} kept slots")
        assert (host(spill[:W * C2]) >= 0).sum() == min(ex[r], C2)
        E.same(host(p["send_ids"][:W * C]), p_want["send_ids"], f"{msg} send_ids")


# =============================================================================================
# 4. gather
def gather_block_rows(dim):
    lanes = min(dim // 4, 64) if dim % 4 == 0 else min(dim, 64)
    return 256 // lanes


@pytest.mark.parametrize("dim", [1, 3, 4, 12, 20, 66, 128, 132, 260, 300])
def test_gather_rows_padded(dim):
    rng = np.random.default_rng(dim)
    n_rows = 23
    shard = rng.standard_normal((n_rows, dim)).astype(np.float32)
    st = dev(shard)
    pb = gather_block_rows(dim)
    assert {12: 85, 20: 51, 128: 8, 132: 7, 260: 4}.get(dim, pb) == pb
    for n in (1, pb - 1, pb + 1, 700):
        ids = rng.integers(-1, n_rows + 1, n).astype(np.int32)
        edge = np.array([-1, n_rows, n_rows - 1, 0, I32_MIN], np.int32)
        k = min(n, edge.size)
        ids[:k] = np.roll(edge, -n)[:k]  # n = 1 meets each edge value over the sizes
        got = k_gather(st, n_rows, dim, dev(ids))
        E.same(host(got), E.gather_padded(shard, n_rows, ids, dim), f"dim {dim} n {n}")
        # no row at all, a null shard: zeros
        got0 = k_gather(None, 0, dim, dev(ids))
        assert not host(got0).view(np.uint32).any(), f"dim {dim} n {n}: null shard"
    assert torch.equal(st, dev(shard))


# =============================================================================================
# 5. mark and classify
def k_classify(recv, W, C, stamp, n_rows, pred):
    rows, slot, cnt = ibuf(W * C), ibuf(W * C), ibuf(W)
    L.call("rs_exchange_classify", L.ptr(recv), W, C, L.ptr(stamp), n_rows, pred, L.ptr(rows),
           L.ptr(slot), L.ptr(cnt), stream())
    return rows, slot, cnt


def check_classify(got, want, W, C, msg):
    rows, slot, cnt = (host(t) for t in got)
    pairs, count = want
    E.same(cnt[:W], count, f"{msg} late_count")
    assert (cnt[W:] == FILL).all() and (rows[W * C:] == FILL).all() and (slot[W * C:] == FILL).all()
    for r in range(W):
        k = int(count[r])
        lr, ls = rows[r * C:(r + 1) * C], slot[r * C:(r + 1) * C]
        assert sorted(zip(lr[:k].tolist(), ls[:k].tolist())) == pairs[r], f"{msg} requester {r}"
        assert (lr[k:] == -1).all() and (ls[k:] == -1).all(), f"{msg} requester {r}: tail of -1"


@pytest.mark.parametrize("W,C", [(3, 5), (2, 70), (3, 70), (8, 70), (4, 64), (1, 70), (5, 1)])
def test_mark_and_classify(W, C):
    rng = np.random.default_rng([W, C])
    n_rows, pred = 41, 7
    # mark: stamps equal to pred, to pred - 1 and to 0; ids with padding and out-of-range values
    stamp0 = rng.choice(np.array([pred, pred - 1, 0], np.int32), n_rows)
    cur = rng.integers(-1, n_rows + 3, W * C).astype(np.int32)
    cur[0] = I32_MIN
    st = ibuf(n_rows)
    st[:n_rows] = dev(stamp0)
    cur_t = dev(cur)
    L.call("rs_exchange_mark", L.ptr(cur_t), cur.size, L.ptr(st), n_rows, pred + 1, stream())
    E.same(host(st[:n_rows]), E.mark(cur, stamp0, n_rows, pred + 1), "mark")
    untouched(st, n_rows, "mark")
    # classify reads a stamp array whose tail holds pred: an id >= n_rows that were looked up
    # there would be listed
    stamp = np.concatenate([stamp0, np.full(TAIL, pred, np.int32)])
    stamp[:3] = [pred, pred - 1, 0]
    std = dev(stamp)
    hot, cold = np.flatnonzero(stamp[:n_rows] == pred), np.flatnonzero(stamp[:n_rows] != pred)
    never = np.array([-1, n_rows, n_rows + 3, I32_MIN], np.int64)  # padding and ids >= n_rows
    miss = lambda k: rng.choice(np.concatenate([cold, never]), k)
    layouts = {"none": miss(W * C), "all": rng.choice(hot, W * C)}
    last = miss(W * C)
    last[(W - 1) * C:] = rng.choice(hot, C)
    layouts["last"] = last
    both = miss(W * C)
    for r in range(W):  # the first and the last slot of every requester
        both[r * C] = rng.choice(hot)
        both[r * C + C - 1] = rng.choice(hot)
    layouts["both_sides"] = both
    mixed = np.where(rng.random(W * C) < 0.5, rng.choice(hot, W * C), miss(W * C))
    layouts["mixed"] = mixed
    for name, recv in layouts.items():
        recv = recv.astype(np.int32)
        want = E.classify(recv, W, C, stamp[:n_rows], n_rows, pred)
        if name == "none":
            assert not want[1].any()
        if name == "all":
            assert (want[1] == C).all()
        if name == "last":
            assert want[1][W - 1] == C and not want[1][:W - 1].any()
        if name == "both_sides":
            assert (want[1] == min(C, 2)).all()
        rt = dev(recv)
        first = k_classify(rt, W, C, std, n_rows, pred)
        second = k_classify(rt, W, C, std, n_rows, pred)
        torch.cuda.synchronize()
        check_classify(first, want, W, C, f"{name} first call")
        check_classify(second, want, W, C, f"{name} second call")
    assert torch.equal(std, dev(stamp))


# =============================================================================================
# 6. late scatter
@pytest.mark.parametrize("dim", [4, 12, 128, 132])
@pytest.mark.parametrize("W,C", [(3, 5), (2, 70)])
def test_scatter_late(W, C, dim):
    rng = np.random.default_rng([W, C, dim])
    for CL in (0, 1, C):
        # each owner's slot list: distinct slots with -1 interleaved (also in the live range
        # k < CL); the entries past CL are live slots too, which a wrong bound would scatter
        hole = rng.random((W, C)) < 0.4
        hole[:, 0] = False
        hole[:, 1:2] = True
        slot = np.stack([rng.permutation(C) for _ in range(W)]).astype(np.int32)
        slot = np.where(hole, -1, slot).astype(np.int32).reshape(-1)
        rows = rng.standard_normal((W * C, dim)).astype(np.float32)
        recv = rng.standard_normal((W * CL, dim)).astype(np.float32)
        rt = fbuf(W * C, dim)
        rt[:W * C] = dev(rows)
        recv_t, slot_t = dev(recv), dev(slot)
        L.call("rs_exchange_scatter_late", L.ptr(recv_t), L.ptr(slot_t), W, C, CL, dim, L.ptr(rt),
               stream())
        want = E.scatter_late(recv, slot, W, C, CL, rows)
        E.same(host(rt[:W * C]), want, f"CL={CL}")
        untouched(rt, W * C, f"CL={CL}")
        live = sum(int(slot[o * C + k] >= 0) for o in range(W) for k in range(CL))
        assert (E.bits(want) != E.bits(rows)).any(1).sum() == live  # rows outside the late slots stay


# =============================================================================================
# 7. ranged dedup
def k_dedup(fn, inp, grad, scaled, mapped, ranges=None, seg_excl=None, ws=None):
    """One call of `fn` (mapped_range over `ranges` = [(lo, hi, seg_ready)]) → (rows, out)."""
    n, D = grad.shape
    sk, pos = dev(inp["sk"].astype(np.int32)), dev(inp["pos"])
    sc = dev(inp["row_scale"]) if scaled else None
    sm = dev(inp["seg_map"]) if mapped else None
    rows, out = ibuf(n), fbuf(inp["n_unique"] + 8 - TAIL, D)
    ws = L.scratch(L.lib().rs_dedup_workspace_size(n, D), DEV) if ws is None else ws
    ks = inp["key_space"]
    head = (L.ptr(sk), L.ptr(pos), n, L.ptr(grad), L.ptr(sc), E.DEDUP_GROUP, D, ks)
    tail = (L.ptr(rows), L.ptr(out), L.ptr(ws), ws.numel(), stream())
    if fn == "rs_embedding_dedup_grad_scaled":
        L.call(fn, *head, *tail)
    elif fn == "rs_embedding_dedup_grad_mapped":
        L.call(fn, *head, L.ptr(sm), *tail)
    else:
        for lo, hi, ready in ranges:
            L.call(fn, *head, lo, hi, ready, L.ptr(seg_excl), L.ptr(sm), *tail)
    torch.cuda.synchronize()
    return host(rows[:n]).astype(np.int64), host(out)


RANGE = "rs_embedding_dedup_grad_mapped_range"


@pytest.mark.parametrize("W,below,cross", E.DEDUP_CASES)
def test_ranged_dedup(W, below, cross):
    inp = E.dedup_input(W, below, cross)
    n, K, ks = E.DEDUP_N, inp["K"], inp["key_space"]
    grad = dev(inp["grad"])
    # the segment ids as rs_unique_inverse leaves them at its workspace's head
    sk, pos = dev(inp["sk"].astype(np.int32)), dev(inp["pos"])
    u = k_unique(sk, pos, n, E.DEDUP_V, W)
    assert int(u["n_unique"][0]) == inp["n_unique"]
    seg = u["ws"][:4 * n].view(torch.int32)
    for scaled in (False, True):
        want = E.dedup_ref(inp, scaled, True)
        whole = k_dedup(RANGE, inp, grad, scaled, True, [(0, ks, 0)])
        halves = k_dedup(RANGE, inp, grad, scaled, True, [(0, K, 0), (K, ks, 1)])
        given = k_dedup(RANGE, inp, grad, scaled, True, [(0, K, 0), (K, ks, 0)], seg_excl=seg)
        for name, got in (("one call", whole), ("two calls, seg_ready", halves),
                          ("two calls, seg_excl given", given)):
            E.same(got[0], want[0], f"{name} scaled={scaled} uniq_rows")
            same_f(got[1], want[1], f"{name} scaled={scaled} uniq_grad")
    # each half alone writes its segments only; a range holding no key writes nothing
    for lo, hi in ((0, K), (K, ks)):
        want = E.dedup_ref(inp, True, True, lo, hi)
        got = k_dedup(RANGE, inp, grad, True, True, [(lo, hi, 0)])
        E.same(got[0], want[0], f"[{lo}, {hi}) uniq_rows")
        same_f(got[1], want[1], f"[{lo}, {hi}) uniq_grad")
        holds = ((inp["sk"] >= lo) & (inp["sk"] < hi)).any()
        assert holds or ((got[0] == FILL).all() and np.isnan(got[1]).all())


@pytest.mark.parametrize("D", [16, 48, 128])
@pytest.mark.parametrize("W,below,cross", [(2, 1041, False), (3, 1070, True), (4, 1024, False)])
def test_dedup_mapped_and_scaled_without_a_map(W, below, cross, D):
    inp = E.dedup_input(W, below, cross)
    grad = dev(inp["grad"][:, :D])
    for scaled in (False, True):
        want = E.dedup_ref(inp, scaled, False, width=D)
        for fn in ("rs_embedding_dedup_grad_mapped", "rs_embedding_dedup_grad_scaled"):
            got = k_dedup(fn, inp, grad, scaled, False)
            E.same(got[0], want[0], f"{fn} scaled={scaled} uniq_rows")
            same_f(got[1], want[1], f"{fn} scaled={scaled} uniq_grad")


@pytest.mark.parametrize("D", [16, 48])
@pytest.mark.parametrize("W,below,cross", E.DEDUP_CASES)
def test_dedup_lower_range_at_other_widths(W, below, cross, D):
    """include/recsys_hip.h: at D != 128 the ranged form takes the ranges [0, key_hi) (the
    generic walk with key_hi as its row count); key_lo != 0 is refused (argument errors)."""
    inp = E.dedup_input(W, below, cross)
    grad = dev(inp["grad"][:, :D])
    K = inp["K"]
    for scaled, mapped in ((False, True), (True, True), (True, False)):
        want = E.dedup_ref(inp, scaled, mapped, 0, K, width=D)
        got = k_dedup(RANGE, inp, grad, scaled, mapped, [(0, K, 0)])
        E.same(got[0], want[0], f"scaled={scaled} mapped={mapped} uniq_rows")
        same_f(got[1], want[1], f"scaled={scaled} mapped={mapped} uniq_grad")


# =============================================================================================
# 8. the simulated world: every stage a kernel, every all-to-all a permute
WORLD_V = {2: 37, 3: 100, 8: 1001}
LR = 0.05


class GpuWorld:
    def __init__(self, W, V, C, D, table, so):
        self.W, self.V, self.C, self.D = W, V, C, D
        self.stride, self.ks = E.stride_of(V, W), E.key_space_of(V, W)
        self.so = so
        self.so_t = None if so is None else dev(so)
        self.shards = [dev(table[o::W]) for o in range(W)]
        self.n_local = [E.shard_rows(V, W, o) for o in range(W)]
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ws = L.Workspace()

    def full_table(self):
        out = np.empty((self.V, self.D), np.float32)
        for o in range(self.W):
            out[o::self.W] = host(self.shards[o])
        return out

    def gather(self, ids_per_owner):
        return [k_gather(self.shards[o], self.n_local[o], self.D, ids_per_owner[o])
                for o in range(self.W)]

    def begin(self, per_rank_ids):
        """Sort … pack on every rank and the row-id permute: reads no table state."""
        W, C = self.W, self.C
        st = []
        for ids in per_rank_ids:
            t = dev(ids)
            n = t.numel()
            s = SortedIds(t, self.V, self.so_t, self.err, self.ws, count_unique=False, world=W)
            u = k_unique(s.rows, s.pos, n, self.V, W)
            send, slot_of, inv_slot = ibuf(W * C), ibuf(max(n, 1)), ibuf(max(n, 1))
            over = torch.zeros(1, dtype=torch.int32, device=DEV)
            exc = torch.zeros(1, dtype=torch.int64, device=DEV)
            L.call("rs_exchange_pack", L.ptr(u["uniq"]), L.ptr(u["n_unique"]),
                   L.ptr(u["owner_counts"]), W, self.stride, C, L.ptr(u["inverse"]), n,
                   L.ptr(send), L.ptr(slot_of), L.ptr(inv_slot), L.ptr(over), stream())
            L.call("rs_exchange_excess", L.ptr(u["owner_counts"]), W, C, L.ptr(exc), stream())
            st.append(dict(s=s, n=n, u=u, send=send[:W * C], slot_of=slot_of, inv_slot=inv_slot,
                           exc=exc))
        C2 = max(int(x["exc"][0]) for x in st)  # the all-reduce (MAX)
        return dict(ranks=st, C2=C2, recv_ids=permute([x["send"] for x in st], C))

    def finish(self, fw, rows_c):
        """The spill round behind the capacity block's rows (gathered now or a step early)."""
        W, C, C2 = self.W, self.C, fw["C2"]
        spill = [torch.zeros(0, dtype=torch.int32, device=DEV)] * W
        if C2:
            spill = []
            for x in fw["ranks"]:
                sp = ibuf(W * C2)
                u = x["u"]
                L.call("rs_exchange_pack_spill", L.ptr(u["uniq"]), L.ptr(u["n_unique"]),
                       L.ptr(u["owner_counts"]), W, self.stride, C, C2, L.ptr(u["inverse"]),
                       x["n"], L.ptr(sp), L.ptr(x["slot_of"]), L.ptr(x["inv_slot"]), None,
                       stream())
                spill.append(sp[:W * C2])
        fw["spill_ids"] = spill
        fw["recv_spill"] = permute(spill, C2)
        rows_s = permute(self.gather(fw["recv_spill"]), C2)
        fw["rows"] = [torch.cat([a, b]) for a, b in zip(rows_c, rows_s)]
        return fw

    def check_forward(self, fw, ref, per_rank_ids, table, msg):
        W, C = self.W, self.C
        assert fw["C2"] == ref["C2"]
        for r, x in enumerate(fw["ranks"]):
            U, n = ref["unique"][r]["n_unique"], x["n"]
            E.same(host(x["send"]), ref["send_ids"][r], f"{msg} rank {r} send_ids")
            E.same(host(fw["spill_ids"][r]), ref["spill_ids"][r], f"{msg} rank {r} spill_ids")
            E.same(host(x["slot_of"][:U]), ref["slot_of"][r], f"{msg} rank {r} slot_of")
            E.same(host(x["inv_slot"][:n]), ref["inv_slot"][r], f"{msg} rank {r} inverse_slot")
            E.same(host(fw["rows"][r]), ref["rows"][r], f"{msg} rank {r} rows")
        got = dict(C2=fw["C2"], rows=[host(t) for t in fw["rows"]],
                   inv_slot=[host(x["inv_slot"][:x["n"]]) for x in fw["ranks"]],
                   send_ids=[host(x["send"]) for x in fw["ranks"]],
                   spill_ids=[host(t) for t in fw["spill_ids"]])
        got["lookup"] = []
        for r in range(W):
            out = np.zeros((got["inv_slot"][r].size, self.D), np.float32)
            ok = got["inv_slot"][r] >= 0
            out[ok] = got["rows"][r][got["inv_slot"][r][ok]]
            got["lookup"].append(out)
        ref_world = E.World(W, self.V, C, table, self.so)
        E.check_lookup(ref_world, got, per_rank_ids, table, msg)

    def backward(self, fw, grads, ref_world, ref_fw, msg):
        """Send blocks (two owner halves at D = 128, as recommender_amd/sharded.py), the owners'
        merge of the received runs and the SGD apply with lr / W."""
        W, C, C2, D = self.W, self.C, fw["C2"], self.D
        ref_send = ref_world.send_blocks(ref_fw, grads)
        send = []
        for r, x in enumerate(fw["ranks"]):
            n = x["n"]
            sg, ur = fbuf(W * (C + C2), D), ibuf(max(n, 1))
            g = dev(grads[r])
            w = L.scratch(L.lib().rs_dedup_workspace_size(max(n, 1), D), DEV)
            seg = x["u"]["ws"]
            K = (W // 2) * self.stride
            for lo, hi, ready in ([(0, K, 0), (K, self.ks, 1)] if D == 128 else [(0, self.ks, 0)]):
                if n:
                    L.call(RANGE, L.ptr(x["s"].rows), L.ptr(x["s"].pos), n, L.ptr(g), None, 1, D,
                           self.ks, lo, hi, ready, L.ptr(seg), L.ptr(x["slot_of"]), L.ptr(ur),
                           L.ptr(sg), L.ptr(w), w.numel(), stream())
            torch.cuda.synchronize()
            same_f(host(sg[:W * (C + C2)]), ref_send[r], f"{msg} rank {r} send block")
            untouched(sg, W * (C + C2), f"{msg} rank {r} send block")
            send.append(sg[:W * (C + C2)])
        gc = permute([s[:W * C] for s in send], C)
        gs = permute([s[W * C:] for s in send], C2)
        lr_w = float(np.float32(LR)) / W
        for o in range(W):
            ids = torch.cat([fw["recv_ids"][o].view(W, C), fw["recv_spill"][o].view(W, C2)],
                            1).reshape(-1).contiguous()
            g = torch.cat([gc[o].view(W, C, D), gs[o].view(W, C2, D)], 1).reshape(-1, D).contiguous()
            s = SortedIds.from_runs(ids, W, self.n_local[o], self.err)
            sr, sp, _ = sort_ids(host(ids), self.n_local[o])
            E.same(host(s.rows), sr.astype(np.int32), f"{msg} owner {o} merged rows")
            E.same(host(s.pos), sp, f"{msg} owner {o} merged pos")
            w = L.scratch(L.lib().rs_apply_workspace_size(s.n, D), DEV)
            L.call("rs_embedding_apply_scaled", L.RS_OPT_SGD, L.ptr(self.shards[o]), None, None,
                   self.n_local[o], D, L.ptr(s.rows), L.ptr(s.pos), s.n, L.ptr(g), None, 1,
                   L.AdamParams(lr_w, 0.0, 0.0, 0.0, 0.0, 0.0), None, L.ptr(w), w.numel(),
                   stream())
        torch.cuda.synchronize()

    def late(self, cur, nxt, early, stamps, seq):
        """The rows of `nxt` gathered before `cur`'s apply, corrected after it: mark, classify,
        the late round's size, the late gather and rs_exchange_scatter_late."""
        W, C, D = self.W, self.C, self.D
        lists, sizes = [], []
        for o in range(W):
            for ids in (cur["recv_ids"][o], cur["recv_spill"][o]):
                if ids.numel():
                    L.call("rs_exchange_mark", L.ptr(ids), ids.numel(), L.ptr(stamps[o]),
                           self.n_local[o], seq, stream())
            rows, slot, cnt = k_classify(nxt["recv_ids"][o], W, C, stamps[o], self.n_local[o], seq)
            mx = torch.zeros(1, dtype=torch.int64, device=DEV)
            L.call("rs_exchange_excess", L.ptr(cnt), W, 0, L.ptr(mx), stream())
            lists.append((rows[:W * C], slot[:W * C]))
            sizes.append(int(mx[0]))
        CL = max(sizes)  # the all-reduce (MAX)
        recv_slot = permute([l[1] for l in lists], C)
        if CL:
            ids_l = [l[0].view(W, C)[:, :CL].contiguous().view(-1) for l in lists]
            recv = permute(self.gather(ids_l), CL)
            for r in range(W):
                L.call("rs_exchange_scatter_late", L.ptr(recv[r]), L.ptr(recv_slot[r]), W, C, CL,
                       D, L.ptr(early[r]), stream())
        torch.cuda.synchronize()
        return CL


@pytest.mark.parametrize("C", [5, 64])
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_simulated_world(W, D, C):
    V = WORLD_V[W]
    slots = D == 16
    so = so_of(V, slots)
    rng = np.random.default_rng([W, D, C])
    table = rng.standard_normal((V, D)).astype(np.float32)
    # step 1's rank 0 spills by construction at the small capacity (one owner holds C + 1 rows)
    first = "one_over" if C == 5 else "zipf"
    steps = [[E.make_ids("oob" if r % 2 else first if r + step == 0 else "zipf", W, V, C,
                         seed=100 * step + r, slots=slots,
                         dtype=np.int32 if (r + step) % 2 else np.int64) for r in range(W)]
             for step in range(2)]
    grads = [[rng.standard_normal((i.size, D)).astype(np.float32) for i in ids] for ids in steps]
    world = GpuWorld(W, V, C, D, table, so)
    ref = E.World(W, V, C, table, so)
    stamps = [torch.zeros(max(n, 1), dtype=torch.int32, device=DEV) for n in world.n_local]

    # step 1: forward, rows gathered now
    fw1 = world.begin(steps[0])
    world.finish(fw1, permute(world.gather(fw1["recv_ids"]), C))
    ref1 = ref.forward(steps[0])
    world.check_forward(fw1, ref1, steps[0], table, "step 1")
    assert (fw1["C2"] > 0) == (C == 5)  # the small capacity spills
    # step 2 begins, and its capacity block's rows are gathered, before step 1's apply
    fw2 = world.begin(steps[1])
    early = [t.clone() for t in permute(world.gather(fw2["recv_ids"]), C)]
    world.backward(fw1, grads[0], ref, ref1, "step 1")
    ref.backward(ref1, grads[0], LR)
    table1 = sharded_sgd_step(table, steps[0], grads[0], LR, W, so)
    E.same(world.full_table(), table1, "table after step 1")
    E.same(ref.full_table(), table1, "restated table after step 1")
    # the early rows + the late round = a fresh gather after the apply
    stale = [host(t) for t in early]
    CL = world.late(fw1, fw2, early, stamps, seq=1)
    fresh = permute(world.gather(fw2["recv_ids"]), C)
    assert CL > 0 and any((E.bits(stale[r]) != E.bits(host(fresh[r]))).any() for r in range(W)), \
        "step 2 requests no row that step 1 updated: the late round is not exercised"
    for r in range(W):
        E.same(host(early[r]), host(fresh[r]), f"rank {r}: rows a step ahead + late rows")
    # step 2 on the corrected rows
    world.finish(fw2, early)
    ref2 = ref.forward(steps[1])
    world.check_forward(fw2, ref2, steps[1], table1, "step 2")
    world.backward(fw2, grads[1], ref, ref2, "step 2")
    E.same(world.full_table(), sharded_sgd_step(table1, steps[1], grads[1], LR, W, so),
           "table after step 2")
    assert int(world.err[0]) & L.RS_ERRBIT_OOB  # the OOB ids were flagged, nothing else


# =============================================================================================
# 9. argument errors: refused before anything is launched
def test_argument_errors():
    W, C, n = 3, 5, 12
    i = ibuf
    outs = []

    def refused(fn, *args):
        with pytest.raises(L.RecsysError):
            L.call(fn, *args, stream())

    def fresh(k=64):
        t = i(k)
        outs.append(t)
        return L.ptr(t)

    ids = dev(np.arange(n, dtype=np.int32))
    uniq, inv, nu, counts = i(64), i(64), torch.ones(1, dtype=torch.int32, device=DEV), i(64)
    counts.zero_()
    pk = lambda w, c: ("rs_exchange_pack", L.ptr(uniq), L.ptr(nu), L.ptr(counts), w, 4, c,
                       L.ptr(inv), n, fresh(), fresh(), fresh(), fresh())
    sp = lambda w, c, c2: ("rs_exchange_pack_spill", L.ptr(uniq), L.ptr(nu), L.ptr(counts), w, 4, c,
                           c2, L.ptr(inv), n, fresh(), fresh(), fresh(), fresh())
    cl = lambda w, c: ("rs_exchange_classify", L.ptr(uniq), w, c, L.ptr(counts), 10, 1, fresh(),
                       fresh(), fresh())
    for w in (0, 1025):  # world 0 and 1025
        refused(*pk(w, C))
        refused(*sp(w, C, 2))
        refused(*cl(w, C))
        refused("rs_exchange_excess", L.ptr(counts), w, C, fresh())
        refused("rs_exchange_scatter_late", fresh(), L.ptr(inv), w, C, 1, 4, fresh())
        refused("rs_unique_inverse", L.ptr(uniq), L.ptr(inv), n, 10, w, fresh(), fresh(), fresh(),
                fresh(), fresh(4096), 4096 * 4)
        refused("rs_sort_ids_sharded", L.ptr(ids), L.RS_ID_I32, n, None, 1, 10, w, fresh(), fresh(),
                fresh(), fresh(), fresh(4096), 4096 * 4)
    refused(*pk(W, 0))  # capacity 0
    refused(*sp(W, 0, 2))
    refused(*sp(W, C, 0))
    refused(*cl(W, 0))
    refused("rs_exchange_scatter_late", fresh(), L.ptr(inv), W, 0, 0, 4, fresh())
    big = 2 ** 21  # W·C = 2^31
    refused(*pk(1024, big))
    refused(*cl(1024, big))
    refused(*sp(1024, big - 1, 1))
    refused("rs_exchange_scatter_late", fresh(), L.ptr(inv), W, C, C + 1, 4, fresh())  # late > C
    refused("rs_exchange_scatter_late", fresh(), L.ptr(inv), W, C, 1, 6, fresh())  # dim 6
    # a row pointer off 16-byte alignment at a multiple-of-4 width (a sliced tensor)
    rows = torch.full((W * C * 4 + 1 + TAIL,), float("nan"), device=DEV)
    recv = torch.zeros(W * 4 + 1, device=DEV)
    outs.append(rows)
    refused("rs_exchange_scatter_late", L.ptr(recv), L.ptr(inv), W, C, 1, 4, L.ptr(rows[1:]))
    refused("rs_exchange_scatter_late", L.ptr(recv[1:]), L.ptr(inv), W, C, 1, 4, L.ptr(rows))
    shard = torch.zeros(10 * 4 + 1, device=DEV)
    idz = torch.zeros(3, dtype=torch.int32, device=DEV)
    refused("rs_gather_rows_padded", L.ptr(shard[1:]), 10, 4, L.ptr(idz), 3, L.ptr(rows))
    refused("rs_gather_rows_padded", L.ptr(shard), 10, 4, L.ptr(idz), 3, L.ptr(rows[1:]))
    # the ranged dedup's key range
    g = torch.zeros(n, 128, device=DEV)
    sk = dev(np.arange(n, dtype=np.int32))
    w = L.scratch(L.lib().rs_dedup_workspace_size(n, 128), DEV)
    out = fbuf(n, 128)
    outs.append(out)
    rng_call = lambda d, lo, hi: (RANGE, L.ptr(sk), L.ptr(ids), n, L.ptr(g), None, 1, d, 20, lo, hi,
                                  0, None, None, fresh(), L.ptr(out), L.ptr(w), w.numel())
    refused(*rng_call(128, 7, 7))    # key_lo >= key_hi
    refused(*rng_call(128, 9, 7))
    refused(*rng_call(128, 0, 21))   # key_hi > n_rows
    refused(*rng_call(16, 5, 20))    # key_lo != 0 at D = 16
    torch.cuda.synchronize()
    for t in outs:
        untouched(t, 0, "an output of a refused call")
