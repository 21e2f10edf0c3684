"""Deterministic inputs, float64 restatements and magnitude bounds for the edge tests of
csrc/eges.hip: the fused match logits, the side pooling in its scalar, half-wave vector and
multi-task forms, and the pair sampler (prefix weights, walks, skip-grams, log-uniform
negatives). tests/test_eges_edges_cpu.py proves each input has the property its name claims and
that a plain fp32 evaluation meets every bound with room; tests/test_eges_edges_gpu.py runs the
inputs through the kernels. NumPy only; nothing here calls a kernel.

The tolerance is the project's: |got - ref64| <= 1e-5 · Σ|terms|, the magnitude sum formed in
float64 per element. Where a kernel's arithmetic is one fp32 operation or a documented order of
adds, the reference is the fp32 NumPy evaluation and the comparison is on bits.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32
RTOL = 1e-5
ATTN_FLOOR = 1e-37  # below it a softmax weight is (nearly) denormal: no relative bound holds
WAVE, WAVES_PER_BLOCK, MAX_SIDE, MAX_TASKS = 64, 4, 16, 4  # csrc/eges.hip


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def sum_seq32(x, axis=-1):
    """Σ along `axis` in float32, one element after the other from 0."""
    x = np.moveaxis(f32(x), axis, 0)
    acc = np.zeros(x.shape[1:], np.float32)
    for v in x:
        acc = (acc + v).astype(np.float32)
    return acc


def sum_tree32(x, axis=-1):
    """Σ along `axis` in float32 as a balanced tree (halves folded onto each other)."""
    x = np.moveaxis(f32(x), axis, 0)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], np.float32)
    while x.shape[0] > 1:
        if x.shape[0] % 2:
            x = np.concatenate([x, np.zeros((1,) + x.shape[1:], np.float32)])
        h = x.shape[0] // 2
        x = (x[:h] + x[h:]).astype(np.float32)
    return x[0]


SUMS32 = {"sequential": sum_seq32, "pairwise": sum_tree32}


def off_by(got, ref, bound, frac=1.0):
    """max over the elements of |got - ref| / (frac · bound) (0 where both are 0; inf for a NaN or
    an element off where the bound is 0)."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    b = frac * np.broadcast_to(np.asarray(bound, np.float64), r.shape)
    assert g.shape == r.shape, (g.shape, r.shape)
    if r.size == 0:
        return 0.0
    err = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / b)
    q = np.where(np.isnan(g) | np.isnan(q), np.inf, q)
    return float(q.max())


def within(got, ref, bound, msg, frac=1.0):
    q = off_by(got, ref, bound, frac)
    print(f"  {msg}: max err/bound {q:.3g}")
    assert q <= 1.0, f"{msg}: off by {q:.3g} x the bound"


# =============================================================================================
# 1. match logits: logits[b, j] = table[ids[b, j]] · hidden[b]
MATCH_ROWS = 37
MATCH_D = (1, 3, 63, 64, 65, 128, 130)  # the 64-lane stride loop at 0, 1, 2 passes, ragged
MATCH_M = (1, 6)
MATCH_B = (1, 3, 4, 5, 9)               # four waves per block: empty waves in the last block
MATCH_KINDS = ("gauss", "cancel", "same_row")


def _match_cases():
    cases = []
    for i, D in enumerate(MATCH_D):
        for j, kind in enumerate(MATCH_KINDS):
            cases.append((D, MATCH_M[(i + j) % 2], MATCH_B[(2 * i + j) % 5],
                          bool((i + j // 2 + j) % 2), kind))
    return tuple(cases)


MATCH_CASES = _match_cases()  # (D, M, B, id64, kind): 21 cases


def match_inputs(D, M, B, kind, n_rows=MATCH_ROWS):
    """table [n_rows, D], ids [B, M] (int64, all valid), hidden [B, D], g [B, M].
    gauss: everything N(0, 1). cancel: hidden[b] = (b + 1)·u with u_{2k} = u_{2k+1}, the rows
    = u with signs + - + - ... (odd rows: - + - + ...): for even D every logit is exactly 0 in
    exact arithmetic, for odd D it is the last term alone. same_row: one example (the last) has
    the same row in all its M slots."""
    rng = np.random.default_rng([D, M, B, MATCH_KINDS.index(kind), 5])
    table = rng.standard_normal((n_rows, D)).astype(np.float32)
    hidden = rng.standard_normal((B, D)).astype(np.float32)
    ids = rng.integers(0, n_rows, (B, M)).astype(np.int64)
    g = rng.standard_normal((B, M)).astype(np.float32)
    if kind == "cancel":
        u = np.repeat(rng.standard_normal((D + 1) // 2), 2)[:D].astype(np.float32)
        sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
        table = (u * sign)[None, :] * np.where(np.arange(n_rows) % 2 == 0, 1.0, -1.0)[:, None]
        table = table.astype(np.float32)
        hidden = (u[None, :] * np.arange(1, B + 1, dtype=np.float32)[:, None]).astype(np.float32)
    if kind == "same_row":
        ids[B - 1, :] = 11
    return table, ids, hidden, g


def match_ref(table, ids, hidden, g, n_rows=None):
    """float64 on the fp32 inputs; an id outside [0, n_rows) reads a zero row.
    → dict(logits, logits_mag = Σ_d |row||h|, grad_rows32 = fp32(g·h) [B, M, D] (one multiply:
    compared on bits), grad_hidden = Σ_j g_j row_j, grad_hidden_mag = Σ_j |g_j||row_j|, valid)."""
    n_rows = table.shape[0] if n_rows is None else n_rows
    ids = np.asarray(ids, np.int64)
    valid = (ids >= 0) & (ids < n_rows)
    t64 = table.astype(np.float64)
    rows = np.where(valid[..., None], t64[np.where(valid, ids, 0)], 0.0)  # [B, M, D]
    h64, g64 = hidden.astype(np.float64), g.astype(np.float64)
    return dict(
        logits=np.einsum("bmd,bd->bm", rows, h64),
        logits_mag=np.einsum("bmd,bd->bm", np.abs(rows), np.abs(h64)),
        grad_rows32=(g[:, :, None] * hidden[:, None, :]).astype(np.float32),
        grad_hidden=np.einsum("bm,bmd->bd", g64, rows),
        grad_hidden_mag=np.einsum("bm,bmd->bd", np.abs(g64), np.abs(rows)),
        valid=valid)


def match_f32(table, ids, hidden, g, order):
    """A plain fp32 evaluation of the same two sums in the summation order `order`."""
    S = SUMS32[order]
    valid = (ids >= 0) & (ids < table.shape[0])
    rows = np.where(valid[..., None], table[np.where(valid, ids, 0)], np.float32(0))
    logits = S(rows * hidden[:, None, :], -1)
    gh = S(g[:, :, None] * rows, 1)
    return logits, gh


def oob_values(n_rows=MATCH_ROWS):
    """(name, value, needs int64): -1, n_rows, 2^32 + 1 (low word 1: must not alias row 1) and
    the smallest int64 (low word 0: must not alias row 0)."""
    return (("minus_one", -1, False), ("n_rows", n_rows, False),
            ("2^32+1", 2 ** 32 + 1, True), ("int64_min", -2 ** 63, True))


# =============================================================================================
# 2. side pooling: hidden[b] = Σ_s a[b, s] side[b, s], a = softmax(w[b]) or 1 / S
POOL_SCALAR_D = (1, 2, 33, 63, 65, 132, 200)
POOL_VECTOR_D = (4, 8, 60, 64, 124, 128)
POOL_B = (1, 2, 3, 7, 8, 9)  # vector form: 2 examples a wave, 8 a block; odd B: an empty half
POOL_S = (1, 2, 3, 15, 16)
LOGIT_KINDS = ("gauss", "equal", "spread60", "offset1e4", "neg1e30")
POOL_MODES = LOGIT_KINDS + ("mean",)
LAYOUTS = ("dense", "ebh", "padded")
NEG_BIG = np.float32(-1e30)


def _pool_cases(ds):
    """Every D under every mode, and under every B and every S (both rotate with the mode)."""
    return tuple((D, POOL_B[(i + j) % 6], POOL_S[(i + 2 * j) % 5], mode)
                 for i, D in enumerate(ds) for j, mode in enumerate(POOL_MODES))


POOL_SCALAR_CASES = _pool_cases(POOL_SCALAR_D)  # (D, B, S, mode): 42 cases
POOL_VECTOR_CASES = _pool_cases(POOL_VECTOR_D)  # 36 cases


def pool_vec_ok(D, sb, ss, offsets=(0,)):
    """csrc/eges.hip pool_vec_ok restated: the half-wave float4 kernels take D % 4 == 0,
    D <= 128, both strides multiples of 4 floats and every pointer on 16 bytes (offsets: each
    pointer's distance in floats from a 16-byte aligned address)."""
    return (D % 4 == 0 and D <= 128 and sb % 4 == 0 and ss % 4 == 0
            and all(o % 4 == 0 for o in offsets))


def pool_route(D, S, sb, ss, offsets=(0,)):
    """'vector', 'scalar' or 'rejected': the contract of rs_side_pool_{fwd,bwd}_strided."""
    if pool_vec_ok(D, sb, ss, offsets):
        return "vector"
    return "scalar" if (sb == S * D and ss == D) else "rejected"


def layout_strides(layout, B, S, D):
    """(sb, ss, floats in the buffer) of side[b, s] at b·sb + s·ss. dense: [B, S, D]. ebh: MMOE's
    [E, B, H] expert outputs seen as [B, E, H]. padded: 4 floats behind every row, 8 more behind
    every example."""
    if layout == "dense":
        return S * D, D, B * S * D
    if layout == "ebh":
        return D, B * D, S * B * D
    ss = D + 4
    sb = S * ss + 8
    return sb, ss, B * sb


def pool_logits(kind, B, S, rng):
    """[B, S] float32 gate logits. gauss: N(0, 1). equal: one value per row. spread60: one entry
    +60, the others -60 (exp(-120) underflows float32: one weight exactly 1, the others exactly
    0). offset1e4: 1e4 + N(0, 1) (exp overflows without the max subtraction). neg1e30: N(0, 1)
    with entry b % S of row b at -1e30 when S >= 2 (its weight is exactly 0)."""
    w = rng.standard_normal((B, S)).astype(np.float32)
    r = np.arange(B)
    if kind == "equal":
        w = np.repeat(w[:, :1], S, 1)
    elif kind == "spread60":
        w = np.full((B, S), -60.0, np.float32)
        w[r, (r + 1) % S] = 60.0
    elif kind == "offset1e4":
        w = (np.float32(1e4) + w).astype(np.float32)
    elif kind == "neg1e30" and S >= 2:
        w[r, r % S] = NEG_BIG
    return w


def pool_inputs(D, B, S, mode, seed=0):
    """side [B, S, D], logits [B, S] (None in mean mode), g [B, D]: N(0, 1) but for the logits."""
    rng = np.random.default_rng([D, B, S, POOL_MODES.index(mode), seed])
    side = rng.standard_normal((B, S, D)).astype(np.float32)
    g = rng.standard_normal((B, D)).astype(np.float32)
    wl = None if mode == "mean" else pool_logits(mode, B, S, rng)
    return side, wl, g


def softmax64(w):
    w = np.asarray(w, np.float64)
    e = np.exp(w - w.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax32(w, subtract_max=True):
    """The kernels' softmax in plain float32 NumPy (sum in s order)."""
    w = f32(w)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (w - w.max(-1, keepdims=True)).astype(np.float32) if subtract_max else w
        e = np.exp(x).astype(np.float32)
        return (e / sum_seq32(e, -1)[..., None]).astype(np.float32)


def pool_fwd_ref(side, wl):
    """float64 forward. softmax: dict(attn, attn32 = attn rounded to float32, the backward's
    input, hidden, hidden_mag = Σ_s a_s |x_s|). mean: dict(hidden32): the fp32 evaluation 'sum s
    ascending from 0, one division by float(S)', compared on bits."""
    S = side.shape[1]
    if wl is None:
        return dict(hidden32=(sum_seq32(side, 1) / np.float32(S)).astype(np.float32))
    a = softmax64(wl)
    x = side.astype(np.float64)
    return dict(attn=a, attn32=a.astype(np.float32), hidden=np.einsum("bs,bsd->bd", a, x),
                hidden_mag=np.einsum("bs,bsd->bd", a, np.abs(x)), side_abs_sum=np.abs(x).sum(1))


def attn_bound(a64):
    return RTOL * a64 + ATTN_FLOOR


def pool_bwd_ref(side, attn32, g):
    """float64 backward as a function of the kernel's own inputs (side, the float32 softmax
    weights, g). softmax: dict(grad_side = a_s g, grad_side_mag = a_s |g|, grad_w = a_s (ga_s -
    Σ_t a_t ga_t) with ga_s = <g, x_s>, grad_w_mag = a_s (Σ_d |g||x_s| + Σ_t a_t Σ_d |g||x_t|)).
    mean (attn32 None): dict(grad_side32 = g / float(S) broadcast over s), on bits."""
    B, S, D = side.shape
    if attn32 is None:
        v = (g / np.float32(S)).astype(np.float32)
        return dict(grad_side32=np.repeat(v[:, None, :], S, 1))
    a, x, g64 = attn32.astype(np.float64), side.astype(np.float64), g.astype(np.float64)
    ga = np.einsum("bd,bsd->bs", g64, x)
    gam = np.einsum("bd,bsd->bs", np.abs(g64), np.abs(x))
    return dict(grad_side=a[:, :, None] * g64[:, None, :],
                grad_side_mag=a[:, :, None] * np.abs(g64)[:, None, :],
                grad_w=a * (ga - (a * ga).sum(-1, keepdims=True)),
                grad_w_mag=a * (gam + (a * gam).sum(-1, keepdims=True)))


def pool_f32(side, wl, g, order, attn32=None, subtract_max=True, shift=0, off_by_one=False):
    """A plain fp32 evaluation of forward and backward, the D sums in the order `order`.
    → dict(attn, hidden, grad_side, grad_w). The last three arguments make it deliberately
    wrong: no max subtraction; the weights applied to side s + shift; the last example of an odd
    batch reading the example before it (an upper half-wave taking its neighbour's index)."""
    Ssum = SUMS32[order]
    a = softmax32(wl, subtract_max)
    x = side
    if off_by_one and side.shape[0] % 2 == 1 and side.shape[0] > 1:
        x = side.copy()
        x[-1] = side[-2]
    aw = np.roll(a, shift, axis=1)
    hidden = sum_seq32(aw[:, :, None] * x, 1)
    ab = a if attn32 is None else attn32
    gs = (ab[:, :, None] * g[:, None, :]).astype(np.float32)
    ga = Ssum(g[:, None, :] * x, -1)
    dot = sum_seq32(ab * ga, -1)
    gw = (ab * (ga - dot[:, None])).astype(np.float32)
    return dict(attn=a, hidden=hidden, grad_side=gs, grad_w=gw)


def hidden_bound(ref):
    """1e-5 · Σ_s a_s |x_s|, plus ATTN_FLOOR · Σ_s |x_s|: a softmax weight under float32's range
    (exp(-120) = 8e-53 is 0 in float32) is granted ATTN_FLOOR absolute by attn_bound, and hidden
    is linear in the weights, so each weight's grant reaches hidden times |x_s|. It only matters
    where every representable weight meets a side value of exactly 0 (a relu output under the
    saturated weight): the float64 value is then 1e-52, the float32 one 0."""
    return RTOL * ref["hidden_mag"] + ATTN_FLOOR * ref["side_abs_sum"]


def pool_check_fwd(attn, hidden, ref, msg, frac=1.0):
    within(attn, ref["attn"], attn_bound(ref["attn"]), f"{msg} attn", frac)
    within(hidden, ref["hidden"], hidden_bound(ref), f"{msg} hidden", frac)


def pool_check_bwd(grad_side, grad_w, ref, msg, frac=1.0):
    within(grad_side, ref["grad_side"], RTOL * ref["grad_side_mag"], f"{msg} grad_side", frac)
    within(grad_w, ref["grad_w"], RTOL * ref["grad_w_mag"], f"{msg} grad_w", frac)


# ---- multi form: T poolings of the same side rows ------------------------------------------
MULTI_T, MULTI_E, MULTI_H, MULTI_B = (1, 2, 4), (1, 8, 16), (4, 80, 128), (1, 7, 9)
# (T, E, H, B, logit kind): a Latin square over the four lists
MULTI_CASES = tuple((MULTI_T[i], MULTI_E[j], MULTI_H[(i + j) % 3], MULTI_B[(i + 2 * j) % 3],
                     LOGIT_KINDS[(3 * i + j) % 5]) for i in range(3) for j in range(3))
MULTI_EXTRA_LD = 3  # columns of the logit buffers behind the T·E the tasks use


def multi_inputs(T, E, H, B, kind, with_bias=False):
    """side [B, E, H], logits [T, B, E], g [T, B, H]; with_bias: side holds pre-activations z
    and bias is [E, H]; z[b, s, 0] = -bias[s, 0] (z + bias exactly 0) where b + s is even, z
    negative on half the entries."""
    rng = np.random.default_rng([T, E, H, B, LOGIT_KINDS.index(kind), int(with_bias)])
    side = rng.standard_normal((B, E, H)).astype(np.float32)
    wl = np.stack([pool_logits(kind, B, E, rng) for _ in range(T)])
    g = rng.standard_normal((T, B, H)).astype(np.float32)
    bias = None
    if with_bias:
        bias = rng.standard_normal((E, H)).astype(np.float32)
        bb, ss = np.nonzero((np.arange(B)[:, None] + np.arange(E)[None, :]) % 2 == 0)
        side[bb, ss, 0] = -bias[ss, 0]
    return side, wl, g, bias


def relu_bias32(z, bias):
    """relu(z + bias[s]) in float32: one add, one max against +0."""
    return np.maximum((z + bias[None, :, :]).astype(np.float32), np.float32(0))


def multi_grad_side_ref(attn32s, gs):
    """Σ_t a_t[s] g_t and its magnitude Σ_t a_t[s] |g_t|, float64."""
    a = np.stack(attn32s).astype(np.float64)  # [T, B, S]
    g64 = np.stack(gs).astype(np.float64)     # [T, B, D]
    return (np.einsum("tbs,tbd->bsd", a, g64), np.einsum("tbs,tbd->bsd", a, np.abs(g64)))


def multi_grad_side_sum32(attn32s, gs):
    """The task-ordered fp32 sum the code documents: each product rounded, added from task 0."""
    acc = None
    for a, g in zip(attn32s, gs):
        q = (a[:, :, None] * g[:, None, :]).astype(np.float32)
        acc = q if acc is None else (acc + q).astype(np.float32)
    return acc


# =============================================================================================
# 3. pair sampler
SCAN_TILE = 4096  # kScanTile of csrc/sort.hip
SEED = 0x0123456789ABCDEF  # both key words of the Philox key in use
STEP = 3

# named nodes of edge_graph
N_OOV, N_HUB, N_EDGELESS, N_ALLZERO, N_ZERO_FIRST, N_ZERO_LAST, N_ZERO_MID = 0, 1, 2, 3, 4, 5, 6
N_SINGLE, N_SELF, N_EXTREME, N_DENORM = 7, 8, 9, 10
N_FILLER0 = 16
HUB_DEGREE = 1200
GRAPH_NODES = (200, 300)  # rs_csr_weight_prefix: one thread a node, 256 a block
DENORMAL = np.float32(1e-40)


@functools.lru_cache(maxsize=None)
def edge_graph(n_nodes):
    """A hand-built CSR graph (indptr int64 [n + 1], indices int32, weights float32).
    Node 0: OOV, no edges. 1: the hub every walk starts at (n_items = 2), 1200 edges, every
    fourth of weight 0 and pointing at node 0 (which no positive edge reaches). 2: no edges.
    3: three edges, all weight 0. 4 / 5 / 6: a weight-0 edge first / last / in the middle, each
    pointing at node 0. 7: a single edge. 8: a self-loop and a way out. 9: a denormal, a 1e30
    and a 1e-3 weight side by side (the float64 prefix absorbs the last). 10: denormal weights
    only. 11-15: plain. From 16 on: filler nodes in a ring with chords back to nodes 1-15."""
    assert n_nodes >= 64
    adj = {v: [] for v in range(n_nodes)}
    special = list(range(2, N_FILLER0))
    for k in range(HUB_DEGREE):
        if k % 4 == 0:
            adj[N_HUB].append((N_OOV, 0.0))
        elif k % 4 == 1:
            adj[N_HUB].append((special[(k // 4) % len(special)], 40.0 + (k % 7)))
        else:
            adj[N_HUB].append((N_FILLER0 + (k * 7) % (n_nodes - N_FILLER0), 0.25 * (1 + k % 5)))
    adj[N_ALLZERO] = [(N_HUB, 0.0), (N_SELF, 0.0), (N_SINGLE, 0.0)]
    adj[N_ZERO_FIRST] = [(N_OOV, 0.0), (N_ZERO_LAST, 1.0), (N_ZERO_MID, 2.0)]
    adj[N_ZERO_LAST] = [(N_ZERO_MID, 1.5), (N_SINGLE, 0.5), (N_OOV, 0.0)]
    adj[N_ZERO_MID] = [(N_SELF, 3.0), (N_OOV, 0.0), (N_EXTREME, 1.0)]
    adj[N_SINGLE] = [(N_HUB, 2.0)]
    adj[N_SELF] = [(N_SELF, 1.0), (N_DENORM, 1.0), (N_EDGELESS, 0.5)]
    adj[N_EXTREME] = [(11, float(DENORMAL)), (12, 1e30), (13, 1e-3)]
    adj[N_DENORM] = [(N_HUB, float(DENORMAL)), (N_ZERO_FIRST, float(DENORMAL))]
    for v in range(11, N_FILLER0):
        adj[v] = [(N_HUB, 1.0), (v - 8, 2.0), (N_ALLZERO, 0.5)]
    for v in range(N_FILLER0, n_nodes):
        nxt = N_FILLER0 + (v - N_FILLER0 + 1) % (n_nodes - N_FILLER0)
        adj[v] = [(nxt, 1.0), (1 + v % 15, 3.0), (N_OOV, 0.0), (N_HUB, 0.75)]
    indptr = np.zeros(n_nodes + 1, np.int64)
    indices, w = [], []
    for v in range(n_nodes):
        indptr[v + 1] = indptr[v] + len(adj[v])
        indices += [t for t, _ in adj[v]]
        w += [x for _, x in adj[v]]
    return indptr, np.asarray(indices, np.int32), np.asarray(w, np.float32)


WALK_COUNTS = (1, 255, 256, 257)
WALK_LENGTHS = (0, 1, 12)
WALK_BASE = 4_000_000_000  # past 2^31: the walk index is a uint32 counter word


def dead_end(graph, v):
    indptr, _, w = graph
    return not (w[indptr[v]:indptr[v + 1]].astype(np.float64).sum() > 0.0)


def check_walks(graph, traces, n_items):
    """The properties of a walk set that need no oracle: column 0 in [1, n_items); each step
    follows an existing edge of positive weight; a walk at a node without positive out-weight is
    -1 from the next entry to the end; a walk elsewhere goes on."""
    indptr, indices, w = graph
    tr = np.asarray(traces)
    assert ((tr[:, 0] >= 1) & (tr[:, 0] < n_items)).all(), "start outside [1, n_items)"
    for row in tr:
        for u, v in zip(row[:-1], row[1:]):
            if u < 0:
                assert v == -1, f"a walk went on after its dead end: {row}"
            elif dead_end(graph, u):
                assert v == -1, f"a step out of node {u}, which has no positive edge: {row}"
            else:
                e = slice(indptr[u], indptr[u + 1])
                assert ((indices[e] == v) & (w[e] > 0)).any(), f"{u} -> {v} is no positive edge: {row}"


# ---- skip-grams -----------------------------------------------------------------------------
def skipgram_slots(length, window):
    return sum(min(length, i + window + 1) - max(0, i - window) - 1 for i in range(length))


# (name, n_traces, len, window, fill). The slot count of a trace is even (every (i, j) comes with
# (j, i)), so n_traces · slots is never 4097: the scan tile is crossed at 4094 / 4096 / 4098 in
# steps of 2 slots and of 6 slots (683 · 6 = 4098).
SKIPGRAM_CASES = (
    ("len1", 5, 1, 3, "valid"),                # zero slots
    ("window_ge_len", 7, 4, 4, "holes"),
    ("window_gt_len", 3, 5, 9, "holes"),
    ("window1", 9, 6, 1, "holes"),
    ("no_traces", 0, 6, 2, "valid"),
    ("all_valid", 11, 7, 3, "valid"),
    ("all_dead", 4, 11, 5, "dead"),
    ("tile_minus_2", 2047, 2, 1, "holes"),
    ("tile_exact", 2048, 2, 1, "holes"),
    ("tile_plus_2", 2049, 2, 1, "holes"),
    ("tile_plus_2_of_6", 683, 3, 2, "holes"),
    ("two_tiles_valid", 4097, 2, 1, "valid"),  # 8194 slots, every flag set
)


def skipgram_traces(n_traces, length, fill):
    """int32 [n_traces, length] of items 1..99. holes: with k = (t + 4) % 6, trace t has a 0 at
    position 0 (k = 1), -1 at the last (k = 2), 0 in the middle (k = 3) (0 and -1 swapped in
    every other group of six traces), -1 from the middle to the end (k = 4), is all -1 (k = 5),
    or is all valid (k = 0: trace 2048, the first behind the scan tile in the two-slot cases,
    is)."""
    rng = np.random.default_rng([n_traces, length, 17])
    tr = rng.integers(1, 100, (n_traces, length)).astype(np.int32)
    if fill == "dead":
        tr[:] = -1
    if fill == "holes":
        t = np.arange(n_traces)
        k = (t + 4) % 6
        hole = np.where((t // 6) % 2 == 0, 0, -1).astype(np.int32)  # 0 and -1 take turns
        tr[k == 1, 0] = hole[k == 1]
        tr[k == 2, -1] = -1 - hole[k == 2]
        tr[k == 3, length // 2] = hole[k == 3]
        tr[k == 4, length // 2:] = -1
        tr[k == 5, :] = -1
    return tr


def skipgram_ref(traces, window):
    """keras skipgrams(negative_samples=0) in enumeration order, entries <= 0 skipped, written
    independently of oracle/eges.py (vectorised over the traces)."""
    tr = np.asarray(traces)
    n, ln = tr.shape
    tgt, ctx = [], []
    cols = [(i, j) for i in range(ln) for j in range(max(0, i - window), min(ln, i + window + 1))
            if j != i]
    if not cols or n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    ii, jj = np.array(cols).T
    a, b = tr[:, ii], tr[:, jj]  # [n, slots]
    keep = (a > 0) & (b > 0)
    return a[keep].astype(np.int32), b[keep].astype(np.int32)


# ---- log-uniform negatives -------------------------------------------------------------------
BIG_RANGE = 2 ** 20 + 3
# (range_max, num_sampled, n_pairs): every size pair of the table, n_pairs in {1, 255, 257}
# (<= 64 for the large table, whose oracle loops in Python)
NEG_CASES = ((1, 1, 1), (1, 1, 257), (2, 1, 255), (2, 2, 257), (20, 20, 1), (20, 20, 255),
             (300, 5, 255), (300, 5, 257), (BIG_RANGE, 5, 1), (BIG_RANGE, 5, 64))
NEG_PAIR_BASE = 3_000_000_123  # past 2^31
RETRY_RANGE, RETRY_SAMPLED, RETRY_PAIRS = 4, 2, 8
RETRY_DRAWS = 4096 * RETRY_SAMPLED  # the kernel's own bound


def log_uniform_cdf(range_max):
    """cdf[k] = floor(log(k + 2) / log(range_max + 1) · 2^32), capped at 2^32 - 1."""
    p = np.log(np.arange(2, range_max + 2, dtype=np.float64)) / np.log(range_max + 1.0)
    return np.minimum(np.floor(p * 4294967296.0), 4294967295.0).astype(np.uint32)


SKEW_RANGE, SKEW_SAMPLED, SKEW_PAIRS = 1000, 5, 257


def skewed_cdf(kind):
    """Hand-made 1000-class tables on which the kernel's float guess exp2(r · log2(1001) / 2^32)
    - 1 is hundreds of classes from the answer, whatever the rounding of exp2f (on the log-uniform
    tables it is off by two at most, and on which side depends on the device's exp2f):
    'down': every entry doubled and capped at 2^32 - 1: only classes 0..30 can be drawn, the
    guess is up to 970 above the answer (the walk down the table).
    'up': every entry halved: the answer is near (guess + 1)^2, or the last class for every draw
    from 2^31 on (the walk up the table and its stop at range_max - 1)."""
    c = log_uniform_cdf(SKEW_RANGE).astype(np.uint64)
    if kind == "down":
        return np.minimum(2 * c, 0xFFFFFFFF).astype(np.uint32)
    return (c // 2).astype(np.uint32)


def log_uniform_ref(cdf, pair_base, n_pairs, num_sampled, seed, step):
    """oracle.eges.log_uniform_sample's rule with all the pairs advanced together, one draw
    index at a time (the oracle's Python loop over pairs and draws takes 5 s for 255 rows of
    20 out of 20); tests/test_eges_edges_cpu.py holds it equal to the oracle."""
    from oracle.eges import PURPOSE_NEG
    from oracle.pinsage import draw

    out = np.full((n_pairs, num_sampled), -1, np.int32)
    got = np.zeros(n_pairs, np.int64)
    gp = pair_base + np.arange(n_pairs, dtype=np.int64)
    active, d = np.arange(n_pairs), 0
    while active.size:
        r = draw(seed, PURPOSE_NEG, gp[active], 0, step, d)
        k = np.minimum(np.searchsorted(cdf, r, side="right"), len(cdf) - 1).astype(np.int32)
        new = ~(out[active] == k[:, None]).any(1)
        rows = active[new]
        out[rows, got[rows]] = k[new]
        got[rows] += 1
        active = active[got[active] < num_sampled]
        d += 1
    return out


def check_negatives(out, range_max, num_sampled):
    out = np.asarray(out)
    assert ((out >= 0) & (out < range_max)).all(), "a class outside [0, range_max)"
    s = np.sort(out, 1)
    assert (s[:, 1:] != s[:, :-1]).all(), "a row repeats a class"
    if num_sampled == range_max:
        assert (s == np.arange(range_max)[None, :]).all(), "not a permutation of all classes"
