"""Inputs and float64 restatements for the edge tests of the three software-pipelined DLRM
kernels of csrc/interaction.hip (dlrm_train_chunk, dlrm_fwd_dx_pipe, dlrm_bwd_pipe). No GPU is
touched here: every builder returns CPU tensors, every restatement computes on the device of its
arguments, so tests/test_dlrm_edges_cpu.py can prove both without the library and
tests/test_dlrm_edges_gpu.py uses them on the card.

`reference` and `close` are the north-star restatement and bound of tests/test_train_unit_gpu.py
(which imports them from here): |got − ref| ≤ 1e-5 · Σ|terms| + 1e-30 per element.
"""
import numpy as np
import torch

NI = 13
EPS = 1e-7
EPS32 = np.float32(1e-7)
HI32 = np.float32(1) - EPS32          # 0.99999988: the clip's upper end as the kernel forms it
GUARD = 64                            # elements behind every output
GUARD_BITS = 0x7FC5A5A5               # a quiet NaN with a recognisable payload
I64_MIN = -2 ** 63


# =============================================================================================
# arithmetic of the launchers
def next_prime(n):
    """The first prime above n."""
    c = n + 1
    while any(c % d == 0 for d in range(2, int(c ** 0.5) + 1)):
        c += 1
    return c


def walk_batch(n_cus):
    """A batch at which every wave of the 256-thread pipelined kernels walks at least two
    examples: above 8 blocks x 4 waves x 2 rounds per CU (more than can be resident at any
    occupancy), and prime, so the last active wave is cut short whatever epw comes out."""
    return next_prime(64 * n_cus)


def nzc_of(F):
    return F * (F - 1) // 2


def grad_width(F, D, compact):
    """Width of the interaction row / its upstream gradient (out_width + D)."""
    return (nzc_of(F) if compact else F * F) + D


def bwd_pipe_instance(F, D, compact):
    """(GREG, KS) of the dlrm_bwd_pipe instantiation launch_bwd picks; None: the generic kernel
    (or inter_bwd_mfma for D != 128)."""
    gw = grad_width(F, D, compact)
    if not (F <= 32 and D == 128 and gw <= 20 * 64):
        return None
    return (8 if gw <= 8 * 64 else 20, 14 if F <= 28 else 16)


def fold_shape(blocks):
    """(per_seg, n_seg, chunks of the last segment) of fold_two_level for `blocks` chunks."""
    per = -(-blocks // 32)
    nseg = -(-blocks // per)
    return per, nseg, blocks - per * (nseg - 1)


def batch_for_blocks(blocks):
    """The smallest batch that gives the train kernel `blocks` blocks at one example per wave."""
    return 4 * (blocks - 1) + 1


# =============================================================================================
# inputs
def relu_dense(B, D, g):
    """The bottom MLP's output as production has it: relu(randn), so about half exact zeros; some
    of them −0.0; column D − 3 all zero (both signs); a few negative entries (which a relu never
    gives, but earlier tests feed) outside that column."""
    d = torch.relu(torch.randn(B, D, generator=g))
    d[::3, 1::9] = -0.0
    d[:, D - 3] = 0.0
    d[1::2, D - 3] = -0.0
    d[::5, 2] = -0.25
    d[3::17, D - 1] = -1.5
    return d


def train_inputs(B, S, D, id64, seed, cards=None, shared=False, oob=False, qscale=0.05):
    """(table, ids, offs, dense, xin, label, q, c) as CPU tensors. cards: rows per slot (default
    40 each); shared: one table of sum(cards) rows for every slot, offs = None."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cards = [40] * S if cards is None else list(cards)
    assert len(cards) == S
    V = int(sum(cards))
    table = torch.randn(V, D, generator=g) * 0.5
    if shared:
        ids = torch.randint(0, V, (B, S), generator=g)
        offs = None
    else:
        ids = torch.stack([torch.randint(0, int(c), (B,), generator=g) for c in cards], 1)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(cards)]), dtype=torch.int64)
    if oob:
        ids[::7, 3 % S] = V   # beyond every slot's range
        ids[::11, 0] = -1
    ids = ids.to(torch.int64 if id64 else torch.int32).contiguous()
    dense = relu_dense(B, D, g)
    xin = torch.rand(B, NI, generator=g)
    label = (torch.rand(B, generator=g) < 0.3).float()
    F = S + 1
    q = torch.randn(nzc_of(F) + D, generator=g) * qscale
    c = torch.tensor([0.1])
    return table, ids, offs, dense, xin, label, q, c


def edge_ids(B, cards, id64, seed):
    """[B, S] ids on a slab of uneven cardinalities: in range everywhere, then per slot the last
    valid id (card − 1) and the out-of-range ones (card, −1; with int64 also 2^32 + 1 and the
    smallest int64) on rows of their own, and row B − 1 out of range in every slot. Returns
    (ids, bad) with bad[b, s] true where the id is out of range."""
    g = np.random.default_rng(seed)
    S = len(cards)
    ids = np.stack([g.integers(0, c, B) for c in cards], 1).astype(np.int64)
    outs = [lambda c: c, lambda c: -1]
    if id64:
        outs += [lambda c: 2 ** 32 + 1, lambda c: I64_MIN]
    assert B >= 2 + (len(outs) + 1) * S
    b = 1
    for s, c in enumerate(cards):
        ids[b, s] = c - 1
        b += 1
        for f in outs:
            ids[b, s] = f(c)
            b += 1
    ids[B - 1] = [outs[s % len(outs)](c) for s, c in enumerate(cards)]
    card = np.asarray(cards, np.int64)[None]
    bad = (ids < 0) | (ids >= card)
    t = torch.from_numpy(ids)
    return (t if id64 else t.to(torch.int32)).contiguous(), bad


def sweep_h():
    """Head pre-activations that cross both ends of the BCE clip: −20 … 20 in 257 steps, then
    15.0 … 17.5 in steps of 0.05 (the float32 sigmoid reaches 1 − eps near 16.1 and 1 near
    17.3)."""
    a = np.linspace(-20.0, 20.0, 257)
    b = 15.0 + 0.05 * np.arange(51)
    return np.concatenate([a, b]).astype(np.float32)


def sweep_classes(y):
    """Boolean masks over float32 predictions: below eps, exactly 1, inside the clip, and the ones
    within a factor 4 of eps on either side of the lower end."""
    y = np.asarray(y, np.float32)
    inside = (y >= EPS32) & (y <= HI32)
    return {"below": y < EPS32, "one": y == np.float32(1), "inside": inside,
            "near_in": inside & (y <= 4 * EPS32), "near_out": (y < EPS32) & (y >= EPS32 / 4)}


def clip_inputs(D, seed):
    """The train kernel's inputs with h_b = dense[b, 0] exactly: q's pair weights 0, q_dense =
    e_0, c = 0; dense[:, 0] = sweep_h(); labels 0, 1 and 0.3 in turn."""
    S = 2
    h = sweep_h()
    B = h.size
    table, ids, offs, dense, xin, label, q, c = train_inputs(B, S, D, False, seed)
    dense[:, 0] = torch.from_numpy(h)
    label = torch.tensor([0.0, 1.0, 0.3]).repeat(B // 3 + 1)[:B].contiguous()
    q = torch.zeros_like(q)
    q[nzc_of(S + 1)] = 1.0
    return table, ids, offs, dense, xin, label, q, torch.zeros(1)


def pow2_inputs(B, S, D, id64, seed):
    """Inputs whose table and dense entries have magnitudes in [2^-6, 2^6], so that 2^±8 times
    them stays far from denormals and overflow."""
    table, ids, offs, dense, xin, label, q, c = train_inputs(B, S, D, id64, seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)

    def draw(shape):
        mag = torch.exp2(torch.rand(shape, generator=g) * 12 - 6)
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        return (mag * sign).clamp(-64, 64)

    return draw(table.shape), ids, offs, draw(dense.shape), xin, label, q, c


# =============================================================================================
# the train step in float64 (moved from tests/test_train_unit_gpu.py; `gscale` and `mutate` added)
def reference(table, ids, offs, dense, xin, label, q, c, S, D, gscale=None, mutate=None):
    """float64: y, G, the unit rows U[b, s] and the batch sums; plus the magnitude bound of each
    (the same sums over |terms|). gscale: dL/dl_b (default 1/B, the mean). offs None: one table
    for every slot. mutate: a deliberately wrong variant (tests/test_dlrm_edges_cpu.py shows that
    autograd tells each from the right one): "relu_ge", "clip_no_upper", "bottom_row"."""
    f = torch.float64
    dev = table.device
    B = ids.shape[0]
    F = S + 1
    gs = 1.0 / B if gscale is None else float(gscale)
    idl = ids.long()
    if offs is None:
        lo = torch.zeros(1, S, dtype=torch.int64, device=dev)
        hi = lo + table.shape[0]
    else:
        lo, hi = offs[:-1][None, :], offs[1:][None, :]
    ok = (idl >= 0) & (idl < hi - lo)
    rowi = torch.where(ok, lo + idl, torch.zeros_like(idl))
    X = torch.cat([table.to(f)[rowi] * ok[..., None], dense.to(f)[:, None, :]], 1)  # [B, F, D]
    iu = torch.triu_indices(F, F, 1, device=dev)
    nz = iu.shape[1]
    qp, qd = q[:nz].to(f), q[nz:].to(f)
    Z = X @ X.transpose(1, 2)
    Zm = (X.abs() @ X.abs().transpose(1, 2))
    z = Z[:, iu[0], iu[1]]
    zm = Zm[:, iu[0], iu[1]]
    h = z @ qp + dense.to(f) @ qd + float(c)
    hm = zm @ qp.abs() + dense.to(f).abs() @ qd.abs() + abs(float(c))
    p = torch.sigmoid(h)
    lb = label.to(f)
    pc = p.clamp(EPS, 1 - EPS)
    loss = -(lb * torch.log(pc + EPS) + (1 - lb) * torch.log(1 - pc + EPS))
    inside = (p >= EPS) & (p <= 1 - EPS)
    if mutate == "clip_no_upper":
        inside = p >= EPS
    dbce = -(lb / (pc + EPS)) + (1 - lb) / ((1 - pc) + EPS)
    G = torch.where(inside, dbce * gs, torch.zeros_like(p)) * p * (1 - p)
    M = torch.zeros(F, F, dtype=f, device=dev)
    M[iu[0], iu[1]] = qp
    Sm = M + M.T
    U = Sm[None] @ X                                      # [B, F, D]
    Um = Sm.abs()[None] @ X.abs()
    zrow = torch.cat([z, dense.to(f)], 1)
    zrm = torch.cat([zm, dense.to(f).abs()], 1)
    live = dense >= 0 if mutate == "relu_ge" else dense > 0
    bot = S - 1 if mutate == "bottom_row" else S
    gbot = torch.where(live, G[:, None] * (U[:, bot] + qd[None]), torch.zeros_like(U[:, S]))
    # error carried into G by h's (|dG/dh| = y(1-y)·gs <= gs/4) on top of G's own magnitude
    gm = G.abs() + hm * gs / 4
    gbm = torch.where(live, gm[:, None] * (Um[:, bot] + qd.abs()[None]),
                      torch.zeros_like(U[:, S]))
    sums = {"A_top": (zrow * G[:, None]).sum(0), "s_top": G.sum(), "loss": loss.sum(),
            "A_bot": xin.to(f).T @ gbot, "s_bot": gbot.sum(0)}
    mags = {"A_top": (zrm * gm[:, None]).sum(0), "s_top": gm.sum(),
            "loss": (dbce.abs() * 0.25 * hm).sum() + 0.1 * loss.abs().sum(),
            "A_bot": xin.to(f).abs().T @ gbm, "s_bot": gbm.sum(0)}
    return p, hm, G, U[:, :S], Um[:, :S], sums, mags, nz, bool((~ok).any())


def close(got, ref, mag, msg, rel=1e-5):
    got = got.double()
    tol = rel * mag + 1e-30
    err = (got - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{msg}: {int(bad.sum())} / {bad.numel()} off, max err/tol "
                                 f"{float((err / tol).max()):.3g}")


# =============================================================================================
# Keras BCE and its derivative from a float32 prediction (the kernel's own y)
def bce_from_y(y, label, gscale):
    """From float32 y: (l, gate, G) in float64. pc = clip(y, eps, 1 − eps), pc + eps and
    (1 − pc) + eps are formed in float32 as the kernel forms them; the logs, the quotients and
    G = [eps <= y <= 1 − eps] · gscale · dBCE/dy · y(1 − y) in float64."""
    y = np.asarray(y, np.float32)
    lb = np.asarray(label, np.float64)
    pc = np.clip(y, EPS32, HI32)
    a = (pc + EPS32).astype(np.float32).astype(np.float64)
    b = ((np.float32(1) - pc) + EPS32).astype(np.float32).astype(np.float64)
    loss = -(lb * np.log(a) + (1 - lb) * np.log(b))
    gate = (y >= EPS32) & (y <= HI32)
    y64 = y.astype(np.float64)
    G = np.where(gate, float(gscale) * (-(lb / a) + (1 - lb) / b), 0.0) * (y64 * (1 - y64))
    return loss, gate, G


# =============================================================================================
# the interaction alone: forward row, head, unit backward, backward
def gather_x(table, ids, offs, dense, S):
    """float64 X [B, F, D] (a zero row for an out-of-range id) and the mask of valid ids."""
    f = torch.float64
    idl = ids.long()
    if offs is None:
        lo = torch.zeros(1, S, dtype=torch.int64, device=table.device)
        hi = lo + table.shape[0]
    else:
        lo, hi = offs[:-1][None, :], offs[1:][None, :]
    ok = (idl >= 0) & (idl < hi - lo)
    rowi = torch.where(ok, lo + idl, torch.zeros_like(idl))
    return torch.cat([table.to(f)[rowi] * ok[..., None], dense.to(f)[:, None, :]], 1), ok


def head_dx_reference(table, ids, offs, dense, q, c, S, act):
    """rs_dlrm_interaction_fwd_head_dx in float64: the compact pairs z, y = act(row·q + c), the
    unit gradient U = (M + Mᵀ)·X with q's dense part added to row S; each with its Σ|terms|."""
    f = torch.float64
    F = S + 1
    X, ok = gather_x(table, ids, offs, dense, S)
    iu = torch.triu_indices(F, F, 1, device=table.device)
    nz = iu.shape[1]
    qp, qd = q[:nz].to(f), q[nz:nz + dense.shape[1]].to(f)
    Xa = X.abs()
    z = (X @ X.transpose(1, 2))[:, iu[0], iu[1]]
    zm = (Xa @ Xa.transpose(1, 2))[:, iu[0], iu[1]]
    h = z @ qp + dense.to(f) @ qd + float(c)
    hm = zm @ qp.abs() + dense.to(f).abs() @ qd.abs() + abs(float(c))
    y = {0: h, 1: torch.relu(h), 2: torch.sigmoid(h)}[act]
    M = torch.zeros(F, F, dtype=f, device=table.device)
    M[iu[0], iu[1]] = qp
    Sm = M + M.T
    U = Sm[None] @ X
    Um = Sm.abs()[None] @ Xa
    U[:, S] += qd
    Um[:, S] += qd.abs()
    return z, zm, y, hm, U, Um, bool((~ok).any())


def bwd_reference(table, ids, offs, dense, gout, S, compact):
    """rs_dlrm_interaction_bwd in float64: with Ssym the symmetrised strict-upper part of the
    upstream gradient, dX = Ssym·X; the bottom row adds the concat's pass-through. Rows of
    out-of-range ids receive their gradient like any other (their X row is zero, the others are
    not). Returns (grad_emb [B, S, D], grad_dense [B, D]) and the Σ_k |g_k|·|x_k| of each."""
    f = torch.float64
    F = S + 1
    D = dense.shape[1]
    B = ids.shape[0]
    X, _ = gather_x(table, ids, offs, dense, S)
    iu = torch.triu_indices(F, F, 1, device=table.device)
    nz = iu.shape[1] if compact else F * F
    g = gout.to(f)
    up = g[:, :iu.shape[1]] if compact else g[:, iu[0] * F + iu[1]]
    Ss = torch.zeros(B, F, F, dtype=f, device=table.device)
    Ss[:, iu[0], iu[1]] = up
    Ss = Ss + Ss.transpose(1, 2)
    dX = Ss @ X
    dXm = Ss.abs() @ X.abs()
    gd = dX[:, S] + g[:, nz:nz + D]
    gdm = dXm[:, S] + g[:, nz:nz + D].abs()
    return dX[:, :S], gd, dXm[:, :S], gdm


# =============================================================================================
# the model's top half as the reference writes it, for autograd (float64, CPU)
def autograd_top_half(table, ids, offs, xin, W, bias, label, q, c, S):
    """Gather, X·Xᵀ strict upper, concat, σ(row·q + c), Keras mean BCE; the bottom output is
    relu(xin·W + bias). Returns (dense, and the gradients of the mean loss with respect to) the
    gathered rows [B, S, D], q, c, W and bias."""
    f = torch.float64
    F = S + 1
    idl = ids.long()
    lo, hi = offs[:-1][None, :], offs[1:][None, :]
    ok = (idl >= 0) & (idl < hi - lo)
    rowi = torch.where(ok, lo + idl, torch.zeros_like(idl))
    emb = (table.to(f)[rowi] * ok[..., None]).detach().requires_grad_(True)
    qv = q.to(f).detach().requires_grad_(True)
    cv = c.to(f).detach().requires_grad_(True)
    Wv = W.to(f).detach().requires_grad_(True)
    bv = bias.to(f).detach().requires_grad_(True)
    dense = torch.relu(xin.to(f) @ Wv + bv)
    X = torch.cat([emb, dense[:, None, :]], 1)
    Z = X @ X.transpose(1, 2)
    iu = torch.triu_indices(F, F, 1)
    row = torch.cat([Z[:, iu[0], iu[1]], dense], 1)
    p = torch.sigmoid(row @ qv + cv)
    lb = label.to(f)
    pc = p.clamp(EPS, 1 - EPS)
    loss = (-(lb * torch.log(pc + EPS) + (1 - lb) * torch.log(1 - pc + EPS))).mean()
    loss.backward()
    return dense.detach(), loss.detach(), emb.grad, qv.grad, cv.grad, Wv.grad, bv.grad
