"""Deterministic inputs for the DIEN recurrence edge tests (tests/test_dien_edges_cpu.py proves
each input has the property its name claims, tests/test_dien_edges_gpu.py runs them through the
kernels of csrc/dien.hip). Builders and oracle evaluation only: numpy and plain torch, nothing
here touches recommender_amd.

Every builder fills the masked steps of its sequences with GARBAGE (1e3, finite): a masked step
carries the state, so nothing a layer returns may depend on what lies there.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import dien as OD

GARBAGE = 1e3

# hm_for of csrc/dien.hip: the unit-count template a hidden size selects
HM_CLASSES = (8, 16, 24, 32, 36, 40, 48, 64)

# (H, the HM class it is claimed to select). Every class has an H below its HM (zero padding in
# stage_gate, `ok = act && k < H`, broadcasts from lanes >= H) and H == HM (no padding at all);
# 24 and 29 are there for that (HM = 24 had no full instance, HM = 32 no padded one).
H_LIST = ((1, 8), (5, 8), (8, 8), (13, 16), (16, 16), (20, 24), (24, 24), (29, 32), (32, 32),
          (33, 36), (36, 36), (37, 40), (40, 40), (47, 48), (48, 48), (50, 64), (64, 64))

MASK_KINDS = ("post", "holes", "late", "empty_row", "word_edges", "full")
WORD_EDGES = (0, 63, 64, 127, 128, 191, 192, 255, 256, 257)  # and T - 1


def _holes_row(T, rng):
    r = rng.random(T) < 0.5
    r[0] = True
    if T >= 3:  # a hole for certain: a masked step between two valid ones
        r[1], r[2] = False, True
    return r


def mask(kind, B, T, rng):
    """bool [B, T], True = valid step.
    post        right-padded; row 0 has length T, row 1 (B >= 2) length 1, the others 1..T
    holes       step 0 valid, every later step valid with p = 1/2; T >= 3: step 1 masked, 2 valid
    late        step 0 masked; the first valid step is 1 in row 0, 1..T-1 elsewhere (T >= 2)
    empty_row   row 0 all masked, row 1 (B >= 2) all valid, the others as "holes"
    word_edges  T >= 300: valid exactly at {0, 63, 64, 127, 128, 191, 192, 255, 256, 257, T-1}
                plus three random steps per row (the ballot words' first and last bits, the step
                on either side of every word boundary, and the byte path from step 256 on)"""
    m = np.zeros((B, T), bool)
    if kind == "post":
        lens = rng.integers(1, T + 1, B)
        lens[0] = T
        if B >= 2:
            lens[1] = 1
        m = np.arange(T)[None, :] < lens[:, None]
    elif kind == "holes":
        for b in range(B):
            m[b] = _holes_row(T, rng)
    elif kind == "late":
        assert T >= 2
        for b in range(B):
            f = 1 if b == 0 else int(rng.integers(1, T))
            m[b, f] = True
            m[b, f + 1:] = rng.random(T - f - 1) < 0.6
    elif kind == "empty_row":
        for b in range(B):
            m[b] = _holes_row(T, rng)
        m[0] = False
        if B >= 2:
            m[1] = True
    elif kind == "word_edges":
        assert T >= 300
        m[:, list(WORD_EDGES) + [T - 1]] = True
        for b in range(B):
            m[b, rng.integers(0, T, 3)] = True
    elif kind == "full":  # every step valid (the compact sequence of the dilation tests)
        m[:] = True
    else:
        raise ValueError(kind)
    return m


def dilate(x, mask_compact, positions, T=None, fill=GARBAGE):
    """x [B, Tc, ...] (every step valid: mask_compact all True) spread to [B, T, ...]: compact
    step i goes to positions[i] (increasing), every other step is masked and holds `fill`.
    Returns (x dilated, mask [B, T])."""
    x = np.asarray(x)
    mc = np.asarray(mask_compact)
    assert mc.all() and mc.shape == x.shape[:2]
    pos = np.asarray(positions)
    assert len(pos) == x.shape[1] and (np.diff(pos) > 0).all() and pos[0] >= 0
    T = int(pos[-1]) + 1 if T is None else T
    assert pos[-1] < T
    out = np.full((x.shape[0], T) + x.shape[2:], fill, x.dtype)
    out[:, pos] = x
    m = np.zeros((x.shape[0], T), bool)
    m[:, pos] = True
    return out, m


# the dilation tests: a compact all-valid sequence of Tc = 11 steps and where its steps go
DILATE_TC = 11
DILATE_POS = {70: (0, 5, 6, 20, 40, 62, 63, 64, 65, 68, 69),
              300: WORD_EDGES + (299,)}
DILATE_LAYER_SPEC = (36, 36, 3, DILATE_TC, "full")  # the compact case of the layer-level check


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _garbage(x, m):
    x = x.copy()
    x[~m] = GARBAGE
    return x


# ---------------------------------------------------------------------------------------------
# layer-level cases: a spec is a hashable tuple, so references are computed once and shared
def gru_inputs(H, X, B, T, kind, seed=0):
    """Keras layouts: kernel [X, 3H], recurrent_kernel [H, 3H], bias [2, 3H]; dout is NOT masked
    (a masked step's output gradient passes to the step before it).
    The recurrent weights are N(0, 1/H) (the size of the layer's orthogonal initialiser): at
    T = 300 the fp32 oracle still meets 2e-5 of the float64 one at this scale, so no case
    needed a smaller one (tests/test_dien_edges_cpu.py checks every case)."""
    rng = np.random.default_rng([seed, H, X, B, T, MASK_KINDS.index(kind)])
    m = mask(kind, B, T, rng)
    lim = np.sqrt(6.0 / (X + 3 * H))
    return dict(
        x=_f32(_garbage(rng.standard_normal((B, T, X)), m)),
        W=_f32(rng.uniform(-lim, lim, (X, 3 * H))),
        U=_f32(rng.standard_normal((H, 3 * H)) / np.sqrt(H)),
        bias=_f32(rng.standard_normal((2, 3 * H)) * 0.3),
        mask=m,
        dout=_f32(rng.standard_normal((B, T, H))))


def augru_inputs(H, X, B, T, kind, seed=0):
    """AUGRUCell layouts: update / reset kernels [H + X, H] on [h, x], candidate [X + H, H] on
    [x, r·h]; att [B, T, 1] in (0, 1) at the valid steps."""
    rng = np.random.default_rng([seed + 1, H, X, B, T, MASK_KINDS.index(kind)])
    m = mask(kind, B, T, rng)
    lim = np.sqrt(6.0 / (X + 2 * H))
    d = dict(x=_f32(_garbage(rng.standard_normal((B, T, X)), m)),
             att=_f32(_garbage(rng.random((B, T, 1)), m)))
    for n in ("u", "r", "h"):
        d["k" + n] = _f32(rng.uniform(-lim, lim, (H + X, H)))
        d["b" + n] = _f32(rng.standard_normal(H) * 0.2)
    d["mask"] = m
    d["dfinal"] = _f32(rng.standard_normal((B, H)))
    return d


def attention_inputs(H, B, L, kind, big=False, seed=0):
    """target [B, 1, H], hs [B, L, H], K [H, H]. big: on top of the noise every h_t gets a
    multiple of q = K·target that makes the score h_t·q ramp from -100 (step 0) to +100 (the
    last step): the row's maximum lies in its last 64-step chunk and exp(s - max over the first
    chunk) would overflow."""
    rng = np.random.default_rng([seed + 2, H, B, L, MASK_KINDS.index(kind), int(big)])
    m = mask(kind, B, L, rng)
    lim = np.sqrt(6.0 / (2 * H))
    K = rng.uniform(-lim, lim, (H, H))
    tg = rng.standard_normal((B, 1, H))
    hs = rng.standard_normal((B, L, H))
    if big:
        q = np.einsum("hx,bx->bh", K, tg[:, 0])
        ramp = np.linspace(-100.0, 100.0, L) if L > 1 else np.array([100.0])
        hs = hs + ramp[None, :, None] * (q / (q * q).sum(-1, keepdims=True))[:, None, :]
    return dict(target=_f32(tg), hs=_f32(_garbage(hs, m)), K=_f32(K), mask=m,
                da=_f32(rng.standard_normal((B, L, 1))))


# --- the GPU module's float64 cases (section A of tests/test_dien_edges_gpu.py) ---------------
GRU_CASES = tuple(
    [(H, H, 5, 9, "holes") for H, _ in H_LIST]
    + [(36, 36, B, 9, k) for k in ("post", "holes", "late", "empty_row") for B in (1, 3, 7)]
    + [(36, 36, 3, 1, "empty_row"), (20, 20, 3, 1, "empty_row")]
    + [(36, 36, 2, 300, "word_edges"), (20, 20, 3, 300, "word_edges")]
    + [(36, 80, 3, 9, "holes"), (36, 80, 3, 9, "empty_row")])     # X > 64: the library GEMMs
AUGRU_CASES = GRU_CASES
ATT_LS = (1, 63, 64, 65, 128, 129, 192, 193, 255, 256)
# (H, B, L, mask kind, big scores). The last is the large-LDS launch, L·(H+1)·4 > 65536; the one
# before it (L = 252: 65520 bytes) is the largest that stays on the ordinary launch.
ATT_CASES = tuple(
    [(36, 5, L, ("late", "holes", "post")[i % 3] if L > 1 else "post", False)
     for i, L in enumerate(ATT_LS)]
    + [(1, 5, 70, "holes", False), (64, 5, 70, "late", False), (36, 3, 1, "empty_row", False),
       (36, 3, 193, "holes", True), (36, 3, 70, "late", True)]
    + [(64, 3, 252, "holes", False), (64, 3, 256, "late", False)])
ATT_BIG_LDS = (64, 3, 256, "late", False)
EVOLVE_CASES = ((36, 3, 9, "holes"), (36, 3, 9, "late"), (20, 3, 70, "holes"))


def att_lds_bytes(H, L):
    """att_fwd_kernel's dynamic LDS: the [L][H + 1] fp32 block of hidden states."""
    return L * (H + 1) * 4


def kernel_inputs(H, B, T, m, seed=0):
    """Operands of the six entry points of csrc/dien.hip themselves (the projections x·W + b
    already formed), for the mask m [B, T]: GRU xw [B, T, 3H], U [H, 3H], rb [3H], dout
    [B, T, H]; AUGRU att [B, T], Kuh / Krh / Khr [H, H], dfinal [B, H]; attention hs [B, T, H],
    q [B, H], da [B, T]. Garbage at the masked steps of xw, att and hs."""
    rng = np.random.default_rng([seed + 3, H, B, T])
    n = rng.standard_normal
    d = dict(xw=_f32(_garbage(n((B, T, 3 * H)), m)), U=_f32(n((H, 3 * H)) / np.sqrt(H)),
             rb=_f32(n(3 * H) * 0.3), dout=_f32(n((B, T, H))),
             att=_f32(_garbage(rng.random((B, T)), m)), dfinal=_f32(n((B, H))),
             hs=_f32(_garbage(n((B, T, H)), m)), q=_f32(n((B, H)) / np.sqrt(H)),
             da=_f32(n((B, T))), mask=np.ascontiguousarray(m, np.uint8))
    for k in ("Kuh", "Krh", "Khr"):
        d[k] = _f32(n((H, H)) / np.sqrt(H))
    return d


# ---------------------------------------------------------------------------------------------
# oracle evaluation (outputs and every gradient) in a dtype on a device
def _leaves(d, names, dtype, device):
    return {n: torch.from_numpy(d[n]).to(device=device, dtype=dtype).requires_grad_(True)
            for n in names}


def _t(a, dtype, device):
    return torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


def eval_gru(d, dtype, device="cpu"):
    """oracle.dien.gru and its gradients: {out, dx, dW, dU, db}."""
    p = _leaves(d, ("x", "W", "U", "bias"), dtype, device)
    out = OD.gru(p["x"], p["W"], p["U"], p["bias"], _t(d["mask"], torch.bool, device))
    g = torch.autograd.grad(out, list(p.values()), _t(d["dout"], dtype, device))
    return dict(out=_np(out), **{k: _np(v) for k, v in zip(("dx", "dW", "dU", "db"), g)})


AUGRU_PARAMS = ("ku", "bu", "kr", "br", "kh", "bh")


def eval_augru(d, dtype, device="cpu"):
    """oracle.dien.augru and its gradients: {final, dx, datt, dku, dbu, dkr, dbr, dkh, dbh}."""
    p = _leaves(d, ("x", "att") + AUGRU_PARAMS, dtype, device)
    out = OD.augru(*p.values(), _t(d["mask"], torch.bool, device))
    g = torch.autograd.grad(out, list(p.values()), _t(d["dfinal"], dtype, device))
    names = ("dx", "datt") + tuple("d" + n for n in AUGRU_PARAMS)
    return dict(final=_np(out), **{k: _np(v) for k, v in zip(names, g)})


def eval_attention(d, dtype, device="cpu"):
    """oracle.dien.attention and its gradients: {a, dtarget, dhs, dK}."""
    p = _leaves(d, ("target", "hs", "K"), dtype, device)
    a = OD.attention(p["target"], p["hs"], p["K"], _t(d["mask"], torch.bool, device))
    g = torch.autograd.grad(a, list(p.values()), _t(d["da"], dtype, device))
    return dict(a=_np(a), **{k: _np(v) for k, v in zip(("dtarget", "dhs", "dK"), g)})


def evolve_inputs(H, B, T, kind, seed=0):
    """DIENAttention then InterestEvolve on the same hidden states (attention_evolve)."""
    a = attention_inputs(H, B, T, kind, seed=seed + 10)
    g = augru_inputs(H, H, B, T, kind, seed + 10)
    d = {k: g[k] for k in AUGRU_PARAMS + ("dfinal",)}
    d.update(target=a["target"], hs=a["hs"], K=a["K"], mask=a["mask"])
    return d


def eval_evolve(d, dtype, device="cpu"):
    """augru(hs, attention(target, hs, K)): {final, dtarget, dhs, dK, dku, ...}."""
    names = ("target", "hs", "K") + AUGRU_PARAMS
    p = _leaves(d, names, dtype, device)
    m = _t(d["mask"], torch.bool, device)
    a = OD.attention(p["target"], p["hs"], p["K"], m)
    out = OD.augru(p["hs"], a, *[p[n] for n in AUGRU_PARAMS], m)
    g = torch.autograd.grad(out, list(p.values()), _t(d["dfinal"], dtype, device))
    return dict(final=_np(out), **{"d" + k: _np(v) for k, v in zip(names, g)})


_BUILD = {"gru": (gru_inputs, eval_gru), "augru": (augru_inputs, eval_augru),
          "att": (attention_inputs, eval_attention), "evolve": (evolve_inputs, eval_evolve)}


@functools.lru_cache(maxsize=None)
def inputs(layer, spec):
    return _BUILD[layer][0](*spec)


@functools.lru_cache(maxsize=None)
def reference(layer, spec, dtype, device="cpu"):
    """The oracle's outputs and gradients for a case, computed once per (dtype, device); the
    arrays are shared: read only."""
    out = _BUILD[layer][1](inputs(layer, spec), dtype, device)
    for v in out.values():
        v.setflags(write=False)
    return out
