"""Inputs and restatements for the fused DIN local-activation tests (CPU and GPU files share
them, so the CPU file bounds the fp32 restatement on exactly the inputs the GPU file runs).

The reference is oracle.dien.local_activation in float64 under torch autograd. The bound is the
fused aux-net's: |got - ref| <= RTOL·(|ref| + max|ref|) per tensor (tests/test_dien_gpu.py).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import dien as OD

RTOL = 2e-5
NAMES = ("rep", "dtarget", "dhis", "dW1", "db1", "dW2", "db2", "dW3", "db3")

# (D, B, L, mask kind): the cases of the GPU file
CASES = [
    (36, 64, 37, "random"),   # holes; tiles with no valid row between live tiles
    (36, 48, 17, "post"),     # the lone row of the second tile; last valid steps at 15 and 16
    (36, 5, 16, "all"),       # exactly one full tile
    (36, 3, 1, "all"),        # L = 1
    (16, 96, 50, "random"),   # the D = 16 build
    (36, 512, 100, "synthetic"),  # the DIN workload's lengths
    (36, 1, 20, "random"),    # B on both sides of the 4 examples a block takes per round
    (36, 2, 20, "random"),
    (36, 3, 20, "random"),
]


def case_id(c):
    return f"D{c[0]}-B{c[1]}-L{c[2]}-{c[3]}"


def make_mask(rng, B, L, kind):
    if kind == "random":
        m = rng.random((B, L)) < 0.3
        if L >= 37:
            m[0, 16:32] = False  # a dead tile between two live ones
            m[0, 3] = m[0, 33] = True
        return m
    if kind == "all":
        return np.ones((B, L), bool)
    if kind == "synthetic":  # recommender_amd.dien.train.synthetic_batch
        lens = np.clip(2 + rng.geometric(0.1, B), 2, L)
        return np.arange(L)[None, :] < lens[:, None]
    assert kind == "post"
    lens = rng.integers(1, L + 1, B)
    lens[:2] = (16, min(17, L))  # last valid steps at 15 and 16
    return np.arange(L)[None, :] < lens[:, None]


def make_params(rng, D):
    """Glorot kernels, biases 0.2·N(0,1): [W1 [4D,80], b1, W2 [80,40], b2, W3 [40,1], b3]."""
    def glorot(a, b):
        lim = (6.0 / (a + b)) ** 0.5
        return rng.uniform(-lim, lim, (a, b)).astype(np.float32)

    def bias(n):
        return (rng.standard_normal(n) * 0.2).astype(np.float32)

    return [torch.from_numpy(x) for x in (glorot(4 * D, 80), bias(80), glorot(80, 40), bias(40),
                                          glorot(40, 1), bias(1))]


@functools.lru_cache(maxsize=None)
def make_inputs(D, B, L, kind, seed=0):
    """CPU fp32 tensors: target [B,1,D], his [B,L,D] (0.5·N(0,1)), mask [B,L] bool, drep [B,D],
    params. Cached: shared, never modified."""
    rng = np.random.default_rng([D, B, L, seed])
    params = make_params(rng, D)
    mask = torch.from_numpy(make_mask(rng, B, L, kind))
    tgt = torch.from_numpy((rng.standard_normal((B, 1, D)) * 0.5).astype(np.float32))
    his = torch.from_numpy((rng.standard_normal((B, L, D)) * 0.5).astype(np.float32))
    drep = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    return dict(D=D, B=B, L=L, target=tgt, his=his, mask=mask, drep=drep, params=params)


def evaluate(inp, dtype=torch.float64, form="literal", device="cpu"):
    """[rep, dtarget, dhis, dW1, db1, dW2, db2, dW3, db3] under torch autograd in `dtype`.
    form "literal": oracle.dien.local_activation; "folded": the algebraic form the kernels build,
    z1 = [h, t⊙h]·[Wb − Wc; Wd] + (b1 + t·(Wa + Wc))."""
    D = inp["D"]
    ps = [x.to(device, dtype).clone().requires_grad_(True) for x in inp["params"]]
    t = inp["target"].to(device, dtype).clone().requires_grad_(True)
    h = inp["his"].to(device, dtype).clone().requires_grad_(True)
    mask = inp["mask"].to(device)
    if form == "literal":
        rep = OD.local_activation(t, h, mask, [(ps[0], ps[1], "sigmoid"), (ps[2], ps[3], "sigmoid"),
                                               (ps[4], ps[5], None)])
    else:
        W = ps[0]
        Wa, Wb, Wc, Wd = W[:D], W[D:2 * D], W[2 * D:3 * D], W[3 * D:]
        z1 = torch.cat([h, t * h], -1) @ torch.cat([Wb - Wc, Wd], 0) + (ps[1] + t @ (Wa + Wc))
        w = torch.sigmoid(torch.sigmoid(z1) @ ps[2] + ps[3]) @ ps[4] + ps[5]
        w = w * mask.unsqueeze(-1).to(dtype)
        rep = (w.transpose(1, 2) @ h).squeeze(1)
    rep.backward(inp["drep"].to(device, dtype))
    out = [rep.detach(), t.grad.reshape(inp["B"], D), h.grad] + [p.grad for p in ps]
    out[7] = out[7].reshape(-1)  # dW3 [40]
    return out


@functools.lru_cache(maxsize=None)
def reference(D, B, L, kind, seed=0):
    """The float64 reference of a case (numpy arrays), computed once."""
    return [x.numpy() for x in evaluate(make_inputs(D, B, L, kind, seed))]


def rel_err(got, ref):
    """max |got - ref| / (|ref| + max|ref|): the bound's left side over its scale."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    den = np.abs(ref) + np.abs(ref).max() + 1e-300
    return float((np.abs(got - ref) / den).max())


def assert_close(got, ref, name, rtol=RTOL):
    e = rel_err(got, ref)
    assert np.isfinite(np.asarray(got)).all(), f"{name}: not finite"
    assert e <= rtol, f"{name}: err / (|ref| + max|ref|) = {e:.3g} > {rtol:g}"


def grid_blocks(B, cus):
    """Blocks of the forward and backward kernels (include/recsys_hip.h): persistent over rounds
    of 4 examples; fwd min(ceil(B / 4), 3·CUs), bwd min(ceil(B / 4), CUs)."""
    rounds = (B + 3) // 4
    return min(rounds, 3 * cus), min(rounds, cus)


def two_round_batch(cus):
    """The smallest B at which every block of both kernels walks at least two rounds, plus a
    ragged last round of 2 examples: 2·(3·CUs) full rounds and half a round."""
    B = 4 * 2 * 3 * cus + 2
    fwd, bwd = grid_blocks(B, cus)
    rounds = (B + 3) // 4
    assert rounds >= 2 * fwd and rounds >= 2 * bwd and B % 4 != 0
    return B


SATURATED = (36, 32, 20, "random")


@functools.lru_cache(maxsize=None)
def make_saturated():
    """The SATURATED case with layer 1 and layer 2 scaled so that their largest pre-activations
    (float64, valid and masked rows alike) are ±60: σ saturates to 0 / 1 and its derivative
    underflows towards 0."""
    base = make_inputs(*SATURATED, seed=1)
    D = base["D"]
    W1, b1, W2, b2, W3, b3 = [p.double() for p in base["params"]]
    t = base["target"].double().expand(-1, base["L"], -1)
    h = base["his"].double()
    x = torch.cat([t, h, t - h, t * h], -1)
    s1 = 60.0 / float((x @ W1 + b1).abs().max())
    h1 = torch.sigmoid(x @ (W1 * s1) + b1 * s1)
    s2 = 60.0 / float((h1 @ W2 + b2).abs().max())
    params = [(W1 * s1).float(), (b1 * s1).float(), (W2 * s2).float(), (b2 * s2).float(),
              base["params"][4], base["params"][5]]
    return {**base, "params": params}


@functools.lru_cache(maxsize=None)
def saturated_reference():
    return [x.numpy() for x in evaluate(make_saturated())]
