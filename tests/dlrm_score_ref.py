"""Inputs and bounds for the tests of the DLRM scoring kernels (rs_dlrm_score, rs_dlrm_score_q8;
include/recsys_hip.h a-4). No GPU is touched here: every builder returns CPU tensors or NumPy
arrays, so tests/test_dlrm_score_cpu.py can prove what tests/test_dlrm_score_gpu.py relies on.

The float64 restatement is tests/dlrm_edges.head_dx_reference (y and Σ|terms| of the
pre-activation); the RS_Q8 restatement and its per-element bound are tests/embedding_q8_ref's."""
import numpy as np
import torch

from tests import dlrm_edges as E
from tests import embedding_q8_ref as Q

SLOTS = [1, 2, 15, 16, 17, 26, 31]   # the dense row in the first or second 16-row block; F = 32
BATCHES = [1, 3, 4, 5, 67]           # part of a block, one block, one wave more, many blocks
DIMS = [64, 128]


def uneven_cards(S):
    """Rows per slot: uneven, with a cardinality-1 slot in the middle (S > 1)."""
    cards = [3 + (7 * s) % 11 for s in range(S)]
    if S > 1:
        cards[S // 2] = 1
    return cards


def score_inputs(B, S, D, id64, seed, shared=False, oob=False):
    """(table, ids, offs, dense, q, c) as CPU tensors: dlrm_edges.train_inputs on a shared table
    or on the uneven slab."""
    table, ids, offs, dense, _, _, q, c = E.train_inputs(B, S, D, id64, seed,
                                                         cards=uneven_cards(S), shared=shared,
                                                         oob=oob)
    return table, ids, offs, dense, q, c


def q8_table(D, n_rows, q_ld=None):
    """(fp32 source [n_rows, D], RS_Q8 bytes uint8 [n_rows, q_ld]) over every family of
    embedding_q8_ref (a constant row has scale 0, the clamp and subnormal rows a subnormal
    scale), quantised by the NumPy restatement."""
    src = Q.table(D, n_rows, flagged=False)
    qt, flagged = Q.quantize(src, q_ld)
    assert not flagged.any()
    return src, qt


def mild_families(D):
    """The families whose products stay finite in fp32 (the float64 and bound comparisons)."""
    fam = Q.families(D)
    keep = ["gauss", "offset", "small", "three_valued", "two_valued", "constant", "zeros", "tie"]
    return np.concatenate([fam[k] for k in keep])


# ---- float64 -------------------------------------------------------------------------------
def preact_terms(table, ids, offs, dense, q, c, S):
    """(h, Σ|terms|) of the pre-activation in float64, written as explicit loops over the pairs
    (the independent statement tests/test_dlrm_score_cpu.py holds head_dx_reference's to)."""
    t = np.asarray(table, np.float64)
    dn = np.asarray(dense, np.float64)
    qq = np.asarray(q, np.float64)
    idl = np.asarray(ids, np.int64)
    B, D = dn.shape
    F = S + 1
    h = np.zeros(B)
    m = np.zeros(B)
    for b in range(B):
        X = np.zeros((F, D))
        for s in range(S):
            lo, card = (0, t.shape[0]) if offs is None else (int(offs[s]), int(offs[s + 1] - offs[s]))
            if 0 <= idl[b, s] < card:
                X[s] = t[lo + idl[b, s]]
        X[S] = dn[b]
        o = 0
        for i in range(F):
            for j in range(i + 1, F):
                prod = X[i] * X[j]
                h[b] += prod.sum() * qq[o]
                m[b] += np.abs(prod).sum() * abs(qq[o])
                o += 1
        h[b] += (dn[b] * qq[o:o + D]).sum() + float(c)
        m[b] += (np.abs(dn[b]) * np.abs(qq[o:o + D])).sum() + abs(float(c))
    return h, m


def quant_bound(table, ids, offs, dense, q, S):
    """The bound on |h(dequantised table) − h(table)| per example, float64. With e_i the vector of
    embedding_q8_ref.bound's per-element bounds of row i (0 for the dense row and for a zero row):
    |Δ(x_i·x_j)| <= ‖e_i‖‖x_j‖ + ‖x_i‖‖e_j‖ + ‖e_i‖‖e_j‖ (Cauchy-Schwarz on x̃_i·x̃_j − x_i·x_j =
    Δ_i·x_j + x_i·Δ_j + Δ_i·Δ_j), and |Δh| <= Σ_o |q_o| |Δz_o| (the dense part of h reads no
    table row)."""
    t = np.asarray(table, np.float64)
    e = Q.bound(np.asarray(table, np.float32))                # [n_rows, 1], per element
    D = t.shape[1]
    en_rows = np.broadcast_to(e, t.shape)
    en_all = np.sqrt((en_rows ** 2).sum(1))                   # ‖e_row‖
    xn_all = np.sqrt((t ** 2).sum(1))
    idl = np.asarray(ids, np.int64)
    dn = np.asarray(dense, np.float64)
    qq = np.abs(np.asarray(q, np.float64))
    B = idl.shape[0]
    F = S + 1
    out = np.zeros(B)
    for b in range(B):
        en, xn = np.zeros(F), np.zeros(F)
        for s in range(S):
            lo, card = (0, t.shape[0]) if offs is None else (int(offs[s]), int(offs[s + 1] - offs[s]))
            if 0 <= idl[b, s] < card:
                en[s], xn[s] = en_all[lo + idl[b, s]], xn_all[lo + idl[b, s]]
        xn[S] = np.sqrt((dn[b] ** 2).sum())
        o = 0
        for i in range(F):
            for j in range(i + 1, F):
                out[b] += qq[o] * (en[i] * xn[j] + xn[i] * en[j] + en[i] * en[j])
                o += 1
    return out


def y_tolerance(hm, y, act, rel=1e-5):
    """The tolerance of y against float64 for a pre-activation of magnitude bound hm, as
    tests/test_dlrm_edges_gpu.py compares rs_dlrm_interaction_fwd_head's: rel·hm for linear and
    relu (1-Lipschitz), rel·(hm / 4 + 0.03 y) for the sigmoid (|dy| <= |dh| / 4, plus a few ulps
    of y for the exponential and the quotient)."""
    return rel * (0.25 * hm + 0.03 * y) if act == 2 else rel * hm


# ---- the model's composed top MLP in float64 -------------------------------------------------
def composed_qc(layers, rows):
    """(q, c, |q| bound, |c| bound) of a [n1, n2, 1] chain over the compact rows in float64: q =
    K1[rows]·K2·K3, c = ((b1·K2) + b2)·K3 + b3, and the same sums over absolute values (the
    Σ|terms| of the composition, which the fp32 composition's rounding is relative to)."""
    f = torch.float64
    K1, K2, K3 = (l.kernel.detach().cpu().to(f) for l in layers)
    b1, b2, b3 = (l.bias.detach().cpu().to(f) for l in layers)
    K1 = K1[rows.cpu()]
    q = (K1 @ K2 @ K3)[:, 0]
    c = ((b1 @ K2 + b2) @ K3 + b3)[0]
    qm = (K1.abs() @ K2.abs() @ K3.abs())[:, 0]
    cm = ((b1.abs() @ K2.abs() + b2.abs()) @ K3.abs() + b3.abs())[0]
    return q, c, qm, cm
