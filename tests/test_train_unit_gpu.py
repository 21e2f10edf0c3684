"""rs_dlrm_train_step_fwd_unit (the chunked train kernel of the production DLRM step: gather,
Z = X·Xᵀ, the composed top-MLP head, Keras BCE, G, the unit gradient rows U = (M + Mᵀ)·X and the
batch sums of the factored MLP backward) against a float64 torch restatement of the same
quantities (ctr/model.py:45-57 with the head composed, ctr/layers.py:23-43). Every product is
bounded per element by its magnitude: |got − ref| ≤ 1e-5 · Σ|terms| (the split-bf16 MFMA keeps
fp32 accuracy relative to that bound); the unit rows by 1e-6 · Σ|terms|, which no
kernel with a part product missing meets. Slot counts on both sides of 16 (the dense
row then sits in the first or second 16-row block of the Uᵀ product), D 128 / 64, int32 / int64
ids, out-of-range ids (zero row + flag), a batch that leaves waves empty. The restatement and the
bound live in tests/dlrm_edges.py, which the edge suite of the same kernels shares."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import x3_model as X3
from tests.dlrm_edges import close as _close, reference as _reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
NI = 13
EPS = 1e-7


def inputs_cpu(B, S, D, V, id64, seed, oob=False):
    """The inputs as CPU tensors (tests/test_x3_model_cpu.py evaluates the CPU model on them)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    table = torch.randn(V, D, generator=g) * 0.5
    ids = torch.randint(0, V // S, (B, S), generator=g)
    if oob:
        ids[::7, 3 % S] = V  # beyond every slot's range
        ids[::11, 0] = -1
    ids = ids.to(torch.int64 if id64 else torch.int32).contiguous()
    offs = torch.arange(S + 1, dtype=torch.int64) * (V // S)
    dense = torch.randn(B, D, generator=g)
    xin = torch.rand(B, NI, generator=g)
    label = (torch.rand(B, generator=g) < 0.3).float()
    F = S + 1
    q = torch.randn(F * (F - 1) // 2 + D, generator=g) * 0.05
    c = torch.tensor([0.1])
    return table, ids, offs, dense, xin, label, q, c


def _inputs(*a, **kw):
    return tuple(t.to(DEV) for t in inputs_cpu(*a, **kw))


def _run(table, ids, offs, dense, xin, label, q, c, S, D):
    B = ids.shape[0]
    V = table.shape[0]
    y = torch.empty(B, device=DEV)
    rows = torch.full((B * S, D), float("nan"), device=DEV)
    sums = torch.empty(512 + 2 + NI * D + D, device=DEV)
    ws_n = L.lib().rs_dlrm_train_workspace_size(B)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    G = torch.full((B,), float("nan"), device=DEV)
    L.call("rs_dlrm_train_step_fwd_unit", L.ptr(table), V, D, L.ptr(ids), L.id_dtype_code(ids), S,
           L.ptr(offs), L.ptr(dense), L.ptr(xin), NI, L.ptr(label), B, L.ptr(q), L.ptr(c), EPS,
           1.0 / B, L.ptr(y), L.ptr(rows), L.ptr(G), L.ptr(sums), L.ptr(ws), ws_n, L.ptr(err),
           L.stream_ptr(table.device))
    torch.cuda.synchronize()
    return y, rows, G, sums, int(err.item())


CASES = [
    (4096, 26, 128, False, False),
    (1000, 26, 128, True, True),
    (777, 8, 128, False, True),
    (2048, 15, 128, True, False),
    (3000, 26, 64, False, False),
    (513, 12, 64, True, True),
]


@pytest.mark.parametrize("B,S,D,id64,oob", CASES)
def test_chunked_train_kernel_vs_float64(B, S, D, id64, oob):
    V = 20_000 * S
    args = _inputs(B, S, D, V, id64, seed=B + S, oob=oob)
    y, U, G, sums, err = _run(*args, S, D)
    p, hm, G64, U64, Um, s64, m64, nz, has_oob = _reference(*args, S, D)
    assert (err != 0) == has_oob == oob
    assert torch.isfinite(G).all() and torch.isfinite(U).all()
    # y = σ(h): |dy| <= |dh| / 4 (+ the sigmoid's own rounding, a few ulps of y)
    _close(y, p, 0.25 * hm + 0.03 * p, "y")
    # the unit rows are sums of at most 27 products: a missing part product is not averaged away
    # there, and the bound is the tight one of tests/x3_model.py (proved on these inputs in
    # tests/test_x3_model_cpu.py). The A_top pair columns sum 513 or more examples, which averages
    # a missing product down to the level of the sum's own rounding: they keep 1e-5, and
    # tests/test_train_x3_gpu.py holds Z to its claim at batch 1.
    print(f"unit rows: max err/mag {X3.max_rel(U.view(B, S, D).cpu(), U64.cpu(), Um.cpu()):.3g}")
    _close(U.view(B, S, D), U64, Um, "unit rows", rel=X3.REL_U_DENSE)
    # G = y(1-y)·dL/dy = (y - label) / B inside the clip: h's error moves it by <= |dh| / (4B)
    dG = (G.double() - G64).abs()
    assert bool((dG <= 2e-6 * G64.abs() + 1e-5 * hm / (4 * B)).all()), float(dG.max())
    a = 512
    _close(sums[:nz + D], s64["A_top"], m64["A_top"], "A_top")
    assert bool((sums[nz + D:a] == 0).all())
    _close(sums[a], s64["s_top"], m64["s_top"], "s_top")
    _close(sums[a + 1], s64["loss"], m64["loss"], "loss")
    _close(sums[a + 2:a + 2 + NI * D].view(NI, D), s64["A_bot"], m64["A_bot"], "A_bot")
    _close(sums[a + 2 + NI * D:], s64["s_bot"], m64["s_bot"], "s_bot")
