"""The D = 128 apply walk (seg_group32_kernel) at the edges of its block shapes: blocks of 32, 16
or 8 half-waves walk an aligned group of 32 tiles, a half-wave taking tiles gi, gi + HW, ...
The cases (tests/apply_edges.py; their structure is checked in tests/test_apply_edges_cpu.py) are
handed to the kernels as sorted keys and positions from oracle.embedding.sort_ids, so the walk is
tested on exactly the tiles the cases describe. Everything is compared bit for bit with
oracle.embedding.segment_sum_tiled followed by the optimizer restatement: SGD (the queued walk),
the emit form (dedup_grad), Keras Adam and row-wise Adagrad (walks that update one run at a
time), the scaled apply and the ranged walk."""
import numpy as np
import pytest
import torch

from oracle import embedding as O
from recommender_amd import _lib as L
from tests import adagrad_ref as R
from tests import apply_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, D = E.V, E.D
LR, EPS = 0.05, 1e-7
f32 = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def same(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    bad = (bits(got) != bits(want)) if want.dtype.kind == "f" else (got != want)
    assert not bad.any(), f"{msg}: {int(bad.sum())} / {bad.size} differ; first at {np.argwhere(bad)[0].tolist()}"


@pytest.fixture(scope="module")
def table():
    """One weight table for the whole module (read-only: every test applies to a device copy)."""
    return np.random.default_rng(11).standard_normal((V, D)).astype(f32)


def _keys(sr, sp):
    return dev(sr.astype(np.int64).astype(np.int32)), dev(sp)


def _params(kind):
    if kind == L.RS_OPT_KERAS_ADAM:
        c = {k: float(x) for k, x in O.keras_adam_coefficients(1, LR, epsilon=EPS).items()}
        return L.AdamParams(c["lr"], c["beta1"], c["beta2"], c["one_minus_beta1"],
                            c["one_minus_beta2"], c["epsilon"])
    return L.AdamParams(float(f32(LR)), 0.0, 0.0, 0.0, 0.0, float(f32(EPS)))


def k_apply(kind, w, m, v, bitmap, sr, sp, grad, row_scale=None, scale_group=1):
    """rs_embedding_apply (or _scaled when row_scale is given) on device copies of the state."""
    n = sr.size
    rows, pos = _keys(sr, sp)
    g, sc = dev(grad), dev(row_scale)
    ws = torch.empty(L.lib().rs_apply_workspace_size(n, D), dtype=torch.uint8, device=DEV)
    p = _params(kind)
    if row_scale is None:
        L.call("rs_embedding_apply", kind, L.ptr(w), L.ptr(m), L.ptr(v), V, D, L.ptr(rows),
               L.ptr(pos), n, L.ptr(g), p, L.ptr(bitmap), L.ptr(ws), ws.numel(), L.stream_ptr(DEV))
    else:
        L.call("rs_embedding_apply_scaled", kind, L.ptr(w), L.ptr(m), L.ptr(v), V, D, L.ptr(rows),
               L.ptr(pos), n, L.ptr(g), L.ptr(sc), scale_group, p, L.ptr(bitmap), L.ptr(ws),
               ws.numel(), L.stream_ptr(DEV))
    if kind == L.RS_OPT_KERAS_ADAM:
        L.call("rs_keras_adam_dense_sweep", L.ptr(w), L.ptr(m), L.ptr(v), V, D, p, L.ptr(bitmap),
               L.stream_ptr(DEV))
    torch.cuda.synchronize()


def k_dedup(sr, sp, grad):
    n = sr.size
    rows, pos = _keys(sr, sp)
    g = dev(grad)
    ur = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ug = torch.full((n, D), 3.0, dtype=torch.float32, device=DEV)
    ws = L.scratch(L.lib().rs_dedup_workspace_size(n, D), DEV)
    L.call("rs_embedding_dedup_grad", L.ptr(rows), L.ptr(pos), n, L.ptr(g), D, V, L.ptr(ur),
           L.ptr(ug), L.ptr(ws), ws.numel(), L.stream_ptr(DEV))
    return host(ur).astype(np.int64), host(ug)


@pytest.mark.parametrize("name", list(E.CASES))
def test_sgd_and_emit_bit_exact(name, table):
    """The queued SGD walk and the emit form on every case: each segment's sum, the table rows
    written once, every other row and every output row past the last segment untouched."""
    ids, grad, sr, sp = E.sorted_case(E.CASES[name])
    ur, ug = E.expected_segments(sr, sp, grad)
    gr, gg = k_dedup(sr, sp, grad)
    same(gr[:ur.size], ur, "uniq_rows")
    same(gg[:ur.size], ug, "uniq_grad")
    assert (gr[ur.size:] == -7).all() and (gg[ur.size:] == 3.0).all(), "wrote past the last segment"
    w = dev(table)
    k_apply(L.RS_OPT_SGD, w, None, None, None, sr, sp, grad)
    same(host(w), O.apply_sgd(table, ur, ug, f32(LR)), "SGD table")


STRUCTURE = [k for k in E.CASES if not k.startswith("tiles")] + ["tiles17_rem1", "tiles49_rem31"]


@pytest.mark.parametrize("name", STRUCTURE)
def test_keras_adam_bit_exact(name, table):
    """A walk that updates one run at a time, with its touched-row bitmap and the dense sweep."""
    ids, grad, sr, sp = E.sorted_case(E.CASES[name])
    ur, ug = E.expected_segments(sr, sp, grad)
    r = np.random.default_rng(9)
    m0 = (r.standard_normal((V, D)) * 0.1).astype(f32)
    v0 = (r.random((V, D)) * 0.1).astype(f32)
    w, m, v = dev(table), dev(m0), dev(v0)
    bm = torch.zeros((V + 31) // 32, dtype=torch.int32, device=DEV)
    k_apply(L.RS_OPT_KERAS_ADAM, w, m, v, bm, sr, sp, grad)
    rw, rm, rv = O.apply_keras_adam(table, m0, v0, ur, ug, O.keras_adam_coefficients(1, LR, epsilon=EPS))
    same(host(m), rm, "m")
    same(host(v), rv, "v")
    same(host(w), rw, "table")


@pytest.mark.parametrize("name", STRUCTURE)
def test_rowwise_adagrad_bit_exact_weights(name, table):
    """Row-wise Adagrad: the weights are bit-equal to the fp32 update evaluated with the row's
    new accumulator as the GPU holds it (the row's sum of squares is reduced across lanes in an
    order the reference does not restate, tests/test_adagrad_gpu.py bounds it), which pins every
    segment sum; untouched rows and accumulators stay as they were."""
    ids, grad, sr, sp = E.sorted_case(E.CASES[name])
    ur, ug = E.expected_segments(sr, sp, grad)
    acc0 = (0.1 + np.random.default_rng(5).random(V)).astype(f32)
    w, acc = dev(table), dev(acc0)
    k_apply(L.RS_OPT_ROWWISE_ADAGRAD, w, acc, None, None, sr, sp, grad)
    got_acc = host(acc)
    same(host(w), R.rowwise_update(table, got_acc, ur, ug, LR, EPS), "table")
    untouched = np.setdiff1d(np.arange(V), ur)
    same(got_acc[untouched], acc0[untouched], "untouched accumulators")
    assert (got_acc[ur] >= acc0[ur]).all()


@pytest.mark.parametrize("name", STRUCTURE)
def test_scaled_apply_bit_exact(name, table):
    """rs_embedding_apply_scaled with scale_group 3: the gradient of position p is
    fmul_rn(row_scale[p // 3], grad[p]), formed in float32 before the tiled sum."""
    S = 3
    ids, grad, sr, sp = E.sorted_case(E.CASES[name])
    scale = np.random.default_rng(3).standard_normal(-(-ids.size // S)).astype(f32)
    ur, ug = E.expected_segments(sr, sp, E.scaled_grad(grad, scale, S))
    w = dev(table)
    k_apply(L.RS_OPT_SGD, w, None, None, None, sr, sp, grad, row_scale=scale, scale_group=S)
    same(host(w), O.apply_sgd(table, ur, ug, f32(LR)), "scaled SGD table")


def test_ranged_walk_bit_exact():
    """rs_embedding_dedup_grad_mapped_range with key_lo > 0 over four groups: one entirely below
    key_lo (skipped), one straddling it, one inside, one entirely at or above key_hi (skipped).
    The segments of the range get the sums of the whole walk; nothing else is written; the two
    adjoining ranges together emit what one call emits."""
    case, lo, hi = E.ranged_case()
    ids, grad, sr, sp = E.sorted_case(case)
    n = ids.size
    key_lo, key_hi = int(sr[lo]), int(sr[hi])
    ur, ug = E.expected_segments(sr, sp, grad)
    rows, pos = _keys(sr, sp)
    g = dev(grad)

    def run(ranges):
        out_r = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        out_g = torch.full((n, D), 3.0, dtype=torch.float32, device=DEV)
        ws = L.scratch(L.lib().rs_dedup_workspace_size(n, D), DEV)
        for a, b, ready in ranges:
            L.call("rs_embedding_dedup_grad_mapped_range", L.ptr(rows), L.ptr(pos), n, L.ptr(g),
                   None, 1, D, V, a, b, ready, None, None, L.ptr(out_r), L.ptr(out_g), L.ptr(ws),
                   ws.numel(), L.stream_ptr(DEV))
        return host(out_r).astype(np.int64), host(out_g)

    def want(ranges):
        wr, wg = np.full(n, -7, np.int64), np.full((n, D), 3.0, f32)
        for a, b, _ in ranges:
            s = np.flatnonzero((ur >= a) & (ur < b))
            wr[s], wg[s] = ur[s], ug[s]
        return wr, wg

    for ranges in ([(key_lo, key_hi, 0)], [(key_hi, V, 0)], [(0, key_lo, 0), (key_lo, V, 1)],
                   [(0, V, 0)]):
        (gr, gg), (wr, wg) = run(ranges), want(ranges)
        same(gr, wr, f"{ranges} uniq_rows")
        same(gg, wg, f"{ranges} uniq_grad")
