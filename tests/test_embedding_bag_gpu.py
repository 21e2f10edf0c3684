"""EmbeddingBag on the GPU against tests/embedding_bag_ref.py (the contract restated in NumPy):
the forward bit for bit, the remap, the remapped apply against the expanded one bit for bit for
all five optimizers (the design's justification: rs_embedding_apply_scaled never needs its
positions to be a permutation), and the Python surface."""
import numpy as np
import pytest
import torch

from oracle import embedding as O
from recommender_amd import _lib as L
from recommender_amd.embedding import Embedding, EmbeddingBag
from recommender_amd.functional import embedding_bag
from recommender_amd.optim import (SortedIds, SparseAdagrad, SparseAdam, SparseSGD, dedup_grad,
                                   densify_grad)
from tests import embedding_bag_ref as R
from tests.conftest import assert_close_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def gpu_fwd(table, ids, n_bags, offsets=None, bag_len=0, valid=None, weights=None, mode=R.SUM,
            slot_offsets=None, id_dtype=np.int64, out=None, out_ld=None, want_scale=True):
    """rs_embedding_bag_fwd: (out, bag_scale, error bits) as NumPy."""
    t, i = dev(table, f32), dev(np.asarray(ids).reshape(-1), id_dtype)
    D = table.shape[1]
    o, v, w, so = dev(offsets, np.int64), dev(valid, np.uint8), dev(weights, f32), dev(slot_offsets)
    if out is None:
        out = torch.full((max(n_bags, 1), D), 777.0, device=DEV)
    scale = torch.full((max(n_bags, 1),), 777.0, device=DEV) if want_scale else None
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_slots = 1 if slot_offsets is None else len(slot_offsets) - 1
    L.call("rs_embedding_bag_fwd", L.ptr(t), table.shape[0], D, L.ptr(i), L.id_dtype_code(i),
           i.numel(), L.ptr(o), n_bags, bag_len, L.ptr(v), L.ptr(w), mode, L.ptr(so), n_slots,
           L.ptr(out), out_ld or D, L.ptr(scale), L.ptr(err), L.stream_ptr(out.device))
    torch.cuda.synchronize()
    sc = None if scale is None else scale.cpu().numpy()[:n_bags]
    return out.cpu().numpy(), sc, int(err.item())


def check_fwd(table, ids, n_bags, **kw):
    ref_kw = {k: v for k, v in kw.items() if k != "id_dtype"}
    ref, rscale, _, flag = R.bag_forward(table, ids, n_bags, **ref_kw)
    out, scale, err = gpu_fwd(table, ids, n_bags, **kw)
    np.testing.assert_array_equal(out[:n_bags].view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(scale, rscale)
    assert bool(err & L.RS_ERRBIT_OOB) == flag
    return out, scale


# ---- forward -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.SUM, R.MEAN])
@pytest.mark.parametrize("D", R.FWD_DIMS)
def test_forward_bitexact_every_width_and_length(D, mode):
    """CSR bags of every length in BAG_LENS (first and last bag empty) over rows whose sum depends
    on the order (tests/test_embedding_bag_cpu.py proves it), both id widths, twice."""
    table, ids, offsets = R.order_sensitive_bags(D)
    nb = len(offsets) - 1
    a, _ = check_fwd(table, ids, nb, offsets=offsets, mode=mode, id_dtype=np.int64)
    b, _ = check_fwd(table, ids, nb, offsets=offsets, mode=mode, id_dtype=np.int32)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))  # reproducible


@pytest.mark.parametrize("D", [1, 18, 128, 260])
@pytest.mark.parametrize("n_bags", R.N_BAGS)
def test_forward_bag_counts_fixed_and_masked(n_bags, D, rng):
    """n_bags on both sides of a block's lane groups; the bag_len form and the [B, L] form with
    a valid mask: holes, late starts, all-zero rows."""
    table = R.order_sensitive_table(D)
    ids = rng.integers(0, table.shape[0], (n_bags, 6))
    check_fwd(table, ids, n_bags, bag_len=6, mode=R.MEAN)
    valid = (rng.random((n_bags, 6)) < 0.6).astype(np.uint8)
    valid[::3, :2] = 0          # late starts
    valid[n_bags // 2] = 0      # an all-zero row
    valid[0] = [1, 0, 1, 0, 0, 1]
    if n_bags > 1:
        valid[-1] = 0
    check_fwd(table, ids, n_bags, bag_len=6, valid=valid, mode=R.MEAN)
    check_fwd(table, ids, n_bags, bag_len=6, valid=valid, mode=R.SUM, id_dtype=np.int32)


def test_forward_empty_shapes(rng):
    table = R.order_sensitive_table(18)
    ids = rng.integers(0, 400, 12)
    # every bag empty (CSR), then n_ids == 0 in both forms, then n_bags == 0
    check_fwd(table, ids, 5, offsets=np.full(6, 4, np.int64), mode=R.MEAN)
    check_fwd(table, ids[:0], 3, offsets=np.zeros(4, np.int64), mode=R.MEAN)
    check_fwd(table, ids[:0], 7, bag_len=0, mode=R.SUM)
    out, _, err = gpu_fwd(table, ids[:0], 0, bag_len=4)
    assert (out == 777.0).all() and err == 0  # nothing written


def test_forward_slab_and_out_of_range():
    ids, offsets, so, bad = R.oob_case()
    table = (np.arange(18 * 3, dtype=f32).reshape(18, 3) + 1)
    _, scale = check_fwd(table, ids, 4, offsets=offsets, slot_offsets=so, mode=R.MEAN)
    np.testing.assert_array_equal(scale, [f32(1) / f32(3)] * 3 + [0.5])  # OOB ids still count
    out, _, err = gpu_fwd(table, ids, 4, offsets=offsets, slot_offsets=so)
    assert err & L.RS_ERRBIT_OOB
    np.testing.assert_array_equal(out[0], table[0] + 0 + table[4])  # the -1 read a zero row
    valid = np.ones(ids.size, np.uint8)
    valid[bad] = 0
    assert gpu_fwd(table, ids, 4, offsets=offsets, slot_offsets=so, valid=valid)[2] == 0
    # one table: -1 and the cardinality
    t1 = R.order_sensitive_table(4)
    i1 = np.array([[3, -1, 5], [400, 2, 2], [1, 2, 3]])
    out, scale = check_fwd(t1, i1, 3, bag_len=3, mode=R.SUM, id_dtype=np.int32)
    np.testing.assert_array_equal(out[1], (np.zeros(4, f32) + t1[2]) + t1[2])
    np.testing.assert_array_equal(scale, [f32(1) / f32(3)] * 3)


def test_forward_slab_uneven_slots_random(rng):
    so = np.array([0, 7, 300, 311], np.int64)
    table = R.order_sensitive_table(36, rows=311)
    card = np.diff(so)
    ids = np.stack([rng.integers(0, card[b % 3], 9) for b in range(64)])
    check_fwd(table, ids, 64, bag_len=9, slot_offsets=so, mode=R.MEAN)


@pytest.mark.parametrize("offsets", [[0, 3, 2, 6, 8], [0, 2, 50, 8], [-1, 4, 8]])
def test_forward_malformed_offsets(offsets, rng):
    """Reversed offsets, offsets past n_ids, a negative start: the bag is empty and flagged."""
    table = R.order_sensitive_table(4)
    ids = rng.integers(0, 400, 8)
    offsets = np.array(offsets, np.int64)
    _, _, err = gpu_fwd(table, ids, len(offsets) - 1, offsets=offsets)
    assert err & L.RS_ERRBIT_OOB
    check_fwd(table, ids, len(offsets) - 1, offsets=offsets, mode=R.MEAN)


@pytest.mark.parametrize("D,ld", [(18, 36), (4, 7), (128, 132), (3, 5)])
def test_forward_strided_out_leaves_the_rest(D, ld, rng):
    table = R.order_sensitive_table(D)
    ids = rng.integers(0, 400, (65, 5))
    wide = torch.full((65, ld), -5.0, device=DEV)
    off = ld - D  # the right-hand column block
    out, _, _ = gpu_fwd(table, ids, 65, bag_len=5, mode=R.MEAN, out=wide[:, off:], out_ld=ld)
    got = wide.cpu().numpy()
    ref, *_ = R.bag_forward(table, ids, 65, bag_len=5, mode=R.MEAN)
    np.testing.assert_array_equal(got[:, off:], ref)
    assert (got[:, :off] == -5.0).all()


def test_forward_weights():
    """Weights 0, negative, 1e30 against a cancelling partner, denormal: each product rounded
    on its own, added in position order."""
    table = np.array([[1.0, -2.0, 3.0], [0.5, 0.25, 1e-3], [1.0, 1.0, 1.0]], f32)
    ids = np.array([[0, 1, 2, 0], [2, 2, 2, 1], [1, 0, 2, 2]])
    w = np.array([[0.0, -1.5, 2.0, 1.0], [1e30, -1e30, 1.0, 3.0], [1e-42, -1e-45, 1e-40, 0.0]], f32)
    out, _ = check_fwd(table, ids, 3, bag_len=4, weights=w, mode=R.SUM)
    np.testing.assert_array_equal(out[1], f32(1.0) + f32(3.0) * table[1])  # 1e30 - 1e30 = 0 first
    assert out[2].any()  # denormal products are kept, not flushed


def test_forward_argument_errors():
    t = torch.zeros(4, 4, device=DEV)
    i = torch.zeros(6, dtype=torch.int64, device=DEV)
    o = torch.zeros(2, 4, device=DEV)
    w = torch.ones(6, device=DEV)

    def call(dim=4, n_ids=6, n_bags=2, bag_len=3, mode=0, out_ld=4, weights=None, table=t, out=o):
        return L.lib().rs_embedding_bag_fwd(L.ptr(table), 4, dim, L.ptr(i), 1, n_ids, None, n_bags,
                                            bag_len, None, L.ptr(weights), mode, None, 1,
                                            L.ptr(out), out_ld, None, None, None)
    assert call(mode=1, weights=w) == L.RS_E_INVALID   # MEAN with weights
    assert call(mode=2) == L.RS_E_INVALID
    assert call(dim=0) == L.RS_E_INVALID
    assert call(out_ld=3) == L.RS_E_INVALID
    assert call(n_ids=5) == L.RS_E_INVALID             # n_ids != n_bags * bag_len
    assert call(table=None) == L.RS_E_INVALID and call(out=None) == L.RS_E_INVALID
    torch.cuda.synchronize()


# ---- remap -------------------------------------------------------------------------------
def gpu_remap(sorted_pos, n_ids, n_bags, offsets=None, bag_len=0):
    out = torch.full_like(sorted_pos, -9)
    L.call("rs_embedding_bag_remap_pos", L.ptr(sorted_pos), n_ids, L.ptr(dev(offsets, np.int64)),
           n_bags, bag_len, L.ptr(out), L.stream_ptr(out.device))
    return out


@pytest.mark.parametrize("form", ["csr", "fixed", "ones", "single"])
def test_remap_matches_restatement(form, rng):
    n = 700
    ids = rng.integers(0, 90, n)
    valid = (rng.random(n) < 0.7).astype(np.uint8)
    if form == "csr":
        cuts = np.sort(rng.integers(0, n + 1, 40))
        offsets, bag_len = np.concatenate([[0], cuts, [n]]).astype(np.int64), 0
    elif form == "fixed":
        offsets, bag_len = None, 7
    elif form == "ones":   # every bag holds one id
        offsets, bag_len = np.arange(n + 1, dtype=np.int64), 0
    else:                  # one bag holds everything
        offsets, bag_len = np.array([0, n], np.int64), 0
    n_bags = n // bag_len if offsets is None else len(offsets) - 1
    s = SortedIds(dev(ids, np.int64), 90, valid=dev(valid), count_unique=False)
    got = gpu_remap(s.pos, n, n_bags, offsets, bag_len).cpu().numpy()
    pos = s.pos.cpu().numpy()
    np.testing.assert_array_equal(got, R.bag_remap(pos, n, n_bags, offsets, bag_len))


# ---- backward: remapped apply == apply of the expanded gradient ---------------------------
OPTS = ["sgd", "lazy", "keras", "adagrad", "rowwise"]
KIND = {"sgd": L.RS_OPT_SGD, "lazy": L.RS_OPT_LAZY_ADAM, "keras": L.RS_OPT_KERAS_ADAM,
        "adagrad": L.RS_OPT_ADAGRAD, "rowwise": L.RS_OPT_ROWWISE_ADAGRAD}
LR, EPS = 0.05, 1e-7


def _state(opt, w0, rng_seed=9):
    r = np.random.default_rng(rng_seed)
    V, D = w0.shape
    w = dev(w0)
    if opt == "sgd":
        return [w, None, None, None]
    if opt in ("lazy", "keras"):
        m = dev(r.standard_normal((V, D)).astype(f32) * 0.1)
        v = dev(r.random((V, D)).astype(f32) * 0.1)
        bm = torch.zeros((V + 31) // 32, dtype=torch.int32, device=DEV) if opt == "keras" else None
        return [w, m, v, bm]
    acc = dev((0.1 + r.random((V, D) if opt == "adagrad" else (V,))).astype(f32))
    return [w, acc, None, None]


def _apply(opt, st, s_rows, s_pos, n, grad, scale, remapped):
    """remapped: rs_embedding_apply_scaled with bag positions, dout and the per-bag scale (NULL
    for the sum), scale_group 1; otherwise the unchanged rs_embedding_apply on expanded rows.
    Keras Adam is followed by its dense sweep. Returns the touched bitmap before the sweep."""
    w, m, v, bm = st
    V, D = w.shape
    c = {k: float(x) for k, x in O.keras_adam_coefficients(1, LR, epsilon=EPS).items()}
    if opt in ("lazy", "keras"):
        p = L.AdamParams(c["lr"], c["beta1"], c["beta2"], c["one_minus_beta1"],
                         c["one_minus_beta2"], c["epsilon"])
    else:
        p = L.AdamParams(float(f32(LR)), 0.0, 0.0, 0.0, 0.0, float(f32(EPS)))
    ws = torch.empty(L.lib().rs_apply_workspace_size(n, D), dtype=torch.uint8, device=DEV)
    if remapped:
        L.call("rs_embedding_apply_scaled", KIND[opt], L.ptr(w), L.ptr(m), L.ptr(v), V, D,
               L.ptr(s_rows), L.ptr(s_pos), n, L.ptr(grad), L.ptr(scale), 1, p, L.ptr(bm),
               L.ptr(ws), ws.numel(), L.stream_ptr(w.device))
    else:
        L.call("rs_embedding_apply", KIND[opt], L.ptr(w), L.ptr(m), L.ptr(v), V, D, L.ptr(s_rows),
               L.ptr(s_pos), n, L.ptr(grad), p, L.ptr(bm), L.ptr(ws), ws.numel(),
               L.stream_ptr(w.device))
    bitmap = None if bm is None else bm.clone()
    if opt == "keras":
        L.call("rs_keras_adam_dense_sweep", L.ptr(w), L.ptr(m), L.ptr(v), V, D, p, L.ptr(bm),
               L.stream_ptr(w.device))
    torch.cuda.synchronize()
    return bitmap


@pytest.mark.parametrize("D", [4, 18, 128])
@pytest.mark.parametrize("opt", OPTS)
def test_remapped_apply_equals_expanded_apply(opt, D, rng):
    w0 = rng.standard_normal((R.V, D)).astype(f32)
    for name, c in R.backward_cases().items():
        for mode in (R.MEAN, R.SUM):
            n, nb = c["ids"].size, c["n_bags"]
            ids, valid = dev(c["ids"]), dev(c["valid"])
            offsets = dev(c["offsets"])
            dout_np = rng.standard_normal((nb, D)).astype(f32)
            dout = dev(dout_np)
            _, scale_np, _, _ = R.bag_forward(np.zeros((R.V, 1), f32), c["ids"], nb, c["offsets"],
                                              c["bag_len"], c["valid"], mode=R.MEAN)
            scale = dev(scale_np) if mode == R.MEAN else None
            s = SortedIds(ids, R.V, valid=valid, count_unique=False)
            # expanded gradient, checked against the restatement
            rows = torch.full((n, D), 3.0, device=DEV)
            L.call("rs_embedding_bag_expand_grad", L.ptr(dout), D, D, n, L.ptr(offsets), nb,
                   c["bag_len"], L.ptr(scale), None, L.ptr(rows), L.stream_ptr(rows.device))
            rows_ref = R.bag_expand(dout_np, n, nb, c["offsets"], c["bag_len"],
                                    scale_np if mode == R.MEAN else None)
            np.testing.assert_array_equal(rows.cpu().numpy(), rows_ref, err_msg=name)
            a, b = _state(opt, w0), _state(opt, w0)
            bag_pos = gpu_remap(s.pos, n, nb, c["offsets"], c["bag_len"])
            bm_a = _apply(opt, a, s.rows, bag_pos, n, dout, scale, True)
            bm_b = _apply(opt, b, s.rows, s.pos, n, rows, None, False)
            for x, y, what in zip(a[:3], b[:3], ("table", "m / accumulator", "v")):
                if x is not None:
                    assert torch.equal(x, y), (name, mode, what)
            if bm_a is not None:
                assert torch.equal(bm_a, bm_b), (name, mode, "touched bitmap")
            if name == "all_masked":
                assert opt == "keras" or torch.equal(a[0], dev(w0))
            # the expanded path against the NumPy reference step, 1e-5 relative
            if opt in ("sgd", "lazy", "adagrad"):
                init = [None if t is None else t.cpu().numpy() for t in _state(opt, w0)[:3]]
                rw, rm, rv = R.ref_step(opt, tuple(init), c["ids"], c["valid"], rows_ref, LR,
                                        eps=EPS)
                assert_close_rel(b[0].cpu().numpy(), rw, msg=f"{name} table")
                if rm is not None:
                    assert_close_rel(b[1].cpu().numpy(), rm, msg=f"{name} m / accumulator")


# ---- module level --------------------------------------------------------------------------
def _opt(kind, tables, fused):
    if kind == "sgd":
        return SparseSGD(tables, lr=LR, fused=fused)
    if kind in ("lazy", "keras"):
        return SparseAdam(tables, lr=LR, mode=kind, fused=fused)
    return SparseAdagrad(tables, lr=LR, rowwise=kind == "rowwise", fused=fused)


def _opt_state(opt, t):
    st = getattr(opt, "state", None)
    if not st:
        return []
    s = st[id(t)]
    return [x for x in (s if isinstance(s, tuple) else (s,)) if x is not None]


def _torch_pool(rows, bag_of_pos, live, n_bags, scale):
    """Plain-lookup rows pooled with torch: index_add_ of the live rows, the mean as a multiply
    by the same bag_scale."""
    idx = torch.nonzero(live).reshape(-1)
    pooled = torch.zeros(n_bags, rows.shape[1], device=DEV).index_add_(0, bag_of_pos[idx], rows[idx])
    return pooled if scale is None else pooled * scale[:, None]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode", ["mean", "sum"])
@pytest.mark.parametrize("kind", OPTS)
def test_module_two_steps_match_plain_lookup(kind, mode, fused, rng):
    """The loss is linear in the pooled rows, so every gradient row is a copy of the upstream
    row times (mean) one rounded 1 / count: the tables must agree bit for bit."""
    Vt, D, nb, Lh = 600, 18, 130, 9
    w0 = rng.standard_normal((Vt, D)).astype(f32)
    bag = EmbeddingBag(Vt, D, mode=mode, device=DEV, weight=torch.from_numpy(w0))
    plain = Embedding(Vt, D, device=DEV, weight=torch.from_numpy(w0))
    ob, op = _opt(kind, bag, fused), _opt(kind, plain, False)
    for step in range(2):
        ids = dev(rng.integers(0, Vt, (nb, Lh)))
        valid = dev((rng.random((nb, Lh)) < 0.7).astype(np.uint8))
        valid[5] = 0
        coef = dev(rng.standard_normal((nb, D)).astype(f32))
        (bag(ids, valid=valid) * coef).sum().backward()
        ob.step()
        count = valid.sum(1).float()
        scale = torch.where(count > 0, 1.0 / count, torch.zeros_like(count)) if mode == "mean" else None
        bag_of_pos = torch.arange(nb, device=DEV).repeat_interleave(Lh)
        rows = plain(ids.reshape(-1), grad_mask=valid.reshape(-1))
        (_torch_pool(rows, bag_of_pos, valid.reshape(-1) != 0, nb, scale) * coef).sum().backward()
        op.step()
        torch.cuda.synchronize()
        assert torch.equal(bag.weight, plain.weight), (kind, mode, fused, step)
        for x, y in zip(_opt_state(ob, bag), _opt_state(op, plain)):
            assert torch.equal(x, y)
    assert not torch.equal(bag.weight, dev(w0))


@pytest.mark.parametrize("kind", ["sgd", "lazy", "adagrad"])
def test_mixed_step_is_one_concatenated_gradient(kind, rng):
    """A plain lookup and a bag lookup of one table in one step: expanded, concatenated,
    deduplicated once — the same as two plain lookups."""
    Vt, D = 300, 4
    w0 = rng.standard_normal((Vt, D)).astype(f32)
    t = EmbeddingBag(Vt, D, mode="mean", device=DEV, weight=torch.from_numpy(w0))
    p = Embedding(Vt, D, device=DEV, weight=torch.from_numpy(w0))
    ot, op = _opt(kind, t, False), _opt(kind, p, False)
    a = dev(rng.integers(0, Vt, 64))
    ids = dev(rng.integers(0, Vt, 200))
    offsets = dev(np.concatenate([[0], np.sort(rng.integers(0, 201, 30)), [200]]).astype(np.int64))
    nb = offsets.numel() - 1
    ca, cb = dev(rng.standard_normal((64, D)).astype(f32)), dev(rng.standard_normal((nb, D)).astype(f32))
    loss = (Embedding.forward(t, a) * ca).sum() + (t(ids, offsets) * cb).sum()
    loss.backward()
    assert t.take_bag_grad() is None  # not the sole contribution
    ot.step()
    lens = offsets[1:] - offsets[:-1]
    bag_of_pos = torch.arange(nb, device=DEV).repeat_interleave(lens)
    scale = torch.where(lens > 0, 1.0 / lens.float(), torch.zeros(nb, device=DEV))
    live = torch.ones(200, dtype=torch.bool, device=DEV)
    loss = (p(a) * ca).sum() + (_torch_pool(p(ids), bag_of_pos, live, nb, scale) * cb).sum()
    loss.backward()
    op.step()
    torch.cuda.synchronize()
    assert torch.equal(t.weight, p.weight)


def test_take_grad_densify_dedup_see_the_expanded_entry(rng):
    Vt, D, nb, Lh = 200, 4, 33, 5
    t = EmbeddingBag(Vt, D, mode="mean", device=DEV)
    ids_np = rng.integers(0, Vt, (nb, Lh))
    valid_np = (rng.random((nb, Lh)) < 0.7).astype(np.uint8)
    coef = rng.standard_normal((nb, D)).astype(f32)

    def backward():
        (t(dev(ids_np), valid=dev(valid_np)) * dev(coef)).sum().backward()
    _, scale, _, _ = R.bag_forward(np.zeros((Vt, D), f32), ids_np, nb, bag_len=Lh, valid=valid_np,
                                   mode=R.MEAN)
    rows_ref = R.bag_expand(coef, nb * Lh, nb, None, Lh, scale)
    backward()
    assert t.has_grad()
    ids, rows, valid = t.take_grad(with_valid=True)
    np.testing.assert_array_equal(ids.cpu().numpy(), ids_np.reshape(-1))
    np.testing.assert_array_equal(rows.cpu().numpy(), rows_ref)
    np.testing.assert_array_equal(valid.cpu().numpy(), valid_np.reshape(-1))
    assert not t.has_grad()
    dense = densify_grad(t, ids, rows, valid=valid).cpu().numpy()
    ref = np.zeros((Vt, D), np.float64)
    live = valid_np.reshape(-1) != 0
    np.add.at(ref, ids_np.reshape(-1)[live], rows_ref[live].astype(np.float64))
    assert_close_rel(dense, ref, msg="densified bag gradient")
    backward()
    ids, rows = t.take_grad()
    ur, ug = dedup_grad(t, ids, rows * dev(valid_np.reshape(-1, 1).astype(f32)))
    assert_close_rel(ug.cpu().numpy(), ref[ur.cpu().numpy()], msg="deduplicated bag gradient")


def test_weighted_sum_expands_and_matches_plain(rng):
    Vt, D, nb, Lh = 300, 18, 40, 6
    w0 = rng.standard_normal((Vt, D)).astype(f32)
    t = EmbeddingBag(Vt, D, mode="sum", device=DEV, weight=torch.from_numpy(w0))
    p = Embedding(Vt, D, device=DEV, weight=torch.from_numpy(w0))
    ot, op = SparseSGD(t, lr=LR), SparseSGD(p, lr=LR)
    ids = dev(rng.integers(0, Vt, (nb, Lh)))
    w = dev(rng.standard_normal((nb, Lh)).astype(f32))
    coef = dev(rng.standard_normal((nb, D)).astype(f32))
    (t(ids, per_sample_weights=w) * coef).sum().backward()
    assert t.take_bag_grad() is None
    ot.step()
    ((p(ids) * w[..., None]).sum(1) * coef).sum().backward()
    op.step()
    assert torch.equal(t.weight, p.weight)


def test_slab_bag_sgd_step(rng):
    """A slab of 3 uneven slots, bag b in slot b % 3: one SGD step through the remapped apply
    against the same update computed in float64."""
    so = np.array([0, 7, 107, 118], np.int64)
    card = np.diff(so)
    D, nb, Lh = 4, 60, 5
    w0 = rng.standard_normal((118, D)).astype(f32)
    t = EmbeddingBag(118, D, mode="mean", device=DEV, weight=torch.from_numpy(w0),
                     slot_offsets=torch.from_numpy(so))
    opt = SparseSGD(t, lr=LR)
    ids_np = np.stack([rng.integers(0, card[b % 3], Lh) for b in range(nb)])
    coef = rng.standard_normal((nb, D)).astype(f32)
    out = t(dev(ids_np))
    ref_out, scale, _, _ = R.bag_forward(w0, ids_np, nb, bag_len=Lh, mode=R.MEAN, slot_offsets=so)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref_out)
    (out * dev(coef)).sum().backward()
    opt.step()
    ref = w0.astype(np.float64)
    for b in range(nb):
        for i in ids_np[b]:
            ref[so[b % 3] + i] -= LR * float(scale[b]) * coef[b].astype(np.float64)
    assert_close_rel(t.weight.cpu().numpy(), ref, msg="slab bag SGD")
    assert not t.oob_detected()


# ---- pooled_history BASE -------------------------------------------------------------------
def _base_models():
    from recommender_amd.dien import BaseModel

    ms = []
    for pooled in (False, True):
        g = torch.Generator(device=DEV)
        g.manual_seed(2)
        ms.append(BaseModel(item_vocab_size=3001, item_embedding_size=18, cat_vocab_size=81,
                            cat_embedding_size=18, mlp_units=[200, 80, 1], device=DEV, generator=g,
                            pooled_history=pooled))
    return ms


def test_pooled_history_matches_default_within_derived_bound():
    """rep = the history mean. Default: torch's sum of the masked rows, divided; pooled: the
    kernel's ordered sum, divided. Both are fp32 sums of the same n = count terms, so each lies
    within R.reorder_bound of the exact sum and the two within twice that; the division adds one
    rounding each (2^-23 relative). One SGD step: the tables move by lr * gradient, and the two
    gradients differ by that relative size, judged at the project's 1e-5 against the size of
    the update."""
    from recommender_amd.dien.layers import compute_his_average
    from recommender_amd.dien.train import synthetic_batch

    base, pooled = _base_models()
    feats, label = synthetic_batch(np.random.default_rng(1), 256, 50, 3001, 81, negatives=False)
    feats = {k: torch.from_numpy(v).to(DEV) for k, v in feats.items()}
    item, cat = feats["pos_his_item"], feats["pos_his_cat"]
    mask = item != 0
    with torch.no_grad():
        his = base.compute_flat_embedding((item, cat))
        ref = compute_his_average(his, mask).cpu().numpy().astype(np.float64)
        got = pooled.pooled_his_average(item, cat, mask).cpu().numpy().astype(np.float64)
        terms = (his * mask[..., None]).cpu().numpy().astype(np.float64)
    cnt = mask.sum(1).cpu().numpy().astype(np.float64)
    bound = 2 * (cnt[:, None] * 2.0 ** -23 * np.abs(terms).sum(1)) / cnt[:, None] \
        + 2.0 ** -22 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"pooled history: max err {err.max():.3g}, max err / bound {(err / bound).max():.3g}")
    assert (err <= bound).all()
    # the models' outputs, then one SGD step on both
    lab = torch.from_numpy(label).to(DEV)
    opts = [SparseSGD([m.item_embedding, m.cat_embedding], lr=1.0) for m in (base, pooled)]
    probs = []
    for m, o in zip((base, pooled), opts):
        prob = m(feats, training=True)
        probs.append(prob.detach().cpu().numpy())
        torch.nn.functional.binary_cross_entropy(prob, lab).backward()
        o.step()
    assert_close_rel(probs[1], probs[0], msg="BASE prob")
    torch.cuda.synchronize()
    fresh = _base_models()[0]
    for name in ("item_embedding", "cat_embedding"):
        w0 = getattr(fresh, name).weight.cpu().numpy()
        w_ref = getattr(base, name).weight.cpu().numpy()
        w_got = getattr(pooled, name).weight.cpu().numpy()
        upd = np.abs(w_ref - w0).max()
        d = np.abs(w_got - w_ref).max()
        print(f"pooled history SGD step, {name}: max diff {d:.3g}, max update {upd:.3g}")
        assert upd > 0
        # 1e-5 of the update, plus the rounding of w - update itself (one ulp of the weights)
        assert d <= 1e-5 * upd + 2.0 ** -23 * np.abs(w0).max()


def test_pooled_history_all_padding_is_finite():
    from recommender_amd.dien.train import synthetic_batch

    _, pooled = _base_models()
    feats, _ = synthetic_batch(np.random.default_rng(1), 16, 20, 3001, 81, negatives=False)
    feats["pos_his_item"][3] = 0
    feats["pos_his_cat"][3] = 0
    feats = {k: torch.from_numpy(v).to(DEV) for k, v in feats.items()}
    with torch.no_grad():
        prob = pooled(feats)
    assert torch.isfinite(prob).all()


# ---- error paths ---------------------------------------------------------------------------
def test_python_error_paths():
    t = EmbeddingBag(50, 4, mode="mean", device=DEV)
    ids = torch.zeros(3, 4, dtype=torch.int64, device=DEV)
    w = torch.ones(3, 4, device=DEV)
    with pytest.raises(ValueError, match="sum"):
        t(ids, per_sample_weights=w)                                  # MEAN with weights
    with pytest.raises(L.RecsysError):                                # and at the C ABI
        L.call("rs_embedding_bag_fwd", L.ptr(t.weight), 50, 4, L.ptr(ids), 1, 12, None, 3, 4,
               None, L.ptr(w), L.RS_BAG_MEAN, None, 1, L.ptr(torch.empty(3, 4, device=DEV)), 4,
               None, None, None)
    with pytest.raises(ValueError, match="gradient"):
        embedding_bag(t, ids, mode="sum", per_sample_weights=w.clone().requires_grad_())
    with pytest.raises(L.RecsysError):                                # n_ids != n_bags * bag_len
        L.call("rs_embedding_bag_fwd", L.ptr(t.weight), 50, 4, L.ptr(ids), 1, 11, None, 3, 4,
               None, None, 0, None, 1, L.ptr(torch.empty(3, 4, device=DEV)), 4, None, None, None)
    with pytest.raises(Exception):
        t(ids.cpu())                                                  # a CPU tensor
    with pytest.raises(ValueError):
        t(ids.reshape(-1))                                            # flat ids need offsets
    k = EmbeddingBag(50, 4, device=DEV)
    SparseAdam(k, mode="keras", fused=True, defer_decay=True)
    with pytest.raises(NotImplementedError, match="presort"):
        k(ids)
    torch.cuda.synchronize()
