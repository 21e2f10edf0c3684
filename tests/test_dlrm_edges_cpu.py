"""What tests/test_dlrm_edges_gpu.py relies on, proven without a GPU: the inputs of
tests/dlrm_edges.py have the properties the GPU tests name, the float64 restatements equal
autograd of the model's top half written the way the reference writes it, deliberately wrong
restatements are caught by that comparison, and the launchers' arithmetic (the walk batch, the
fold's segments, which dlrm_bwd_pipe instantiation an input reaches) is what the tests assume."""
import numpy as np
import pytest
import torch

from oracle.ctr import bce, bce_grad
from tests import dlrm_edges as E


# =============================================================================================
# arithmetic
def test_walk_batch_is_prime_and_above_every_residency():
    assert E.walk_batch(256) == 16411
    for cus in (1, 64, 228, 256, 304):
        b = E.walk_batch(cus)
        assert b > 64 * cus and all(b % d for d in range(2, int(b ** 0.5) + 1))
        # at most 8 blocks x 4 waves per CU and 2 rounds: ceil(b / slots) >= 2, and a prime b is
        # no multiple of any epw >= 2, nor of 4·epw
        for per_cu in range(1, 9):
            for rounds in (1, 2):
                epw = -(-b // (cus * per_cu * 4 * rounds))
                assert epw >= 2 and b % epw != 0


def test_bwd_pipe_instantiations():
    """Which (GREG, KS) each tested shape reaches; <8, 16> cannot be reached: F >= 29 makes the
    compact row 534 floats wide, more than 8 x 64."""
    assert E.grad_width(29, 128, True) == 534 > 512
    seen = set()
    for S in (1, 15, 16, 26, 27, 28, 31):
        for compact in (True, False):
            seen.add(E.bwd_pipe_instance(S + 1, 128, compact))
    assert seen == {(8, 14), (20, 14), (20, 16)}
    assert E.bwd_pipe_instance(27, 128, False) == (20, 14) and E.grad_width(27, 128, False) == 857
    assert E.bwd_pipe_instance(28, 128, True) == (8, 14)
    assert E.bwd_pipe_instance(29, 128, True) == (20, 16)
    assert E.bwd_pipe_instance(32, 128, False) == (20, 16)
    assert E.bwd_pipe_instance(33, 128, True) is None
    assert all(E.bwd_pipe_instance(F, 128, c) != (8, 16) for F in range(2, 40) for c in (0, 1))


def test_fold_segments():
    """The batches of the fold cases: 1 and 2 chunks, then 33 and 65 (a ragged last segment)."""
    assert [-(-b // 4) for b in (1, 2, 3, 4, 5, 7)] == [1, 1, 1, 1, 2, 2]
    assert E.batch_for_blocks(33) == 129 and E.batch_for_blocks(65) == 257
    assert E.fold_shape(33) == (2, 17, 1)
    assert E.fold_shape(65) == (3, 22, 2)
    assert E.fold_shape(1) == (1, 1, 1) and E.fold_shape(2) == (1, 2, 1)


# =============================================================================================
# inputs
@pytest.mark.parametrize("B,D", [(131, 128), (131, 64), (7, 128), (509, 128)])
def test_relu_dense_properties(B, D):
    d = E.relu_dense(B, D, torch.Generator().manual_seed(B + D)).numpy()
    zero = d == 0
    assert 0.30 <= zero.mean() <= 0.70
    assert zero[:, D - 3].all()
    assert np.signbit(d[zero]).any() and (~np.signbit(d[zero])).any()
    assert np.signbit(d[:, D - 3]).any() and (~np.signbit(d[:, D - 3])).any()
    assert 1 <= (d < 0).sum() <= 0.05 * d.size and not (d[:, D - 3] < 0).any()


def test_sweep_classes():
    h = E.sweep_h()
    assert h.size == 257 + 51 and h[0] == -20 and h[256] == 20 and h[257] == 15
    with np.errstate(over="ignore"):
        y = (np.float32(1) / (np.float32(1) + np.exp(-h))).astype(np.float32)
    first = {k: int(v[:257].sum()) for k, v in E.sweep_classes(y).items()}
    assert first == {"below": 25, "one": 22, "inside": 210, "near_in": 9, "near_out": 9}
    assert all(int(v.sum()) >= 5 for v in E.sweep_classes(y).values())
    # the second sweep crosses the upper end: predictions on 1 − eps itself (1 / (1 + ulp), the
    # last value below 1 this form of the sigmoid can give), below it, and exactly 1
    hi = y[257:]
    assert (hi < E.HI32).sum() >= 5 and (hi == E.HI32).sum() >= 5 and (hi == 1).sum() >= 5
    assert float(E.HI32) == 0.9999998807907104
    # so a prediction above 1 − eps is exactly 1, where y(1 − y) = 0 and G = 0 whatever the gate
    # says: the gate's upper end shows in no output (its lower end does)
    assert ((y > E.HI32) == (y == 1)).all()


def test_clip_inputs_make_h_the_sweep():
    table, ids, offs, dense, xin, label, q, c = E.clip_inputs(64, 3)
    S = 2
    p, hm, *_ = E.reference(table, ids, offs, dense, xin, label, q, c, S, 64)
    h = torch.log(p / (1 - p))
    assert torch.equal(dense[:, 0], torch.from_numpy(E.sweep_h()))
    inside = (p > 1e-6) & (p < 1 - 1e-6)
    assert torch.allclose(h[inside], dense[:, 0].double()[inside], rtol=1e-6, atol=1e-9)
    assert sorted(set(label.tolist())) == pytest.approx([0.0, 0.3, 1.0])
    assert float(c) == 0 and int((q != 0).sum()) == 1


@pytest.mark.parametrize("id64", [False, True])
def test_edge_ids(id64):
    cards = [1, 7, 300, 2, 1]
    ids, bad = E.edge_ids(40, cards, id64, 5)
    v = ids.numpy().astype(np.int64)
    assert ids.dtype == (torch.int64 if id64 else torch.int32)
    for s, c in enumerate(cards):
        col = v[:-1, s]
        assert (col == c - 1).any() and (col == c).any() and (col == -1).any()
        if id64:
            assert (col == 2 ** 32 + 1).any() and (col == E.I64_MIN).any()
    assert bad[-1].all() and not bad[0].any()
    assert (bad == ((v < 0) | (v >= np.asarray(cards)[None]))).all()
    # a row holds at most one out-of-range id, except the last
    assert (bad[:-1].sum(1) <= 1).all()


def test_pow2_inputs_range():
    table, _, _, dense, *_ = E.pow2_inputs(131, 5, 128, False, 9)
    for t in (table, dense):
        a = t.abs()
        assert float(a.min()) >= 2.0 ** -6 and float(a.max()) <= 2.0 ** 6
        assert bool((t < 0).any()) and bool((t > 0).any())
    assert bool(torch.isfinite(table * 2.0 ** 8).all())


def test_train_inputs_oob_and_slab():
    cards = [1, 7, 300, 2, 1]
    table, ids, offs, *_ = E.train_inputs(50, 5, 64, True, 1, cards=cards)
    assert offs.tolist() == [0, 1, 8, 308, 310, 311] and table.shape[0] == 311
    assert bool((ids >= 0).all()) and bool((ids < torch.tensor(cards)[None]).all())
    _, ids, offs, *_ = E.train_inputs(50, 5, 64, False, 1, shared=True, oob=True)
    assert offs is None and int(ids.max()) == 200 and int(ids.min()) == -1


# =============================================================================================
# the restatements against autograd
def _model(seed, qscale=0.05):
    B, S, D = 96, 5, 16
    cards = [1, 7, 30, 2, 9]
    table, ids, offs, _, xin, _, q, c = E.train_inputs(B, S, D, True, seed, cards=cards,
                                                       oob=True, qscale=qscale)
    g = torch.Generator().manual_seed(seed + 100)
    W = torch.randn(E.NI, D, generator=g, dtype=torch.float64)
    bias = torch.randn(D, generator=g, dtype=torch.float64) * 0.3
    bias[D - 3] = -100.0     # an all-zero relu column
    label = torch.tensor([0.0, 1.0, 0.3]).repeat(B // 3)
    return dict(table=table.double(), ids=ids, offs=offs, xin=xin.double(), W=W, bias=bias,
                label=label, q=q.double(), c=c.double(), S=S, D=D)


def _both(m, mutate=None):
    dense, loss, g_emb, g_q, g_c, g_W, g_b = E.autograd_top_half(
        m["table"], m["ids"], m["offs"], m["xin"], m["W"], m["bias"], m["label"], m["q"], m["c"],
        m["S"])
    p, hm, G, U, Um, sums, mags, nz, has_oob = E.reference(
        m["table"], m["ids"], m["offs"], dense, m["xin"], m["label"], m["q"], m["c"], m["S"],
        m["D"], mutate=mutate)
    pairs = {"rows": (G[:, None, None] * U, g_emb), "A_top": (sums["A_top"], g_q),
             "s_top": (sums["s_top"], g_c[0]), "A_bot": (sums["A_bot"], g_W),
             "s_bot": (sums["s_bot"], g_b), "loss": (sums["loss"] / p.numel(), loss)}
    rel = {k: float((a - b).abs().max() / b.abs().max()) for k, (a, b) in pairs.items()}
    return rel, p, dense, has_oob


def test_reference_equals_autograd():
    """G_b·U_b, A_top, s_top, A_bot, s_bot and the loss of the restatement against float64
    autograd, on inputs with out-of-range ids, exact zeros in the relu output and predictions on
    both sides of both clip ends."""
    m = _model(7, qscale=4.0)
    rel, p, dense, has_oob = _both(m)
    assert has_oob
    assert int((p < E.EPS).sum()) >= 3 and int((p > 1 - E.EPS).sum()) >= 3
    assert int(((p >= E.EPS) & (p <= 1 - E.EPS)).sum()) >= 10
    assert 0.3 <= float((dense == 0).double().mean()) <= 0.7 and bool((dense[:, -3] == 0).all())
    assert all(v <= 1e-12 for v in rel.values()), rel
    rel, *_ = _both(_model(8))       # the unsaturated head of the other tests
    assert all(v <= 1e-12 for v in rel.values()), rel


@pytest.mark.parametrize("mutate,hit", [("relu_ge", ("A_bot", "s_bot")),
                                        ("clip_no_upper", ("rows", "A_top", "s_top")),
                                        ("bottom_row", ("A_bot", "s_bot"))])
def test_wrong_restatements_are_caught(mutate, hit):
    rel, *_ = _both(_model(7, qscale=4.0), mutate=mutate)
    for k in hit:
        assert rel[k] > 1e-6, (k, rel[k])


def test_reference_shared_table_equals_one_slot_range():
    """offs = None (one table for every slot) is offs = [0, V] for each slot."""
    table, ids, offs, dense, xin, label, q, c = E.train_inputs(20, 3, 16, False, 4, shared=True,
                                                               oob=True)
    a = E.reference(table, ids, None, dense, xin, label, q, c, 3, 16)
    V = table.shape[0]
    X, ok = E.gather_x(table, ids, None, dense, 3)
    assert bool((ok == ((ids >= 0) & (ids < V))).all()) and a[-1]
    assert torch.equal(X[:, :3][ok], table.double()[ids.long()[ok]])
    assert bool((X[:, :3][~ok] == 0).all()) and torch.equal(X[:, 3], dense.double())


def test_bce_from_y_equals_oracle():
    """The BCE restatement the GPU tests evaluate on the kernel's y, against oracle.ctr's Keras
    BCE and its derivative on float32 predictions of the sweep (the oracle takes its logs in
    float32: 2e-7 of each term)."""
    h = E.sweep_h()
    with np.errstate(over="ignore"):
        y = (np.float32(1) / (np.float32(1) + np.exp(-h))).astype(np.float32)
    for lab in (0.0, 1.0, 0.3):
        lb = np.full(y.shape, lab, np.float32)
        loss, gate, G = E.bce_from_y(y, lb, 1.0 / y.size)
        ref = bce(lb, y).astype(np.float64)
        terms = np.abs(lab * np.log(np.clip(y, E.EPS32, E.HI32) + E.EPS32)) + np.abs(
            (1 - lab) * np.log(1 - np.clip(y, E.EPS32, E.HI32) + E.EPS32))
        assert (np.abs(loss - ref) <= 2e-7 * terms + 1e-9).all()
        dref = bce_grad(lb, y).astype(np.float64)
        assert ((dref == 0) == ((~gate) | (dref == 0))).all() and (dref[~gate] == 0).all()
        y64 = y.astype(np.float64)
        dterms = (lab / (y64 + 1e-7) + (1 - lab) / (1 - y64 + 1e-7)) / y.size
        assert (np.abs(G - dref * y64 * (1 - y64)) <= 1e-6 * dterms * y64 * (1 - y64)).all()
    # saturated rows: the float32 clip gives log(2·eps32 as float32), not float64's log(2e-7)
    sat, _, _ = E.bce_from_y(np.float32([1.0]), [0.0], 1.0)
    assert 15.3 < float(sat[0]) < 15.45


def test_head_dx_and_bwd_references_agree_with_autograd():
    """U (with q's dense part on row S) is d(row·q)/dX, and bwd_reference is the vector-Jacobian
    product of the interaction row, compact and not."""
    B, S, D = 9, 4, 8
    F = S + 1
    table, ids, offs, dense, _, _, q, c = E.train_inputs(B, S, D, False, 2, cards=[3, 1, 5, 2],
                                                         oob=True)
    table, dense, q = table.double(), dense.double(), q.double()
    z, zm, y, hm, U, Um, has_oob = E.head_dx_reference(table, ids, offs, dense, q, c, S, 0)
    X, _ = E.gather_x(table, ids, offs, dense, S)
    Xv = X.clone().requires_grad_(True)
    iu = torch.triu_indices(F, F, 1)
    Z = Xv @ Xv.transpose(1, 2)
    row = torch.cat([Z[:, iu[0], iu[1]], Xv[:, S]], 1)
    (row @ q + float(c)).sum().backward()
    assert has_oob and float((Xv.grad - U).abs().max()) <= 1e-12 * float(U.abs().max())
    assert torch.allclose(row[:, :z.shape[1]].detach(), z) and torch.allclose((row @ q + 0.1).detach(), y)
    g = torch.Generator().manual_seed(3)
    for compact in (True, False):
        gw = E.grad_width(F, D, compact)
        gout = torch.randn(B, gw + 3, generator=g, dtype=torch.float64)
        ge, gd, gem, gdm = E.bwd_reference(table, ids, offs, dense, gout, S, compact)
        Xv = X.clone().requires_grad_(True)
        Z = Xv @ Xv.transpose(1, 2)
        if compact:
            full = torch.cat([Z[:, iu[0], iu[1]], Xv[:, S]], 1)
        else:
            keep = torch.triu(torch.ones(F, F), 1).bool()
            full = torch.cat([(Z * keep).reshape(B, F * F), Xv[:, S]], 1)
        (full * gout[:, :gw]).sum().backward()
        assert float((Xv.grad[:, :S] - ge).abs().max()) <= 1e-12 * float(ge.abs().max())
        assert float((Xv.grad[:, S] - gd).abs().max()) <= 1e-12 * float(gd.abs().max())
        assert bool((gem >= ge.abs() - 1e-12).all()) and bool((gdm >= gd.abs() - 1e-12).all())
