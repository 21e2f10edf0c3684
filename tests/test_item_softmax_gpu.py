"""rs_item_softmax_fwd / _bwd on the GPU against tests/item_softmax_ref.py: every output within
4 × rho32 (the float32 restatement's pooled error) of the float64 restatement, the structural
cases (a dominant column on every tile, wave-round and split boundary), targets, ids, bias,
magnitudes, non-finite inputs, splits, bit-reproducibility, graph replay, argument errors and the
Python surfaces. Every call goes through the C entry points with 64 guard elements of a fixed NaN
pattern behind each output and NaN in the [dim, ld) padding of the inputs.

Kernel worst ratios seen on an MI355X are recorded in DESIGN.md §4.13."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import item_softmax_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GUARD = 64
GUARD_BITS = 0x7FC12345  # a NaN with a payload
_WORST = {n: 0.0 for n in R.OUT}  # the kernel's worst error / rho32 over the pooled cases so far


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)


def placed(a, ld, offset):
    """a's rows at stride ld, `offset` floats into a NaN-filled buffer: (view, ld)."""
    ld = a.shape[1] if ld is None else ld
    w = max(ld, a.shape[1])  # an ld below dim (an argument error) is passed on, not laid out
    buf = torch.full((a.shape[0] * w + offset + 4,), float("nan"), device=DEV)
    view = buf[offset:offset + a.shape[0] * w].view(a.shape[0], w)
    view[:, :a.shape[1]] = dev(a, f32)
    return view, ld


def guarded(n):
    return torch.full((n + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV)


def taken(t, n):
    a = t.cpu().numpy()
    assert (a[n:] == GUARD_BITS).all(), "wrote behind the output"
    return a[:n].view(f32)


def run(c, n_splits=None, q_ld=None, i_ld=None, q_off=0, i_off=0, g_ld=None, want=("dq", "dv"),
        ws_bytes=None, expect=0, lse_in=None):
    """forward then backward of case c through the C entry points → {loss, lse, dq, dv}."""
    lib = L.lib()
    q, v = c["q"], c["v"]
    B, dim = q.shape
    M = v.shape[0]
    ns = c.get("n_splits", 1) if n_splits is None else n_splits
    tq, q_ld = placed(q, q_ld, q_off)
    tv, i_ld = placed(v, i_ld, i_off)
    tt, tb, ti = dev(c.get("targets"), np.int32), dev(c.get("bias"), f32), dev(c.get("ids"), np.int64)
    need = lib.rs_item_softmax_workspace_size(B, M, dim, ns)
    ws_bytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((ws_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    loss, lse = guarded(B), guarded(B)
    st_ = L.stream_ptr(tq.device)
    st = lib.rs_item_softmax_fwd(L.ptr(tq), q_ld, B, L.ptr(tv), i_ld, M, dim, L.ptr(tt),
                                 c.get("inv_temp", 1.0), L.ptr(tb), L.ptr(ti), ns, L.ptr(loss),
                                 L.ptr(lse), L.ptr(ws), ws_bytes, st_)
    torch.cuda.synchronize()
    assert st == expect, (st, lib.rs_last_error())
    assert (ws[ws_bytes:] == 0xAB).all()
    if st != 0:
        assert (loss == GUARD_BITS).all() and (lse == GUARD_BITS).all()  # nothing written
        return None
    out = {"loss": taken(loss, B).copy(), "lse": taken(lse, B).copy()}
    if not want:
        return out
    g_ld = dim if g_ld is None else g_ld
    g = dev(np.ones(B, f32) if c.get("g") is None else c["g"], f32)
    gq, gv = guarded(B * g_ld), guarded(M * g_ld)
    lse_t = lse[:B].view(torch.float32) if lse_in is None else dev(lse_in, f32)
    st = lib.rs_item_softmax_bwd(L.ptr(tq), q_ld, B, L.ptr(tv), i_ld, M, dim, L.ptr(tt),
                                 c.get("inv_temp", 1.0), L.ptr(tb), L.ptr(ti), ns, L.ptr(lse_t),
                                 L.ptr(g), L.ptr(gq) if "dq" in want else None, g_ld,
                                 L.ptr(gv) if "dv" in want else None, g_ld, L.ptr(ws), ws_bytes, st_)
    torch.cuda.synchronize()
    assert st == 0, (st, lib.rs_last_error())
    assert (ws[ws_bytes:] == 0xAB).all()
    for n, t, rows in (("dq", gq, B), ("dv", gv, M)):
        a = taken(t, rows * g_ld)
        if n not in want:
            assert (a.view(np.int32) == GUARD_BITS).all()
            continue
        a = a.reshape(rows, g_ld)
        assert (a[:, dim:].view(np.int32) == GUARD_BITS).all(), "wrote the [dim, ld) padding"
        out[n] = a[:, :dim].copy()
    return out


def same_bits(a, b):
    return all((a[n].view(np.uint32) == b[n].view(np.uint32)).all() for n in a)


@pytest.fixture(scope="module")
def tau():
    rho, mag = R.rho32(), R.rho32(mag=True)
    print("\n  rho32: " + " ".join(f"{n}={r:.3g}" for n, r in rho.items()))
    print("  rho32 (magnitude cases): " + " ".join(f"{n}={r:.3g}" for n, r in mag.items()))
    return {False: {n: 4 * r for n, r in rho.items()}, True: {n: 4 * r for n, r in mag.items()}}


def check(name, tau, got=None, ref=None, mag=False, **kw):
    """Case `name` (or the given result) against its float64 reference under 4 × rho32."""
    if got is None:
        c, ref, _ = R.case(name)
        got = run(c, **kw)
    for n in got:
        assert R.same_pattern(got[n], ref[n]), f"{name}: NaN / inf pattern of {n}"
    ratios = {n: r for n, r in R.ratios(dict(ref, **got), ref).items() if n in got}
    if not mag:
        for n, r in ratios.items():
            _WORST[n] = max(_WORST[n], r / (tau[False][n] / 4))
    print(f"\n  {name}: " + " ".join(f"{n}={r:.3g}" for n, r in ratios.items())
          + " | worst / rho32 so far: " + " ".join(f"{n}={r:.3g}" for n, r in _WORST.items()))
    bad = {n: f"{r:.3g} > {tau[mag][n]:.3g}" for n, r in ratios.items() if not r <= tau[mag][n]}
    assert not bad, f"{name}: above 4·rho32: {bad}"
    return got


# ---- accuracy over the shapes ------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] in "BM" or n.startswith("dim")])
def test_shapes(name, tau):
    check(name, tau)


@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith(("targets", "ids", "dup"))])
def test_targets_and_ids(name, tau):
    got = check(name, tau)
    if name == "ids_equal":  # each row keeps its target only
        assert (got["loss"] == 0).all() and (got["dq"] == 0).all() and (got["dv"] == 0).all()


@pytest.mark.parametrize("ns", R.SPLITS)
@pytest.mark.parametrize("as_target", [True, False])
def test_dominant_column_on_every_boundary(ns, as_target, tau):
    """Dropping or doubling the column would move lse by 30 or more: a million times tau."""
    names = [n for n in R.CASES if n.startswith(f"dom_{ns}_{int(as_target)}_")]
    assert len(names) == len(R.edge_columns(300, ns))
    for n in names:
        check(n, tau)


@pytest.mark.parametrize("name", list(R.MAG_CASES))
def test_logits_of_1e4_stay_finite(name, tau):
    got = check(name, tau, mag=True)
    assert all(np.isfinite(a).all() for a in got.values())


def test_grad_loss_zero_rows_and_six_decades(tau):
    got = check("zero_g", tau)
    assert (got["dq"][[1, 7, 33, 38]] == 0).all() and (got["dq"][2] != 0).any()


# ---- access paths ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,q_ld,i_ld,q_off,i_off", [(20, 24, 28, 0, 0), (20, 21, 23, 0, 0),
                                                       (20, 20, 20, 1, 3), (255, 256, 256, 0, 0),
                                                       (64, 64, 64, 0, 0)])
def test_strided_and_misaligned_rows_give_the_same_bits(dim, q_ld, i_ld, q_off, i_off, tau):
    """ld > dim with NaN padding; an ld or a base that is no multiple of 16 bytes takes the
    element loads: the same bits as contiguous aligned rows (dim 255 takes them either way)."""
    c = R.random_case(700 + dim, 33, 70, dim)
    ref = R.evaluate(c)
    base = check(f"contiguous dim {dim}", tau, got=run(c, n_splits=2), ref=ref)
    got = run(c, n_splits=2, q_ld=q_ld, i_ld=i_ld, q_off=q_off, i_off=i_off, g_ld=dim + 5)
    assert same_bits(base, got)
    if dim % 4 == 0:  # both bases one float off: element loads on both sides
        assert same_bits(base, run(c, n_splits=2, q_off=1, i_off=1))


# ---- bias, non-finite values -------------------------------------------------------------------
def test_inf_bias_on_a_negative_is_the_column_removed(tau):
    c, d, keep = R.inf_bias_case()
    gc = check("inf bias", tau, got=run(c), ref=R.evaluate(c))
    gd = check("column removed", tau, got=run(d), ref=R.evaluate(d))
    assert (gc["dv"][~keep] == 0).all()
    ref = R.evaluate(d)
    check("inf bias vs removed", tau, got=dict(gc, dv=gc["dv"][keep]), ref=ref)


def test_nan_query_row_poisons_only_what_the_contract_says(tau):
    for ns in (1, 2):
        c = R.nan_query_case(3)
        got = check(f"nan row, {ns} splits", tau, got=run(c, n_splits=ns), ref=R.evaluate(c))
        assert np.isnan(got["loss"][3]) and np.isnan(got["dq"][3]).all()
        assert np.isfinite(np.delete(got["dq"], 3, 0)).all() and np.isnan(got["dv"]).all()


def test_targets_outside_the_items_are_nan_rows_that_add_nothing(tau):
    c = R.random_case(3, 40, 70, 12)
    c["targets"][[1, 35]] = [-1, 70]
    got = check("bad targets", tau, got=run(c, n_splits=2), ref=R.evaluate(c))
    assert np.isnan(got["loss"][[1, 35]]).all() and (got["dq"][[1, 35]] == 0).all()


def test_infinite_logits_have_the_reference_pattern(tau):
    c = R.random_case(4, 3, 5, 4, ids=None)
    c["bias"][:] = [np.inf, 0, 0, 0, -np.inf]
    c["targets"][:] = [1, 0, 4]
    check("infinite logits", tau, got=run(c), ref=R.evaluate(c))


# ---- splits, determinism -----------------------------------------------------------------------
@pytest.mark.parametrize("ns", R.SPLITS + (0,))
def test_splits_accuracy_and_two_runs_bit_equal(ns, tau):
    c, ref, _ = R.case("splits1")
    a = check(f"splits {ns}", tau, got=run(c, n_splits=ns), ref=ref)
    assert same_bits(a, run(c, n_splits=ns))


@pytest.mark.parametrize("ns", R.SPLITS)
def test_a_prefix_of_the_rows_gives_the_same_row_bits(ns):
    c, _, _ = R.case("splits1")
    full = run(c, n_splits=ns)
    for k in (1, 33, 64):
        d = dict(c, q=c["q"][:k], targets=c["targets"][:k], g=c["g"][:k])
        part = run(d, n_splits=ns)
        for n in ("loss", "lse", "dq"):
            assert (part[n].view(np.uint32) == full[n][:k].view(np.uint32)).all(), (n, k)


def test_more_splits_than_rows(tau):
    """Ranges of no rows at all (7 ranges over 2 items and over 1 query) merge as nothing."""
    # a dominant negative: well conditioned (a random 1 x 2 case whose target wins has p_t - 1
    # and p_other cancel, and the float32 restatement itself is then outside the pool's rho32)
    c = R.dominant_case(1, 2, 5, 1, False, n_splits=7)
    ref = R.evaluate(c)
    ctl = R.ratios(R.evaluate(c, np.float32), ref)
    assert all(ctl[n] <= tau[False][n] / 4 for n in R.OUT), ctl
    check("1 x 2, 7 splits", tau, got=run(c), ref=ref)


def test_either_gradient_alone():
    c, _, _ = R.case("B33")
    both = run(c)
    for want in (("dq",), ("dv",)):
        one = run(c, want=want)
        assert (one[want[0]].view(np.uint32) == both[want[0]].view(np.uint32)).all()


def test_graph_replay_on_refilled_inputs_equals_eager():
    lib = L.lib()
    B, M, dim, ns = 65, 200, 24, 2
    a, b = R.random_case(31, B, M, dim, n_splits=ns), R.random_case(32, B, M, dim, n_splits=ns)
    tq, tv = torch.empty(B, dim, device=DEV), torch.empty(M, dim, device=DEV)
    tt = torch.empty(B, dtype=torch.int32, device=DEV)
    tb, tg = torch.empty(M, device=DEV), torch.empty(B, device=DEV)
    ti = torch.empty(M, dtype=torch.int64, device=DEV)
    outs = [torch.empty(n, device=DEV) for n in (B, B, B * dim, M * dim)]
    need = lib.rs_item_softmax_workspace_size(B, M, dim, ns)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def fill(c):
        for t, k in ((tq, "q"), (tv, "v"), (tt, "targets"), (tb, "bias"), (tg, "g"), (ti, "ids")):
            t.copy_(dev(c[k]))

    def step():
        st = L.stream_ptr(tq.device)
        L.call("rs_item_softmax_fwd", L.ptr(tq), dim, B, L.ptr(tv), dim, M, dim, L.ptr(tt), 1.0,
               L.ptr(tb), L.ptr(ti), ns, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(ws), need, st)
        L.call("rs_item_softmax_bwd", L.ptr(tq), dim, B, L.ptr(tv), dim, M, dim, L.ptr(tt), 1.0,
               L.ptr(tb), L.ptr(ti), ns, L.ptr(outs[1]), L.ptr(tg), L.ptr(outs[2]), dim,
               L.ptr(outs[3]), dim, L.ptr(ws), need, st)

    fill(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill(b)
    graph.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in outs]
    eager = run(b)
    for g_, n in zip(got, R.OUT):
        assert (g_.view(np.uint32) == eager[n].reshape(-1).view(np.uint32)).all(), n


# ---- errors ------------------------------------------------------------------------------------
def test_argument_errors():
    lib = L.lib()
    c = R.random_case(1, 5, 9, 8)
    run(c, q_ld=7, expect=-1, want=())
    run(c, i_ld=7, expect=-1, want=())
    run(c, n_splits=-1, expect=-1, want=())
    run(c, n_splits=1025, ws_bytes=1 << 20, expect=-1, want=())
    run(dict(c, inv_temp=float("inf")), expect=-1, want=())
    run(dict(c, targets=None, q=np.zeros((10, 8), f32)), expect=-1, want=())  # row 9 has no column
    need = lib.rs_item_softmax_workspace_size(5, 9, 8, 1)
    assert need > 0
    run(c, ws_bytes=need // 4, expect=-1, want=())
    run(c, ws_bytes=need)
    t = torch.zeros(64, device=DEV)
    st = L.stream_ptr(t.device)
    p = L.ptr(t)
    for dim in (0, 257):
        assert lib.rs_item_softmax_fwd(p, 300, 1, p, 300, 1, dim, None, 1.0, None, None, 1, p, p,
                                       p, 256, st) == -1
    assert lib.rs_item_softmax_fwd(p, 8, 1, p, 8, 0, 8, None, 1.0, None, None, 1, p, p, p, 256,
                                   st) == -1  # no items
    assert lib.rs_item_softmax_fwd(p, 8, 1, p, 8, 1 << 31, 8, None, 1.0, None, None, 1, p, p, p,
                                   256, st) == -1
    assert lib.rs_item_softmax_fwd(p, 8, -1, p, 8, 1, 8, None, 1.0, None, None, 1, p, p, p, 256,
                                   st) == -1
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.rs_item_softmax_fwd(args[0], 8, 1, args[1], 8, 1, 8, None, 1.0, None, None, 1,
                                       args[2], args[3], p, 256, st) == -1
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    bwd = lambda lse, g, gq, gi, gq_ld=8: lib.rs_item_softmax_bwd(
        p, 8, 1, p, 8, 1, 8, None, 1.0, None, None, 1, lse, g, gq, gq_ld, gi, 8, L.ptr(ws), 4096, st)
    assert bwd(None, p, p, p) == -1 and bwd(p, None, p, p) == -1 and bwd(p, p, None, None) == -1
    assert bwd(p, p, p, p, gq_ld=7) == -1
    assert bwd(p, p, p, p) == 0
    # no queries: a no-op that needs nothing
    assert lib.rs_item_softmax_fwd(None, 8, 0, None, 8, 0, 8, None, 1.0, None, None, 0, None, None,
                                   None, 0, st) == 0
    assert lib.rs_item_softmax_workspace_size(0, 9, 8, 1) == 0
    torch.cuda.synchronize()


# ---- the Python surfaces -----------------------------------------------------------------------
def _torch_loss(q, v, t, temperature, log_q, ids, reduction):
    z = (q @ v.T) / temperature
    if log_q is not None:
        z = z - log_q[None]
    if ids is not None:
        drop = (ids[None, :] == ids[t][:, None]) & (torch.arange(v.shape[0], device=q.device)[None] != t[:, None])
        z = z.masked_fill(drop, float("-inf"))
    loss = torch.logsumexp(z, 1) - z[torch.arange(q.shape[0], device=q.device), t]
    return loss if reduction == "none" else loss.sum() if reduction == "sum" else loss.mean()


def grad_ratio(got, ref):
    """The worst error of a gradient matrix under the measure of R.ratios."""
    blank = {k: np.zeros((1, 1)) for k in R.OUT}
    return R.ratios(dict(blank, dq=got), dict(blank, dq=ref))["dq"]


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_functional_against_torch_float64_autograd(reduction, tau):
    from recommender_amd import functional as RF
    from recommender_amd import nn as RN

    c, _, _ = R.case("B65")
    q = dev(c["q"]).requires_grad_()
    v = dev(c["v"]).requires_grad_()
    t, lq, ids = dev(c["targets"]), dev(c["bias"]), dev(c["ids"])
    w = dev(c["g"])
    loss = RF.item_softmax_loss(q, v, t, temperature=0.5, log_q=lq, item_ids=ids,
                                reduction=reduction)
    (loss * w).sum().backward() if reduction == "none" else loss.backward()
    q64 = q.detach().double().requires_grad_()
    v64 = v.detach().double().requires_grad_()
    ref = _torch_loss(q64, v64, t.long(), 0.5, lq.double(), ids, reduction)
    (ref * w.double()).sum().backward() if reduction == "none" else ref.backward()
    lt = tau[False]["loss"] * (65 if reduction == "sum" else 1)
    assert (loss.detach().double() - ref.detach()).abs().max().item() <= lt
    for n, got, r in (("dq", q.grad, q64.grad), ("dv", v.grad, v64.grad)):
        ratio = grad_ratio(got.cpu().numpy(), r.cpu().numpy())
        assert ratio <= tau[False][n], (n, ratio)
    mod = RN.ItemSoftmaxLoss(temperature=0.5, reduction=reduction)
    again = mod(q.detach(), v.detach(), t, log_q=lq, item_ids=ids)
    assert torch.equal(again, loss.detach())
    # the in-batch form: targets None, no ids, no log_q, rows of a wider matrix
    wide = torch.randn(40, 64, device=DEV)
    a, b = wide[:, :24].clone().requires_grad_(), wide[:, 32:56]
    l1 = RF.item_softmax_loss(a, b, reduction=reduction)
    l2 = _torch_loss(a.detach().double(), b.double(), torch.arange(40, device=DEV), 1.0, None, None,
                     reduction)
    assert (l1.detach().double() - l2).abs().max().item() <= tau[False]["loss"] * (40 if reduction == "sum" else 1)


def test_memory_condition():
    """Forward + backward at B = M = 4096, D = 64 raises the peak by less than B·M·4 bytes over
    the inputs, outputs and gradients: no [B, M] buffer exists."""
    from recommender_amd import functional as RF

    B = M = 4096
    q = torch.randn(B, 64, device=DEV).requires_grad_()
    v = torch.randn(M, 64, device=DEV).requires_grad_()
    RF.item_softmax_loss(q[:64], v[:64]).backward()  # the library is loaded, nothing is lazy
    q.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = RF.item_softmax_loss(q, v, temperature=0.1)
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    grads = q.grad.numel() * 4 + v.grad.numel() * 4 + 4
    print(f"\n  peak over the inputs: {extra / 2**20:.2f} MiB, gradients {grads / 2**20:.2f} MiB")
    assert np.isfinite(loss.item())
    assert extra - grads < B * M * 4


def _eges(seed=3):
    from recommender_amd.eges import train as T

    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    model = T.build("EGES", 500, 20, 30, embedding_size=32, device=DEV, generator=g)
    rng = np.random.default_rng(seed)
    batch = T.synthetic_batch(rng, 48, 500, 20, 30)
    batch[3][5, 0] = batch[3][9, 0]  # an accidental hit
    *inp, lab = (dev(a) for a in batch)
    return T, model, tuple(inp), lab


def test_eges_inbatch_step_against_torch_ops(tau):
    """One EGESStep(loss="inbatch") step: its loss and the gradients it hands on — to the hidden
    vectors (and through them to the side tables) and, as sparse rows, to the output table —
    against the same loss written with torch ops in float64; then the same step in a graph."""
    T, model, inp, lab = _eges()
    step = T.EGESStep(model, loss="inbatch", temperature=0.25)
    seen = {}
    get_hidden, accumulate = model.get_hidden, model.output_embedding.accumulate_grad

    def hidden_kept(x):
        h = get_hidden(x)
        h.retain_grad()
        seen["hidden"] = h
        return h

    def rows_kept(ids, rows, *a, **kw):
        seen["ids"], seen["rows"] = ids.clone(), rows.clone()
        return accumulate(ids, rows, *a, **kw)

    model.get_hidden, model.output_embedding.accumulate_grad = hidden_kept, rows_kept
    before = model.output_embedding.weight.detach().clone()
    loss = step(inp, lab)
    model.get_hidden, model.output_embedding.accumulate_grad = get_hidden, accumulate
    pos = inp[3][:, 0].long()
    h64 = seen["hidden"].detach().reshape(48, -1).double().requires_grad_()
    r64 = before[pos].double().requires_grad_()
    ref = _torch_loss(h64, r64, torch.arange(48, device=DEV), 0.25, None, pos, "mean")
    ref.backward()
    assert abs(loss.item() - ref.item()) <= tau[False]["loss"]
    assert torch.equal(seen["ids"].reshape(-1).long(), pos)
    got_h = seen["hidden"].grad.reshape(48, -1).cpu().numpy()
    got_r = seen["rows"].reshape(48, -1).cpu().numpy()
    assert grad_ratio(got_h, h64.grad.cpu().numpy()) <= tau[False]["dq"]
    assert grad_ratio(got_r, r64.grad.cpu().numpy()) <= tau[False]["dv"]
    moved = (model.output_embedding.weight.detach() != before).any(1).nonzero().reshape(-1)
    assert set(moved.tolist()) <= set(pos.tolist()) and len(moved) > 0  # the sparse apply
    # the same step captured in a graph: one stream, no host synchronisation in the loss
    step.static_step(inp, lab)
    replay = step.capture(inp, lab)
    assert np.isfinite(replay().item())


def test_eges_default_loss_is_bit_equal_to_the_sigmoid_step():
    import torch.nn.functional as F

    T, model, inp, lab = _eges()
    loss = T.EGESStep(model)(inp, lab)
    T2, model2, inp2, lab2 = _eges()
    logits = model2(inp2)
    ref = F.binary_cross_entropy_with_logits(logits, lab2)
    assert torch.equal(loss, ref.detach())
