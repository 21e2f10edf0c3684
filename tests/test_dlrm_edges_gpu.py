"""The three software-pipelined DLRM kernels of csrc/interaction.hip at their slot, batch, clip
and walk edges, through the C entry points (L.call):

  A  dlrm_train_chunk   rs_dlrm_train_step_fwd_unit, its _nofold form + rs_dlrm_train_fold
  B  dlrm_fwd_dx_pipe   rs_dlrm_interaction_fwd_head_dx (and inter_fwd_mfma<DX>, its other route)
  C  dlrm_bwd_pipe      rs_dlrm_interaction_bwd, rs_dlrm_interaction_bwd_rank1

Inputs, float64 restatements and the bound |got − ref| ≤ 1e-5 · Σ|terms| come from
tests/dlrm_edges.py (proven in tests/test_dlrm_edges_cpu.py). Every output has 64 guard elements
of a fixed NaN bit pattern behind it, compared as int32 after each call. Invariances (the walk
against windows run alone, the two routes of B, rank-one against materialised, one call against
two, two runs, power-of-two scaling) are bit-exact. The gate of the BCE clip and G are checked
against the kernel's own float32 y. The walk batch is the first prime above 64 x the CU count, at
which every wave walks at least two examples and the last one is cut short."""
import ctypes as C

import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import dlrm_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NI = E.NI
WIN = 509
NAN = float("nan")


def dev(inp):
    return tuple(None if t is None else t.to(DEV) for t in inp)


def stream():
    return L.stream_ptr(torch.device(DEV))


def code_of(ids):
    return L.id_dtype_code(ids)


class Out:
    """A float32 output of n elements with E.GUARD guard elements behind it."""

    def __init__(self, n, fill=None, lead=0):
        self.n, self.lead = int(n), lead
        self.buf = torch.full((lead + self.n + E.GUARD,), E.GUARD_BITS, dtype=torch.int32,
                              device=DEV)
        self.t = self.buf[lead:lead + self.n].view(torch.float32)
        if fill is not None:
            self.t.fill_(fill)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.lead)

    def check(self, msg):
        assert bool((self.buf[self.lead + self.n:] == E.GUARD_BITS).all()), f"{msg}: guard overwritten"
        assert bool((self.buf[:self.lead] == E.GUARD_BITS).all()), f"{msg}: written before the start"


def walk_batch():
    return E.walk_batch(torch.cuda.get_device_properties(0).multi_processor_count)


def windows(B):
    """First, middle and last window of WIN consecutive examples (the last holds the cut wave)."""
    return [0, (B // 2) // 4 * 4 + 1, B - WIN]


def cut(inp, w, per_example):
    """The examples [w, w + WIN) of an input tuple (per_example: which entries are per example)."""
    return tuple(t[w:w + WIN].contiguous() if i in per_example and t is not None else t
                 for i, t in enumerate(inp))


# =============================================================================================
# A. the train kernel
def sums_len(D):
    return 512 + 2 + NI * D + D


def run_train(inp, S, D, gscale=None, err_flag=True, two_call=False, keep=None, **over):
    """One train step on guarded outputs; `over` replaces arguments by name (for the refusals).
    Returns dict(y, rows [B·S, D], G, sums, err, outs)."""
    table, ids, offs, dense, xin, label, q, c = inp
    B, V = ids.shape[0], table.shape[0]
    y, rows, G, sums = Out(B, NAN), Out(B * S * D, NAN), Out(B, NAN), Out(sums_len(D), NAN)
    ws_n = L.lib().rs_dlrm_train_workspace_size(B)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if err_flag else None
    a = dict(table=L.ptr(table), n_rows=V, D=D, ids=L.ptr(ids), id_dtype=code_of(ids), n_slots=S,
             slot_offsets=L.ptr(offs), dense=L.ptr(dense), xin=L.ptr(xin), n_in=NI,
             label=L.ptr(label), batch=B, q=L.ptr(q), c=L.ptr(c), eps=E.EPS,
             loss_scale=1.0 / B if gscale is None else gscale, y=y.ptr(), unit_rows=rows.ptr(),
             g_rows=G.ptr(), sums=sums.ptr(), workspace=L.ptr(ws), ws_bytes=ws_n,
             err_flag=L.ptr(err), stream=stream())
    a.update(over)
    outs = dict(y=y, rows=rows, G=G, sums=sums)
    if keep is not None:
        keep.update(outs)
    try:
        if two_call:
            L.call("rs_dlrm_train_step_fwd_unit_nofold",
                   *[v for k, v in a.items() if k != "sums"])
            L.call("rs_dlrm_train_fold", a["workspace"], a["ws_bytes"], a["batch"], a["D"],
                   a["id_dtype"], a["sums"], a["stream"])
        else:
            L.call("rs_dlrm_train_step_fwd_unit", *a.values())
    finally:
        torch.cuda.synchronize()
        for k, o in outs.items():
            o.check(k)
    return dict(y=y.t, rows=rows.t.view(B * S, D), G=G.t, sums=sums.t,
                err=int(err.item()) if err_flag else None, outs=outs)


def same_train(a, b, msg, sums=True):
    for k in ("y", "rows", "G") + (("sums",) if sums else ()):
        assert torch.equal(a[k], b[k]), f"{msg}: {k} differs"


def check_from_y(out, label, gscale, msg=""):
    """The clip gate, G and the loss sum against Keras BCE evaluated on the kernel's own y."""
    y = out["y"].cpu().numpy()
    g = out["G"].cpu().numpy().astype(np.float64)
    loss, gate, Gy = E.bce_from_y(y, label.cpu().numpy(), gscale)
    assert ((g == 0) == ~gate).all(), f"{msg} gate: G == 0 on {int((g == 0).sum())} rows, " \
                                      f"outside the clip {int((~gate).sum())}"
    dg = np.abs(g - Gy)
    print(f"{msg} G from y: max rel {float((dg[gate] / np.abs(Gy[gate])).max()) if gate.any() else 0:.3g}")
    assert (dg <= 2e-6 * np.abs(Gy)).all(), f"{msg} G from y"
    got = float(out["sums"][513])
    print(f"{msg} loss {got!r} vs {loss.sum()!r}, bound {1e-5 * np.abs(loss).sum():.3g}")
    assert abs(got - loss.sum()) <= 1e-5 * np.abs(loss).sum(), f"{msg} loss sum"
    return loss, gate, Gy


def check_sums(out, s64, m64, nz, D, loss=True):
    s = out["sums"]
    a = 512
    E.close(s[:nz + D], s64["A_top"], m64["A_top"], "A_top")
    assert bool((s[nz + D:a] == 0).all()), "A_top padding"
    E.close(s[a], s64["s_top"], m64["s_top"], "s_top")
    if loss:
        E.close(s[a + 1], s64["loss"], m64["loss"], "loss")
    E.close(s[a + 2:a + 2 + NI * D].view(NI, D), s64["A_bot"], m64["A_bot"], "A_bot")
    E.close(s[a + 2 + NI * D:], s64["s_bot"], m64["s_bot"], "s_bot")
    # an all-zero dense column passes no bottom gradient at all
    assert bool((s[a + 2:a + 2 + NI * D].view(NI, D)[:, D - 3] == 0).all()), "A_bot of a zero column"
    assert float(s[a + 2 + NI * D + D - 3]) == 0.0, "s_bot of a zero column"


def check_train(out, inp, S, D, gscale=None, msg=""):
    """Everything test_chunked_train_kernel_vs_float64 checks, plus the checks on the kernel's
    own y and the exact zeros of an all-zero dense column."""
    B = inp[1].shape[0]
    gs = 1.0 / B if gscale is None else gscale
    p, hm, G64, U64, Um, s64, m64, nz, has_oob = E.reference(*inp, S, D, gscale=gs)
    assert (out["err"] != 0) == has_oob, f"{msg} err flag {out['err']}, oob {has_oob}"
    y, U, G = out["y"], out["rows"], out["G"]
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(U).all()) and bool(torch.isfinite(y).all())
    assert bool(torch.isfinite(out["sums"]).all())
    E.close(y, p, 0.25 * hm + 0.03 * p, f"{msg} y")
    E.close(U.view(B, S, D), U64, Um, f"{msg} unit rows")
    dG = (G.double() - G64).abs()
    assert bool((dG <= 2e-6 * G64.abs() + 1e-5 * hm * gs / 4).all()), float(dG.max())
    check_sums(out, s64, m64, nz, D)
    check_from_y(out, inp[5], gs, msg)
    return has_oob


TRAIN_PER_EXAMPLE = (1, 3, 4, 5)   # ids, dense, xin, label


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("S", [1, 2, 15, 16, 17, 27])
def test_train_slot_edges(S, D):
    """S on both sides of 16 and at both limits (F = 28 fills the kernel's LDS rows), B = 131 not
    a multiple of 4, both id widths across the set, out-of-range ids on every other case."""
    B = 131
    id64 = (S + D // 64) % 2 == 1
    oob = S in (2, 16, 27)
    inp = dev(E.train_inputs(B, S, D, id64, seed=S * 7 + D, oob=oob))
    out = run_train(inp, S, D)
    assert check_train(out, inp, S, D) == oob
    same_train(out, run_train(inp, S, D), "second run")
    same_train(out, run_train(inp, S, D, two_call=True), "nofold + fold")


@pytest.mark.parametrize("S,D", [(26, 128), (3, 64)])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 7, E.batch_for_blocks(33), E.batch_for_blocks(65)])
def test_train_batch_edges(B, S, D):
    """Batches that leave waves inactive and give the fold 1, 2, 33 and 65 chunks."""
    inp = dev(E.train_inputs(B, S, D, B % 2 == 1, seed=B + S))
    out = run_train(inp, S, D)
    assert check_train(out, inp, S, D) is False
    same_train(out, run_train(inp, S, D, two_call=True), "nofold + fold")


def test_train_refusals():
    """Arguments the launcher refuses before it launches anything: the outputs keep their fill."""
    S, D, B = 3, 64, 8
    inp = dev(E.train_inputs(B, S, D, False, seed=1))

    def refused(inp, S, D, **over):
        keep = {}
        with pytest.raises(L.RecsysError):
            run_train(inp, S, D, keep=keep, **over)
        assert all(bool(torch.isnan(o.t).all()) for o in keep.values()), f"{over}: output written"

    refused(dev(E.train_inputs(B, 28, 128, False, seed=2)), 28, 128)
    refused(dev(E.train_inputs(B, S, 32, False, seed=3)), S, 32)
    refused(inp, S, D, n_in=12)
    refused(inp, S, D, batch=0)
    refused(inp, S, D, loss_scale=0.0)
    shifted = torch.zeros(inp[0].numel() + 4, device=DEV)
    refused(inp, S, D, table=C.c_void_p(shifted.data_ptr() + 4))
    refused(inp, S, D, ws_bytes=L.lib().rs_dlrm_train_workspace_size(B) - 1)
    refused(inp, S, D, g_rows=None)
    check_train(run_train(inp, S, D), inp, S, D)


@pytest.fixture(scope="module")
def walk():
    """The walk-batch runs of the train kernel, computed once per (S, D)."""
    cache = {}

    def get(S, D, oob):
        if (S, D) not in cache:
            B = walk_batch()
            inp = dev(E.train_inputs(B, S, D, S == 27, seed=S + D, oob=oob))
            cache[(S, D)] = (inp, run_train(inp, S, D, gscale=1.0 / B))
        return cache[(S, D)]

    yield get
    cache.clear()


WALK_CASES = [(3, 64, False), (3, 128, False), (27, 128, True)]


def chunked_reference_sums(inp, S, D, gs, step=2048):
    """The batch sums and their magnitudes of a large batch, summed over slices of examples."""
    B = inp[1].shape[0]
    tot, mag, any_oob, nz = None, None, False, 0
    for w in range(0, B, step):
        sub = tuple(t[w:w + step] if i in TRAIN_PER_EXAMPLE else t for i, t in enumerate(inp))
        *_, s64, m64, nz, has_oob = E.reference(*sub, S, D, gscale=gs)
        any_oob |= has_oob
        tot = s64 if tot is None else {k: tot[k] + v for k, v in s64.items()}
        mag = m64 if mag is None else {k: mag[k] + v for k, v in m64.items()}
    return tot, mag, nz, any_oob


@pytest.mark.parametrize("S,D,oob", WALK_CASES)
def test_train_walk(walk, S, D, oob):
    """Every wave walks two or more examples and the last active wave is cut short: y, G and
    the unit rows of three windows run as batches of their own are bit-equal to the big run's,
    the windows agree with float64, the big run's sums do, and the clamped prefetch past the end
    raises no error flag."""
    inp, big = walk(S, D, oob)
    B = inp[1].shape[0]
    gs = 1.0 / B
    assert B % 4 != 0 and B > 64 * torch.cuda.get_device_properties(0).multi_processor_count
    assert bool(torch.isfinite(big["rows"]).all())
    for w in windows(B):
        sub = cut(inp, w, TRAIN_PER_EXAMPLE)
        out = run_train(sub, S, D, gscale=gs)
        assert torch.equal(out["y"], big["y"][w:w + WIN]), f"y of window {w}"
        assert torch.equal(out["G"], big["G"][w:w + WIN]), f"G of window {w}"
        assert torch.equal(out["rows"], big["rows"][w * S:(w + WIN) * S]), f"rows of window {w}"
        check_train(out, sub, S, D, gscale=gs, msg=f"window {w}")
    s64, m64, nz, has_oob = chunked_reference_sums(inp, S, D, gs)
    assert has_oob == oob and (big["err"] != 0) == oob
    check_sums(big, s64, m64, nz, D)
    check_from_y(big, inp[5], gs, "walk")


@pytest.mark.parametrize("S,D,oob", WALK_CASES)
def test_train_walk_two_calls(walk, S, D, oob):
    """_nofold followed by rs_dlrm_train_fold is the one call, bit for bit, at the walk batch."""
    inp, big = walk(S, D, oob)
    same_train(big, run_train(inp, S, D, gscale=1.0 / inp[1].shape[0], two_call=True),
               "nofold + fold")


@pytest.mark.parametrize("D", [128, 64])
def test_train_relu_gate(D):
    """dense as a relu's output: exact zeros of both signs pass no bottom gradient (the gate is
    dense > 0), down to an all-zero column whose sums are exactly 0."""
    S, B = 26, 131
    inp = dev(E.train_inputs(B, S, D, D == 64, seed=D))
    dense = inp[3]
    assert bool((dense[:, D - 3] == 0).all()) and bool((dense < 0).any())
    out = run_train(inp, S, D)
    check_train(out, inp, S, D)
    # a column of −0.0 only, and one that is zero except for one live example
    d2 = dense.clone()
    d2[:, 5] = -0.0
    d2[:, 6] = 0.0
    d2[77, 6] = 0.5
    inp2 = inp[:3] + (d2,) + inp[4:]
    out2 = run_train(inp2, S, D)
    check_train(out2, inp2, S, D)
    bot = out2["sums"][514:514 + NI * D].view(NI, D)
    assert bool((bot[:, 5] == 0).all()) and float(out2["sums"][514 + NI * D + 5]) == 0.0
    # column 6: only example 77 contributes, so A_bot[:, 6] = xin[77] * s_bot[6] exactly
    s6 = out2["sums"][514 + NI * D + 6]
    assert float(s6) != 0.0 and torch.equal(bot[:, 6], inp[4][77] * s6)


@pytest.mark.parametrize("D", [128, 64])
def test_train_clip_gate(D):
    """A head that saturates: h_b = dense[b, 0] sweeps both ends of the BCE clip. The gate is
    exactly that of Keras on the kernel's own float32 y, G inside it and the loss sum follow from
    that y, s_top and A_top are the float64 sums of G(y)·row, and the loss sum does not depend on
    loss_scale. (Measured: dropping the gate's lower end leaves G != 0 on 25 rows and fails this
    test; dropping its upper end changes no output, because the float32 sigmoid 1 / (1 + e) is
    either <= 1 − eps = 1 / (1 + ulp) or exactly 1, where y(1 − y) = 0 —
    tests/test_dlrm_edges_cpu.py::test_sweep_classes.)"""
    S = 2
    inp_cpu = E.clip_inputs(D, seed=D)
    inp = dev(inp_cpu)
    B = inp[1].shape[0]
    nz = E.nzc_of(S + 1)
    outs = {}
    for gs in (1.0 / B, 1.0):
        out = run_train(inp, S, D, gscale=gs)
        outs[gs] = out
        y = out["y"].cpu().numpy()
        cls = E.sweep_classes(y)
        assert all(int(v.sum()) >= 5 for v in cls.values()), {k: int(v.sum()) for k, v in cls.items()}
        assert out["err"] == 0
        loss, gate, Gy = check_from_y(out, inp[5], gs, f"clip scale {gs:g}")
        assert int((~gate).sum()) >= 40 and int(gate.sum()) >= 200
        # the sums of G(y)·row in float64: row = [z (pairs), dense]
        X, _ = E.gather_x(*inp[:4], S)
        iu = torch.triu_indices(S + 1, S + 1, 1, device=DEV)
        z = (X @ X.transpose(1, 2))[:, iu[0], iu[1]]
        zm = (X.abs() @ X.abs().transpose(1, 2))[:, iu[0], iu[1]]
        row = torch.cat([z, inp[3].double()], 1)
        rowm = torch.cat([zm, inp[3].double().abs()], 1)
        G64 = torch.from_numpy(Gy).to(DEV)
        s = out["sums"]
        E.close(s[512], G64.sum(), G64.abs().sum(), "s_top")
        E.close(s[:nz + D], (row * G64[:, None]).sum(0), (rowm * G64.abs()[:, None]).sum(0), "A_top")
        assert bool((s[nz + D:512] == 0).all())
        # pair weights are 0: U's table rows are 0, the bottom gradient is G·e_0 behind the gate
        assert bool((out["rows"] == 0).all())
        live = (inp[3][:, 0] > 0).double()
        E.close(s[514 + NI * D], (G64 * live).sum(), (G64.abs() * live).sum(), "s_bot[0]")
        assert bool((s[514 + NI * D + 1:] == 0).all())
    a, b = outs[1.0 / B], outs[1.0]
    assert torch.equal(a["y"], b["y"])
    assert torch.equal(a["sums"][513], b["sums"][513]), "the loss sum is unscaled"
    assert not torch.equal(a["G"], b["G"])


@pytest.mark.parametrize("id64", [False, True])
def test_train_id_edges(id64):
    """A slab of uneven cardinalities (two of them 1): ids at card − 1 read their row; card, −1,
    2^32 + 1 and the smallest int64 read a zero row and set the flag; an example with every id out
    of range; a NULL flag changes nothing else."""
    cards = [1, 7, 300, 2, 1]
    S, D, B = 5, 128, 40
    table, _, offs, dense, xin, label, q, c = E.train_inputs(B, S, D, id64, seed=11, cards=cards)
    ids, bad = E.edge_ids(B, cards, id64, seed=12)
    inp = dev((table, ids, offs, dense, xin, label, q, c))
    out = run_train(inp, S, D)
    assert check_train(out, inp, S, D) is True
    same_train(out, run_train(inp, S, D, err_flag=False), "NULL err_flag")
    # in range only: no flag
    ok_rows = torch.from_numpy(~bad.any(1)).to(DEV)
    sub = tuple(t[ok_rows].contiguous() if i in TRAIN_PER_EXAMPLE else t for i, t in enumerate(inp))
    o2 = run_train(sub, S, D, gscale=1.0 / B)
    assert o2["err"] == 0
    assert torch.equal(o2["rows"].view(-1, S, D), out["rows"].view(B, S, D)[ok_rows])
    # the example with no valid id, alone: its pairs are those of zero rows (exactly 0), its unit
    # rows are (M + Mᵀ)[s, S]·dense, the same bits as inside the batch
    last = tuple(t[B - 1:].contiguous() if i in TRAIN_PER_EXAMPLE else t for i, t in enumerate(inp))
    o1 = run_train(last, S, D, gscale=1.0 / B)
    assert o1["err"] != 0
    assert bool((o1["sums"][:E.nzc_of(S + 1)] == 0).all()), "pairs of an all-zero-row example"
    assert torch.equal(o1["rows"], out["rows"][(B - 1) * S:])
    assert torch.equal(o1["y"], out["y"][B - 1:]) and torch.equal(o1["G"], out["G"][B - 1:])
    check_train(o1, last, S, D, gscale=1.0 / B)


@pytest.mark.parametrize("id64,D", [(False, 128), (True, 64)])
def test_train_shared_table(id64, D):
    """slot_offsets = NULL: one table of n_rows rows for every slot; ids of n_rows and −1 are out
    of range."""
    S, B = 6, 131
    inp = dev(E.train_inputs(B, S, D, id64, seed=21, shared=True, oob=True))
    assert inp[2] is None
    out = run_train(inp, S, D)
    assert check_train(out, inp, S, D) is True
    clean = dev(E.train_inputs(B, S, D, id64, seed=21, shared=True))
    assert check_train(run_train(clean, S, D), clean, S, D) is False


@pytest.mark.parametrize("D", [128, 64])
def test_train_power_of_two_scaling(D):
    """U is linear in X and every step of it (the bf16 split, the MFMA sums) is exact under a
    common power-of-two scale: the unit rows of 2^±8·(table, dense) are 2^±8 times the rows."""
    S, B = 17, 131
    inp = dev(E.pow2_inputs(B, S, D, D == 64, seed=31))
    base = run_train(inp, S, D)["rows"]
    assert bool(torch.isfinite(base).all()) and bool((base != 0).any())
    for k in (8, -8):
        f = 2.0 ** k
        scaled = (inp[0] * f,) + inp[1:3] + (inp[3] * f,) + inp[4:]
        rows = run_train(scaled, S, D)["rows"]
        assert torch.equal(rows, base * f), f"scale 2^{k}"


# =============================================================================================
# B. forward + unit backward
HEAD_PER_EXAMPLE = (1, 3)


def head_inputs(B, S, id64, seed, oob):
    table, ids, offs, dense, _, _, q, c = E.train_inputs(B, S, 128, id64, seed, oob=oob)
    return dev((table, ids, offs, dense, q, torch.tensor([0.3])))


def run_head_dx(inp, S, extra, act, **over):
    """rs_dlrm_interaction_fwd_head_dx with out_stride = nzc + D + extra on guarded outputs."""
    table, ids, offs, dense, q, c = inp
    D = dense.shape[1]
    B, V = ids.shape[0], table.shape[0]
    stride = E.nzc_of(S + 1) + D + extra
    out, y = Out(B * stride, NAN), Out(B, NAN)
    ue, ud = Out(B * S * D, NAN), Out(B * D, NAN)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = dict(table=L.ptr(table), n_rows=V, D=D, ids=L.ptr(ids), id_dtype=code_of(ids), n_slots=S,
             slot_offsets=L.ptr(offs), dense=L.ptr(dense), batch=B, out=out.ptr(),
             out_stride=stride, q=L.ptr(q), c=L.ptr(c), act=act, y=y.ptr(), dxu_emb=ue.ptr(),
             dxu_dense=ud.ptr(), err_flag=L.ptr(err), stream=stream())
    a.update(over)
    outs = dict(out=out, y=y, dxu_emb=ue, dxu_dense=ud)
    try:
        L.call("rs_dlrm_interaction_fwd_head_dx", *a.values())
    finally:
        torch.cuda.synchronize()
        for k, o in outs.items():
            o.check(k)
    return dict(out=out.t.view(B, stride), y=y.t, ue=ue.t.view(B, S, D), ud=ud.t.view(B, D),
                err=int(err.item()), outs=outs)


def same_head(a, b, w, msg):
    """Two runs of different stride: the first w columns, y and both unit gradients bit-equal;
    the padding of each exactly 0."""
    for o in (a, b):
        assert bool((o["out"][:, w:] == 0).all()), f"{msg}: padding"
    assert torch.equal(a["out"][:, :w], b["out"][:, :w]), f"{msg}: row"
    for k in ("y", "ue", "ud"):
        assert torch.equal(a[k], b[k]), f"{msg}: {k}"
    assert a["err"] == b["err"]


def check_head(o, inp, S, act, msg):
    table, ids, offs, dense, q, c = inp
    D = dense.shape[1]
    z, zm, y, hm, U, Um, has_oob = E.head_dx_reference(table, ids, offs, dense, q, c, S, act)
    nz = z.shape[1]
    assert (o["err"] != 0) == has_oob
    E.close(o["out"][:, :nz], z, zm, f"{msg} pairs")
    assert torch.equal(o["out"][:, nz:nz + D], dense), f"{msg} dense part"
    # sigmoid: |dy| <= |dh| / 4 (+ its own rounding, a few ulps of y)
    E.close(o["y"], y, 0.25 * hm + 0.03 * y if act == 2 else hm, f"{msg} y")
    E.close(o["ue"], U[:, :S], Um[:, :S], f"{msg} unit emb")
    E.close(o["ud"], U[:, S], Um[:, S], f"{msg} unit dense")
    return has_oob


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("S", [1, 15, 16, 27, 28, 31])
def test_head_dx_routes(S, act):
    """out_stride − (nzc + D) of 1 and 64 take the pipelined kernel at S <= 27, 0 and 65 (and every
    stride at S >= 28) inter_fwd_mfma<DX>: the two routes agree bit for bit, both against
    float64."""
    B = 131
    id64 = (S + act) % 2 == 0
    oob = act != 1
    inp = head_inputs(B, S, id64, seed=S + act, oob=oob)
    w = E.nzc_of(S + 1) + 128
    runs = {e: run_head_dx(inp, S, e, act) for e in (0, 1, 64, 65)}
    for e, o in runs.items():
        assert check_head(o, inp, S, act, f"stride +{e}") == oob
    for e in (1, 64, 65):
        same_head(runs[0], runs[e], w, f"stride +0 vs +{e}")


def test_head_dx_walk():
    """The pipelined walk (stride + 1) against the one-example-per-wave kernel (stride + 0) on the
    same walk batch: no tolerance."""
    S, act = 27, 2
    B = walk_batch()
    inp = head_inputs(B, S, True, seed=5, oob=True)
    pipe = run_head_dx(inp, S, 1, act)
    mfma = run_head_dx(inp, S, 0, act)
    assert pipe["err"] != 0
    same_head(mfma, pipe, E.nzc_of(S + 1) + 128, "walk")
    w = windows(B)[-1]
    sub = cut(inp, w, HEAD_PER_EXAMPLE)
    alone = run_head_dx(sub, S, 1, act)
    for k in ("out", "y", "ue", "ud"):
        assert torch.equal(alone[k], pipe[k][w:w + WIN]), f"last window: {k}"
    check_head(alone, sub, S, act, "last window")
    # no live id out of range: the clamped prefetch past the end sets no flag
    clean = head_inputs(B, S, False, seed=6, oob=False)
    assert run_head_dx(clean, S, 1, act)["err"] == 0


def test_head_dx_refusals():
    B = 8
    inp = head_inputs(B, 3, False, seed=1, oob=False)

    def refused(inp, S, extra, act, **over):
        with pytest.raises(L.RecsysError):
            run_head_dx(inp, S, extra, act, **over)

    refused(head_inputs(B, 32, False, seed=2, oob=False), 32, 1, 2)
    t64 = E.train_inputs(B, 3, 64, False, seed=3)
    refused(dev((t64[0], t64[1], t64[2], t64[3], t64[6], t64[7])), 3, 1, 2)
    refused(inp, 3, 1, 2, out_stride=E.nzc_of(4) + 128 - 1)
    refused(inp, 3, 1, 3)
    check_head(run_head_dx(inp, 3, 1, 2), inp, 3, 2, "valid")


# =============================================================================================
# C. the pipelined backward
BWD_PER_EXAMPLE = (1, 3)


def bwd_inputs(B, S, id64, seed, oob, D=128):
    table, ids, offs, dense, *_ = E.train_inputs(B, S, D, id64, seed, oob=oob)
    return dev((table, ids, offs, dense))


def make_gout(B, width, pad, seed):
    """[B, width + pad] upstream gradient; the pad columns hold NaN (read, by design, never used)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, width + pad, generator=g)
    t[:, width:] = NAN
    return t.to(DEV)


def run_bwd(inp, S, compact, gout, shift=0):
    """rs_dlrm_interaction_bwd on guarded outputs; shift: grad_dense starts `shift` floats into
    its allocation (1: four bytes off the 16-byte alignment)."""
    table, ids, offs, dense = inp
    D = dense.shape[1]
    B, V = ids.shape[0], table.shape[0]
    ge, gd = Out(B * S * D, NAN), Out(B * D, NAN, lead=shift)
    try:
        L.call("rs_dlrm_interaction_bwd", L.ptr(table), V, D, L.ptr(ids), code_of(ids), S,
               L.ptr(offs), L.ptr(dense), B, 1 if compact else 0, L.ptr(gout), gout.shape[1],
               ge.ptr(), gd.ptr(), stream())
    finally:
        torch.cuda.synchronize()
        ge.check("grad_emb")
        gd.check("grad_dense")
    return ge.t.view(B, S, D), gd.t.view(B, D)


def run_rank1(inp, S, G, p):
    table, ids, offs, dense = inp
    D = dense.shape[1]
    B, V = ids.shape[0], table.shape[0]
    ge, gd = Out(B * S * D, NAN), Out(B * D, NAN)
    try:
        L.call("rs_dlrm_interaction_bwd_rank1", L.ptr(table), V, D, L.ptr(ids), code_of(ids), S,
               L.ptr(offs), L.ptr(dense), B, L.ptr(G), L.ptr(p), p.numel(), ge.ptr(), gd.ptr(),
               stream())
    finally:
        torch.cuda.synchronize()
        ge.check("grad_emb")
        gd.check("grad_dense")
    return ge.t.view(B, S, D), gd.t.view(B, D)


def check_bwd(got, inp, S, compact, gout, msg):
    ge, gd = got
    r_e, r_d, m_e, m_d = E.bwd_reference(*inp, gout, S, compact)
    assert bool(torch.isfinite(ge).all()) and bool(torch.isfinite(gd).all()), f"{msg}: not finite"
    E.close(ge, r_e, m_e, f"{msg} grad_emb")
    E.close(gd, r_d, m_d, f"{msg} grad_dense")


def rank1_operands(B, width, pad, seed):
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(B, generator=g).to(DEV)
    p = torch.randn(width + pad, generator=g)
    p[width:] = NAN
    return G, p.to(DEV)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("S", [1, 15, 16, 26, 27, 28, 31])
def test_bwd_pipe(S, compact, pad):
    """Every reachable instantiation of dlrm_bwd_pipe with a gather source — <8, 14>, <20, 14>
    (non-compact at F = 27, 28), <20, 16> (F = 29, 32) — at grad_stride = gw and gw + 3 (the
    clamped reads), with out-of-range ids (whose rows still receive their gradient) and a relu's
    dense; compact: the rank-one form is bit-equal to the backward of the materialised G ⊗ p."""
    B, F = 131, S + 1
    assert E.bwd_pipe_instance(F, 128, compact) is not None
    id64 = (S + pad) % 2 == 0
    inp = bwd_inputs(B, S, id64, seed=S + pad, oob=True)
    gw = E.grad_width(F, 128, compact)
    gout = make_gout(B, gw, pad, seed=S)
    got = run_bwd(inp, S, compact, gout)
    check_bwd(got, inp, S, compact, gout, "bwd")
    if compact:
        G, p = rank1_operands(B, gw, pad, seed=S + 50)
        mat = run_bwd(inp, S, True, (G[:, None] * p[None, :]).contiguous())
        r1 = run_rank1(inp, S, G, p)
        assert torch.equal(r1[0], mat[0]) and torch.equal(r1[1], mat[1]), "rank-one vs materialised"
        check_bwd(r1, inp, S, True, G[:, None] * p[None, :], "rank-one")


@pytest.mark.parametrize("compact", [True, False])
def test_bwd_fallbacks(compact):
    """F = 33 and a grad_dense four bytes off alignment leave the pipelined kernel for the generic
    one: same contract, same bound."""
    B = 131
    inp = bwd_inputs(B, 32, True, seed=3, oob=True)
    gout = make_gout(B, E.grad_width(33, 128, compact), 3, seed=4)
    assert E.bwd_pipe_instance(33, 128, compact) is None
    check_bwd(run_bwd(inp, 32, compact, gout), inp, 32, compact, gout, "F = 33")
    inp = bwd_inputs(B, 26, False, seed=5, oob=True)
    gout = make_gout(B, E.grad_width(27, 128, compact), 0, seed=6)
    off = run_bwd(inp, 26, compact, gout, shift=1)
    check_bwd(off, inp, 26, compact, gout, "misaligned grad_dense")
    check_bwd(run_bwd(inp, 26, compact, gout), inp, 26, compact, gout, "aligned")


@pytest.mark.parametrize("S,compact", [(3, True), (27, True), (27, False)])
def test_bwd_walk(S, compact):
    """The walk batch: per example bit-equal to three windows run alone (which agree with
    float64); compact: rank-one bit-equal to materialised there too."""
    B, F = walk_batch(), S + 1
    pad = 3 if S == 27 else 0
    inp = bwd_inputs(B, S, S == 27, seed=S, oob=True)
    gw = E.grad_width(F, 128, compact)
    if compact:
        G, p = rank1_operands(B, gw, pad, seed=S + 60)
        gout = (G[:, None] * p[None, :]).contiguous()
    else:
        gout = make_gout(B, gw, pad, seed=S + 61)
    ge, gd = run_bwd(inp, S, compact, gout)
    if compact:
        r1 = run_rank1(inp, S, G, p)
        assert torch.equal(r1[0], ge) and torch.equal(r1[1], gd), "rank-one vs materialised"
    for w in windows(B):
        sub = cut(inp, w, BWD_PER_EXAMPLE)
        gsub = gout[w:w + WIN].contiguous()
        we, wd = run_bwd(sub, S, compact, gsub)
        assert torch.equal(we, ge[w:w + WIN]), f"grad_emb of window {w}"
        assert torch.equal(wd, gd[w:w + WIN]), f"grad_dense of window {w}"
        check_bwd((we, wd), sub, S, compact, gsub, f"window {w}")
