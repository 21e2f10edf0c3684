"""The MLP-head kernels at their edges: the activation-backward column sums of csrc/dense.hip
(rs_act_bwd_colsum, _ld, _groups), csrc/batchnorm.hip, csrc/loss.hip (BCE) and csrc/metrics.hip
(AUC). Inputs, float64 restatements and bounds come from tests/head_edges.py, whose properties
tests/test_head_edges_cpu.py proves.

The C ABI is called directly (L.call) wherever the Python wrapper hides the edge: alignment, row
strides, the saved batch statistics, null pointers. Every output and workspace is prefilled
with a NaN bit pattern (SENT); a workspace is allocated with guard words behind the reported
size and passed with the reported size; guards, padding columns and the elements past an
output's end must come back untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.metrics import keras_auc
from recommender_amd import _lib as L
from recommender_amd import functional as F
from recommender_amd.metrics import AUC, auc_from_counts
from tests import head_edges as E
from tests.conftest import assert_close_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC12345  # a quiet NaN with a payload no kernel produces
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent_buf(n):
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENT)
    return t


def is_sent(t):
    return bool((t.view(torch.int32) == SENT).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stream():
    return L.stream_ptr(torch.device(DEV))


class Strided:
    """A [B, N] float matrix with row stride ld that starts `off` floats into a 16-byte aligned,
    SENT-filled buffer; everything around the matrix is padding that nobody may write."""

    def __init__(self, B, N, ld=None, off=0, data=None):
        self.shape, self.ld, self.off = (B, N), (N if ld is None else ld), off
        self.flat = sent_buf(off + B * self.ld + 8)
        assert self.flat.data_ptr() % 16 == 0
        self.mat = torch.as_strided(self.flat, (B, N), (self.ld, 1), off)
        self.imat = torch.as_strided(self.flat.view(torch.int32), (B, N), (self.ld, 1), off)
        if data is not None:
            self.mat.copy_(dev(data))

    @property
    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + 4 * self.off)

    def numpy(self):
        return self.mat.cpu().numpy()

    def padding_untouched(self):
        pad = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(pad, self.shape, (self.ld, 1), self.off).fill_(False)
        return bool((self.flat.view(torch.int32)[pad] == SENT).all())


# =============================================================================================
# 1. activation backward + column sums
def run_colsum(dy, y, act, lds=None, off=0, entry="rs_act_bwd_colsum", null_outputs=False):
    """→ (dz [B, N] or None, db [N]) as NumPy. off: every matrix starts `off` floats past a
    16-byte boundary; lds = (ld_dy, ld_y, ld_dz) (entry rs_act_bwd_colsum_ld)."""
    B, N = dy.shape
    lg, ly, lz = lds or (N, N, N)
    G = Strided(B, N, lg, off, dy)
    Y = Z = None
    if act or not null_outputs:
        Y = Strided(B, N, ly, off, y if act else np.zeros_like(dy))
        Z = Strided(B, N, lz, off)
    db = sent_buf(N + 8)
    nbytes = L.lib().rs_act_bwd_colsum_workspace_size(B, N)
    assert nbytes == E.n_chunks(B) * N * 4
    ws = sent_buf(nbytes // 4 + GUARD)
    yp, zp = (Y.ptr, Z.ptr) if Y is not None else (None, None)
    if entry == "rs_act_bwd_colsum":
        assert lds is None
        L.call(entry, G.ptr, yp, B, N, act, zp, L.ptr(db), L.ptr(ws), nbytes, stream())
    else:
        L.call(entry, G.ptr, lg, yp, ly, B, N, act, zp, lz, L.ptr(db), L.ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    assert is_sent(ws[nbytes // 4:]), "workspace guard written"
    assert is_sent(db[N:]), "db written past N"
    assert np.array_equal(bits(G.numpy()), bits(dy)) and G.padding_untouched(), "dy modified"
    if Y is not None:
        assert Y.padding_untouched() and Z.padding_untouched(), "padding columns written"
    if act == 0:
        assert Z is None or is_sent(Z.flat), "act 0 wrote dz"
        return None, db[:N].cpu().numpy()
    return Z.numpy(), db[:N].cpu().numpy()


def check_colsum_values(dy, y, act, dz, db, msg):
    B = dy.shape[0]
    if act == 1:
        want = np.where(y > 0, dy, np.float32(0))
        assert np.array_equal(bits(dz), bits(want)), f"{msg}: relu dz differs"
        assert not dz[y == 0].any(), f"{msg}: y = ±0 let a gradient through"
    elif act == 2:
        ref = E.act_bwd_f64(dy, y, 2)
        err = np.abs(dz - ref)
        assert (err <= E.SIGMOID_RTOL * np.abs(ref)).all(), \
            f"{msg}: sigmoid dz off by {float((err / np.abs(ref)).max() / E.U32):.2f} x 2^-24"
    own = dy if act == 0 else dz
    ref = own.astype(np.float64).sum(0)
    bound = E.colsum_db_bound(own, E.n_chunks(B))
    err = np.abs(db - ref)
    ratio = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0).max())
    print(f"  {msg}: db max err/bound {ratio:.3g}")
    assert (err <= bound).all(), f"{msg}: db column(s) {np.flatnonzero(err > bound)} off ({ratio:.3g})"


@pytest.mark.parametrize("N,B,act", E.COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_values_and_paths(N, B, act):
    """dz and db of one case, and the same data three ways: 16-byte aligned and contiguous (the
    float4 kernel when N % 4 == 0), from a view one float off (scalar), with strides that are no
    multiple of 4 (scalar). Both kernels give a row to the same row lane and fold in the same
    order, and the build has fp contraction off: dz and db are bit-equal across the three."""
    dy, y = E.colsum_inputs(N, B, act)
    dz, db = run_colsum(dy, y, act)
    check_colsum_values(dy, y, act, dz, db, f"colsum N {N} B {B} act {act}")
    dz1, db1 = run_colsum(dy, y, act, off=1)
    dz2, db2 = run_colsum(dy, y, act, lds=E.misaligned_lds(N), entry="rs_act_bwd_colsum_ld")
    for name, z, b in (("one float off", dz1, db1), ("ld % 4 != 0", dz2, db2)):
        assert np.array_equal(bits(db), bits(b)), f"db differs on the path '{name}'"
        if act:
            assert np.array_equal(bits(dz), bits(z)), f"dz differs on the path '{name}'"


@pytest.mark.parametrize("N,B,act", [(4, 513, 0), (64, 1025, 1), (132, 513, 2), (17, 513, 1),
                                     (1, 2048, 2)])
def test_colsum_ld_three_strides(N, B, act):
    """dy, y and dz with three different row strides (multiples of 4: the float4 kernel for the
    first three) equal the contiguous call bit for bit; act 0 accepts null y and dz."""
    dy, y = E.colsum_inputs(N, B, act)
    dz, db = run_colsum(dy, y, act)
    dz1, db1 = run_colsum(dy, y, act, lds=E.vector_lds(N), entry="rs_act_bwd_colsum_ld",
                          null_outputs=True)
    assert np.array_equal(bits(db), bits(db1))
    if act:
        assert np.array_equal(bits(dz), bits(dz1))
    else:
        _, db2 = run_colsum(dy, y, 0, null_outputs=True)
        assert np.array_equal(bits(db), bits(db2))


@pytest.mark.parametrize("widths", E.ESMM_BLOCKS, ids=str)
@pytest.mark.parametrize("act", [1, 2])
def test_colsum_ld_esmm_column_blocks(widths, act):
    """The ESMM shared-input layer: y and dz are column blocks of one [B, ΣN] buffer, db a slice
    of one [ΣN] vector, dy a contiguous [B, n] gradient per block. Each block equals the
    contiguous call bit for bit and leaves its neighbours alone."""
    B, Nt = 513, sum(widths)
    Yb, Zb = Strided(B, Nt), Strided(B, Nt)
    db = sent_buf(Nt + 8)
    done, o = [], 0
    for n in widths:
        dy, y = E.colsum_inputs(n, B, act, seed=o)
        Yb.mat[:, o:o + n] = dev(y)
        want_dz, want_db = run_colsum(dy, y, act)
        g = dev(dy)
        nbytes = L.lib().rs_act_bwd_colsum_workspace_size(B, n)
        ws = sent_buf(nbytes // 4 + GUARD)
        L.call("rs_act_bwd_colsum_ld", L.ptr(g), n, C.c_void_p(Yb.flat.data_ptr() + 4 * o), Nt, B, n,
               act, C.c_void_p(Zb.flat.data_ptr() + 4 * o), Nt, C.c_void_p(db.data_ptr() + 4 * o),
               L.ptr(ws), nbytes, stream())
        torch.cuda.synchronize()
        done.append((o, n, want_dz, want_db))
        for o2, n2, wz, wb in done:  # this block, and the earlier ones still as they were
            assert np.array_equal(bits(Zb.mat[:, o2:o2 + n2].cpu().numpy()), bits(wz))
            assert np.array_equal(bits(db[o2:o2 + n2].cpu().numpy()), bits(wb))
        o += n
        assert bool((Zb.imat[:, o:] == SENT).all()) and is_sent(db[o:]), "a later block was written"
        assert is_sent(ws[nbytes // 4:]) and Zb.padding_untouched()


GROUP_CASES = [(g, c, N, act) for g, c in E.GROUP_SHAPES for N in E.GROUP_N for act in (1, 2)]


@pytest.mark.parametrize("groups,cpg,N,act", GROUP_CASES)
def test_colsum_groups_equal_separate_calls(groups, cpg, N, act):
    """rs_act_bwd_colsum_groups on [groups·Bg, N] equals `groups` calls of rs_act_bwd_colsum on the
    row groups bit for bit: what MMOE relies on when B % 512 decides between the two."""
    Bg = cpg * E.COL_ROWS
    B = groups * Bg
    dy, y = E.colsum_inputs(N, B, act)
    G, Y, Z = Strided(B, N, data=dy), Strided(B, N, data=y), Strided(B, N)
    db = sent_buf(groups * N + 8)
    nbytes = L.lib().rs_act_bwd_colsum_workspace_size(B, N)
    ws = sent_buf(nbytes // 4 + GUARD)
    L.call("rs_act_bwd_colsum_groups", G.ptr, Y.ptr, B, N, act, groups, Z.ptr, L.ptr(db), L.ptr(ws),
           nbytes, stream())
    torch.cuda.synchronize()
    assert is_sent(ws[nbytes // 4:]) and is_sent(db[groups * N:]) and Z.padding_untouched()
    dz, dbs = Z.numpy(), db[:groups * N].cpu().numpy().reshape(groups, N)
    for g in range(groups):
        rows = slice(g * Bg, (g + 1) * Bg)
        wz, wb = run_colsum(dy[rows], y[rows], act)
        assert np.array_equal(bits(dz[rows]), bits(wz)), f"group {g}: dz differs"
        assert np.array_equal(bits(dbs[g]), bits(wb)), f"group {g}: db differs"
    check_colsum_values(dy[:Bg], y[:Bg], act, dz[:Bg], dbs[0], f"groups {groups}x{cpg} N {N}")


def test_colsum_argument_edges():
    N = 12
    db = sent_buf(N + 8)
    ws = sent_buf(GUARD)
    # B = 0: db zeroed, nothing else touched (y / dz / dy never read)
    L.call("rs_act_bwd_colsum", None, None, 0, N, 0, None, L.ptr(db), L.ptr(ws), 0, stream())
    torch.cuda.synchronize()
    assert not db[:N].view(torch.int32).any() and is_sent(db[N:]) and is_sent(ws)
    dy, y = E.colsum_inputs(N, 1024, 1)
    g, yy, z = dev(dy), dev(y), sent_buf(1024 * N)
    need = L.lib().rs_act_bwd_colsum_workspace_size(1024, N)
    wsb = sent_buf(need // 4 + GUARD)
    args = (L.ptr(g), L.ptr(yy), 1024, N, 1)
    with pytest.raises(L.RecsysError, match="workspace too small"):
        L.call("rs_act_bwd_colsum", *args, L.ptr(z), L.ptr(db), L.ptr(wsb), need - 4, stream())
    for lds in ((N - 1, N, N), (N, N - 1, N), (N, N, N - 1)):
        with pytest.raises(L.RecsysError, match="row strides"):
            L.call("rs_act_bwd_colsum_ld", L.ptr(g), lds[0], L.ptr(yy), lds[1], 1024, N, 1, L.ptr(z),
                   lds[2], L.ptr(db), L.ptr(wsb), need, stream())
    with pytest.raises(L.RecsysError):  # relu without y / dz
        L.call("rs_act_bwd_colsum", L.ptr(g), None, 1024, N, 1, None, L.ptr(db), L.ptr(wsb), need,
               stream())
    grp = lambda B, act, n: L.call("rs_act_bwd_colsum_groups", L.ptr(g), L.ptr(yy), B, N, act, n,  # noqa: E731
                                   L.ptr(z), L.ptr(db), L.ptr(wsb), need, stream())
    with pytest.raises(L.RecsysError):
        grp(1024, 0, 2)       # act 0
    with pytest.raises(L.RecsysError):
        grp(1024, 1, 3)       # B % n_groups != 0
    with pytest.raises(L.RecsysError):
        grp(1024, 1, 4)       # groups of 256 rows: not whole chunks
    with pytest.raises(L.RecsysError, match="workspace too small"):
        L.call("rs_act_bwd_colsum_groups", L.ptr(g), L.ptr(yy), 1024, N, 1, 2, L.ptr(z), L.ptr(db),
               L.ptr(wsb), need - 4, stream())
    torch.cuda.synchronize()
    assert is_sent(z) and is_sent(wsb) and is_sent(db[N:]), "a refused call wrote something"


# =============================================================================================
# 2. batch norm
def bn_ws(B, Cc):
    nbytes = L.lib().rs_batch_norm_workspace_size(B, Cc)
    assert nbytes >= 2 * -(-B // E.BN_ROWS) * Cc * 4
    return sent_buf(nbytes // 4 + GUARD), nbytes


def vec_buf(a):
    t = sent_buf(a.size + 8)
    t[:a.size] = dev(a)
    return t


def run_bn_fwd(d, momentum, training):
    B, Cc = d["x"].shape
    x, ga, be = dev(d["x"]), dev(d["gamma"]), dev(d["beta"])
    mm, mv = vec_buf(d["mm"]), vec_buf(d["mv"])
    y, sm, si = sent_buf(B * Cc + 8), sent_buf(Cc + 8), sent_buf(Cc + 8)
    ws, nbytes = bn_ws(B, Cc)
    L.call("rs_batch_norm_fwd", L.ptr(x), B, Cc, L.ptr(ga), L.ptr(be), E.BN_EPS, momentum,
           int(training), L.ptr(mm), L.ptr(mv), L.ptr(y), L.ptr(sm), L.ptr(si), L.ptr(ws), nbytes,
           stream())
    torch.cuda.synchronize()
    assert is_sent(ws[nbytes // 4:]) and is_sent(y[B * Cc:]), "workspace guard / y tail written"
    for t in (sm, si, mm, mv):
        assert is_sent(t[Cc:]), "a per-column output was written past C"
    assert torch.equal(x, dev(d["x"]))
    if not training:
        assert is_sent(ws), "inference touched the workspace"
    return dict(y=y[:B * Cc].view(B, Cc).cpu().numpy(), mean=sm[:Cc].cpu().numpy(),
                invstd=si[:Cc].cpu().numpy(), mm=mm[:Cc].cpu().numpy(), mv=mv[:Cc].cpu().numpy())


def run_bn_bwd(d, mean, invstd, training):
    B, Cc = d["x"].shape
    dx, dg, dbt = sent_buf(B * Cc + 8), sent_buf(Cc + 8), sent_buf(Cc + 8)
    ws, nbytes = bn_ws(B, Cc)
    dy, x, m, r, ga = (dev(a) for a in (d["dy"], d["x"], mean, invstd, d["gamma"]))  # kept alive
    L.call("rs_batch_norm_bwd", L.ptr(dy), L.ptr(x), B, Cc, L.ptr(m), L.ptr(r), L.ptr(ga),
           int(training), L.ptr(dx), L.ptr(dg), L.ptr(dbt), L.ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    assert torch.equal(dy, dev(d["dy"])) and torch.equal(x, dev(d["x"]))
    assert is_sent(ws[nbytes // 4:]) and is_sent(dx[B * Cc:]) and is_sent(dg[Cc:]) and is_sent(dbt[Cc:])
    return dict(dx=dx[:B * Cc].view(B, Cc).cpu().numpy(), dgamma=dg[:Cc].cpu().numpy(),
                dbeta=dbt[:Cc].cpu().numpy())


def close64(got, r64, r32, msg, extra=0.0):
    """conftest.assert_close_f64 at its defaults, the figure (max err / tol) printed first.
    extra: a per-element term added to the tolerance (only where the caller derives one)."""
    g = np.asarray(got, np.float64)
    spread = np.max([np.abs(np.asarray(s, np.float64) - r64) for s in r32], axis=0)
    tol = 1e-5 * np.abs(r64) + 4.0 * spread + 1e-7 * np.abs(r64).max() + extra
    err = np.abs(g - r64)
    print(f"  {msg}: max err/tol {float((err / np.maximum(tol, 1e-300)).max()):.3g}")
    assert g.shape == r64.shape and np.isfinite(g).all(), msg
    if np.any(extra):
        assert (err <= tol).all(), f"{msg}: {int((err > tol).sum())} / {err.size} elements off"
    else:
        assert_close_f64(got, r64, list(r32), msg)


@pytest.mark.parametrize("C_,B", E.BN_CASES)
def test_batch_norm_training(C_, B):
    """rs_batch_norm_fwd (training) at momentum 0.99 and 0: y, the saved mean and invstd, the
    moving statistics after Keras' update, against float64 on the same fp32 inputs, with the
    eager fallback on two row orders as the fp32 samples. Then the structured columns."""
    d = E.bn_inputs(C_, B)
    for momentum in (0.99, 0.0):
        if momentum == 0.0 and C_ >= 4:
            # mv - (mv - var)·1 rounds at mv's ulp; from 0 the update returns the batch value
            d = dict(d, mm=d["mm"].copy(), mv=d["mv"].copy())
            d["mm"][E.COL_BIG] = d["mv"][E.COL_BIG] = 0.0
        got = run_bn_fwd(d, momentum, True)
        r = E.bn_fwd_f64(d["x"], d["gamma"], d["beta"], d["mm"], d["mv"], momentum, True)
        s = E.bn_eager_samples(d, momentum, True)
        tag = f"bn C {C_} B {B} momentum {momentum}"
        for k in ("mean", "invstd", "mm", "mv"):
            close64(got[k], r[k], [t[k] for t in s], f"{tag} {k}")
        # y is computed from the saved mean, a float: off by up to an ulp of the mean whatever the
        # algorithm, which moves y by ulp32(mean)·invstd·|gamma|. Intrinsic to the interface.
        intrinsic = E.ulp32(r["mean"]) * r["invstd"] * np.abs(d["gamma"].astype(np.float64))
        close64(got["y"], r["y"], [t["y"] for t in s], f"{tag} y", extra=intrinsic[None, :])
        if C_ < 4:
            continue
        eps = float(np.float32(E.BN_EPS))
        # constant column: mean exact, variance exactly 0, invstd = rsqrt(eps), y = beta
        c = E.COL_CONST
        assert got["mean"][c] == 2.5
        assert abs(got["invstd"][c] - eps ** -0.5) <= 2 * E.U32 * eps ** -0.5
        assert np.array_equal(bits(got["y"][:, c]), bits(np.full(B, d["beta"][c])))
        # 1000 + 0.01·N(0,1): the batch variance back from save_invstd, and at momentum 0 from
        # the moving variance, within 1e-5 relative of float64 plus the fp32 samples' spread
        c = E.COL_BIG
        v64 = r["var"][c]
        spread = max(abs(float(t["var"][c]) - v64) for t in s)
        bound = 1e-5 * v64 + spread
        # var + eps = invstd^-2: invstd's own rounding (2^-24 relative, rsqrtf 1 ulp) comes back
        # as 2·2·2^-24·(var + eps) and is part of what save_invstd can say about var
        v_inv = float(got["invstd"][c]) ** -2.0 - eps
        inv_bound = bound + 4 * E.U32 * (v64 + eps)
        print(f"  {tag} big column: var {v64:.6g}, from invstd {v_inv:.6g} "
              f"(err/bound {abs(v_inv - v64) / inv_bound:.3g})")
        assert abs(v_inv - v64) <= inv_bound
        if momentum == 0.0:
            print(f"  {tag} big column: moving var {got['mv'][c]:.6g} "
                  f"(err/bound {abs(got['mv'][c] - v64) / bound:.3g})")
            assert abs(float(got["mv"][c]) - v64) <= bound
            assert abs(float(got["mm"][c]) - r["mean"][c]) <= E.ulp32(r["mean"][c])


@pytest.mark.parametrize("C_,B", E.BN_CASES)
def test_batch_norm_inference_and_backward(C_, B):
    """Inference: y from the moving statistics, which stay bit-unchanged (momentum 0 and 0.99).
    rs_batch_norm_bwd as a function of its own inputs (the saved statistics of the training
    forward), training and inference, against float64 with two fp32 row orders as samples."""
    d = E.bn_inputs(C_, B)
    for momentum in (0.99, 0.0):
        got = run_bn_fwd(d, momentum, False)
        r = E.bn_fwd_f64(d["x"], d["gamma"], d["beta"], d["mm"], d["mv"], momentum, False)
        s = E.bn_eager_samples(d, momentum, False)
        assert np.array_equal(bits(got["mm"]), bits(d["mm"])) and np.array_equal(bits(got["mv"]), bits(d["mv"]))
        assert np.array_equal(bits(got["mean"]), bits(d["mm"]))
        close64(got["invstd"], r["invstd"], [t["invstd"] for t in s], f"bn inference C {C_} B {B} invstd")
        close64(got["y"], r["y"], [t["y"] for t in s], f"bn inference C {C_} B {B} y")
    fwd = run_bn_fwd(d, 0.99, True)
    perm = np.random.default_rng(B).permutation(B)
    for training in (True, False):
        got = run_bn_bwd(d, fwd["mean"], fwd["invstd"], training)
        args = (d["dy"], d["x"], fwd["mean"], fwd["invstd"], d["gamma"], training)
        r = E.bn_bwd(*args)
        s = [E.bn_bwd(*args, np.float32), E.bn_bwd(*args, np.float32, perm)]
        for k in ("dx", "dgamma", "dbeta"):
            close64(got[k], r[k], [t[k] for t in s], f"bn bwd C {C_} B {B} training {training} {k}")
        if not training:  # dx = gamma·r·dy: two fp32 products
            want = (d["gamma"] * fwd["invstd"]) * d["dy"]
            assert np.array_equal(bits(got["dx"]), bits(want))


def test_batch_norm_argument_edges():
    d = E.bn_inputs(4, 65)
    x = dev(d["x"])
    v = [sent_buf(16) for _ in range(6)]
    y = sent_buf(65 * 4)
    ws, nbytes = bn_ws(65, 4)

    def fwd(B, Cc, training, nb):
        L.call("rs_batch_norm_fwd", L.ptr(x), B, Cc, L.ptr(v[0]), L.ptr(v[1]), E.BN_EPS, 0.99, training,
               L.ptr(v[2]), L.ptr(v[3]), L.ptr(y), L.ptr(v[4]), L.ptr(v[5]), L.ptr(ws), nb, stream())

    def bwd(B, Cc, nb):
        L.call("rs_batch_norm_bwd", L.ptr(x), L.ptr(x), B, Cc, L.ptr(v[0]), L.ptr(v[1]), L.ptr(v[2]), 1,
               L.ptr(y), L.ptr(v[4]), L.ptr(v[5]), L.ptr(ws), nb, stream())

    for B, Cc in ((0, 4), (65, 0)):
        with pytest.raises(L.RecsysError):
            fwd(B, Cc, 1, nbytes)
        with pytest.raises(L.RecsysError):
            bwd(B, Cc, nbytes)
    with pytest.raises(L.RecsysError, match="workspace too small"):
        fwd(65, 4, 1, nbytes - 4)
    with pytest.raises(L.RecsysError, match="workspace too small"):
        bwd(65, 4, nbytes - 4)
    torch.cuda.synchronize()
    assert is_sent(y) and is_sent(ws) and all(is_sent(t) for t in v)


# =============================================================================================
# 3. BCE
RED = {"none": 0, "sum": 1, "mean": 2}


def run_bce_fwd(p, y, red):
    n = p.size
    out = sent_buf((n if red == 0 else 1) + 8)
    nbytes = L.lib().rs_bce_workspace_size(n)
    ws = sent_buf(nbytes // 4 + GUARD)
    pt, yt = dev(p), dev(y)  # kept alive over the call
    L.call("rs_bce_fwd", L.ptr(pt), L.ptr(yt), n, float(E.BCE_EPS), red, L.ptr(out), L.ptr(ws),
           nbytes, stream())
    torch.cuda.synchronize()
    k = n if red == 0 else 1
    assert is_sent(out[k:]) and is_sent(ws[nbytes // 4:]), "output tail / workspace guard written"
    return out[:k].cpu().numpy()


def run_bce_bwd(p, y, red, g):
    n = p.size
    dp = sent_buf(n + 8)
    pt, yt, gt = dev(p), dev(y), dev(g)  # kept alive over the call
    L.call("rs_bce_bwd", L.ptr(pt), L.ptr(yt), n, float(E.BCE_EPS), red, L.ptr(gt), L.ptr(dp),
           stream())
    torch.cuda.synchronize()
    assert is_sent(dp[n:]), "grad_p written past n"
    return dp[:n].cpu().numpy()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", E.BCE_N)
def test_bce_forward(n, soft):
    """Per example and both reduced forms against float64: 1e-5·|ref| + 2^-22 per element; the
    sums add depth·2^-24·Σ|l_i|, depth = a thread's passes + 8 tree levels + the block count."""
    p, y, _, _ = E.bce_inputs(n, soft)
    l64 = E.bce_f64(p, y)
    none = run_bce_fwd(p, y, 0)
    assert none.shape == (n,) and (np.abs(none - l64) <= E.bce_elem_tol(l64)).all()
    s, m = run_bce_fwd(p, y, 1)[0], run_bce_fwd(p, y, 2)[0]
    if n == 0:
        assert s == 0 and m == 0
        return
    tol = E.bce_sum_tol(l64)
    print(f"  bce n {n}: sum err/tol {abs(s - l64.sum()) / tol:.3g}, "
          f"mean err/tol {abs(m - l64.mean()) / (tol / n):.3g}")
    assert abs(s - l64.sum()) <= tol
    assert abs(m - l64.mean()) <= tol / n


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", E.BCE_N)
def test_bce_backward(n, soft):
    """grad_out random per element ('none') and the scalars 0.37 and -2.5 ('sum', 'mean'),
    against float64, judged on the size of the two terms (they cancel for soft labels); exactly
    0 outside [eps, 1 - eps], non-zero at both inclusive ends."""
    p, y, g, pos = E.bce_inputs(n, soft)
    d64, mag = E.bce_grad_f64(p, y)
    inside = (p >= E.BCE_EPS) & (p <= E.BCE_HI)
    runs = [(0, g, g.astype(np.float64))]
    for gs in (0.37, -2.5):
        gv = np.array([gs, 7.0, 7.0], np.float32)  # only grad_out[0] counts
        runs += [(1, gv, float(gv[0])), (2, gv, float(gv[0]) / max(n, 1))]
    for red, gout, geff in runs:
        dp = run_bce_bwd(p, y, red, gout)
        err = np.abs(dp - geff * d64)
        assert (err <= E.BCE_RTOL * np.abs(geff) * mag).all(), (red, float(gout[0]) if n else None)
        assert not dp[~inside].any(), "gradient outside the clip"
        if len(pos) >= 5:
            assert dp[pos[2]] != 0 and dp[pos[4]] != 0, "no gradient at an inclusive end"


def test_bce_planted_values_under_every_label():
    pl = E.bce_planted()
    p = np.tile(pl, 3)
    y = np.repeat(np.array([0.0, 1.0, 0.3], np.float32), len(pl))
    l64 = E.bce_f64(p, y)
    assert (np.abs(run_bce_fwd(p, y, 0) - l64) <= E.bce_elem_tol(l64)).all()
    g = np.linspace(-2, 3, p.size).astype(np.float32)
    d64, mag = E.bce_grad_f64(p, y)
    dp = run_bce_bwd(p, y, 0, g)
    assert (np.abs(dp - g * d64) <= E.BCE_RTOL * np.abs(g) * mag).all()
    inside = np.tile([False, False, True, False, True, False, True, False, False], 3)
    assert not dp[~inside].any() and dp[inside].all()


def test_bce_nan_prediction_is_nan():
    """A NaN prediction gives a NaN loss for that example, NaN reduced losses and a NaN gradient
    there (oracle.ctr.bce / bce_grad, the reference's ops): a diverged model must not report a
    finite loss. Every other element is as without the NaN."""
    n = 1025
    p, y, g, _ = E.bce_inputs(n, True)
    nan_at = [0, 300, 1024]
    p[nan_at] = np.nan
    ok = ~np.isnan(p)
    l64 = E.bce_f64(p, y)
    none = run_bce_fwd(p, y, 0)
    assert np.isnan(none[nan_at]).all() and (np.abs(none[ok] - l64[ok]) <= E.bce_elem_tol(l64[ok])).all()
    assert np.isnan(run_bce_fwd(p, y, 1)[0]) and np.isnan(run_bce_fwd(p, y, 2)[0])
    d64, mag = E.bce_grad_f64(p, y)
    for red, gout, geff in ((0, g, g.astype(np.float64)), (1, g[:1], float(g[0])), (2, g[:1], float(g[0]) / n)):
        dp = run_bce_bwd(p, y, red, gout)
        assert np.isnan(dp[nan_at]).all()
        scale = (geff[ok] if red == 0 else geff)
        assert (np.abs(dp[ok] - scale * d64[ok]) <= E.BCE_RTOL * np.abs(scale) * mag[ok]).all()
    # and through the layer: loss and gradient of the model's head
    pt = dev(p).requires_grad_()
    loss = F.binary_crossentropy(dev(y), pt, "mean")
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(pt.grad[nan_at]).all() and torch.isfinite(pt.grad[dev(ok)]).all()


# =============================================================================================
# 4. AUC
def counts_of(m):
    return m.counts.cpu().numpy()


@pytest.mark.parametrize("T", E.AUC_T)
def test_auc_on_threshold_predictions(T):
    """Every interior threshold, its float32 neighbours, 0, -0.0 and 1, labels cycling through
    {0, 1, 0.5, -1, 2}: the bucket counts equal the literal `p > t_i` counts of the oracle
    (cumulated back to buckets), result() its trapezoid."""
    p, y, neg, pos, roc = E.auc_reference(T)
    m = AUC(num_thresholds=T)
    h = p.size // 3
    for a, b in ((0, h), (h, p.size)):
        m.update_state(dev(y[a:b]), dev(p[a:b]))
    c = counts_of(m)
    assert np.array_equal(c[0], neg) and np.array_equal(c[1], pos)
    assert abs(m.result() - roc) < 1e-12
    if T <= 200:  # the oracle itself (the T x n matrix fits)
        ref, tp, fp = keras_auc(y, p, T)
        assert np.array_equal(np.cumsum(c[1][::-1])[::-1][1:], tp.astype(np.int64))
        assert np.array_equal(np.cumsum(c[0][::-1])[::-1][1:], fp.astype(np.int64))
        assert abs(m.result() - ref) < 1e-12


@pytest.mark.parametrize("preset", [2 ** 24 - 1, 2 ** 32 - 3])
def test_auc_counters_are_64_bit(preset):
    """A bucket preset just under 2^24 (float32's integers) and 2^32 (a 32-bit word) takes ten more
    hits exactly, for a positive and a negative bucket."""
    T = 200
    m = AUC(num_thresholds=T)
    thr = E.keras_thresholds(T)
    pn, pp = np.float32(0.25), np.float32(0.75)
    bn_, bp = int((thr < pn).sum()), int((thr < pp).sum())
    m.counts[0, bn_] = preset
    m.counts[1, bp] = preset
    before = counts_of(m).copy()
    m.update_state(dev(np.array([0, 1] * 10, np.float32)), dev(np.array([pn, pp] * 10, np.float32)))
    want = before.copy()
    want[0, bn_] += 10
    want[1, bp] += 10
    assert np.array_equal(counts_of(m), want) and want[0, bn_] == preset + 10


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_auc_sizes(n):
    """One block minus one, one block, one block plus one; n = 0 leaves everything untouched."""
    T = 200
    p, y, *_ = E.auc_reference(T)
    p, y = p[:n], y[:n]
    m = AUC(num_thresholds=T)
    m.counts.copy_(torch.arange(2 * (T + 1), device=DEV).view(2, T + 1))
    m.err_flag.fill_(0)
    before = counts_of(m).copy()
    m.update_state(dev(y), dev(p))
    thr = E.keras_thresholds(T)
    tp, fp = E.literal_tp_fp(p, y, thr)
    add = np.stack([E.buckets_from_cumulative(fp, int((y == 0).sum())),
                    E.buckets_from_cumulative(tp, int((y != 0).sum()))])
    assert np.array_equal(counts_of(m), before + add) and add.sum() == n
    assert int(m.err_flag.item()) == 0


@pytest.mark.parametrize("bad", [np.nan, -1e-8, float(np.nextafter(np.float32(1), np.float32(2)))])
def test_auc_out_of_range_raises(bad):
    m = AUC()
    m.update_state(dev(np.array([1, 0, 1], np.float32)), dev(np.array([0.2, bad, 1.0], np.float32)))
    with pytest.raises(ValueError):
        m.result()
    ok = AUC()
    ok.update_state(dev(np.array([1, 0, 1], np.float32)), dev(np.array([0.0, -0.0, 1.0], np.float32)))
    ok.result()


def test_auc_null_err_flag():
    """The C ABI with a null err_flag: 1.5 and -1 are counted in buckets T and 0, no error."""
    T = 3
    thr = dev(E.keras_thresholds(T))
    counts = torch.zeros(2 * (T + 1) + 8, dtype=torch.int64, device=DEV)
    counts[2 * (T + 1):] = -7
    p, y = dev(np.array([1.5, -1.0, 0.75], np.float32)), dev(np.array([1, 0, 2], np.float32))
    L.call("rs_auc_update", L.ptr(p), L.ptr(y), 3, L.ptr(thr), T, L.ptr(counts), None, stream())
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert (c[2 * (T + 1):] == -7).all()
    assert c[:2 * (T + 1)].reshape(2, T + 1).tolist() == [[1, 0, 0, 0], [0, 0, 1, 1]]
    with pytest.raises(L.RecsysError):
        L.call("rs_auc_update", L.ptr(p), L.ptr(y), 3, L.ptr(thr), 1, L.ptr(counts), None, stream())


@pytest.mark.parametrize("curve,method", [("ROC", "minoring"), ("ROC", "majoring"),
                                          ("PR", "interpolation"), ("PR", "minoring"),
                                          ("PR", "majoring")])
def test_auc_summation_methods_on_ties(curve, method):
    """ROC minoring / majoring, PR interpolation and the PR Riemann sums on a tie-heavy input:
    result() equals auc_from_counts fed the oracle's literal counts."""
    T = 200
    p, y = E.tie_heavy(T)
    m = AUC(num_thresholds=T, curve=curve, summation_method=method)
    m.update_state(dev(y), dev(p))
    _, tp, fp = keras_auc(y, p, T)
    pos = E.buckets_from_cumulative(tp.astype(np.int64), int((y != 0).sum()))
    neg = E.buckets_from_cumulative(fp.astype(np.int64), int((y == 0).sum()))
    c = counts_of(m)
    assert np.array_equal(c[0], neg) and np.array_equal(c[1], pos)
    want = auc_from_counts(neg, pos, curve, method)
    assert abs(m.result() - want) < 1e-12 and 0 < want < 1
    if curve == "ROC":  # minoring <= trapezoid <= majoring, strictly apart on ties
        mid = auc_from_counts(neg, pos, "ROC", "interpolation")
        assert (want < mid) if method == "minoring" else (want > mid)
