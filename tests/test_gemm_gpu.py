"""rs_gemm_x3 (csrc/gemm.hip: fp32 GEMM on the bf16 matrix cores, each operand split into three
bf16 parts, six part products) against a float64 torch evaluation of the same product. Bound per
element: |got - ref| <= 4e-6 · Σ_k |a_mk||b_kn| (+ the same for the bias), i.e. ≈64 fp32 ulps of the
term magnitude — an fp32 fma chain of these lengths errs by far less than its worst case K·u; the
library fp32 GEMM (hipBLASLt) is held to the same bound on the same inputs as a control. All four
operand layouts (the Dense layer's forward ta 0 tb 0, dgrad ta 0 tb 1, wgrad ta 1 tb 0, and ta 1
tb 1), edge tiles (M, N, K not multiples of the 128 / 32 tiles), batches with strides, the
split-K fold, bias and relu / sigmoid epilogues."""
import ctypes

import pytest
import torch

from recommender_amd import _lib as L
from tests import x3_model as X
from tests.dlrm_edges import GUARD, GUARD_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _op(t, trans):
    return t.transpose(-1, -2) if trans else t


def _run(A, B, M, N, K, ta, tb, batch, bias, act, splits):
    C = torch.full((batch, M, N), float("nan"), device=DEV)
    ws_n = L.lib().rs_gemm_x3_workspace_size(M, N, batch, splits)
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device=DEV)
    lda = A.shape[-1]
    ldb = B.shape[-1]
    L.call("rs_gemm_x3", ta, tb, M, N, K, L.ptr(A), lda, A[0].numel(), L.ptr(B), ldb,
           B[0].numel(), L.ptr(C), N, M * N, batch, L.ptr(bias),
           0 if bias is None else bias.shape[-1], act, splits, L.ptr(ws), ws.numel(),
           L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return C


def _act(x, act):
    return torch.relu(x) if act == 1 else (torch.sigmoid(x) if act == 2 else x)


@pytest.mark.parametrize("M,N,K,ta,tb,batch,splits,act", [
    (4096, 360, 324, 0, 0, 1, 1, 1),      # ESMM tower layer 1 forward (relu)
    (4096, 324, 360, 0, 1, 1, 1, 0),      # its dgrad
    (324, 360, 8192, 1, 0, 1, 16, 0),     # its wgrad, split-K
    (1000, 200, 1604, 0, 0, 3, 1, 2),     # batched, edge tiles, sigmoid
    (132, 76, 36, 1, 1, 2, 1, 0),
    (260, 80, 4100, 1, 0, 2, 7, 1),       # batched split-K with a ragged last split
    (8, 4, 4, 0, 0, 1, 1, 0),
])
def test_gemm_x3_vs_float64(M, N, K, ta, tb, batch, splits, act):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a_shape = (batch, K, M) if ta else (batch, M, K)
    b_shape = (batch, N, K) if tb else (batch, K, N)
    A = torch.randn(*a_shape, device=DEV, generator=g)
    B = torch.randn(*b_shape, device=DEV, generator=g) * 0.1
    bias = torch.randn(batch, N, device=DEV, generator=g)
    C = _run(A, B, M, N, K, ta, tb, batch, bias, act, splits)
    a64, b64 = _op(A, ta).double(), _op(B, tb).double()
    z64 = a64 @ b64 + bias.double()[:, None, :]
    mag = a64.abs() @ b64.abs() + bias.double().abs()[:, None, :]
    ref = _act(z64, act)
    # the activations' slopes are <= 1: the pre-activation bound carries over
    tol = 4e-6 * mag + 1e-30
    err = (C.double() - ref).abs()
    assert torch.isfinite(C).all()
    assert bool((err <= tol).all()), f"max err/tol {float((err / tol).max()):.3g}"
    # control: the library fp32 GEMM on the same inputs meets the same bound
    z32 = torch.baddbmm(bias[:, None, :], _op(A, ta), _op(B, tb))
    assert bool(((_act(z32, act).double() - ref).abs() <= tol).all())


def test_gemm_x3_rejects_unaligned_shapes():
    A = torch.zeros(1, 6, 6, device=DEV)
    with pytest.raises(L.RecsysError):
        _run(A, A, 6, 6, 6, 0, 0, 1, None, 0, 1)


# =============================================================================================
# The accuracy claim and the addressing, on inputs where a missing or misplaced part product
# shows (tests/x3_model.py; the bounds are proved against the CPU model and its mutants in
# tests/test_x3_model_cpu.py). Every call below runs with leading dimensions and batch strides
# larger than the natural ones, NaN in the operands' padding, and C inside a buffer of a fixed
# NaN bit pattern: between C's rows, between the batches and 64 elements behind it, compared as
# int32 after the call.
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _place(op, trans, ld_pad, gap):
    """op(X) [batch, R, C] on the CPU → (device buffer, ld, batch stride) of X as stored (the
    transpose when trans), rows ld_pad apart more than their width, batches `gap` further, the
    padding NaN."""
    st = op.transpose(1, 2) if trans else op
    b, r, c = st.shape
    ld = c + ld_pad
    stride = r * ld + gap
    buf = torch.full((max(b * stride, 4),), float("nan"))
    torch.as_strided(buf, (b, r, c), (stride, ld, 1)).copy_(st)
    return buf.to(DEV), ld, stride


class Call:
    """One rs_gemm_x3 call on op(A) [batch, M, K], op(B) [batch, K, N] (CPU tensors)."""

    def __init__(self, opA, opB, ta, tb, bias=None, act=0, splits=1, pads=(4, 8, 3), gaps=(12, 4, 7)):
        if opA.dim() == 2:
            opA, opB = opA[None], opB[None]
        self.batch, self.M, self.K = opA.shape
        self.N = opB.shape[2]
        self.ta, self.tb, self.act, self.splits = ta, tb, act, splits
        self.A, self.lda, self.sA = _place(opA, ta, pads[0], gaps[0])
        self.B, self.ldb, self.sB = _place(opB, tb, pads[1], gaps[1])
        self.ldc = self.N + pads[2]
        self.sC = self.M * self.ldc + gaps[2]
        self.cbuf = torch.full((self.batch * self.sC + GUARD,), GUARD_BITS, dtype=torch.int32,
                               device=DEV)
        self.bias = None if bias is None else bias.to(DEV).contiguous()
        self.sbias = 0 if bias is None or bias.dim() == 1 else bias.shape[-1]
        ws_n = L.lib().rs_gemm_x3_workspace_size(self.M, self.N, self.batch, splits)
        self.ws = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=DEV)
        self.ws_n = ws_n
        self.args = dict(ta=ta, tb=tb, M=self.M, N=self.N, K=self.K, A=L.ptr(self.A), lda=self.lda,
                         sA=self.sA, B=L.ptr(self.B), ldb=self.ldb, sB=self.sB,
                         C=L.ptr(self.cbuf), ldc=self.ldc, sC=self.sC, batch=self.batch,
                         bias=L.ptr(self.bias), sbias=self.sbias, act=act, splits=splits,
                         ws=L.ptr(self.ws), ws_n=ws_n)

    def run(self, **over):
        a = dict(self.args, **over)
        L.call("rs_gemm_x3", *[a[k] for k in ("ta", "tb", "M", "N", "K", "A", "lda", "sA", "B",
                                              "ldb", "sB", "C", "ldc", "sC", "batch", "bias",
                                              "sbias", "act", "splits", "ws", "ws_n")],
               L.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        return self

    def c_bits(self):
        """C [batch, M, N] as int32 on the CPU, after checking every element around it."""
        view = (self.batch, self.M, self.N), (self.sC, self.ldc, 1)
        around = torch.ones(self.cbuf.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(around, *view).fill_(False)
        assert int(around.sum()) >= GUARD
        assert bool((self.cbuf[around] == GUARD_BITS).all()), "written outside C"
        return torch.as_strided(self.cbuf, *view).contiguous().cpu()

    def c(self):
        return self.c_bits().view(torch.float32)

    def untouched(self):
        return bool((self.cbuf == GUARD_BITS).all())


def _bits(t):
    """fp32 → int32 bits with −0 folded into +0 (a sum of zeros from a zero accumulator has no
    sign to keep)."""
    return (t.float() + 0.0).contiguous().view(torch.int32)


def _same_bits(got, want, msg):
    g, w = _bits(got), _bits(want)
    bad = g != w
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())} / {bad.numel()} elements differ"


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3, 9])
@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_generalised_permutation_is_bit_exact(ta, tb, side, splits):
    """One operand has a single 0 / ±1 / ±2^k entry per dot product, the other is full-mantissa
    randn: C is the selected, scaled rows (columns) of that operand bit for bit. M, N, K off the
    128 / 32 tiles; batch 2 (a random selection and a cyclic one, which carries every element 37
    places: across K-steps and 64-row quadrants); split-K 3 (K = 100: 64 + a ragged 36) and 9
    (more than the four K-steps: partials of exact zeros plus one term)."""
    M, N, K = 132, 260, 100
    g = torch.Generator().manual_seed(17 + splits)
    opA, opB, want = [], [], []
    for shift in (None, 37):
        if side == "A":
            idx, sc = X.gen_perm(M, 3, shift, k=K)
            a = torch.zeros(M, K)
            a[torch.arange(M), idx] = sc
            b = torch.randn(K, N, generator=g)
            want.append(sc[:, None] * b[idx])
        else:
            idx, sc = X.gen_perm(N, 4, shift, k=K)
            b = torch.zeros(K, N)
            b[idx, torch.arange(N)] = sc
            a = torch.randn(M, K, generator=g)
            want.append(a[:, idx] * sc[None, :])
        opA.append(a)
        opB.append(b)
    call = Call(torch.stack(opA), torch.stack(opB), ta, tb, splits=splits).run()
    _same_bits(call.c(), torch.stack(want), "C")


@pytest.mark.parametrize("rot", range(6))
@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_part_product_probes_are_exact(ta, tb, side, rot):
    """One term per dot product, the term a probe pair of one of the six part products: the true
    product is an fp32 number and needs that part product. Over rot every product type sits at
    every k of a K-step (every lane group and element of the bf8 fragments); M = N = 132 covers
    every 16x16 tile of a wave's 4x4 and an edge tile."""
    opA, opB = X.one_term_case("probe", side, 5, rot=rot)
    want = opA.double() @ opB.double()
    assert bool((want.float().double() == want).all())
    call = Call(opA, opB, ta, tb).run()
    _same_bits(call.c(), want.float(), f"probes rot {rot}")


def _few_term(kind, rel, ta, tb, side, seed):
    opA, opB = X.one_term_case(kind, side, seed)
    ref = opA.double() @ opB.double()
    got = Call(opA, opB, ta, tb).run().c()[0]
    worst = X.max_rel(got, ref, ref.abs())
    print(f"rs_gemm_x3 {kind} ta {ta} tb {tb} side {side}: max err/|a·b| {worst / X.U:.3f} U "
          f"(bound {rel / X.U:g} U)")
    assert bool(torch.isfinite(got).all())
    assert bool(((got.double() - ref).abs() <= rel * ref.abs()).all()), f"{worst / X.U:.3f} U"


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_one_term_precision(ta, tb, side):
    """Full-mantissa random pairs, one per dot product: |got − a·b| <= REL_FEW |a·b|. The clean
    scheme errs by 1.1 U here, a single missing 2^-16-class product by 120 U or more
    (tests/test_x3_model_cpu.py). Measured on the MI355X: 2.23 U in every layout
    (the bf16 MFMA's adder does not round to nearest)."""
    _few_term("few", X.REL_FEW, ta, tb, side, 1)


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_split_rounds_to_nearest(ta, tb, side):
    """Pairs whose low mantissa bits are ones and whose product is all but an fp32 number: exact
    to 2^-30 with the rounding split, 5.9 U off with a truncating one; bound REL_TRUNC = 2.9 U
    (on the MI355X the rounding split measures 1 ulp = 1.97 U: the MFMA's own adder)."""
    _few_term("trunc", X.REL_TRUNC, ta, tb, side, 2)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_dense_small_k(ta, tb):
    """Dense randn at K = 100, where a missing product is not yet averaged away: bound REL_DENSE ·
    Σ|terms|. CPU model: clean 7.2e-8, the weakest single-drop mutant 1.66e-6; measured on the
    MI355X: the kernel 6.45e-8, the library 2.34e-7 (rel must be >= 4x the kernel's and <= half
    the mutant's). The
    library fp32 GEMM is held to the same bound as the control."""
    opA, opB = X.dense_operands()
    ref = opA.double() @ opB.double()
    mag = opA.double().abs() @ opB.double().abs()
    got = Call(opA, opB, ta, tb).run().c()[0]
    worst = X.max_rel(got, ref, mag)
    lib = (opA.to(DEV) @ opB.to(DEV)).cpu()
    print(f"rs_gemm_x3 dense K=100 ta {ta} tb {tb}: max err/mag {worst:.3g}, library "
          f"{X.max_rel(lib, ref, mag):.3g} (bound {X.REL_DENSE:g})")
    assert bool(((got.double() - ref).abs() <= X.REL_DENSE * mag).all()), worst
    assert bool(((lib.double() - ref).abs() <= X.REL_DENSE * mag).all())


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x3_integer_data_is_exact(ta, tb, splits):
    """Integer operands |v| <= 255, dense in K = 200 (every sum below 2^24): C is the integer
    product exactly, whatever the order — any k dropped or counted twice, any seam error shows."""
    ops = [X.int_operands(260, 200, 132, 20 + i) for i in range(2)]
    opA = torch.stack([o[0] for o in ops])
    opB = torch.stack([o[1] for o in ops])
    want = opA.double() @ opB.double()
    assert float(want.abs().max()) < 2 ** 24
    got = Call(opA, opB, ta, tb, splits=splits).run().c()
    assert bool((got.double() == want).all()), int((got.double() != want).sum())


# ---------------------------------------------------------------------------------------------
def _act64(x, act):
    return torch.relu(x) if act == 1 else (torch.sigmoid(x) if act == 2 else x)


def _close_act(got, z64, act):
    """act(z) for an exact pre-activation z: bit-equal for none / relu; the fp32 sigmoid
    1 / (1 + expf(−z)) is within 16 U of the result (expf 2 ulp, the sum and the quotient 1 ulp
    each, with room)."""
    want = _act64(z64, act)
    if act == 2:
        assert bool(((got.double() - want).abs() <= 16 * X.U * want + 1e-37).all())
    else:
        assert bool((got.double() == want).all())


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_bias", [False, True])
def test_gemm_x3_k_zero_gives_the_activated_bias(with_bias, act):
    M, N, batch = 8, 132, 2
    bias = torch.arange(-N, N, dtype=torch.float32).view(batch, N) / 8 if with_bias else None
    for splits in (1, 4):
        call = Call(torch.zeros(batch, M, 0), torch.zeros(batch, 0, N), 0, 0, bias=bias, act=act,
                    splits=splits).run()
        z = torch.zeros(batch, M, N, dtype=torch.float64)
        if with_bias:
            z += bias.double()[:, None, :]
        _close_act(call.c(), z, act)


def test_gemm_x3_empty_m_or_n_writes_nothing():
    for M, N in ((0, 8), (8, 0), (0, 0)):
        call = Call(torch.ones(1, M, 8), torch.ones(1, 8, N), 0, 0)
        call.run()
        assert call.untouched()
        call.run(A=None, B=None, C=None)       # nothing to read or write: no pointer needed


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("splits,ta,tb", [(2, 0, 0), (3, 1, 0), (9, 0, 1), (64, 1, 1)])
def test_gemm_x3_split_k_applies_bias_and_activation_once(splits, ta, tb, act):
    """Split-K with a bias and relu / sigmoid on small integers (exact partial sums, about half of
    them negative): the bias is added and the activation applied in the fold only. splits 9 and 64
    exceed the three K-steps of K = 68; the workspace is sized by the requested count."""
    M, N, K, batch = 132, 68, 68, 2
    ops = [X.int_operands(M, K, N, 30 + i, amax=3) for i in range(batch)]
    opA = torch.stack([o[0] for o in ops])
    opB = torch.stack([o[1] for o in ops])
    g = torch.Generator().manual_seed(splits)
    bias = torch.randint(-9, 10, (batch, N), generator=g).float()
    z = opA.double() @ opB.double() + bias.double()[:, None, :]
    call = Call(opA, opB, ta, tb, bias=bias, act=act, splits=splits).run()
    _close_act(call.c(), z, act)
    one = Call(opA, opB, ta, tb, bias=bias, act=act, splits=1).run()
    if act != 2:
        _same_bits(call.c(), one.c(), "split against unsplit")


# ---------------------------------------------------------------------------------------------
def _refused(call, **over):
    with pytest.raises(L.RecsysError):
        call.run(**over)
    torch.cuda.synchronize()
    assert call.untouched(), f"C or its guards written by a refused call {over}"


def test_gemm_x3_refusals_leave_c_untouched():
    M, N, K = 8, 12, 68
    g = torch.Generator().manual_seed(0)
    opA, opB = torch.randn(2, M, K, generator=g), torch.randn(2, K, N, generator=g)
    for ta, tb in LAYOUTS:
        c = Call(opA, opB, ta, tb)
        _refused(c, A=ctypes.c_void_p(c.A.data_ptr() + 4))
        _refused(c, B=ctypes.c_void_p(c.B.data_ptr() + 8))
        _refused(c, lda=c.lda + 2)
        _refused(c, ldb=c.ldb + 1)
        _refused(c, sA=c.sA + 2)
        _refused(c, sB=c.sB - 1)
        _refused(c, lda=(M if ta else K) - 4)
        _refused(c, ldb=(K if tb else N) - 4)
        _refused(c, ldc=N - 1)
        _refused(c, act=3)
        _refused(c, act=-1)
        _refused(c, A=None)
        _refused(c, B=None)
        _refused(c, C=None)
        _refused(c, M=M + 2)
        _refused(c, N=N + 1)
        _refused(c, K=K + 2)
        _refused(c, batch=0)
        _refused(c, splits=0)
        c.run()
        assert not c.untouched()
    # split-K: K = 68 at splits 2 is two K ranges (64 + 4): the partials need a workspace
    c = Call(opA, opB, 1, 0, splits=2)
    assert c.ws_n == L.lib().rs_gemm_x3_workspace_size(M, N, 2, 2) > 0
    _refused(c, ws_n=c.ws_n - 256)
    _refused(c, ws=None)
    _refused(c, ws=None, ws_n=0)
    # ... and none when the effective count is 1 (splits 2 of a single K-step)
    Call(opA[:, :, :32], opB[:, :32], 1, 0, splits=2).run(ws=None, ws_n=0).c_bits()
    # batch x splits up to 65535 blocks in z
    nb = 65536
    big = Call(torch.zeros(nb, 4, 4), torch.zeros(nb, 4, 4), 0, 0, pads=(0, 0, 0), gaps=(0, 0, 0))
    _refused(big)
