"""dlrm_train_chunk (rs_dlrm_train_step_fwd_unit) held to the fp32 accuracy claim of its split-bf16
products, on inputs where a missing or misplaced part product shows: Uᵀ = Xᵀ·(M + Mᵀ) (mfma6_xs,
through the chunk image, the transposed read, the staging tile and S's split parts) under pair
weights that form a perfect matching, so every element of U is one product; Z = X·Xᵀ (mfma6)
through the A_top sums at batch 1, where sums[k] = fl(z_k · G) with the kernel's own G (one
rounding: az += zr · G from zero, and the block and two-level folds add exact zeros), on examples
whose z are single products; and integer data at full density. The inputs and bounds are those of
tests/x3_model.py, proved against the CPU model and its mutants in tests/test_x3_model_cpu.py.
D = 128 runs with S = 27 (F = 28: the Z blocks c00 / c01 / c11 are all live, the dense row sits
in the second 16-row block), D = 64 with S = 11 (one block)."""
import pytest
import torch

from recommender_amd import _lib as L
from tests import x3_model as X
from tests.dlrm_edges import EPS, GUARD, GUARD_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda"
NI = X.NI
ATOP = 512


class Train:
    """One allocation set for (B, S, D); run() copies the inputs in, calls the kernel and
    synchronises once. The outputs sit in front of guard elements."""

    def __init__(self, B, S, D):
        self.B, self.S, self.D = B, S, D
        f = dict(device=DEV)
        self.table = torch.empty(S * B, D, **f)
        self.ids = torch.empty(B, S, dtype=torch.int32, **f)
        self.offs = torch.empty(S + 1, dtype=torch.int64, **f)
        self.dense = torch.empty(B, D, **f)
        self.xin = torch.empty(B, NI, **f)
        self.label = torch.empty(B, **f)
        self.q = torch.empty(S * (S + 1) // 2 + D, **f)
        self.c = torch.empty(1, **f)
        self.sizes = dict(y=B, rows=B * S * D, G=B, sums=ATOP + 2 + NI * D + D)
        self.out = {k: torch.empty(n + GUARD, dtype=torch.int32, **f) for k, n in self.sizes.items()}
        self.ws_n = L.lib().rs_dlrm_train_workspace_size(B)
        self.ws = torch.empty(self.ws_n, dtype=torch.uint8, **f)
        self.err = torch.zeros(1, dtype=torch.int32, **f)

    def run(self, inp):
        B, S, D = self.B, self.S, self.D
        for dst, src in zip((self.table, self.ids, self.offs, self.dense, self.xin, self.label,
                             self.q, self.c), inp):
            assert dst.shape == src.shape and dst.dtype == src.dtype
            dst.copy_(src)
        for o in self.out.values():
            o.fill_(GUARD_BITS)
        self.err.zero_()
        o = self.out
        L.call("rs_dlrm_train_step_fwd_unit", L.ptr(self.table), S * B, D, L.ptr(self.ids),
               L.id_dtype_code(self.ids), S, L.ptr(self.offs), L.ptr(self.dense), L.ptr(self.xin),
               NI, L.ptr(self.label), B, L.ptr(self.q), L.ptr(self.c), EPS, 1.0 / B,
               L.ptr(o["y"]), L.ptr(o["rows"]), L.ptr(o["G"]), L.ptr(o["sums"]), L.ptr(self.ws),
               self.ws_n, L.ptr(self.err), L.stream_ptr(torch.device(DEV)))
        got = {k: v.cpu() for k, v in o.items()}        # synchronises
        r = {}
        for k, n in self.sizes.items():
            assert bool((got[k][n:] == GUARD_BITS).all()), f"{k}: guard overwritten"
            r[k] = got[k][:n].view(torch.float32)
        r["rows"] = r["rows"].view(B, S, D)
        r["err"] = int(self.err.item())
        return r


def _bits(t):
    return (t.float() + 0.0).contiguous().view(torch.int32)   # −0 folded into +0


def _same_bits(got, want, msg):
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())} / {bad.numel()} elements differ"


def _g_of(r):
    """The kernel's own G of a batch-1 call: finite, nonzero (y inside the clip)."""
    G = r["G"].double()[0]
    assert bool(torch.isfinite(G)) and float(G) != 0.0, f"G = {float(G)}, y = {float(r['y'][0])}"
    return G


def _bad_ids(B, S):
    """Out-of-range ids: a slot of the first block, one of the last block, the dense row's
    partners among them over the matchings."""
    return [(1, 0, B), (1, S - 1, -1), (2, S // 2, B + 5), (B - 1, 1, -7)]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_unit_rows_are_bit_exact_under_a_pow2_matching(S, D):
    """Pair weights ±1 / ±2^k on a perfect matching, full-mantissa rows: unit_rows[b, i] =
    w_i · X_b[partner(i)] bit for bit — the partner in the same and in the other 16-row block, a
    slot paired with the dense row, and rows of out-of-range ids (their own X is zero, they
    still receive their partner's row; their partner receives zeros)."""
    B = 9
    tr = Train(B, S, D)
    for mi in range(3):
        Xc, q, w, partner = X.u_case("pow2", S, D, B, mi, 40 + mi)
        inp, Xe = X.train_case(Xc, q, bad_ids=_bad_ids(B, S))
        r = tr.run(inp)
        assert r["err"] != 0
        want = w[None, :S, None] * Xe[:, partner][:, :S]
        _same_bits(r["rows"], want, f"matching {mi}")


def _u_precision(kind, rel, S, D):
    B = 9
    tr = Train(B, S, D)
    worst = 0.0
    for mi, seed in X.U_CASES:
        Xc, q, w, partner = X.u_case(kind, S, D, B, mi, seed)
        inp, Xe = X.train_case(Xc, q)
        r = tr.run(inp)
        assert r["err"] == 0
        ref = w.double()[None, :S, None] * Xe.double()[:, partner][:, :S]
        worst = max(worst, X.max_rel(r["rows"], ref, ref.abs()))
        assert bool(((r["rows"].double() - ref).abs() <= rel * ref.abs()).all()), \
            f"matching {mi}: {worst / X.U:.3f} U"
    print(f"train U {kind} D {D}: max err/|q·x| {worst / X.U:.3f} U (bound {rel / X.U:g} U)")


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_unit_rows_one_term_precision(S, D):
    """Full-mantissa weights on the matchings: |U − q·x| <= REL_FEW |q·x| (clean model 1.1 U, a
    missing 2^-16-class product 120 U or more). Measured on the MI355X: 2.2 U."""
    _u_precision("few", X.REL_FEW, S, D)


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_unit_rows_split_rounds_to_nearest(S, D):
    """The truncation-sensitive pairs: bound REL_TRUNC = 2.9 U (the rounding split in the model
    < 2^-30, on the MI355X 1 ulp = 1.97 U from the MFMA's own adder; a truncating split 5.9 U)."""
    _u_precision("trunc", X.REL_TRUNC, S, D)


# ---------------------------------------------------------------------------------------------
def _z_columns(kind, D):
    """few: every column. trunc: every k position of a 32-column chunk once, over all chunks."""
    return list(range(D)) if kind == "few" else [k + 32 * (k % (D // 32)) for k in range(32)]


def _z_precision(kind, rel, S, D):
    F = S + 1
    nz = F * (F - 1) // 2
    iu = torch.triu_indices(F, F, 1)
    tr = Train(1, S, D)
    worst = 0.0
    for col in _z_columns(kind, D):
        Xc, q, x = X.z_column_case(kind, S, D, col, 3)
        inp, _ = X.train_case(Xc, q, label=torch.tensor([float(col % 2)]))
        r = tr.run(inp)
        G = _g_of(r)
        ref = x.double()[iu[0]] * x.double()[iu[1]] * G
        got = r["sums"][:nz]
        worst = max(worst, X.max_rel(got, ref, ref.abs()))
        assert bool(((got.double() - ref).abs() <= (rel + 2.0 ** -23) * ref.abs()).all()), \
            f"column {col}: {worst / X.U:.3f} U"
        # the dense part of A_top: fl(dense · G), and the zero padding
        _same_bits(r["sums"][nz:nz + D], (Xc[0, S].double() * G).float(), f"column {col} dense·G")
        assert bool((r["sums"][nz + D:ATOP] == 0).all())
    print(f"train Z {kind} D {D}: max err/|z·G| {worst / X.U:.3f} U (bound {rel / X.U:g} + 2 U)")


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_pair_sums_one_term_precision(S, D):
    """Batch 1, every row nonzero in one column only, every column in turn (every k position of
    every chunk): |sums[k] − z_k G| <= (REL_FEW + 2^-23) |z_k G|. Measured on the MI355X: 2.8 U
    (the product by G adds its rounding)."""
    _z_precision("few", X.REL_FEW, S, D)


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_pair_sums_split_rounds_to_nearest(S, D):
    _z_precision("trunc", X.REL_TRUNC, S, D)


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_pair_sums_part_product_probes_are_exact(S, D):
    """Matched pairs of rows, each pair in a column of its own holding a probe pair: that z is the
    exact fp32 product (which needs the probed part product), so sums[k] = fl(z · G) bit for bit
    and every other pair sum is zero. The walk puts every product type at every k position."""
    F = S + 1
    nz = F * (F - 1) // 2
    tr = Train(1, S, D)
    for t in range(X.Z_PROBE_LAUNCHES[D]):
        Xc, q, pairs = X.z_probe_case(S, D, t)
        inp, _ = X.train_case(Xc, q, label=torch.tensor([float(t % 2)]))
        r = tr.run(inp)
        G = _g_of(r)
        want = torch.zeros(nz, dtype=torch.float64)
        for i, j, col, _ in pairs:
            z = Xc[0, i, col].double() * Xc[0, j, col].double()
            assert float(z.float()) == float(z)
            want[X.compact_index(i, j, F)] = z * G
        _same_bits(r["sums"][:nz], want.float(), f"launch {t}")
        _same_bits(r["sums"][nz:nz + D], (Xc[0, S].double() * G).float(), f"launch {t} dense·G")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_integer_data_is_exact(S, D):
    """Integer table and dense entries |v| <= 15, pair weights 0 / ±1, full density in D and F: U
    is the integer result exactly; at batch 1 the A_top pair sums are fl(z · G) with the integer
    z."""
    F = S + 1
    nz = F * (F - 1) // 2
    iu = torch.triu_indices(F, F, 1)
    B = 9
    Xc, q, _ = X.int_train_case(S, D, B, 60)
    inp, Xe = X.train_case(Xc, q, bad_ids=_bad_ids(B, S))
    r = Train(B, S, D).run(inp)
    want = (X.pair_weights(q, F)[None] @ Xe.double())[:, :S]
    assert float(want.abs().max()) < 2 ** 24
    assert bool((r["rows"].double() == want).all()), int((r["rows"].double() != want).sum())
    tr = Train(1, S, D)
    for seed in range(61, 65):
        Xc, q, c = X.int_train_case(S, D, 1, seed)
        inp, _ = X.train_case(Xc, q, c=c, label=torch.tensor([float(seed % 2)]))
        r = tr.run(inp)
        assert float(r["y"][0]) == 0.5
        G = _g_of(r)
        Z = Xc[0].double() @ Xc[0].double().T
        _same_bits(r["sums"][:nz], (Z[iu[0], iu[1]] * G).float(), f"seed {seed} z·G")
        _same_bits(r["sums"][nz:nz + D], (Xc[0, S].double() * G).float(), f"seed {seed} dense·G")
        want = (X.pair_weights(q, F) @ Xc[0].double())[:S]
        assert bool((r["rows"][0].double() == want).all())
