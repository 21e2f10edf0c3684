"""The proof of tests/x3_model.py, without a GPU: the split is exact, every one of the six part
products has exact probes, exact multiplications stay exact in the model, and every precision
bound the GPU tests of rs_gemm_x3 and dlrm_train_chunk use separates the clean model from the
mutants it is there to kill, on the very inputs those tests use: the clean model's max error is
at least 4x below the bound, the mutants' at least 2x above. That is a condition on the bound,
checked here, not a measurement."""
import pytest
import torch

from tests import x3_model as X

N_FEW = 4096


def _f32(v):
    return torch.tensor([v], dtype=torch.float64).float()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncate", [False, True])
def test_split_is_exact(truncate):
    """h + m + l == x for magnitudes 2^-60 .. 2^60: far from bf16's overflow (2^128) and from its
    denormals (l is about 2^-16 |x| >= 2^-76, the smallest normal 2^-126)."""
    g = torch.Generator().manual_seed(0)
    n = 200_000
    e = torch.randint(-60, 61, (n,), generator=g).double()
    x = (torch.randn(n, generator=g).double() * torch.exp2(e)).float()
    x = torch.cat([x, torch.tensor([0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -23, 2 - 2.0 ** -23,
                                    1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23])])
    h, m, l = X.split(x, truncate)
    for p in (h, m, l):                      # each part is a bf16 number
        assert bool((p.to(torch.bfloat16).float() == p).all())
    assert bool(((h.double() + m.double() + l.double()) == x.double()).all())
    if not truncate:                         # round to nearest: the parts shrink by 2^-8 each
        ok = x != 0
        assert bool((m.abs()[ok] <= 2.0 ** -8 * h.abs()[ok]).all())
        assert bool((l.abs()[ok] <= 2.0 ** -16 * h.abs()[ok]).all())


def test_split_rounds_to_nearest_even():
    h, _, _ = X.split(_f32(1 + 2.0 ** -8))          # a tie: to the even neighbour 1
    assert float(h) == 1.0
    h, _, _ = X.split(_f32(1 + 2.0 ** -7 + 2.0 ** -8))  # a tie: up to the even 1 + 2^-6
    assert float(h) == 1 + 2.0 ** -6
    h, m, l = X.split(_f32(1 + 2.0 ** -7 - 2.0 ** -23))
    assert (float(h), float(m), float(l)) == (1 + 2.0 ** -7, -2.0 ** -23, 0.0)
    h, m, l = X.split(_f32(1 + 2.0 ** -7 - 2.0 ** -23), truncate=True)
    assert (float(h), float(m), float(l)) == (1.0, 2.0 ** -7 - 2.0 ** -15, 2.0 ** -15 - 2.0 ** -23)


@pytest.mark.parametrize("name,a,b", X.probes())
def test_each_product_has_an_exact_probe(name, a, b):
    ta, tb = _f32(a), _f32(b)
    assert float(ta) == a and float(tb) == b
    exact = ta.double() * tb.double()
    assert bool(exact.float().double() == exact)          # the true product is an fp32 number
    assert bool(X.product(ta, tb).double() == exact)      # the full model returns it
    assert bool(X.product(ta, tb, drop=(name,)).double() != exact)   # without that product: not
    # through a K-step with the term at any position, both accumulation forms
    A = torch.zeros(1, 32)
    B = torch.zeros(32, 1)
    A[0, 13], B[13, 0] = ta[0], tb[0]
    for reacc in (True, False):
        assert bool(X.matmul(A, B, reacc=reacc).double() == exact)
        assert bool(X.matmul(A, B, drop=(name,), reacc=reacc).double() != exact)


def test_probe_operands_cover_all_six():
    a, b, names = X.probe_operands(36)
    assert set(names) == set(X.ORDER)
    assert bool((X.product(a, b).double() == a.double() * b.double()).all())


@pytest.mark.parametrize("reacc", [True, False])
def test_exact_multiplications_stay_exact(reacc):
    """A product with a 0 / ±1 / ±2^k generalised permutation is bit-exact, from either side."""
    n = 100
    g = torch.Generator().manual_seed(3)
    Bm = torch.randn(n, 70, generator=g)
    for shift in (None, 33):
        perm, scale = X.gen_perm(n, 5, shift)
        assert bool((scale == 0).any()) and bool((scale.abs() == 1).any())
        P = torch.zeros(n, n)
        P[torch.arange(n), perm] = scale
        want = scale[:, None] * Bm[perm]
        got = X.matmul(P, Bm, reacc=reacc)
        assert (X.np_i32(got + 0.0) == X.np_i32(want + 0.0)).all()
        got = X.matmul(Bm.T.contiguous(), P.T.contiguous(), reacc=reacc)
        assert (X.np_i32(got + 0.0) == X.np_i32(want.T + 0.0)).all()


def test_integer_products_are_exact():
    A, B = X.int_operands(40, 200, 36, 7)
    want = A.double() @ B.double()
    assert float(want.abs().max()) < 2 ** 24
    for reacc in (True, False):
        assert bool((X.matmul(A, B, reacc=reacc).double() == want).all())
        # |v| <= 255 is 8 bits: all of it is in h, so these tests are about the k range and the
        # seams, not about the small products
        assert not bool((X.matmul(A, B, drop=("hh",), reacc=reacc).double() == want).all())
        assert bool((X.matmul(A[:, :-1], B[:-1], reacc=reacc).double() != want).any())


# ---------------------------------------------------------------------------------------------
# the discrimination condition of every precision bound
def _margins(clean, mutants, rel):
    assert 4 * clean <= rel, f"clean {clean:.3g} is not 4x below the bound {rel:.3g}"
    for name, v in mutants.items():
        assert v >= 2 * rel, f"mutant {name}: {v:.3g} is not 2x above the bound {rel:.3g}"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_few_term_bound_kills_every_dropped_product(seed):
    """REL_FEW on independent full-mantissa pairs (the GPU tests' own inputs follow below)."""
    a, b = X.few_term_operands(N_FEW, seed)
    ref = a.double() * b.double()
    mag = ref.abs()
    clean = X.max_rel(X.product(a, b), ref, mag)
    mut = {d: X.max_rel(X.product(a, b, drop=(d,)), ref, mag) for d in X.ORDER}
    print(f"few-term seed {seed}: clean {clean / X.U:.2f} U, mutants",
          {k: round(v / X.U, 1) for k, v in mut.items()})
    _margins(clean, mut, X.REL_FEW)
    # the truncating split cannot meet these margins on random operands under any bound of this
    # form: its error is at most 2^-21 |a·b| (8 U) against the clean 1 - 1.5 U. It is worse than
    # the clean model here; trunc_operands and REL_TRUNC carry its discrimination.
    tr = X.max_rel(X.product(a, b, truncate=True), ref, mag)
    assert 3 * clean < tr <= 9 * X.U


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_trunc_bound_kills_the_truncating_split(seed):
    a, b = X.trunc_operands(N_FEW, seed)
    ref = a.double() * b.double()
    mag = ref.abs()
    clean = X.max_rel(X.product(a, b), ref, mag)
    mut = {"truncate": X.max_rel(X.product(a, b, truncate=True), ref, mag),
           "hm": X.max_rel(X.product(a, b, drop=("hm",)), ref, mag),
           "mh": X.max_rel(X.product(a, b, drop=("mh",)), ref, mag)}
    print(f"trunc seed {seed}: clean {clean / X.U:.4f} U, mutants",
          {k: round(v / X.U, 2) for k, v in mut.items()})
    _margins(clean, mut, X.REL_TRUNC)


def _one_term_figures(a, b, drops=X.ORDER):
    """(clean, {mutant: max err / |a·b|}) of element-wise pairs (broadcast)."""
    ref = a.double() * b.double()
    mag = ref.abs()
    clean = X.max_rel(X.product(a, b), ref, mag)
    mut = {d: X.max_rel(X.product(a, b, drop=(d,)), ref, mag) for d in drops}
    mut["truncate"] = X.max_rel(X.product(a, b, truncate=True), ref, mag)
    return clean, mut


def _check_family(kind, clean, mut, what):
    print(f"{what} {kind}: clean {clean / X.U:.4f} U, mutants",
          {k: round(v / X.U, 2) for k, v in mut.items()})
    if kind == "few":      # every dropped product; the truncating split is trunc's business
        tr = mut.pop("truncate")
        _margins(clean, mut, X.REL_FEW)
        assert clean < tr <= 9 * X.U
    else:                  # l = 0 under rounding: m·m, h·l, l·h do not exist here
        _margins(clean, {k: mut[k] for k in ("truncate", "hm", "mh", "hh")}, X.REL_TRUNC)


@pytest.mark.parametrize("kind", ["few", "trunc"])
@pytest.mark.parametrize("side", ["A", "B"])
def test_gemm_one_term_bounds_on_the_gpu_tests_inputs(side, kind):
    """tests/test_gemm_gpu.py: test_gemm_x3_one_term_precision (seed 1) and
    test_gemm_x3_split_rounds_to_nearest (seed 2), through the model's K-steps."""
    A, B = X.one_term_case(kind, side, {"few": 1, "trunc": 2}[kind])
    assert int((A != 0).sum(1).max()) == 1 or int((B != 0).sum(0).max()) == 1
    ref = A.double() @ B.double()
    mag = ref.abs()
    clean = X.max_rel(X.matmul(A, B), ref, mag)
    mut = {d: X.max_rel(X.matmul(A, B, drop=(d,)), ref, mag) for d in X.ORDER}
    mut["truncate"] = X.max_rel(X.matmul(A, B, truncate=True), ref, mag)
    _check_family(kind, clean, mut, f"gemm side {side}")


@pytest.mark.parametrize("rot", range(6))
@pytest.mark.parametrize("side", ["A", "B"])
def test_gemm_probe_case_is_exact_and_needs_every_product(side, rot):
    A, B = X.one_term_case("probe", side, 5, rot=rot)
    want = A.double() @ B.double()
    assert bool((want.float().double() == want).all())
    assert bool((X.matmul(A, B).double() == want).all())
    for d in X.ORDER:
        assert bool((X.matmul(A, B, drop=(d,)).double() != want).any())


def test_gemm_probe_walk_puts_every_product_at_every_k():
    seen = set()
    for rot in range(6):
        for k in range(68):
            seen.add((k % 32, (k + rot) % 6))
    assert len(seen) == 32 * 6


@pytest.mark.parametrize("kind", ["few", "trunc"])
@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_train_u_bounds_on_the_gpu_tests_inputs(S, D, kind):
    """tests/test_train_x3_gpu.py: _u_precision (B = 9, X.U_CASES). mfma6_xs has X as
    the A operand and the weights as B with the l·h / h·l instructions swapped: in the model's
    order the weight is the a of the pair."""
    cleans, muts = [], []
    for mi, seed in X.U_CASES:
        Xc, q, w, partner = X.u_case(kind, S, D, 9, mi, seed)
        c, m = _one_term_figures(w[None, :S, None], Xc[:, partner][:, :S])
        cleans.append(c)
        muts.append(m)
    mut = {k: max(m[k] for m in muts) for k in muts[0]}
    _check_family(kind, max(cleans), mut, f"train U D {D}")


@pytest.mark.parametrize("kind", ["few", "trunc"])
@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_train_z_bounds_on_the_gpu_tests_inputs(S, D, kind):
    """tests/test_train_x3_gpu.py: _z_precision (seed 3), all its columns together. The bound there
    is (rel + 2^-23) |z·G|: 2^-23 pays for the rounding of fl(z·G); what is left for z is rel."""
    F = S + 1
    iu = torch.triu_indices(F, F, 1)
    cols = list(range(D)) if kind == "few" else [k + 32 * (k % (D // 32)) for k in range(32)]
    assert {c % 32 for c in cols} == set(range(32)) and {c // 32 for c in cols} == set(range(D // 32))
    xs = torch.stack([X.z_column_case(kind, S, D, c, 3)[2] for c in cols])
    clean, mut = _one_term_figures(xs[:, iu[0]], xs[:, iu[1]])
    _check_family(kind, clean, mut, f"train Z D {D}")


@pytest.mark.parametrize("S,D", X.TRAIN_SHAPES)
def test_train_z_probe_walk(S, D):
    """Every launch: the matched z are exact fp32 products that need their part product; over the
    launches every product type sits at every k position of a chunk, in every chunk, and (F = 28)
    in all three Z blocks."""
    F = S + 1
    seen, chunks, blocks = set(), set(), set()
    for t in range(X.Z_PROBE_LAUNCHES[D]):
        Xc, q, pairs = X.z_probe_case(S, D, t)
        assert int((Xc != 0).sum()) == F
        for i, j, col, name in pairs:
            assert i < j
            a, b = Xc[0, i, col:col + 1], Xc[0, j, col:col + 1]
            exact = a.double() * b.double()
            assert bool(exact.float().double() == exact)
            assert bool(X.product(a, b).double() == exact)
            assert bool(X.product(a, b, drop=(name,)).double() != exact)
            seen.add((col % 32, name))
            chunks.add(col // 32)
            blocks.add((i // 16, j // 16, name))
    assert len(seen) == 32 * 6 and chunks == set(range(D // 32))
    assert len(blocks) == (18 if F > 16 else 6)


def test_integer_train_case_is_exact_in_fp32():
    for S, D in X.TRAIN_SHAPES:
        Xc, q, c = X.int_train_case(S, D, 1, 61)
        assert float(torch.tensor(c).float()) == c and abs(c) < 2 ** 24
        assert float(Xc.abs().max()) <= 15 and bool((q == q.round()).all())


def test_dense_bound_kills_every_dropped_product():
    """REL_DENSE on dense_operands, for both accumulation forms."""
    A, B = X.dense_operands()
    ref = A.double() @ B.double()
    mag = A.double().abs() @ B.double().abs()
    for reacc in (True, False):
        clean = X.max_rel(X.matmul(A, B, reacc=reacc), ref, mag)
        mut = {d: X.max_rel(X.matmul(A, B, drop=(d,), reacc=reacc), ref, mag) for d in X.ORDER}
        print(f"dense reacc {reacc}: clean {clean:.3g}, mutants",
              {k: float(f"{v:.3g}") for k, v in mut.items()})
        _margins(clean, mut, X.REL_DENSE)


@pytest.mark.parametrize("case", range(6))
def test_unit_row_bound_on_the_dense_train_test_inputs(case):
    """tests/test_train_unit_gpu.py's unit rows (its first 512 examples): REL_U_DENSE."""
    from tests import dlrm_edges as E
    from tests.test_train_unit_gpu import CASES, inputs_cpu

    B, S, D, id64, oob = CASES[case]
    table, ids, offs, dense, _, _, q, _ = inputs_cpu(B, S, D, 20_000 * S, id64, seed=B + S, oob=oob)
    Xf = E.gather_x(table, ids[:512], offs, dense[:512], S)[0].float()
    Sm = X.pair_weights(q, S + 1)
    ref = (Sm[None] @ Xf.double())[:, :S]
    mag = (Sm.abs()[None] @ Xf.double().abs())[:, :S]
    Sf = Sm.float()[None]
    clean = X.max_rel(X.matmul(Sf, Xf)[:, :S], ref, mag)
    mut = {d: X.max_rel(X.matmul(Sf, Xf, drop=(d,))[:, :S], ref, mag) for d in X.ORDER}
    print(f"unit rows {CASES[case]}: clean {clean:.3g}, mutants",
          {k: float(f"{v:.3g}") for k, v in mut.items()})
    _margins(clean, mut, X.REL_U_DENSE)


def test_matchings_are_perfect_and_cross_the_blocks():
    for F in (28, 14):
        ms = X.matchings(F)
        same = cross = dense_lo = False
        for p in ms:
            assert sorted(p) == list(range(F))
            assert all(p[p[i]] == i and p[i] != i for i in range(F))
            for i in range(F):
                same |= i // 16 == p[i] // 16
                cross |= i // 16 != p[i] // 16
            dense_lo |= p[F - 1] < 16
        assert same and dense_lo and (cross or F <= 16)
        q, w = X.matching_q(F, 8, ms[1], X.pow2_weights(F, 0))
        assert int((q != 0).sum()) == F // 2 and bool((w != 0).all())
        iu = torch.triu_indices(F, F, 1)
        M = torch.zeros(F, F)
        M[iu[0], iu[1]] = q[:iu.shape[1]]
        Sm = M + M.T
        assert bool((Sm[torch.arange(F), torch.tensor(ms[1])] == w).all())
