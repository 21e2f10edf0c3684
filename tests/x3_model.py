"""A CPU model of the split-bf16 products of csrc/mfma_x3.hpp and the inputs of the tests that hold
rs_gemm_x3 and dlrm_train_chunk to their fp32 accuracy claim. Plain torch on the CPU: no GPU and no
library is touched here, so tests/test_x3_model_cpu.py can prove the model, the probes and the
discrimination of every precision bound, and the GPU tests use the very same inputs and bounds.

The scheme: every fp32 operand is split x = h + m + l into three bf16 parts (split_pair: round to
nearest even, residuals exact in fp32) and a product a·b is the fp32 sum of six part products in
the order of mfma6: m·m, h·l, l·h, h·m, m·h, h·h (mfma6_xs: the same order, operand roles
swapped). A bf16·bf16 product is exact in fp32; one MFMA instruction is modelled as the exact
(float64) sum of its part products over the 32-deep step plus the accumulator, rounded to fp32
once.

Mutants (the `mutate=` convention of tests/dlrm_edges.py::reference): `drop=` names the products to
leave out, `truncate=True` splits by truncation instead of rounding. A truncating split is still
exact (three 8-bit parts hold 24 bits), but its m and l are up to twice as large and one-signed,
so the three products the scheme never forms (m·l, l·m, l·l) grow from <= 2^-24 to <= 2^-21 of
|a·b|.
"""
import torch

ORDER = ("mm", "hl", "lh", "hm", "mh", "hh")      # mfma6: smallest first
U = 2.0 ** -24                                    # the fp32 unit roundoff

# ---------------------------------------------------------------------------------------------
# the precision bounds of the GPU tests, in units of |a·b| (few-term) or Σ|terms| (dense);
# tests/test_x3_model_cpu.py proves for each, on the inputs the GPU test uses: the clean model's
# max error is >= 4x below, the mutants the family is there to kill are >= 2x above.
#
# One nonzero term per dot product, full-mantissa random operands (one_term_case, u_case,
# z_column_case "few"). The clean model errs by at most 1.5 U (the final rounding, U, and the three
# products never formed); a single dropped product of the 2^-16 class reaches 120-220 U over a few
# thousand pairs (60 U where one side has only a few dozen distinct values: the weights of u_case).
# The MI355X measures 2.2 U: the bf16 MFMA's adder does not round to nearest (see REL_TRUNC).
REL_FEW = 16 * U
# One nonzero term, operands whose product is all but an fp32 number and whose low mantissa bits
# are ones ("trunc"): the rounding split gives l = 0 and an error below 2^-30 in the model, the
# truncating split 5.9 U = 3 ulps of the product. The MI355X returns the neighbouring fp32 number
# on some of these pairs, 1 ulp = 1.97 U: its MFMA adds the small addends h·m + m·h to h·h
# rounding down, where the model rounds to nearest. The bound sits between 1 and 3 ulps, half the
# mutant's error. (On random operands no bound of this form separates the two splits by the 8x the
# margins ask for: the truncating split's error is at most 2^-21 = 8 U there, the clean one 1.5 U.)
REL_TRUNC = 2.9 * U
# Dense random data, K = 100 (dense_operands, rs_gemm_x3): clean model 7.2e-8, the weakest
# single-drop mutant 1.66e-6; measured on the MI355X: the kernel 6.45e-8, the library GEMM 2.34e-7.
REL_DENSE = 6e-7
# The unit rows of tests/test_train_unit_gpu.py (dense, 9 to 27 terms): clean model 6.7e-8, the
# weakest single-drop mutant 3.7e-6; measured on the MI355X: 1.27e-7.
REL_U_DENSE = 1e-6


def _bf16_rne(x):
    return x.to(torch.bfloat16).float()


def _bf16_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split(x, truncate=False):
    """(h, m, l) as fp32 tensors holding bf16 values, h + m + l == x (split_pair)."""
    x = x.float()
    cvt = _bf16_trunc if truncate else _bf16_rne
    h = cvt(x)
    r1 = x - h
    m = cvt(r1)
    l = cvt(r1 - m)
    return h, m, l


def _parts(a, b, truncate):
    ah, am, al = split(a, truncate)
    bh, bm, bl = split(b, truncate)
    return {"mm": (am, bm), "hl": (ah, bl), "lh": (al, bh), "hm": (ah, bm), "mh": (am, bh),
            "hh": (ah, bh)}


def product(a, b, drop=(), truncate=False):
    """Element-wise a·b as a dot product with one nonzero term comes out of mfma6 (from a zero
    accumulator): the six exact part products added in order, each sum rounded to fp32."""
    p = _parts(a, b, truncate)
    c = torch.zeros(torch.broadcast_shapes(a.shape, b.shape), dtype=torch.float64)
    for name in ORDER:
        if name in drop:
            continue
        x, y = p[name]
        c = (c + x.double() * y.double()).float().double()
    return c.float()


def matmul(A, B, drop=(), truncate=False, kstep=32, reacc=True):
    """A [.., M, K] · B [.., K, N] in steps of `kstep`. reacc (rs_gemm_x3): every step's six
    products are summed from zero and the step sum is added to the running sum in fp32; not reacc
    (dlrm_train_chunk's Z): the six instructions of every step add to the running accumulator."""
    K = A.shape[-1]
    acc = torch.zeros(*A.shape[:-1], B.shape[-1], dtype=torch.float64)
    for k0 in range(0, K, kstep):
        p = _parts(A[..., k0:k0 + kstep], B[..., k0:k0 + kstep, :], truncate)
        c = torch.zeros_like(acc) if reacc else acc
        for name in ORDER:
            if name in drop:
                continue
            x, y = p[name]
            c = (c + x.double() @ y.double()).float().double()
        acc = (acc + c).float().double() if reacc else c
    return acc.float()


def max_rel(got, ref, mag):
    """max |got − ref| / mag over the elements with mag > 0 (float64 ref and mag)."""
    e = (got.double() - ref).abs()
    ok = mag > 0
    return float((e[ok] / mag[ok]).max())


# ---------------------------------------------------------------------------------------------
# probes: one exact pair per product
_P = {
    "mm": (1 + 2.0 ** -10, 1 + 2.0 ** -11),
    "hl": (1.0, 1 + 2.0 ** -10 + 2.0 ** -22),
    "lh": (1 + 2.0 ** -10 + 2.0 ** -22, 1.0),
    "hm": (1.0, 1 + 2.0 ** -10),
    "mh": (1 + 2.0 ** -10, 1.0),
    "hh": (1.5, 1.25),
}
_VARIANTS = ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-4.0, -0.125), (2.0 ** 20, 2.0 ** -30),
             (2.0 ** -40, -2.0 ** 12))


def probes():
    """[(product name, a, b)]: the six pairs, each also with signs and power-of-two scales. The
    true product a·b is an fp32 number, the full model returns it, and the model without the
    named product does not."""
    return [(n, a * sa, b * sb) for n, (a, b) in _P.items() for sa, sb in _VARIANTS]


def probe_operands(n):
    """(a, b, names): n probe pairs, cycling through probes()."""
    ps = probes()
    idx = [i % len(ps) for i in range(n)]
    a = torch.tensor([ps[i][1] for i in idx], dtype=torch.float64).float()
    b = torch.tensor([ps[i][2] for i in idx], dtype=torch.float64).float()
    return a, b, [ps[i][0] for i in idx]


def few_term_operands(n, seed):
    """(a, b): n pairs of full-mantissa values (randn times a power of two in 2^-8 .. 2^8)."""
    g = torch.Generator().manual_seed(seed)

    def draw():
        return torch.randn(n, generator=g) * torch.exp2(torch.randint(-8, 9, (n,), generator=g).float())

    return draw(), draw()


def trunc_operands(n, seed):
    """(a, b): a = ±2^e (1 + 2^-7 − ka 2^-23), b likewise with kb = 128 − ka, ka in 1 .. 127. The
    bits below the bf16 head are ones: rounding gives h = 1 + 2^-7, m = −k 2^-23, l = 0 and a·b =
    an fp32 number + ka kb 2^-46; truncation gives h = 1, m = 2^-7 − 2^-15, l = (256 − k) 2^-23,
    whose missing m·l + l·m is 1.5 · 2^-22."""
    g = torch.Generator().manual_seed(seed)
    ka = torch.randint(1, 128, (n,), generator=g).double()
    kb = 128 - ka

    def val(k):
        s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        e = torch.randint(-6, 7, (n,), generator=g).double()
        return (s * torch.exp2(e) * (1 + 2.0 ** -7 - k * 2.0 ** -23)).float()

    return val(ka), val(kb)


def gen_perm(n, seed, shift=None, k=None):
    """A generalised permutation of n: (perm, scale) with scale in {±1, ±2^k, some 0}. shift: the
    cyclic permutation i -> (i + shift) % n instead of a random one (carries every element the
    same distance, across tile seams). k: n indices into range(k) instead (a selection: one
    nonzero per vector of a rectangular operand)."""
    g = torch.Generator().manual_seed(seed)
    if k is not None:
        perm = (torch.arange(n) + shift) % k if shift is not None else torch.randint(0, k, (n,), generator=g)
    else:
        perm = (torch.arange(n) + shift) % n if shift is not None else torch.randperm(n, generator=g)
    k = torch.randint(-6, 7, (n,), generator=g).float()
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    scale = s * torch.exp2(k)
    scale[torch.rand(n, generator=g) < 0.1] = 0.0
    scale[::5] = torch.where(scale[::5] != 0, torch.sign(scale[::5]), scale[::5])  # plain ±1 too
    return perm, scale


def _signs_scales(shape, g, lo=-6, hi=6):
    s = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    return s * torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).double())


def one_term_case(kind, side, seed, M=132, N=132, K=68, rot=0):
    """(op(A) [M, K], op(B) [K, N]) with one nonzero term per dot product. side "A": row m of
    op(A) is nonzero only at k = (5 m + 3) % K and op(B) is dense, so C[m, n] = A[m, k_m] B[k_m,
    n]; side "B": column n of op(B) is nonzero only at k_n and op(A) is dense. Every k of the
    K range (two 32-deep steps and a ragged one) is used. The a of a pair is always in op(A), the b
    in op(B). kind: "few" full-mantissa random pairs; "trunc" the pairs of trunc_operands (class
    ka by k); "probe" the pairs of probes(), the product type of position k being (k + rot) % 6, so
    rot = 0 .. 5 puts every type at every k."""
    g = torch.Generator().manual_seed(seed)
    R = M if side == "A" else N            # vectors of the sparse operand
    J = N if side == "A" else M            # vectors of the dense one
    kmap = (5 * torch.arange(R) + 3) % K
    assert R >= K and len(set(kmap.tolist())) == K
    if kind == "few":
        sp = torch.randn(R, generator=g).double() * _signs_scales((R,), g, -8, 8).abs()
        dn = torch.randn(K, J, generator=g).double() * _signs_scales((K, J), g, -8, 8).abs()
    elif kind == "trunc":
        ka = torch.randint(1, 128, (K,), generator=g).double()
        ks, kd = (ka, 128 - ka)
        sp = _signs_scales((R,), g) * (1 + 2.0 ** -7 - ks[kmap] * 2.0 ** -23)
        dn = _signs_scales((K, J), g) * (1 + 2.0 ** -7 - kd[:, None] * 2.0 ** -23)
    elif kind == "probe":
        ps = probes()
        k = torch.arange(K)
        pidx = ((k + rot) % 6) * len(_VARIANTS) + (k // 6 + rot) % len(_VARIANTS)
        pa = torch.tensor([ps[i][1] for i in pidx.tolist()], dtype=torch.float64)
        pb = torch.tensor([ps[i][2] for i in pidx.tolist()], dtype=torch.float64)
        vs, vd = (pa, pb) if side == "A" else (pb, pa)
        sp = vs[kmap] * _signs_scales((R,), g, -3, 3)
        dn = vd[:, None] * _signs_scales((K, J), g, -3, 3)
    else:
        raise ValueError(kind)
    sp, dn = sp.float(), dn.float()
    if side == "A":
        A = torch.zeros(M, K)
        A[torch.arange(M), kmap] = sp
        return A, dn.contiguous()
    B = torch.zeros(K, N)
    B[kmap, torch.arange(N)] = sp
    return dn.T.contiguous(), B


# ---------------------------------------------------------------------------------------------
# dense data
DENSE ={"M": 260, "N": 200, "K": 100, "seed": 11}


def dense_operands():
    """(A [M, K], B [K, N]) dense randn, the shape of DENSE: M crosses two 128-tiles, K is three
    full 32-deep steps and a ragged one."""
    g = torch.Generator().manual_seed(DENSE["seed"])
    return (torch.randn(DENSE["M"], DENSE["K"], generator=g),
            torch.randn(DENSE["K"], DENSE["N"], generator=g) * 0.5)


def int_operands(M, K, N, seed, amax=255):
    """Integer-valued (A, B) with |v| <= amax. |Σ| <= K amax² must stay below 2^24 for the product
    to be exact in fp32 whatever the order: K <= 258 at amax 255."""
    assert K * amax * amax < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-amax, amax + 1, (M, K), generator=g).float(),
            torch.randint(-amax, amax + 1, (K, N), generator=g).float())


# ---------------------------------------------------------------------------------------------
# dlrm_train_chunk: matchings of the F = S + 1 fields and single-column examples
def compact_index(i, j, F):
    """Position of pair (i < j) in the strict upper triangle, row-major (torch.triu_indices)."""
    return i * F - i * (i + 1) // 2 + (j - i - 1)


def matchings(F):
    """Perfect matchings of the F fields as partner lists (F even). Between them the partner lies
    in the same 16-row block and in the other one, and the dense row F − 1 is paired with a slot
    of either block."""
    assert F % 2 == 0
    h = F // 2
    out = []
    out.append([i ^ 1 for i in range(F)])                         # neighbours: same block
    out.append([(i + h) % F for i in range(F)])                   # i <-> i + F/2: across blocks
    out.append([F - 1 - i for i in range(F)])                     # mirror: 0 <-> dense row
    return out


def matching_q(F, D, partner, weights):
    """q [nzc + D] with pair weight weights[min(i, j)] on every matched pair, 0 elsewhere, and a
    zero dense part; and the [F] weight each field's partner row arrives with."""
    nzc = F * (F - 1) // 2
    q = torch.zeros(nzc + D)
    w = torch.zeros(F)
    for i, j in enumerate(partner):
        assert partner[j] == i and i != j
        lo, hi = min(i, j), max(i, j)
        q[compact_index(lo, hi, F)] = weights[lo]
        w[i] = weights[lo]
    return q, w


def pow2_weights(F, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-5, 6, (F,), generator=g).float()
    s = torch.where(torch.rand(F, generator=g) < 0.5, -1.0, 1.0)
    w = s * torch.exp2(k)
    w[::3] = torch.sign(w[::3])
    return w


U_CASES = [(mi, 50 + mi + 10 * rep) for mi in range(3) for rep in range(3)]   # (matching, seed)
TRAIN_SHAPES = ((27, 128), (11, 64))   # (S, D): F = 28 has all three Z blocks live, F = 12 one
NI = 13


def train_case(X, q, c=0.0, label=None, bad_ids=()):
    """The train kernel's inputs (CPU) for the examples X [B, F, D]: slot s of example b reads
    table row s·B + b = X[b, s] (id b of B), the dense row is X[b, F − 1]. bad_ids: (b, s, id)
    with id outside 0 .. B − 1, whose X row the kernel replaces by zeros. Returns the input tuple
    in the order of tests/dlrm_edges.py and the effective X (float32, bad rows zeroed)."""
    B, F, D = X.shape
    S = F - 1
    table = X[:, :S].transpose(0, 1).reshape(S * B, D).contiguous()
    ids = torch.arange(B, dtype=torch.int32)[:, None].repeat(1, S)
    Xe = X.clone()
    for b, s, bad in bad_ids:
        assert not 0 <= bad < B
        ids[b, s] = bad
        Xe[b, s] = 0
    offs = torch.arange(S + 1, dtype=torch.int64) * B
    g = torch.Generator().manual_seed(B + F)
    xin = torch.rand(B, NI, generator=g)
    label = (torch.arange(B) % 2).float() if label is None else label
    return (table, ids.contiguous(), offs, X[:, S].contiguous(), xin, label, q.float(),
            torch.tensor([float(c)])), Xe


def u_case(kind, S, D, B, mi, seed):
    """A perfect matching as q's pair weights: row i of U is w_i · X[partner(i)], one product per
    element. kind "pow2": weights ±1 / ±2^k, X full-mantissa (U is exact); "few": weights and X
    full-mantissa random; "trunc": the pairs of trunc_operands (class ka by matched pair). Returns
    (X [B, F, D], q, w [F], partner)."""
    F = S + 1
    g = torch.Generator().manual_seed(seed)
    partner = matchings(F)[mi]
    lo = torch.tensor([min(i, p) for i, p in enumerate(partner)])
    if kind == "pow2":
        wl = pow2_weights(F, seed)
        X = torch.randn(B, F, D, generator=g) * 0.5
    elif kind == "few":
        wl = (torch.randn(F, generator=g).double() * _signs_scales((F,), g, -4, 4).abs()).float()
        X = (torch.randn(B, F, D, generator=g).double() * _signs_scales((B, F, D), g, -4, 4).abs()).float()
    elif kind == "trunc":
        ka = torch.randint(1, 128, (F,), generator=g).double()
        wl = (_signs_scales((F,), g, -3, 3) * (1 + 2.0 ** -7 - ka * 2.0 ** -23)).float()
        kx = (128 - ka)[lo]                       # the class of the rows matched with weight lo
        X = (_signs_scales((B, F, D), g, -3, 3) * (1 + 2.0 ** -7 - kx[None, :, None] * 2.0 ** -23)).float()
    else:
        raise ValueError(kind)
    q, w = matching_q(F, D, partner, wl)
    return X, q, w, partner


def z_column_case(kind, S, D, col, seed):
    """One example whose rows are nonzero in column `col` only, so z_ij = x_i[col] · x_j[col] (the
    a of the pair is the row with the smaller index). kind "few": full-mantissa random values;
    "trunc": ±2^e (1 + 2^-7 − 64 · 2^-23), the trunc_operands class with ka = kb = 64 for every
    pair. q is small and random, so the head stays well inside the clip. Returns (X [1, F, D], q,
    x [F])."""
    F = S + 1
    g = torch.Generator().manual_seed(seed * 1000 + col)
    if kind == "few":
        x = (torch.randn(F, generator=g).double() * _signs_scales((F,), g, -2, 2).abs()).float()
    else:
        x = (_signs_scales((F,), g, -2, 2) * (1 + 2.0 ** -7 - 64 * 2.0 ** -23)).float()
    X = torch.zeros(1, F, D)
    X[0, :, col] = x
    q = torch.cat([torch.randn(F * (F - 1) // 2, generator=g) * 0.002, torch.zeros(D)])
    iu = torch.triu_indices(F, F, 1)
    h = float((x.double()[iu[0]] * x.double()[iu[1]] * q[:iu.shape[1]].double()).sum())
    assert abs(h) < 8
    return X, q, x


Z_PROBE_LAUNCHES = {128: 30, 64: 80}


def z_probe_case(S, D, t):
    """Launch t of the probe walk: the fields are matched in pairs (matchings(F)[t % 3]) and pair
    number p has its two rows nonzero in a column of its own, (t + 9 p) % D (D = 128) or
    (t + 5 p) % D (D = 64), holding a probe pair of product type (t + 2 p) % 6: that z is the exact
    probe product, every other z an exact zero. Returns (X [1, F, D], q, pairs [(i, j, col,
    type name)])."""
    F = S + 1
    partner = matchings(F)[t % 3]
    step = 9 if D == 128 else 5
    X = torch.zeros(1, F, D, dtype=torch.float64)
    pairs = []
    p = 0
    for i in range(F):
        j = partner[i]
        if j < i:
            continue
        col = (t + step * p) % D
        name = ORDER[(t + 2 * p) % 6]
        sa, sb = _VARIANTS[(t // 6 + p) % 4]            # the variants with |a·b| near 1
        X[0, i, col] = _P[name][0] * sa
        X[0, j, col] = _P[name][1] * sb
        pairs.append((i, j, col, name))
        p += 1
    assert len({c for _, _, c, _ in pairs}) == len(pairs)
    g = torch.Generator().manual_seed(t)
    q = torch.cat([torch.randn(F * (F - 1) // 2, generator=g) * 0.05, torch.zeros(D)])
    return X.float(), q, pairs


def int_train_case(S, D, B, seed):
    """Integer-valued X (|v| <= 15, dense in D and F) and 0 / ±1 pair weights (all pairs, a third
    of them zero): U and Z are integers below 2^24, exact in any order. c cancels example 0's
    Σ q·z (an integer the fp32 head sums exactly), so at batch 1 the head is 0, y = 1/2 and
    G != 0. Returns (X, q, c)."""
    F = S + 1
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-15, 16, (B, F, D), generator=g).float()
    nz = F * (F - 1) // 2
    q = torch.cat([torch.randint(-1, 2, (nz,), generator=g).float(), torch.zeros(D)])
    iu = torch.triu_indices(F, F, 1)
    Z = X[0].double() @ X[0].double().T
    z = Z[iu[0], iu[1]]
    assert float((z.abs() * q[:nz].abs().double()).sum()) < 2 ** 24
    return X, q, -float((z * q[:nz].double()).sum())


def pair_weights(q, F):
    """S = M + Mᵀ [F, F] (float64) from q's pair weights."""
    iu = torch.triu_indices(F, F, 1)
    M = torch.zeros(F, F, dtype=torch.float64)
    M[iu[0], iu[1]] = q[:iu.shape[1]].double()
    return M + M.T


def np_i32(t):
    """The bits of an fp32 tensor as an int32 numpy array (for exact comparisons; NaN-safe)."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy()
