"""The DIEN aux-loss kernels (csrc/dien_aux.hip) and the valid-row products (csrc/dien_proj.hip)
at their tile, dispatch, count and persistent-loop edges. Cases, masks and float64 references come
from tests/dien_rows_edges.py, whose properties tests/test_dien_rows_edges_cpu.py proves.

1  rs_valid_rows bit-exact against np.flatnonzero;
2  rs_masked_proj / _dx / _dx_acc / _wgrad against float64 on the listed rows, each element within
   the fp32 fma chain's worst case (n + 1)·2^-24·Σ|a·b|, and their exact contracts (untouched
   rows and padding columns, zeros, the addend's bits, determinism);
3  rs_dien_aux_fwd / _bwd / _bwd_acc against oracle.dien.aux_loss under float64 autograd, per
   example within τ·(|ref| + the example's largest) and τ·Σ_b|g_b| for the parameter gradients,
   τ = 4·ρ32 (ρ32: the same oracle in fp32, pooled over the case list), and their exact contracts
   (zero rows, acc_hidden, batch position, the NaN pattern of an example without a valid row);
4  the fused InterestExtract node bit-identical to the GRU followed by the aux loss.
"""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from recommender_amd.dien import layers as DL
from tests import dien_rows_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def st():
    return L.stream_ptr(DEV)


def sentinel(*shape):
    """A buffer no kernel result looks like: 1000.5 + (i mod 251)."""
    n = int(np.prod(shape))
    return (torch.arange(n, device=DEV) % 251 + 1000.5).to(torch.float32).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def valid_rows(m):
    """rs_valid_rows on a device mask [R] with idx prefilled: (idx [max(R, 1)], count [1])."""
    R = m.numel()
    idx = torch.full((max(R, 1),), E.VR_SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = L.scratch(L.lib().rs_valid_rows_workspace_size(R), idx.device)
    L.call("rs_valid_rows", L.ptr(m) if R else None, R, L.ptr(idx), L.ptr(cnt), L.ptr(ws),
           ws.numel(), st())
    return idx, cnt


# ---- 1. the valid-row list ---------------------------------------------------------------------
@pytest.mark.parametrize("R", E.VR_RS)
def test_valid_rows_bit_exact(R):
    rng = np.random.default_rng(R)
    for kind in E.VR_KINDS:
        m = E.vr_mask(kind, R, rng)
        idx, cnt = valid_rows(dev(m))
        ref = E.valid_rows_ref(m)
        n = int(cnt.item())
        got = host(idx)
        assert n == len(ref), (kind, n, len(ref))
        assert np.array_equal(got[:n], ref), kind
        assert (got[n:] == E.VR_SENTINEL).all(), f"{kind}: idx written past the count"


def test_valid_rows_empty():
    idx, cnt = valid_rows(torch.empty(0, dtype=torch.uint8, device=DEV))
    assert int(cnt.item()) == 0 and int(idx.item()) == E.VR_SENTINEL


# ---- 2. the products ---------------------------------------------------------------------------
def _within(got, ref, bound, msg):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ok = err <= bound
    assert ok.all(), (f"{msg}: {int((~ok).sum())} / {ok.size} off, worst err/bound "
                      f"{E.worst_ratio(err, bound):.3g}")


@pytest.mark.parametrize("K,N", E.PROJ_PAIRS)
def test_masked_proj(K, N):
    rng = np.random.default_rng([1, K, N])
    W = rng.standard_normal((K, N)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    Wd, bd = dev(W), dev(b)
    call = 0
    for count in E.PROJ_COUNTS:
        for R in sorted({max(count, 1), count + 37}):
            call += 1
            ldx, ldy = K + 3 * (call % 2), N + 5 * (call // 2 % 2)
            bias = None if call % 3 == 0 else b
            m = E.count_mask(R, count, rng, values=(1, 2, 255))
            xb = rng.standard_normal((R, ldx)).astype(np.float32)
            y = sentinel(R, ldy)
            y0 = host(y)
            idx, cnt = valid_rows(dev(m))
            xd = dev(xb)
            L.call("rs_masked_proj", L.ptr(xd), ldx, L.ptr(Wd),
                   None if bias is None else L.ptr(bd), L.ptr(idx), L.ptr(cnt), R, K, N, L.ptr(y),
                   ldy, st())
            got = host(y)
            rows = E.valid_rows_ref(m)
            msg = f"proj K={K} N={N} count={count} R={R} ldx={ldx} ldy={ldy} bias={bias is not None}"
            ref, bound = E.proj_ref(xb[:, :K], W, bias, rows)
            _within(got[rows, :N], ref, bound, msg)
            assert np.array_equal(got[m == 0], y0[m == 0]), msg + ": an unlisted row was written"
            assert np.array_equal(got[:, N:], y0[:, N:]), msg + ": a padding column was written"


@pytest.mark.parametrize("N", E.DX_NS)
@pytest.mark.parametrize("K", E.DX_KS)
def test_masked_dx_and_dx_acc(K, N):
    rng = np.random.default_rng([2, K, N])
    W = rng.standard_normal((K, N)).astype(np.float32)
    Wd = dev(W)
    call = 0
    for count in E.DX_COUNTS:
        for R in E.dx_rs(count):
            call += 1
            ldd, lddx, ldadd = N + call % 2, K + 3 * (call // 2 % 2), K + 2 * (call // 4 % 2)
            m = E.count_mask(R, count, rng, values=(1, 2, 255))
            d = rng.standard_normal((R, ldd)).astype(np.float32)
            add = rng.standard_normal((R, ldadd)).astype(np.float32)
            md, dd, ad = dev(m), dev(d), dev(add)
            idx, cnt = valid_rows(md)
            rows = E.valid_rows_ref(m)
            for with_add in (False, True):
                dx = sentinel(R + 16, lddx)  # 16 rows past R: a wave's 16-row group ends there
                dx0 = host(dx)
                if with_add:
                    L.call("rs_masked_dx_acc", L.ptr(dd), ldd, L.ptr(Wd), L.ptr(md), L.ptr(idx),
                           L.ptr(cnt), R, K, N, L.ptr(ad), ldadd, L.ptr(dx), lddx, st())
                else:
                    L.call("rs_masked_dx", L.ptr(dd), ldd, L.ptr(Wd), L.ptr(md), L.ptr(idx),
                           L.ptr(cnt), R, K, N, L.ptr(dx), lddx, st())
                msg = (f"dx K={K} N={N} count={count} R={R} ldd={ldd} lddx={lddx} ldadd={ldadd} "
                       f"add={with_add}")
                full = host(dx)
                assert np.array_equal(full[R:], dx0[R:]), msg + ": a row past R was written"
                got, dx0 = full[:R], dx0[:R]
                ref, bound = E.dx_ref(d[:, :N], W, add[:, :K] if with_add else None, rows)
                _within(got[rows, :K], ref, bound, msg)
                want = add[m == 0][:, :K] if with_add else np.zeros((R - count, K), np.float32)
                assert np.array_equal(bits(got[m == 0][:, :K]), bits(want)), msg + ": masked rows"
                assert np.array_equal(got[:, K:], dx0[:, K:]), msg + ": a padding column was written"


@pytest.mark.parametrize("K,N", E.WGRAD_PAIRS)
def test_masked_wgrad(K, N):
    rng = np.random.default_rng([3, K, N])
    Rmax = max(E.WGRAD_COUNTS) + 300
    lda, ldd = K + 2, N + 3
    Ab = rng.standard_normal((Rmax, lda)).astype(np.float32)
    Db = rng.standard_normal((Rmax, ldd)).astype(np.float32)
    Abd, Dbd = dev(Ab), dev(Db)
    for i, count in enumerate(E.WGRAD_COUNTS):
        R = count + (300 if count > 100 else 29)
        m = E.count_mask(R, count, rng, values=(1, 2, 255))
        vr = valid_rows(dev(m))
        sums = i % 3 != 2
        C, s = DL._masked_wgrad(Abd[:R, :K], 0, Dbd[:R, :N], vr, sums=sums)
        rows = E.valid_rows_ref(m)
        rC, rs, bC, bs = E.wgrad_ref(Ab[:R, :K], Db[:R, :N], rows)
        msg = f"wgrad K={K} N={N} count={count} R={R} per={E.wgrad_per(count)}"
        _within(host(C), rC, bC, msg)
        if sums:
            _within(host(s), rs, bs, msg + " column sums")
        else:
            assert s is None
        if count == 0:
            assert (C == 0).all() and (s == 0).all(), msg
        if count in (0, 17, 65, 8193):  # a second run: the same bits
            C2, s2 = DL._masked_wgrad(Abd[:R, :K], 0, Dbd[:R, :N], vr, sums=sums)
            assert torch.equal(C, C2) and (s is None or torch.equal(s, s2)), msg + ": not deterministic"


@pytest.mark.parametrize("K,N", [(36, 108), (64, 192), (20, 109)])
@pytest.mark.parametrize("B,T", [(6, 9), (40, 17)])
def test_masked_wgrad_shifted_and_strided(K, N, B, T):
    """shift_L = T: listed first steps take a zero A row, a listed row whose predecessor is
    unlisted still reads it. A and D are column views of wider buffers (lda / ldd beyond the
    width), as the AUGRU's [R, 3H] and [R, 4H] blocks."""
    rng = np.random.default_rng([4, K, N, B])
    R = B * T
    m = E.shift_mask(B, T, rng)
    vr = valid_rows(dev(m.reshape(-1)))
    rows = E.valid_rows_ref(m)
    Ab = rng.standard_normal((R, 4 * K)).astype(np.float32)
    Db = rng.standard_normal((R, N + 2 * K)).astype(np.float32)
    A, D = Ab[:, 3 * K:], Db[:, K:K + N]
    Ad, Dd = dev(Ab)[:, 3 * K:], dev(Db)[:, K:K + N]
    assert DL._ld(Ad) == 4 * K and DL._ld(Dd) == N + 2 * K
    for shift in (T, 0):
        C, s = DL._masked_wgrad(Ad, shift, Dd, vr)
        rC, rs, bC, bs = E.wgrad_ref(A, D, rows, shift)
        _within(host(C), rC, bC, f"wgrad shift={shift} K={K} N={N} R={R}")
        _within(host(s), rs, bs, f"column sums shift={shift}")


def test_product_argument_errors_launch_nothing():
    """K = 65, N = 193, ldx < K and a too-small wgrad workspace are refused, outputs untouched."""
    R, K, N = 8, 36, 108
    m = torch.ones(R, dtype=torch.uint8, device=DEV)
    idx, cnt = valid_rows(m)
    x, d = sentinel(R, 200), sentinel(R, 200)
    W = sentinel(65, 193)
    out = sentinel(R, 200)
    out0 = out.clone()
    ws = L.scratch(L.lib().rs_masked_wgrad_workspace_size(K, N), out.device)
    for k, n in ((65, N), (K, 193)):
        with pytest.raises(L.RecsysError):
            L.call("rs_masked_proj", L.ptr(x), 200, L.ptr(W), None, L.ptr(idx), L.ptr(cnt), R, k, n,
                   L.ptr(out), 200, st())
        with pytest.raises(L.RecsysError):
            L.call("rs_masked_dx", L.ptr(d), 200, L.ptr(W), L.ptr(m), L.ptr(idx), L.ptr(cnt), R, k,
                   n, L.ptr(out), 200, st())
        with pytest.raises(L.RecsysError):
            L.call("rs_masked_dx_acc", L.ptr(d), 200, L.ptr(W), L.ptr(m), L.ptr(idx), L.ptr(cnt), R,
                   k, n, L.ptr(x), 200, L.ptr(out), 200, st())
        with pytest.raises(L.RecsysError):
            L.call("rs_masked_wgrad", L.ptr(x), 200, 0, L.ptr(d), 200, L.ptr(idx), L.ptr(cnt), k, n,
                   L.ptr(out), None, L.ptr(ws), ws.numel(), st())
    with pytest.raises(L.RecsysError):
        L.call("rs_masked_proj", L.ptr(x), K - 1, L.ptr(W), None, L.ptr(idx), L.ptr(cnt), R, K, N,
               L.ptr(out), 200, st())
    with pytest.raises(L.RecsysError):
        L.call("rs_masked_wgrad", L.ptr(x), 200, 0, L.ptr(d), 200, L.ptr(idx), L.ptr(cnt), K, N,
               L.ptr(out), None, L.ptr(ws), ws.numel() - 256, st())
    torch.cuda.synchronize()
    assert torch.equal(out, out0)


# ---- 3. the aux loss ---------------------------------------------------------------------------
def to_dev(d):
    return {k: dev(v) for k, v in d.items()}


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _aux_args(t):
    B, Lh, H = t["hidden"].shape
    return ([L.ptr(t[n]) for n in ("hidden", "pos", "neg", "mask")] + [B, Lh, H, H]
            + [L.ptr(t[n]) for n in E.AUX_PARAMS])


def n_param(H):
    return 2 * H * 80 + 80 + 80 * 40 + 40 + 40 + 1


def k_aux_fwd(t):
    aux = nan(t["hidden"].shape[0])
    L.call("rs_dien_aux_fwd", *_aux_args(t), L.ptr(aux), st())
    return aux


def k_aux_bwd(t, upstream=None, plain=False):
    """rs_dien_aux_bwd_acc with acc_hidden = 0 (outputs prefilled with NaN) or, given `upstream`,
    acc_hidden = 1 on a copy of it; plain: the rs_dien_aux_bwd entry point."""
    B, Lh, H = t["hidden"].shape
    dh = nan(B, Lh, H) if upstream is None else upstream.clone()
    dp, dn, dpar = nan(B, Lh, H), nan(B, Lh, H), nan(n_param(H))
    ws = L.scratch(L.lib().rs_dien_aux_workspace_size(B, Lh, H, H), dh.device)
    if plain:
        L.call("rs_dien_aux_bwd", *_aux_args(t), L.ptr(t["daux"]), L.ptr(dh), L.ptr(dp), L.ptr(dn),
               L.ptr(dpar), L.ptr(ws), ws.numel(), st())
    else:
        L.call("rs_dien_aux_bwd_acc", *_aux_args(t), L.ptr(t["daux"]), L.ptr(dh),
               0 if upstream is None else 1, L.ptr(dp), L.ptr(dn), L.ptr(dpar), L.ptr(ws),
               ws.numel(), st())
    return dict(dhidden=dh, dpos=dp, dneg=dn, dparams=dpar)


def split_params(dpar, H):
    out, o = {}, 0
    for n, shape in zip(E.AUX_PARAMS, ((2 * H, 80), (80,), (80, 40), (40,), (40, 1), (1,))):
        k = int(np.prod(shape))
        out["d" + n] = dpar[o:o + k].reshape(shape)
        o += k
    assert o == dpar.numel()
    return out


def aux_run(t):
    """Forward and backward (acc_hidden = 0) on device inputs: numpy {aux, dhidden, ..., dW1, ..}
    and the raw device outputs."""
    aux = k_aux_fwd(t)
    g = k_aux_bwd(t)
    got = dict(aux=host(aux), **{n: host(g[n]) for n in ("dhidden", "dpos", "dneg")})
    got.update({n: host(v) for n, v in split_params(g["dparams"], t["hidden"].shape[2]).items()})
    return got, aux, g


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_RATIOS = {}


@pytest.fixture(scope="module")
def tau():
    """{"pooled": 4·ρ32, tensor: 4·ρ32 of that tensor}, ρ32 the fp32 oracle's worst ratio over the
    whole case list (computed once). The pooled figure is the bound; the per-tensor ones (each
    at most the pooled one) are held too, so that the per-example outputs are not judged by the
    parameter gradients' figure."""
    specs = E.AUX_CASES + E.persistent_cases(cus())
    rho = E.rho32(specs)
    by = E.rho32_by_tensor(specs)
    print(f"\n  rho32 over {len(specs)} cases ({cus()} CUs): {rho:.4g}  tau = {4 * rho:.4g}")
    print("  rho32 by tensor: " + " ".join(f"{n}={r:.3g}" for n, r in by.items()))
    assert 0 < rho < np.inf and max(by.values()) == rho
    return dict({n: 4 * r for n, r in by.items()}, pooled=4 * rho)


def check_aux_case(spec, tau_):
    d, r64, mag, ctl = E.aux_case(spec)
    t = to_dev(d)
    got, aux, g = aux_run(t)
    ratios = E.aux_ratios(got, r64, mag)
    worst = max(ratios, key=ratios.get)
    for n, r in ratios.items():
        _RATIOS[n] = max(_RATIOS.get(n, 0.0), r)
    print(f"  aux{spec}: kernel worst ratio {ratios[worst]:.4g} ({worst}), control "
          f"{max(ctl.values()):.4g}, tau {tau_['pooled']:.4g}")
    print("    kernel/control by tensor: "
          + " ".join(f"{n}={r:.3g}/{ctl[n]:.3g}" for n, r in ratios.items()))
    print("    kernel worst so far: " + " ".join(f"{n}={r:.3g}" for n, r in _RATIOS.items()))
    assert max(ctl.values()) <= tau_["pooled"] / 4
    bad = {n: f"{r:.3g} > {tau_[n]:.3g}" for n, r in ratios.items() if not r <= tau_[n]}
    assert not bad, f"aux{spec}: ratios above 4·rho32: {bad}"
    return d, t, got, aux, g


def check_zero_rows(d, g, msg):
    """Row 0 of dpos / dneg, row L - 1 of dhidden and the rows of masked steps: exactly 0."""
    v = d["mask"] != 0
    B, Lh = v.shape
    dh, dp, dn = (host(g[n]) for n in ("dhidden", "dpos", "dneg"))
    assert (dp[:, 0] == 0).all() and (dn[:, 0] == 0).all(), msg + ": row 0 of dpos / dneg"
    assert (dh[:, Lh - 1] == 0).all(), msg + ": dhidden[:, L-1]"
    assert (dh[:, :-1][~v[:, 1:]] == 0).all(), msg + ": dhidden of a masked step"
    assert (dp[:, 1:][~v[:, 1:]] == 0).all() and (dn[:, 1:][~v[:, 1:]] == 0).all(), \
        msg + ": dpos / dneg of a masked step"


def dead_rows(mask):
    """bool [B, L]: hidden rows in backward tiles that are not live."""
    B, Lh = mask.shape
    live = set(E.aux_live_items(mask))
    out = np.ones((B, Lh), bool)
    for i in live:
        tile, b = divmod(i, B)
        out[b, 16 * tile:16 * tile + 16] = False
    return out


def check_acc_hidden(d, t, g, msg):
    """acc_hidden = 1 on a random upstream: rows of tiles without a valid step keep the upstream's
    bits, every other row is upstream + (the acc_hidden = 0 result) — one fp32 addition, which
    commutes; dpos, dneg and the parameter gradients are the same bits as without it."""
    B, Lh, H = d["hidden"].shape
    up = dev(np.random.default_rng(B * Lh).standard_normal((B, Lh, H)).astype(np.float32))
    a = k_aux_bwd(t, upstream=up)
    dead = dev(dead_rows(d["mask"]))
    assert torch.equal(a["dhidden"][dead], up[dead]), msg + ": a dead tile's rows were touched"
    assert torch.equal(a["dhidden"], up + g["dhidden"]), msg + ": not upstream + the aux part"
    for n in ("dpos", "dneg", "dparams"):
        assert torch.equal(a[n], g[n]), f"{msg}: {n} differs between acc_hidden = 1 and 0"


@pytest.mark.parametrize("spec", E.AUX_CASES, ids=lambda s: "-".join(map(str, s)))
def test_aux_vs_float64(spec, tau):
    d, t, got, aux, g = check_aux_case(spec, tau)
    msg = f"aux{spec}"
    check_zero_rows(d, g, msg)
    check_acc_hidden(d, t, g, msg)
    p = k_aux_bwd(t, plain=True)  # the rs_dien_aux_bwd entry point: the same bits
    for n in p:
        assert torch.equal(p[n], g[n]), f"{msg}: rs_dien_aux_bwd {n}"


@pytest.mark.parametrize("which", ["backward", "forward", "odd"])
def test_aux_persistent_loops(which, tau):
    """More live pairs than blocks (backward: >= 3 rounds for some blocks, one-ahead fetch and
    two-ahead item_of), more example pairs than the forward grid with an odd B, and an odd
    live-item count whose last pair (one item) comes in a block's third round."""
    n = cus()
    spec = E.persistent_cases(n)[("backward", "forward", "odd").index(which)]
    H, B, Lh, _ = spec
    if which == "backward":
        assert E.bwd_rounds(2 * B, n)[0] >= 3
    elif which == "odd":
        assert B % 2 == 1 and E.bwd_rounds(B, n)[0] >= 3
    else:
        assert E.fwd_rounds(B, n)[:2] == (2, 1) and B % 2 == 1
    d, t, got, aux, g = check_aux_case(spec, tau)
    check_zero_rows(d, g, f"aux{spec}")
    check_acc_hidden(d, t, g, f"aux{spec}")
    g2 = k_aux_bwd(t)
    assert torch.equal(g2["dparams"], g["dparams"]), "parameter gradients differ between two runs"


@pytest.mark.parametrize("H,Lh,kind", [(36, 18, "random"), (16, 34, "bytes"), (36, 33, "post")])
def test_aux_batch_position_is_bit_exact(H, Lh, kind):
    """aux[b] and the three input-gradient blocks of an example are the same bits alone (B = 1),
    first of 5 and last of 5."""
    d = E.aux_inputs(H, 5, Lh, kind, seed=9)
    per = E.AUX_IN + ("mask", "daux")

    def run(order):
        t = to_dev({k: (np.ascontiguousarray(v[order]) if k in per else v) for k, v in d.items()})
        got, aux, g = aux_run(t)
        return got

    for e in (0, 2):
        others = [b for b in range(5) if b != e]
        alone, first, last = run([e]), run([e] + others), run(others + [e])
        for n in E.AUX_OUT:
            assert np.array_equal(bits(alone[n][0]), bits(first[n][0])), (n, e, "first of 5")
            assert np.array_equal(bits(alone[n][0]), bits(last[n][4])), (n, e, "last of 5")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("H,Lh", [(36, 18), (36, 17), (16, 34), (36, 2)])
def test_aux_nan_pattern(H, Lh, acc, tau):
    """Example 2 of 5 has no valid aux row (Σ mask[b, 1:] = 0): isnan of every output equals isnan
    of the float64 reference — NaN in dhidden[b, :L-1], dpos[b, 1:], dneg[b, 1:], aux[b] and
    every parameter gradient; dhidden[b, L-1], dpos[b, 0] and dneg[b, 0] are exactly 0 (the
    upstream's bits under acc_hidden); the other examples stay finite and within bound."""
    d = E.nan_case(H, Lh)
    r64 = E.aux_eval(d, torch.float64)
    t = to_dev(d)
    B = 5
    up = dev(np.random.default_rng(Lh).standard_normal((B, Lh, H)).astype(np.float32))
    aux = host(k_aux_fwd(t))
    g = k_aux_bwd(t, upstream=up if acc else None)
    got = dict(aux=aux, **{n: host(g[n]) for n in ("dhidden", "dpos", "dneg")})
    got.update({n: host(v) for n, v in split_params(g["dparams"], H).items()})
    for n, r in r64.items():  # a finite upstream does not move the pattern
        assert np.array_equal(np.isnan(got[n].reshape(r.shape)), np.isnan(r)), \
            f"{n}: NaN pattern differs from the reference (acc_hidden = {acc})"
    ex = host(g["dhidden"])[2]
    fin = ~np.isnan(r64["dhidden"][2])
    assert fin[Lh - 1].all() and fin.sum() == H
    if acc:
        assert np.array_equal(bits(ex[fin]), bits(host(up)[2][fin])), \
            "dhidden[b, L-1] of the empty example is not the upstream's bits"
    else:
        assert (ex[fin] == 0).all(), "dhidden[b, L-1] of the empty example"
    assert (got["dpos"][2, 0] == 0).all() and (got["dneg"][2, 0] == 0).all()
    keep = [0, 1, 3, 4]
    if not acc:  # under acc_hidden the aux part is upstream-rounded: bit-checked in the case tests
        for n in E.AUX_OUT:
            assert np.isfinite(got[n][keep]).all(), n
            r = E.worst_ratio(np.abs(got[n][keep].astype(np.float64) - r64[n][keep]),
                              E.example_scale(r64[n][keep]))
            print(f"  nan case H={H} L={Lh} {n}: ratio {r:.4g}")
            assert r <= tau[n], (n, r, tau[n])
    else:
        assert np.isfinite(host(g["dhidden"])[keep]).all()
        plain = k_aux_bwd(t)
        assert torch.equal(torch.nan_to_num(g["dhidden"], nan=7e33),
                           torch.nan_to_num(up + plain["dhidden"], nan=7e33))


def test_aux_argument_errors():
    """L = 1, widths that are no multiple of 4 and a too-small workspace raise; (20, 20) is not
    built (RS_E_UNSUPPORTED); B = 0 returns cleanly with dparams all 0."""
    d = E.aux_inputs(36, 2, 4, "all")
    t = to_dev(d)
    B, Lh, H = 2, 4, 36

    def bwd(args, ws_cut=0, Hn=H):
        dh, dp, dn, dpar = nan(B, Lh, 40), nan(B, Lh, 40), nan(B, Lh, 40), sentinel(n_param(40))
        ws = L.scratch(L.lib().rs_dien_aux_workspace_size(B, Lh, 36, 36) + 4096, dh.device)
        L.call("rs_dien_aux_bwd", *args, L.ptr(t["daux"]), L.ptr(dh), L.ptr(dp), L.ptr(dn),
               L.ptr(dpar), L.ptr(ws), ws.numel() - ws_cut, st())
        return dpar

    def args(B_, L_, H_, E_):
        a = _aux_args(t)
        a[4:8] = [B_, L_, H_, E_]
        return a

    aux = nan(B)
    for bad in (args(B, 1, H, H), args(B, Lh, 18, 18), args(B, Lh, 34, 38)):
        with pytest.raises(L.RecsysError):
            L.call("rs_dien_aux_fwd", *bad, L.ptr(aux), st())
        with pytest.raises(L.RecsysError):
            bwd(bad)
    for fn in (lambda: L.call("rs_dien_aux_fwd", *args(B, Lh, 20, 20), L.ptr(aux), st()),
               lambda: bwd(args(B, Lh, 20, 20))):
        with pytest.raises(L.RecsysError, match=f"status {L.RS_E_UNSUPPORTED}"):
            fn()
    with pytest.raises(L.RecsysError):
        bwd(_aux_args(t), ws_cut=4096 + 1)  # one byte short
    torch.cuda.synchronize()
    assert torch.isnan(aux).all()
    # B = 0 (the pointers stay those of real buffers: a null pointer is refused before B is read)
    L.call("rs_dien_aux_fwd", *args(0, Lh, H, H), L.ptr(aux), st())
    dh = nan(1, Lh, H)
    dpar = sentinel(n_param(H))
    ws = L.scratch(L.lib().rs_dien_aux_workspace_size(0, Lh, H, H), dh.device)
    L.call("rs_dien_aux_bwd", *args(0, Lh, H, H), L.ptr(t["daux"]), L.ptr(dh), L.ptr(dh),
           L.ptr(dh), L.ptr(dpar), L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    assert (dpar == 0).all() and torch.isnan(aux).all() and torch.isnan(dh).all()


# ---- 4. the fused node equals its two halves ---------------------------------------------------
@pytest.mark.parametrize("B,Lh,kind", E.FUSED_CASES)
def test_interest_extract_node_equals_gru_then_aux(B, Lh, kind):
    """InterestExtract.forward (_InterestExtractFn: rs_dien_aux_bwd_acc and rs_masked_dx_acc in
    place) against the same module's GRU followed by compute_auxiliary_loss, on the same
    parameters, inputs and upstream (dhidden, daux): every output and gradient bit-identical —
    the fused backward only moves two two-addend fp32 additions into the kernels."""
    H = 36
    gen = torch.Generator(device=DEV).manual_seed(B + Lh)
    ie = DL.InterestExtract(H, H, device=DEV, generator=gen)
    with torch.no_grad():
        ie.gru.bias.copy_(torch.randn(ie.gru.bias.shape, generator=gen, device=DEV) * 0.2)
        for l in ie.auxiliary_net.layers:
            l.bias.copy_(torch.randn(l.bias.shape, generator=gen, device=DEV) * 0.2)
    rng = np.random.default_rng([B, Lh])
    if kind == "post":
        lens = rng.integers(2, Lh + 1, B)
        m = np.arange(Lh)[None] < lens[:, None]
    else:
        m = rng.random((B, Lh)) < 0.5
        m[:, 1] = True
    mask = dev(m)
    x = [dev((rng.standard_normal((B, Lh, H)) * 0.5).astype(np.float32)) for _ in range(2)]
    dhid = dev(rng.standard_normal((B, Lh, H)).astype(np.float32))
    daux = dev(rng.standard_normal(B).astype(np.float32))
    params = list(ie.parameters())
    names = ["dpos", "dneg"] + ["d" + n for n, _ in ie.named_parameters()]

    def run(fused):
        pos, neg = (t.clone().requires_grad_(True) for t in x)
        if fused:
            hid, aux = ie((pos, neg), mask=mask)
            assert "_InterestExtractFn" in type(hid.grad_fn).__name__, "not the fused node"
        else:
            hid = ie.gru(pos, mask=mask)
            aux = ie.compute_auxiliary_loss((hid, pos, neg), mask=mask)
            assert "_AuxLossFn" in type(aux.grad_fn).__name__
        g = torch.autograd.grad([hid, aux], [pos, neg] + params, [dhid.clone(), daux.clone()])
        return dict(hidden=hid.detach(), aux=aux.detach(), **dict(zip(names, g)))

    a, b = run(True), run(False)
    assert len(a) == 2 + 2 + 9
    for n in a:
        assert torch.isfinite(a[n]).all(), n
        assert torch.equal(a[n], b[n]), (f"{n}: fused and unfused differ, max "
                                         f"{float((a[n] - b[n]).abs().max()):.3g}")
