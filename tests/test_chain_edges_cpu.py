"""The cases of tests/test_chain_edges_gpu.py have the property their name claims (which kernel
of csrc/dense.hip they take, idle threads, chunk and segment counts), the references of
tests/chain_edges.py agree with float64 autograd of the layer-by-layer chain, the integer inputs
meet the condition that makes their GPU comparison exact, and the Gaussian bounds hold for the
kernels' summation order replayed in fp32 — all without a GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import chain_edges as E

F32 = np.float32


def axis(cases, name):
    return {getattr(c, name) for c in cases}


# ---- 1. rs_chain_reduce: regimes ---------------------------------------------------------------
def test_reduce_cases_cover_every_axis():
    cs = E.REDUCE_CASES
    assert len(set(cs)) == len(cs) and 45 <= len(cs) <= 55
    by = {k: [c for c in cs if E.case_regime(c)["kernel"] == k] for k in ("vec", "quad", "outer")}
    assert axis(by["vec"], "n0") == set(E.VEC_N0) and axis(by["vec"], "pad") == set(E.VEC_PADS)
    assert axis(by["quad"], "nl") == set(E.QUAD_NL)
    assert axis(by["outer"], "nl") == set(E.OUTER_NL) | {8, 64}
    want_b = set(E.REDUCE_SMALL_B) | set(E.REDUCE_LARGE_B)
    for k, group in by.items():
        assert axis(group, "B") == want_b, k
        assert any(c.pad for c in group), f"{k}: no case with ldx > n0"
        narrowest = min(c.n0 * c.nl for c in group)
        assert all(c.n0 * c.nl == narrowest for c in group if c.B >= 4096), k
        if k != "vec":
            assert axis(group, "n0") == set(E.NARROW_N0), k
            assert {E.case_regime(c)["n0max"] for c in group} == {16, 32}
            assert {E.case_regime(c)["n0max"] for c in group if c.n0 in (17, 32)} == {32}


def test_reduce_vec_regimes():
    r = {n0: E.reduce_regime(n0, 1) for n0 in (4, 8, 12, 512, 516, 1024)}
    assert (r[4]["cgp"], r[4]["P"], r[4]["idle"]) == (1, 256, 0)
    assert (r[8]["cgp"], r[8]["P"]) == (2, 128)
    assert (r[12]["cgp"], r[12]["P"], r[12]["idle"]) == (4, 64, 64)  # one dead group of 64 phases
    assert (r[512]["cgp"], r[512]["P"], r[512]["idle"]) == (128, 2, 0)
    assert (r[516]["cgp"], r[516]["P"], r[516]["idle"]) == (256, 1, 127)  # 127 dead groups
    assert (r[1024]["cgp"], r[1024]["P"], r[1024]["idle"]) == (256, 1, 0)
    # P = 256 phases over a 128-row chunk: phases 128.. see no row
    assert r[4]["P"] > E.CHUNK


def test_reduce_quad_and_outer_regimes():
    q = {nl: E.reduce_regime(1, nl) for nl in E.QUAD_NL}
    assert all(v["kernel"] == "quad" for v in q.values())
    assert {nl: (v["P"], v["idle"]) for nl, v in q.items()} == {
        4: (256, 0), 12: (85, 1), 64: (16, 0), 200: (5, 6), 256: (4, 0)}
    o = {nl: E.reduce_regime(1, nl) for nl in E.OUTER_NL}
    assert all(v["kernel"] == "outer" for v in o.values())
    assert {nl: (v["P"], v["idle"]) for nl, v in o.items()} == {
        2: (128, 0), 3: (64, 64), 5: (32, 96), 129: (1, 127), 255: (1, 1)}
    assert E.reduce_regime(16, 4)["n0max"] == 16 and E.reduce_regime(17, 4)["n0max"] == 32
    assert E.reduce_regime(16, 3)["n0max"] == 16 and E.reduce_regime(17, 3)["n0max"] == 32


def test_each_misaligned_buffer_alone_routes_to_outer():
    mis = [c for c in E.REDUCE_CASES if c.dy_off or c.y_off or c.g_off]
    assert len(mis) == 6 and axis(mis, "nl") == {8, 64}
    for nl in (8, 64):
        offs = {(c.dy_off, c.y_off, c.g_off) for c in mis if c.nl == nl}
        assert offs == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
    for c in mis:
        assert E.reduce_regime(c.n0, c.nl)["kernel"] == "quad"
        assert E.case_regime(c)["kernel"] == "outer"
        if c.g_off:  # without g_out its alignment does not count
            assert E.case_regime(c, has_g=False)["kernel"] == "quad"


def test_fold_plans():
    f = {B: E.fold_plan(B) for B in (0, 1, 127, 128, 129, 4096, 4097, 8320)}
    assert f[0]["nchunks"] == 0
    assert [f[B]["nchunks"] for B in (1, 127, 128, 129)] == [1, 1, 1, 2]
    assert f[4096] == dict(nchunks=32, per=1, nseg=32, last=1)
    assert f[4097] == dict(nchunks=33, per=2, nseg=17, last=1)
    assert f[8320] == dict(nchunks=65, per=3, nseg=22, last=2)
    for B in range(1, 40 * E.CHUNK, 97):
        p = E.fold_plan(B)
        assert p["nseg"] <= E.KSEG and (p["nseg"] - 1) * p["per"] + p["last"] == p["nchunks"]
        assert 1 <= p["last"] <= p["per"]


def test_reduce_refusals_and_routing_predicates():
    ok = dict(n0=4, nl=1, ldx=4, act=0, B=5)
    assert E.reduce_accepts(**ok)
    for change in (dict(n0=33, nl=2, ldx=33), dict(nl=257), dict(n0=1028, ldx=1028), dict(n0=6, ldx=8),
                   dict(ldx=6), dict(x_off=1), dict(act=3), dict(act=1, has_y=False)):
        assert not E.reduce_accepts(**{**ok, **change}), change
    assert E.reduce_accepts(32, 256, 32, 2, 7) and E.reduce_accepts(1024, 1, 1024, 1, 7)
    assert E.nn_routes_fused(4, 1, 4) and E.nn_routes_fused(32, 2, 35)
    assert not E.nn_routes_fused(33, 2, 33) and not E.nn_routes_fused(4, 1, 4, x_off=1)
    assert not E.nn_routes_fused(6, 1, 8) and not E.nn_routes_fused(4, 1, 4, unit_stride=False)
    assert E.reduce_workspace_bytes(0, 4, 1) == (1 + 32) * 5 * 4 + 256
    assert E.reduce_workspace_bytes(129, 2, 3) == (2 + 32) * 9 * 4 + 256


def test_reduce_depth_is_the_codes_chain():
    vec4, quad12 = E.reduce_regime(4, 1), E.reduce_regime(1, 12)
    assert E.reduce_depth(vec4, 128) == 1 + 256 + 1 + 3 + 1 + 3
    assert E.reduce_depth(vec4, 8320) == 1 + 256 + 1 + 3 + 6 + 3
    assert E.reduce_depth(quad12, 129) == 2 + 85 + 1 + 3 + 1 + 3
    assert E.reduce_depth(E.reduce_regime(1, 129), 4097) == 128 + 1 + 1 + 3 + 5 + 3


# ---- 1b. rs_chain_reduce: inputs ---------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
def test_reduce_int_inputs_make_the_comparison_exact(act):
    """Σ_b |x·g| < 2^24 for every output: every partial sum in any order is an integer below
    2^24, so fp32 never rounds. Column 0 of x and g are positive: nothing cancels in A[0, :], s."""
    for c in E.REDUCE_CASES:
        x, dy, y = E.reduce_inputs(c, act, "int")
        out, G, mag = E.reduce_ref(x, dy, y, act, c.n0)
        assert mag.size == 0 or mag.max() < E.TWO24
        assert (out == np.rint(out)).all() and (x[:, :c.n0] == np.rint(x[:, :c.n0])).all()
        assert np.isnan(x[:, c.n0:]).all() and x.shape[1] == c.n0 + c.pad
        assert (x[:, 0] >= 1).all() and (dy >= 1).all() and (dy <= 3).all() and (G >= 0).all()
        assert np.abs(x[:, :c.n0]).max(initial=0) <= 3
        if act == 1 and y.size >= 8:
            zero = y == 0
            assert (zero & np.signbit(y)).any() and (zero & ~np.signbit(y)).any() and (y > 0).any()
            assert (G[zero] == 0).all() and (G[~zero] == dy[~zero]).all()
        if act == 0:
            assert np.isnan(y).all()
        if c.B:  # a dropped or doubled row changes s and A[0, :]
            assert (out[-c.nl:] >= 0).all() and (mag[:c.nl] == out[:c.nl]).all()


@pytest.mark.parametrize("c", [E.RC(12, 1, 4, 129), E.RC(4, 1, 0, 4097), E.RC(17, 12, 3, 129),
                               E.RC(1, 4, 0, 4097), E.RC(16, 5, 1, 127), E.RC(1, 129, 0, 129)], ids=str)
def test_reduce_bound_holds_for_the_kernels_order_in_fp32(c):
    x, dy, y = E.reduce_inputs(c, 2, "gauss")
    out, G, mag = E.reduce_ref(x, dy, y, 2, c.n0)
    G32 = dy * (y * (F32(1) - y))
    assert (np.abs(G32 - G) <= E.SIGMOID_RTOL * np.abs(G)).all()
    reg = E.case_regime(c)
    emu = E.emulate_reduce(x, G32, c.n0, reg, c.B)
    bound = E.reduce_bound(mag, reg, c.B, 2)
    assert emu.dtype == F32 and (np.abs(emu - out) <= bound).all()
    assert (np.abs(emu - out) > 0).any()  # the emulation is a real fp32 evaluation
    # in integers the emulated order is exact, like the kernel's
    xi, dyi, yi = E.reduce_inputs(c, 1, "int")
    outi, Gi, _ = E.reduce_ref(xi, dyi, yi, 1, c.n0)
    assert np.array_equal(E.emulate_reduce(xi, Gi.astype(F32), c.n0, reg, c.B), outi.astype(F32))


# ---- 2. the references against float64 autograd of the layer-by-layer chain --------------------
def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def close(a, b, msg):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, msg
    assert np.abs(a - b).max(initial=0) <= 1e-11 * max(1.0, np.abs(b).max(initial=0)), msg


TORCH_ACT = (lambda v: v, torch.relu, torch.sigmoid)


@pytest.mark.parametrize("c", [E.CHAIN3_CASES[i] for i in (1, 4, 7, 11)], ids=str)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_top_chain_references_match_autograd(c, act):
    """y = act(((x·K1[rows] + b1)·K2 + b2)·K3 + b3), L = Σ dy·y in float64 autograd against
    reduce_ref → chain3_grads_ref (every gradient; the input gradient is G ⊗ p) and
    chain3_compose_ref → rowdot_ref (the forward)."""
    d = E.chain3_inputs(c, "gauss")
    rng = np.random.default_rng(c.n0 + act)
    B = 37
    x = rng.standard_normal((B, c.n0)).astype(F32)
    dy = rng.standard_normal((B, 1)).astype(F32)
    P = {k: t64(d[k]).requires_grad_() for k in ("K1", "K2", "K3") }
    P.update({k: t64(d[k]).requires_grad_() for k in ("b1", "b2", "b3") if d[k] is not None})
    xt = t64(x).requires_grad_()
    K1r = P["K1"] if d["rows"] is None else P["K1"][torch.from_numpy(d["rows"].astype(np.int64))]
    h = xt @ K1r + (P["b1"] if "b1" in P else 0)
    h = h @ P["K2"] + (P["b2"] if "b2" in P else 0)
    yt = TORCH_ACT[act]((h @ P["K3"] + (P["b3"] if "b3" in P else 0)).reshape(B, 1))
    (yt * t64(dy)).sum().backward()
    y = yt.detach().numpy().astype(F32)
    out, G, _ = E.reduce_ref(x, dy, y, act, c.n0)
    if act:  # G from the fp32 y: recompute from the float64 y for the comparison
        G = E.act_bwd_f64(dy.astype(np.float64), yt.detach().numpy(), act)
        out = np.concatenate([(x.astype(np.float64).T @ G).reshape(-1), G.sum(0)])
    dd = dict(d, A=out[:c.n0], s=out[c.n0:])
    v, e, m = E.chain3_grads_ref(dd)
    for name, par in (("dK1", "K1"), ("dK2", "K2"), ("dK3", "K3"), ("db1", "b1"), ("db2", "b2"), ("db3", "b3")):
        if par in P:
            close(v[name], P[par].grad.numpy(), name)
    close(G * v["p"][None, :], xt.grad.numpy(), "dx = G ⊗ p")
    if d["rows"] is not None:
        outside = np.setdiff1d(np.arange(d["n_full0"]), d["rows"])
        assert len(outside) == E.C3_EXTRA and not v["dK1"][outside].any()
    vc, _, _ = E.chain3_compose_ref(d)
    close(vc["q"], v["p"], "q == p")
    if c.n0 % 4 == 0:
        yr, _, _ = E.rowdot_ref(x, vc["q"], vc["c"], act)
        close(yr, yt.detach().numpy()[:, 0], "composed forward")
    else:
        close(E.act_fwd_f64(x.astype(np.float64) @ vc["q"] + vc["c"][0], act), yt.detach().numpy()[:, 0], "fwd")


@pytest.mark.parametrize("m,w,act", [(1, (4, 68, 132), 2), (15, (132, 4, 68), 1), (13, (12, 8, 4), 0)])
def test_narrow_chain_references_match_autograd(m, w, act):
    """The bottom chain [m -> w1 -> w2 -> w3] the way rs_dlrm_dense_tail factors it: P = [A; s]
    (reduce_ref), dK3 = R̃2ᵀ·P (outer_ref), P2 = P·K3ᵀ (rt_ref), dK2 = [K1; b1]ᵀ·P2, P1 = P2·K2ᵀ
    = [dK1; db1], db2 = P2[m], db3 = P[m]; forward act(x·Q + c) with [Q; c] from aug_ref twice."""
    rng = np.random.default_rng(m)
    B = 29
    g = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    K, b = [g(m, w[0]), g(w[0], w[1]), g(w[1], w[2])], [g(w[0]), g(w[1]), g(w[2])]
    x, dy = g(B, m), g(B, w[2])
    P = [t64(k).requires_grad_() for k in K + b]
    h = t64(x)
    for i in range(3):
        h = h @ P[i] + P[3 + i]
    yt = TORCH_ACT[act](h)
    (yt * t64(dy)).sum().backward()
    comp2, _, _ = E.aug_ref(dict(M=K[0], cin=b[0], K=K[1], b=b[1]))
    comp3, _, _ = E.aug_ref(dict(M=comp2[:m], cin=comp2[m], K=K[2], b=b[2]))
    yr, _, _ = E.narrow_ref(x, comp3, act)
    close(yr, yt.detach().numpy(), "composed forward")
    G = E.act_bwd_f64(dy.astype(np.float64), yt.detach().numpy(), act)
    Pm = np.vstack([x.astype(np.float64).T @ G, G.sum(0)[None]])
    out, _, _ = E.reduce_ref(x, G.astype(np.float64), None, 0, m)
    close(out.reshape(m + 1, w[2]), Pm, "reduce_ref layout [A; s]")
    dk3, _, _ = E.outer_ref(comp2[:m], comp2[m], Pm, w[1])
    P2, _, _ = E.rt_ref(Pm, K[2])
    dk2, _, _ = E.outer_ref(K[0], b[0], P2, w[0])
    P1, _, _ = E.rt_ref(P2, K[1])
    for got, par, name in ((P1[:m], 0, "dK1"), (dk2, 1, "dK2"), (dk3, 2, "dK3"), (P1[m], 3, "db1"),
                           (P2[m], 4, "db2"), (Pm[m], 5, "db3")):
        close(got, P[par].grad.numpy(), name)
    # rlast NULL is a zero row
    a, _, _ = E.outer_ref(K[0], None, P2, w[0])
    close(a, dk2 - np.outer(b[0].astype(np.float64), P2[m]), "outer without rlast")


# ---- 3. chain3 --------------------------------------------------------------------------------
def test_chain3_cases_cover_every_axis():
    cs = E.CHAIN3_CASES
    assert axis(cs, "n0") == set(E.C3_N0) and axis(cs, "n1") == set(E.C3_N1)
    assert axis(cs, "n2") == set(E.C3_N2)
    for sub in (False, True):
        assert {(c.b1, c.b2) for c in cs if c.subset == sub} == {(a, b) for a in (0, 1) for b in (0, 1)}
        assert {c.b3 for c in cs if c.subset == sub} == {False, True}
    d = E.chain3_inputs(next(c for c in cs if c.subset), "int")
    assert d["n_full0"] == d["A"].size + 37 and len(set(d["rows"])) == d["A"].size
    assert (d["rows"] != np.sort(d["rows"])).any(), "rows not permuted"
    assert (d["inv"][d["rows"]] == np.arange(d["A"].size)).all() and (d["inv"] == -1).sum() == 37


@pytest.mark.parametrize("c", E.CHAIN3_CASES, ids=str)
def test_chain3_int_inputs_make_the_comparison_exact(c):
    d = E.chain3_inputs(c, "int")
    v, e, m = E.chain3_grads_ref(d)
    vc, ec, mc = E.chain3_compose_ref(d)
    for name, mag in list(m.items()) + list(mc.items()):
        assert np.max(mag) < E.TWO24, (name, np.max(mag))
    for name, val in list(v.items()) + list(vc.items()):
        assert (val == np.rint(val)).all(), name
    assert d["s"][0] >= 1 and np.abs(d["K1"]).max() <= 2 and np.abs(d["A"]).max() <= 3
    emu = E.emulate_chain3(d)  # the kernels' order, in integers: exact
    for name in emu:
        ref = vc[name] if name in ("q", "c") else v[name]
        assert np.array_equal(emu[name], ref.astype(F32)), name


@pytest.mark.parametrize("c", [E.CHAIN3_CASES[i] for i in (0, 4, 9)], ids=str)
def test_chain3_bounds_hold_for_the_kernels_order_in_fp32(c):
    d = E.chain3_inputs(c, "gauss")
    v, e, _ = E.chain3_grads_ref(d)
    vc, ec, _ = E.chain3_compose_ref(d)
    emu = E.emulate_chain3(d)
    for name in emu:
        ref, err = (vc[name], ec[name]) if name in ("q", "c") else (v[name], e[name])
        assert emu[name].dtype == F32
        assert (np.abs(emu[name] - ref) <= err).all(), name


# ---- 4. the weight-sized products ---------------------------------------------------------------
def test_aug_cases():
    cs = E.AUG_CASES
    assert axis(cs, "m") == set(E.AUG_M) and axis(cs, "k") == set(E.AUG_K) | {512}
    assert axis(cs, "n") == set(E.AUG_N) and axis(cs, "pad") == {0, 3}
    assert {(c.cin, c.b) for c in cs} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert all(E.aug_accepts(c.m, c.k, c.n, c.k + c.pad) for c in cs)
    assert {c.m < 16 for c in cs} == {True, False}  # both MR instances
    big = [c for c in cs if (c.m + 1) * c.k == E.AUG_LDS]
    assert len(big) == 1 and E.aug_staging_trips(big[0].m, big[0].k) >= 2
    assert all(E.aug_staging_trips(c.m, c.k) == 1 for c in cs if c not in big)
    assert any(c.m == 0 and not c.cin for c in cs), "m = 0 without cin: the all-zero M̃"
    # the 128-deep unroll: [(main, tail) of wave 0, of wave 15]
    assert E.aug_unrolled_trips(127) == [(1, 0), (0, 7)]
    assert E.aug_unrolled_trips(128) == [(1, 0), (1, 0)]
    assert E.aug_unrolled_trips(129) == [(1, 1), (1, 0)]
    assert not E.aug_accepts(33, 4, 4, 4) and not E.aug_accepts(0, 16897, 1, 16897)
    assert E.aug_accepts(0, 16896, 1, 16896) and not E.aug_accepts(1, 4, 4, 3)


def test_rt_and_outer_cases():
    assert {c[0] for c in E.RT_CASES} == set(E.RT_M) and {c[1] for c in E.RT_CASES} == set(E.RT_K)
    assert {c[2] for c in E.RT_CASES} == set(E.RT_N) and len(set(E.RT_CASES)) == 10
    assert all((m + 1) * k <= E.AUG_LDS for m, k, _ in E.RT_CASES)
    cs = E.OUTER_CASES
    assert axis(cs, "m") == set(E.OUT_M) and axis(cs, "na") == set(E.OUT_NA)
    assert axis(cs, "nb") == set(E.OUT_NB) and axis(cs, "pad") == {0, 5}
    assert {c.m + c.rlast for c in cs} == {0, 1, 2, 7, 8, 9, 10, 32, 33}  # around the 8-row batches
    R, rl, P = E.outer_inputs(E.OUTER(0, False, 5, 4, 0), "int")
    out, _, _ = E.outer_ref(R, rl, P, 5)
    assert out.shape == (5, 4) and not out.any()
    R, rl, P = E.outer_inputs(E.OUTER(7, False, 5, 4, 2), "int")
    assert np.isnan(P[7]).all() and np.isnan(R[:, 5:]).all()
    assert np.isfinite(E.outer_ref(R, rl, P, 5)[0]).all()


def test_product_int_inputs_make_the_comparison_exact():
    for c in E.AUG_CASES:
        out, _, mag = E.aug_ref(E.aug_inputs(c, "int"))
        assert mag.max() < E.TWO24 and (out == np.rint(out)).all()
        assert np.array_equal(E.emulate_aug(E.aug_inputs(c, "int")), out.astype(F32))
    for m, k, n in E.RT_CASES:
        P, K = E.rt_inputs(m, k, n, "int")
        out, _, mag = E.rt_ref(P, K)
        assert mag.max() < E.TWO24 and (out == np.rint(out)).all()
        assert np.array_equal(E.emulate_rt(P, K), out.astype(F32))
    for c in E.OUTER_CASES:
        R, rl, P = E.outer_inputs(c, "int")
        out, _, mag = E.outer_ref(R, rl, P, c.na)
        assert mag.max(initial=0) < E.TWO24 and (out == np.rint(out)).all()


def test_product_bounds_hold_for_the_kernels_order_in_fp32():
    for c in (E.AUG_CASES[3], E.AUG_CASES[4], E.AUG_CASES[12]):
        d = E.aug_inputs(c, "gauss")
        out, err, _ = E.aug_ref(d)
        emu = E.emulate_aug(d)
        assert emu.dtype == F32 and (np.abs(emu - out) <= err).all() and (emu != out).any()
    for m, k, n in E.RT_CASES[3:6]:
        P, K = E.rt_inputs(m, k, n, "gauss")
        out, err, _ = E.rt_ref(P, K)
        assert (np.abs(E.emulate_rt(P, K) - out) <= err).all()
    for c in (E.OUTER_CASES[5], E.OUTER_CASES[11]):
        R, rl, P = E.outer_inputs(c, "gauss")
        out, err, _ = E.outer_ref(R, rl, P, c.na)
        Rt = R[:, :c.na] if rl is None else np.vstack([R[:, :c.na], rl[None]])
        acc = np.zeros((c.na, c.nb), F32)
        for r in range(Rt.shape[0]):
            acc = acc + Rt[r][:, None] * P[r][None, :]
        assert (np.abs(acc - out) <= err).all()


# ---- 5. the forwards ----------------------------------------------------------------------------
def test_forward_cases():
    cs = E.FWD_CASES
    assert axis(cs, "n0") == set(E.FWD_N0) and axis(cs, "n") == set(E.FWD_N)
    assert axis(cs, "B") == set(E.FWD_B) and axis(cs, "act") == {0, 1, 2}
    assert any(c.padx for c in cs) and any(c.pady for c in cs)
    assert all(E.narrow_trips(c.B)[1] <= 1 for c in cs)
    B, n0, n = E.FWD_BIG
    assert B == 262209 and E.narrow_trips(B) == (4096, 2) and E.narrow_trips(B - 65) == (4096, 1)
    assert B * n * 4 < 4.5e6  # the largest buffer of the GPU file
    rc = E.ROWDOT_CASES
    assert {c[0] for c in rc} == set(E.ROWDOT_N0) and {c[1] for c in rc} == set(E.ROWDOT_B)
    assert {c[3] for c in rc} == {0, 1, 2} and any(c[2] for c in rc)
    assert [E.rowdot_depth_act(n) for n in (4, 256, 260, 1024)] == [11, 11, 15, 23]


def test_forward_int_inputs_and_bounds():
    for c in E.FWD_CASES + (E.FWD(E.FWD_BIG[1], E.FWD_BIG[2], 300, 0, 0, 1),):
        x, Qa = E.narrow_inputs(c.n0, c.n, c.B, c.padx, "int")
        y, _, mag = E.narrow_ref(x, Qa, 1)
        assert mag.max(initial=0) < E.TWO24 and (y == np.rint(y)).all()
        if c.B > 8:
            assert (y == 0).any() and (y > 0).any()  # relu cuts
    for n0, B, pad, act in E.ROWDOT_CASES:
        x, q, cc = E.rowdot_inputs(n0, B, pad, "int")
        y, _, mag = E.rowdot_ref(x, q, cc, 0)
        assert mag.max(initial=0) < E.TWO24
        assert np.array_equal(E.emulate_rowdot(x, q, cc), y.astype(F32))
    for n0, B, pad, act in [c for c in E.ROWDOT_CASES if c[1]][:4]:
        x, q, cc = E.rowdot_inputs(n0, B, pad, "gauss")
        v, err, _ = E.rowdot_ref(x, q, cc, 0)
        assert (np.abs(E.emulate_rowdot(x, q, cc) - v) <= err).all()
        # the fp32 sigmoid of the fp32 pre-activation stays inside the sigmoid bound
        y, erry, _ = E.rowdot_ref(x, q, cc, 2)
        pre = E.emulate_rowdot(x, q, cc)
        y32 = F32(1) / (F32(1) + np.exp(-pre))
        assert y32.dtype == F32 and (np.abs(y32 - y) <= erry).all()
    x, Qa = E.narrow_inputs(15, 12, 65, 3, "gauss")
    v, err, _ = E.narrow_ref(x, Qa, 0)
    acc = np.zeros((65, 12), F32)
    for k in range(15):
        acc = acc + x[:, k, None] * Qa[None, k]
    assert (np.abs((acc + Qa[15]) - v) <= err).all()


# ---- 6. the dense tail --------------------------------------------------------------------------
def test_tail_cases():
    cs = E.TAIL_CASES
    assert axis(cs, "m") == {1, 15} and {(c.n0, c.n1, c.n2) for c in cs} == {(5, 17, 65), (48, 64, 1)}
    assert {w for c in cs for w in (c.b1, c.b2, c.b3)} == {4, 68, 132}
    assert axis(cs, "subset") == {False, True} and sorted(axis(cs, "p_off")) == [0, 1]
    assert all(E.tail_accepts(c) for c in cs)
    assert any(w % 64 for c in cs for w in (c.b1, c.b2, c.b3))
    assert not E.tail_accepts(cs[0]._replace(m=16)) and not E.tail_accepts(cs[0]._replace(b2=6))


def test_fma32_is_the_exact_fused_multiply_add():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = rng.standard_normal(4000).astype(F32)
    # planted: a·b = 2^-24 - 2^-70 on c = 1 + 2^-23: the float64 sum rounds onto the midpoint of
    # two fp32 values, where rounding again would go up to the even one; the true sum is below
    a[0], b[0], c[0] = F32(2.0 ** -12) * (F32(1) + F32(2.0 ** -23)), F32(2.0 ** -12) * (F32(1) - F32(2.0 ** -23)), F32(1) + F32(2.0 ** -23)
    a[1], b[1], c[1] = F32(2.0 ** -24), F32(1), F32(1) + F32(2.0 ** -23)  # an exact tie: to even
    got = E.fma32(a, b, c)
    assert got[0] == F32(1) + F32(2.0 ** -23) and got[1] == F32(1) + F32(2.0 ** -22)
    for i in range(300):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = F32(float(exact))
        cands = [np.nextafter(near, F32(-np.inf)), near, np.nextafter(near, F32(np.inf))]
        best = min(abs(Fraction(float(x)) - exact) for x in cands)
        assert abs(Fraction(float(got[i])) - exact) == best, i
    assert (got != a * b + c).any(), "no element tells fmaf from multiply-then-add"
    assert np.array_equal(E.sgd_fma(c, b, 0.05), E.fma32(np.full(4000, -F32(0.05), F32), b, c))
