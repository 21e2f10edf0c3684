"""The inputs of tests/test_dien_edges_gpu.py have the property their name claims, and the
semantics those tests rely on hold for the oracle (oracle/dien.py) — all without a GPU."""
import numpy as np
import pytest
import torch

from oracle import dien as OD
from tests import dien_edges as E

RTOL = 2e-5  # the project's DIEN bound: 2e-5 of the tensor's largest value


def _rng():
    return np.random.default_rng(11)


@pytest.mark.parametrize("B,T", [(2, 9), (3, 9), (7, 70), (5, 1)])
def test_post_mask(B, T):
    m = E.mask("post", B, T, _rng())
    lens = m.sum(1)
    assert (m == (np.arange(T)[None, :] < lens[:, None])).all(), "not right-padded"
    assert (lens >= 1).all() and (lens == T).any() and (lens == 1).any()


@pytest.mark.parametrize("B,T", [(1, 9), (5, 9), (7, 70), (3, 3)])
def test_holes_mask(B, T):
    m = E.mask("holes", B, T, _rng())
    assert m[:, 0].all()
    for row in m:  # a masked step with a valid one on either side
        v = np.flatnonzero(row)
        assert (np.diff(v) > 1).any()


@pytest.mark.parametrize("B,T", [(1, 9), (5, 9), (7, 70), (3, 2), (5, 256)])
def test_late_mask(B, T):
    m = E.mask("late", B, T, _rng())
    assert not m[:, 0].any() and m.any(1).all()
    assert m.argmax(1)[0] == 1 and (m.argmax(1) >= 1).all()


@pytest.mark.parametrize("B,T", [(2, 9), (3, 9), (7, 70), (3, 1)])
def test_empty_row_mask(B, T):
    m = E.mask("empty_row", B, T, _rng())
    assert (~m).all(1).any() and m.all(1).any()
    if B > 2 and T >= 3:
        assert m[2, 0] and (np.diff(np.flatnonzero(m[2])) > 1).any()
    assert not E.mask("empty_row", 1, 9, _rng()).any()  # B = 1: the empty row alone


def test_word_edges_mask():
    T = 300
    m = E.mask("word_edges", 5, T, _rng())
    want = list(E.WORD_EDGES) + [T - 1]
    assert m[:, want].all()
    assert ((m.sum(1) >= len(want)) & (m.sum(1) <= len(want) + 3)).all()
    for q in range(4):  # every 64-step ballot word has its first and its last bit set
        assert m[:, 64 * q].all() and m[:, 64 * q + 63].all()
    assert (m[:, 256:].sum(1) >= 2).all()  # the byte path: at least two steps from 256 on
    with pytest.raises(AssertionError):
        E.mask("word_edges", 2, 299, _rng())


def _hm_for(H):
    """csrc/dien.hip hm_for, restated."""
    for hm in (8, 16, 24, 32, 36, 40, 48, 64):
        if H <= hm:
            return hm
    return 0


def test_h_list_covers_every_template():
    assert {1, 5, 8, 13, 16, 20, 32, 33, 36, 37, 40, 47, 48, 50, 64} <= {h for h, _ in E.H_LIST}
    for H, hm in E.H_LIST:
        assert _hm_for(H) == hm, (H, hm)
    for hm in E.HM_CLASSES:
        hs = [H for H, c in E.H_LIST if c == hm]
        assert any(H < hm for H in hs) and any(H == hm for H in hs), hm
    assert {50, 64} <= {H for H, c in E.H_LIST if c == 64}
    assert _hm_for(65) == 0
    assert {s[0] for s in E.GRU_CASES} >= {h for h, _ in E.H_LIST}


def test_case_lists_hold_what_the_gpu_module_claims():
    # the large-LDS attention launch and the largest case that stays on the ordinary one
    by_lds = sorted(E.ATT_CASES, key=lambda s: E.att_lds_bytes(s[0], s[2]))
    assert by_lds[-1] == E.ATT_BIG_LDS and E.att_lds_bytes(64, 256) > 65536
    assert E.att_lds_bytes(by_lds[-2][0], by_lds[-2][2]) <= 65536
    assert {s[2] for s in E.ATT_CASES if s[0] == 36 and s[1] == 5} == set(E.ATT_LS)
    assert {"late", "holes"} <= {s[3] for s in E.ATT_CASES}
    for spec in E.ATT_CASES:
        if spec[4]:  # |h·q| reaches about 100, and the largest score is not in the first chunk
            d = E.inputs("att", spec)
            q = np.einsum("hx,bx->bh", d["K"].astype(np.float64), d["target"][:, 0].astype(np.float64))
            s = np.einsum("blh,bh->bl", d["hs"].astype(np.float64), q)
            s = np.where(d["mask"], s, -np.inf)
            assert (s.max(1) > 80).all() and (s.max(1) < 130).all()
            if spec[2] > 128:
                assert (s.max(1) - s[:, :64].max(1) > 89).all()  # exp of it overflows fp32
    for layer, cases in (("gru", E.GRU_CASES), ("augru", E.AUGRU_CASES)):
        assert {(s[2], s[4]) for s in cases if s[0] == s[1] == 36 and s[3] == 9} >= {
            (B, k) for B in (1, 3, 7) for k in ("post", "holes", "late", "empty_row")}
        assert any(s[1] > 64 for s in cases) and any(s[3] == 1 for s in cases)
        assert {s[0] for s in cases if s[3] == 300} == {36, 20}
        for spec in cases:  # garbage at every masked step, and only there
            d = E.inputs(layer, spec)
            assert (d["x"][~d["mask"]] == E.GARBAGE).all()
            assert (np.abs(d["x"][d["mask"]]) < 10).all()


def test_dilate():
    x = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
    y, m = E.dilate(x, np.ones((2, 3), bool), (1, 4, 5), T=8)
    assert y.shape == (2, 8, 2) and m.sum() == 6 and m[:, [1, 4, 5]].all()
    assert (y[:, [1, 4, 5]] == x).all() and (y[~m] == E.GARBAGE).all()
    for T, pos in E.DILATE_POS.items():
        assert len(pos) == E.DILATE_TC and pos[0] == 0 and pos[-1] == T - 1
    assert set(E.WORD_EDGES) <= set(E.DILATE_POS[300])
    assert {63, 64} <= set(E.DILATE_POS[70])


@pytest.mark.parametrize("T", sorted(E.DILATE_POS))
def test_oracle_is_exact_under_dilation(T):
    """The semantics the GPU tests rely on: inserting masked steps (holding garbage) changes no
    bit of the float64 oracle at the valid steps; a masked step repeats the state before it
    (0 before the first valid step); the AUGRU's final state is unchanged."""
    H, B, Tc = 20, 3, E.DILATE_TC
    pos = np.array(E.DILATE_POS[T])
    pos = np.where(pos == 0, 2, pos) if T == 70 else pos  # T = 70: also masked leading steps
    pos.sort()
    g = E.gru_inputs(H, H, B, Tc, "post")
    ones = np.ones((B, Tc), bool)
    f64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    W, U, bias = f64(g["W"]), f64(g["U"]), f64(g["bias"])
    xc = E.gru_inputs(H, H, B, Tc, "holes")["x"]
    xc = np.where(np.abs(xc) < 10, xc, 0.5).astype(np.float32)  # all steps valid: no garbage
    xd, md = E.dilate(xc, ones, pos, T)
    oc = OD.gru(f64(xc), W, U, bias, torch.from_numpy(ones)).numpy()
    od = OD.gru(f64(xd), W, U, bias, torch.from_numpy(md)).numpy()
    assert np.array_equal(od[:, pos], oc)
    carried = np.zeros_like(od)
    prev = np.zeros((B, H))
    j = 0
    for t in range(T):
        if md[0, t]:
            prev = oc[:, j]
            j += 1
        carried[:, t] = prev
    assert np.array_equal(od, carried)
    assert pos[0] == 0 or (od[:, :pos[0]] == 0).all()

    a = E.augru_inputs(H, H, B, Tc, "post")
    par = [f64(a[n]) for n in E.AUGRU_PARAMS]
    ac = np.random.default_rng(3).random((B, Tc, 1)).astype(np.float32)
    ad, _ = E.dilate(ac, ones, pos, T)
    fc = OD.augru(f64(xc), f64(ac), *par, torch.from_numpy(ones)).numpy()
    fd = OD.augru(f64(xd), f64(ad), *par, torch.from_numpy(md)).numpy()
    assert np.array_equal(fc, fd)


_ALL = ([("gru", s) for s in E.GRU_CASES + (E.DILATE_LAYER_SPEC,)]
        + [("augru", s) for s in E.AUGRU_CASES + (E.DILATE_LAYER_SPEC,)]
        + [("att", s) for s in E.ATT_CASES] + [("evolve", s) for s in E.EVOLVE_CASES])


@pytest.mark.parametrize("layer", ["gru", "augru", "att", "evolve"])
def test_fp32_oracle_meets_the_project_bound(layer):
    """On every input of the GPU module the fp32 oracle is within 2e-5·max|ref| of the float64
    one, outputs and gradients: the bound is attainable by an fp32 evaluation (no case needed
    its weight scale reduced, the T = 300 recurrences included)."""
    worst = 0.0
    for lay, spec in _ALL:
        if lay != layer:
            continue
        r64 = E.reference(lay, spec, torch.float64)
        r32 = E.reference(lay, spec, torch.float32)
        for k, r in r64.items():
            assert np.isfinite(r).all() and np.isfinite(r32[k]).all(), (lay, spec, k)
            err = float(np.abs(r32[k] - r).max()) if r.size else 0.0
            bound = RTOL * float(np.abs(r).max())
            assert err <= bound, (lay, spec, k, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    print(f"{layer}: worst fp32 err / bound {worst:.3g}")
