"""The cases of tests/apply_edges.py have the structure they claim, read off the sorted keys of
oracle.embedding.sort_ids: tile counts, live tiles of the last group, the tiles a named run starts
and ends in, which half-wave walks them at each block shape, where the sentinels begin."""
import numpy as np
import pytest

from oracle import embedding as O
from tests import apply_edges as E

T, G, V = E.T, E.G, E.V


@pytest.mark.parametrize("name", list(E.CASES))
def test_case_has_the_structure_it_claims(name):
    case = E.CASES[name]
    cl = case["claims"]
    ids, grad, sr, sp = E.sorted_case(case)
    n = ids.size
    assert n == sum(case["lens"]) + case["oob"] and grad.shape == (n, E.D)
    assert (np.diff(sr.astype(np.int64)) >= 0).all() and sorted(sp.tolist()) == list(range(n))
    head, length, rows = E.run_table(sr)
    assert length.tolist() == list(case["lens"])  # the runs, in order, as listed
    nv = int(length.sum())
    assert (sr[nv:] == V).all() and n - nv == case["oob"]
    n_tiles = -(-n // T)
    if "n_tiles" in cl:
        assert n_tiles == cl["n_tiles"]
    if "last_group_live" in cl:
        assert (n_tiles - 1) % G + 1 == cl["last_group_live"]
    if "n_mod" in cl:
        assert n % T == cl["n_mod"]
    if "n_runs" in cl:
        assert head.size == cl["n_runs"]
    if "n_valid" in cl:
        assert nv == cl["n_valid"]
    if "first_all_sentinel_tile" in cl:
        t = cl["first_all_sentinel_tile"]
        assert t < n_tiles and (sr[t * T:] == V).all() and (sr[(t - 1) * T:t * T] < V).any()
    if "run" in cl:
        i = int(np.flatnonzero(head == cl["run"])[0])  # a run starts exactly there
        first, last = head[i] // T, (head[i] + length[i] - 1) // T
        assert (first, last) == (cl["first_tile"], cl["last_tile"])
        if "starts_on_edge" in cl:
            assert (head[i] % T == 0) == cl["starts_on_edge"]
            assert ((head[i] + length[i]) % T == 0) == cl["ends_on_edge"]
    for t in cl.get("singleton_tiles", ()):
        assert np.unique(sr[t * T:(t + 1) * T]).size == T
    for t in cl.get("one_run_tiles", ()):
        k = sr[t * T:(t + 1) * T]
        assert (k == k[0]).all() and sr[t * T - 1] != k[0] and sr[(t + 1) * T] != k[0]
    for t, want in cl.get("runs_ending_in_tile", {}).items():
        end = head + length - 1
        inside = (end // T == t) & (head // T == t)  # runs that start and end in tile t
        assert int(inside.sum()) == want


def test_tile_counts_cover_every_block_shape_edge():
    """n_tiles 1, HW - 1, HW, HW + 1 for HW = 8, 16, 32 and a second group with 17 live tiles,
    each with n a multiple of 32, n % 32 = 1 and n % 32 = 31."""
    seen = {(c["claims"]["n_tiles"], c["claims"]["n_mod"]) for k, c in E.CASES.items()
            if k.startswith("tiles")}
    want = {1, 32 + 17}
    for hw in E.SHAPES:
        want |= {hw - 1, hw, hw + 1}
    assert {t for t, _ in seen} == want
    assert all((t, m) in seen for t in want for m in (0, 1, 31))


def test_named_runs_sit_where_the_half_wave_maps_say():
    """Half-wave gi of a block of HW walks tiles gi, gi + HW, ... of its group (round r = tile
    // HW): the cases named after a placement have it at the shapes they name."""
    own = lambda tile, hw: (tile % G) % hw
    rnd = lambda tile, hw: (tile % G) // hw
    c = E.CASES["run_over_one_halfwaves_tiles"]["claims"]
    for hw in (16, 8):  # head and last tile in one half-wave's list, different rounds
        assert own(c["first_tile"], hw) == own(c["last_tile"], hw)
        assert rnd(c["first_tile"], hw) != rnd(c["last_tile"], hw)
    c = E.CASES["run_over_two_adjacent_tiles"]["claims"]
    for hw in E.SHAPES:
        assert own(c["first_tile"], hw) != own(c["last_tile"], hw)
    c = E.CASES["run_across_rounds_mid_tile"]["claims"]
    assert rnd(c["first_tile"], 16) == 0 and rnd(c["last_tile"], 16) == 1
    assert rnd(c["first_tile"], 8) == 0 and rnd(c["last_tile"], 8) == 2
    c = E.CASES["run_into_short_group"]["claims"]
    assert c["last_group_live"] < min(E.SHAPES) and c["first_tile"] // G != c["last_tile"] // G
    c = E.CASES["sentinel_tail_after_16_tiles"]["claims"]
    assert c["n_valid"] > 16 * T and c["first_all_sentinel_tile"] == 17  # tile 16 = round 1 of gi 0
    assert E.CASES["sentinel_tail_after_8_tiles"]["claims"]["first_all_sentinel_tile"] == 8


def test_ranged_case_groups_sit_around_the_key_bounds():
    case, lo, hi = E.ranged_case()
    ids, grad, sr, sp = E.sorted_case(case)
    assert ids.size == 4 * E.GROUP
    key_lo, key_hi = int(sr[lo]), int(sr[hi])
    grp = lambda g: sr[g * E.GROUP:(g + 1) * E.GROUP].astype(np.int64)
    assert (grp(0) < key_lo).all()                                  # entirely below key_lo
    assert (grp(1) < key_lo).any() and (grp(1) >= key_lo).any()     # straddles it
    assert lo % T != 0 and sr[lo - 1] != sr[lo]                     # inside a tile, between runs
    assert ((grp(2) >= key_lo) & (grp(2) < key_hi)).all()           # inside the range
    assert (grp(3) >= key_hi).all() and 0 < key_lo < key_hi < V     # entirely at or above key_hi


def test_expected_values_follow_the_tiled_order():
    """The helper's expectations are the oracle's: a scaled gradient is one fp32 multiply before
    the tiled sum, and a run's sum differs from the plain left-to-right sum where tiles cut it
    (the order is the tiled one, not any order)."""
    case = E.CASES["run_over_one_halfwaves_tiles"]
    ids, grad, sr, sp = E.sorted_case(case)
    ur, ug = E.expected_segments(sr, sp, grad)
    head, length, rows = E.run_table(sr)
    assert ur.tolist() == rows.tolist()
    i = int(np.argmax(length))
    seq = np.zeros(E.D, np.float32)
    for p in sp[head[i]:head[i] + length[i]]:
        seq = seq + grad[p]
    assert np.allclose(ug[i], seq, rtol=1e-4, atol=1e-4) and (ug[i] != seq).any()
    scale = np.random.default_rng(1).standard_normal(-(-ids.size // 3)).astype(np.float32)
    sg = E.scaled_grad(grad, scale, 3)
    assert sg.dtype == np.float32 and (sg[4] == scale[1] * grad[4]).all()
