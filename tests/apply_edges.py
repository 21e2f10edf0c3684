"""Cases for the D = 128 apply walk's block shapes (seg_group32_kernel in
recommender_amd/csrc/embedding.hip): a block of HW half-waves (HW = 32, 16 or 8) walks one aligned
group of 32 tiles of 32 sorted entries, half-wave gi taking tiles gi, gi + HW, gi + 2 HW, ...

A case is a list of run lengths in sorted-key order (a run = the entries of one row) plus a number
of out-of-range ids, which sort behind every row as sentinels. Each case names the structure it
is there for in `claims`; tests/test_apply_edges_cpu.py checks the claims against
oracle.embedding.sort_ids, tests/test_apply_block_shapes_gpu.py runs the kernels on the cases.
Expected values come from oracle.embedding.segment_sum_tiled (the statement of the order of
additions) followed by the optimizer restatements the other tests use."""
from __future__ import annotations

import numpy as np

from oracle import embedding as O

T = O.DEDUP_TILE   # entries per tile
G = O.FIX_CHUNK    # tiles per group
GROUP = T * G      # entries per group
SHAPES = (32, 16, 8)  # half-waves per block the kernel can be built with
V, D = 50_000, 128
f32 = np.float32


def mixed_runs(n, seed):
    """Run lengths summing to n: singletons, short runs, runs longer than a tile and a few longer
    than eight tiles, in a seeded random order."""
    rng = np.random.default_rng(seed)
    lens, left = [], n
    while left > 0:
        kind = rng.integers(0, 10)
        m = 1 if kind < 4 else int(rng.integers(2, 12)) if kind < 8 else \
            int(rng.integers(T, 3 * T)) if kind < 9 else int(rng.integers(8 * T, 20 * T))
        m = min(m, left)
        lens.append(m)
        left -= m
    return lens


def _tile_count_cases():
    """n_tiles around the block shapes; the last tile full, one entry, or 31 entries."""
    out = {}
    for tiles in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 32 + 17):
        for rem in (T, 1, T - 1):
            n = (tiles - 1) * T + rem
            out[f"tiles{tiles}_rem{rem % T}"] = dict(
                lens=mixed_runs(n, 1000 * tiles + rem), oob=0,
                claims=dict(n_tiles=tiles, last_group_live=(tiles - 1) % G + 1, n_mod=rem % T))
    return out


def _structure_cases():
    c = {}
    # tiles 3..19 are exactly one run: its head tile 3 and its last tile 19 are walked by the
    # same half-wave at HW = 16 (3, 19) and at HW = 8 (3, 11, 19, 27); singletons around it
    c["run_over_one_halfwaves_tiles"] = dict(
        lens=[1] * (3 * T) + [17 * T] + [1] * (4 * T + 5), oob=0,
        claims=dict(run=3 * T, first_tile=3, last_tile=19, starts_on_edge=True, ends_on_edge=True))
    # tiles 4 and 5 are exactly one run: adjacent tiles, different half-waves at every shape
    c["run_over_two_adjacent_tiles"] = dict(
        lens=[1] * (4 * T) + [2 * T] + [1] * (3 * T), oob=0,
        claims=dict(run=4 * T, first_tile=4, last_tile=5, starts_on_edge=True, ends_on_edge=True))
    # a run from inside tile 5 to inside tile 22: head in round 0 of every shape, end in round 1
    # of HW = 16 and round 2 of HW = 8, both ends inside their tiles
    c["run_across_rounds_mid_tile"] = dict(
        lens=[1] * (5 * T + 7) + [17 * T + 4] + [3] * 40, oob=0,
        claims=dict(run=5 * T + 7, first_tile=5, last_tile=22, starts_on_edge=False,
                    ends_on_edge=False))
    # a run from the group's first tile to its last, whole group; a second group follows
    c["run_over_whole_group"] = dict(
        lens=[GROUP] + [1] * (2 * T + 3), oob=0,
        claims=dict(run=0, first_tile=0, last_tile=G - 1, starts_on_edge=True, ends_on_edge=True))
    # the same from inside tile 0 to inside tile 31
    c["run_first_to_last_tile_inside"] = dict(
        lens=[5, GROUP - 5 - 3, 1, 1, 1] + [2] * 20, oob=0,
        claims=dict(run=5, first_tile=0, last_tile=G - 1, starts_on_edge=False,
                    ends_on_edge=False))
    # a run crossing the group edge into a last group with 5 live tiles (fewer than any HW)
    c["run_into_short_group"] = dict(
        lens=[1] * (GROUP - 24) + [24 + 3 * T + 9] + [1] * (T + 10), oob=0,
        claims=dict(run=GROUP - 24, first_tile=G - 1, last_tile=G + 3, starts_on_edge=False,
                    ends_on_edge=False, n_tiles=G + 5, last_group_live=5))
    # one run over everything: three whole groups, and three groups less a bit
    c["one_run_three_groups"] = dict(
        lens=[3 * GROUP], oob=0,
        claims=dict(run=0, first_tile=0, last_tile=3 * G - 1, n_tiles=3 * G, n_runs=1))
    c["one_run_three_groups_ragged"] = dict(
        lens=[2 * GROUP + 17 * T + 1], oob=0,
        claims=dict(run=0, first_tile=0, last_tile=2 * G + 17, n_tiles=2 * G + 18, n_runs=1,
                    last_group_live=18))
    # tiles of 32 singletons beside a tile that is one run; tile 2 has 31 singletons (an odd
    # number of runs ending inside the tile: the queue of two flushes half full) and the first
    # entry of a run that fills tile 3; tile 5 holds three runs
    c["singleton_tiles_beside_run_tile"] = dict(
        lens=[1] * T + [T] + [1] * (T - 1) + [1 + T] + [1] * T + [10, 11, 11], oob=0,
        claims=dict(run=3 * T - 1, first_tile=2, last_tile=3, starts_on_edge=False,
                    ends_on_edge=True, singleton_tiles=(0, 4), one_run_tiles=(1,),
                    runs_ending_in_tile={2: 31, 5: 3}))
    # out-of-range ids: rows fill 16 tiles and 5 entries of tile 16; the rest, into a second
    # group, is sentinels: at HW = 16 every half-wave but one has rows in its first tile and
    # none in its second
    c["sentinel_tail_after_16_tiles"] = dict(
        lens=mixed_runs(16 * T + 5, 77), oob=(G + 1) * T + 7 - (16 * T + 5),
        claims=dict(n_tiles=G + 2, n_valid=16 * T + 5, first_all_sentinel_tile=17))
    # the same after 8 tiles (HW = 8: rows in the first round only), ending on a tile edge
    c["sentinel_tail_after_8_tiles"] = dict(
        lens=mixed_runs(8 * T, 78), oob=9 * T + 1,
        claims=dict(n_tiles=18, n_valid=8 * T, first_all_sentinel_tile=8))
    # a run that ends where the sentinels begin, mid-tile, after crossing tiles
    c["run_up_to_sentinels"] = dict(
        lens=[1] * (2 * T) + [2 * T + 9], oob=T,
        claims=dict(run=2 * T, first_tile=2, last_tile=4, starts_on_edge=True, ends_on_edge=False,
                    n_valid=4 * T + 9, first_all_sentinel_tile=5))
    return c


CASES = {**_tile_count_cases(), **_structure_cases()}


def build(case, seed=0):
    """ids int64 [n] in a shuffled position order, with the case's runs on ascending rows of
    [0, V) and its out-of-range ids (V + something, or negative), and the gradient rows [n, D]."""
    rng = np.random.default_rng([seed, len(case["lens"]), sum(case["lens"])])
    rows = np.sort(rng.choice(V, len(case["lens"]), replace=False))
    ids = np.repeat(rows, case["lens"]).astype(np.int64)
    oob = np.where(rng.random(case["oob"]) < 0.5, V + rng.integers(0, 9, case["oob"]), -1)
    ids = np.concatenate([ids, oob.astype(np.int64)])
    ids = ids[rng.permutation(ids.size)]
    grad = rng.standard_normal((ids.size, D)).astype(f32)
    return ids, grad


def sorted_case(case, seed=0):
    """(ids, grad, sorted_rows uint32, sorted_pos int32) of a case."""
    ids, grad = build(case, seed)
    sr, sp, _ = O.sort_ids(ids, V)
    return ids, grad, sr, sp


def run_table(sr):
    """(start, length, row) of every run of valid rows in the sorted keys."""
    nv = int((sr < V).sum())
    k = sr[:nv].astype(np.int64)
    head = np.flatnonzero(np.r_[True, k[1:] != k[:-1]]) if nv else np.zeros(0, np.int64)
    return head, np.diff(np.r_[head, nv]), k[head]


def scaled_grad(grad, row_scale, scale_group):
    """fmul_rn(row_scale[p // scale_group], grad[p]) in float32, the scaled apply's gradient."""
    sc = np.asarray(row_scale, f32)[np.arange(grad.shape[0]) // scale_group]
    return (sc[:, None] * grad).astype(f32)


def expected_segments(sr, sp, grad):
    """(uniq_rows int64, uniq_grad) in the kernel's order of additions."""
    ur, ug = O.segment_sum_tiled(sr, sp, grad, V)
    return ur.astype(np.int64), ug


def ranged_case():
    """Four groups of mixed runs and key bounds for the ranged walk: group 0 lies entirely below
    key_lo, group 1 straddles it (inside a tile, between two runs), group 2 is inside the range
    and group 3 lies entirely at or above key_hi. Returns (case, lo_entry, hi_entry): key_lo /
    key_hi are the keys of the runs starting at those sorted entries."""
    lens = []
    for g in range(4):
        part = mixed_runs(GROUP - 1, 500 + g)  # every group ends on a run end: a singleton closes it
        lens += part + [1]
    case = dict(lens=lens, oob=0, claims=dict(n_tiles=4 * G))
    head = np.cumsum([0] + lens[:-1])
    lo = int(head[head >= GROUP + 10 * T + 5][0])
    hi = 3 * GROUP
    assert hi in set(head.tolist())
    return case, lo, hi
