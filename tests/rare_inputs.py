"""Inputs that reach the kernels' rarely taken paths (not a test module): rs_masked_topk's
candidate regimes and the open-addressing tables of csrc/hashtab.hpp near and at full load.

The two NumPy models here (topk_candidates, probe_table) only CLASSIFY inputs, so that
tests/test_rare_inputs_cpu.py can assert on the CPU that each input reaches the path its name
claims. Expected outputs never come from them: the GPU tests compare with oracle/pinsage.py and
with a plain dict."""
import numpy as np

# ---------------------------------------------------------------------------------------------
# rs_masked_topk (csrc/recommend.hip masked_topk_kernel)
# ---------------------------------------------------------------------------------------------
TOPK_THREADS = 256  # kTopkThreads: item i belongs to thread i % 256
TOPK_WAVE = 64      # nc <= 64: one wave sorts the candidates
TOPK_CAND = 2048    # kTopkCand: LDS candidate slots; nc beyond → lists rebuilt from the row


def masked_row(row, excluded=None):
    """The row the kernel ranks: excluded items at -inf."""
    r = np.array(row, np.float32, copy=True)
    if excluded is not None and len(excluded):
        r[np.asarray(excluded)] = -np.inf
    return r


def _theta_rank(row, K):
    I = row.size
    order = np.lexsort((np.arange(I), -row.astype(np.float64)))  # (score desc, item asc)
    rank = np.empty(I, np.int64)
    rank[order] = np.arange(I)
    best = np.full(TOPK_THREADS, I, np.int64)  # a thread without items ranks after every item
    np.minimum.at(best, np.arange(I) % TOPK_THREADS, rank)
    return rank, int(np.sort(best)[K - 1])


def topk_candidates(row, K):
    """nc of pass 2: θ = the K-th best of the 256 per-thread bests; the items ranking <= θ.
    `row` has its exclusions applied (masked_row)."""
    rank, theta = _theta_rank(np.asarray(row, np.float32), K)
    return int((rank <= theta).sum())


def topk_candidate_owners(row, K):
    """Candidates per owning thread (i % 256), [256]: what each thread's register list holds
    when the lists are built from the whole row (nc > 2048), and which threads' items fill the
    LDS list otherwise (there, list slot c goes to thread c % 256: a thread holds more than one
    candidate exactly when nc > 256)."""
    row = np.asarray(row, np.float32)
    rank, theta = _theta_rank(row, K)
    return np.bincount(np.flatnonzero(rank <= theta) % TOPK_THREADS, minlength=TOPK_THREADS)


def hot_row(I, K, rng, base=0):
    """Background integers in [-20, 20); the items of threads base .. base+K-2 at 1000 + [0, 50)
    (every one of them a candidate), those of thread base+K-1 at 400 but one at 500 (θ):
    nc = (K - 1) · (items per hot thread) + 1."""
    assert 1 <= K and base + K <= TOPK_THREADS
    row = rng.integers(-20, 20, I).astype(np.float32)
    res = np.arange(I) % TOPK_THREADS
    hot = (res >= base) & (res < base + K - 1)
    row[hot] = 1000 + rng.integers(0, 50, int(hot.sum()))
    th = np.flatnonzero(res == base + K - 1)
    row[th] = 400
    row[rng.choice(th)] = 500
    return row


# tests/test_pinsage_eval_gpu.py::test_masked_topk_bit_exact's cases (R, I, K, exclusions)
COMMON_TOPK_CASES = [(7, 5, 5, False), (64, 100, 10, True), (33, 3706, 10, True),
                     (5, 3706, 17, True), (9, 1000, 33, False), (4, 27278, 64, True),
                     (3, 40, 1, True)]


def common_topk_case(R, I, K, excl):
    """(scores, user ids, item ids of the distinct exclusion edges or None) of such a case."""
    rng = np.random.default_rng(R * 1000 + K)
    scores = rng.integers(-20, 20, (R, I)).astype(np.float32)  # dense ties
    if not excl:
        return scores, None, None
    u = np.repeat(np.arange(R), rng.integers(0, min(I, 50), R))
    it_ = rng.integers(0, I, u.size)
    key = np.unique(u * I + it_)
    return scores, key // I, key % I


def _csr(lists):
    ip = np.zeros(len(lists) + 1, np.int64)
    ip[1:] = np.cumsum([len(x) for x in lists])
    it = np.concatenate([np.asarray(x, np.int32) for x in lists]) if lists else np.zeros(0, np.int32)
    return ip, it.astype(np.int32)


def _excl_some(row, rng, n_random=30, n_hot=3):
    """A user's exclusion list: random items plus a few of the best ones (θ's item first)."""
    top = np.lexsort((np.arange(row.size), -row.astype(np.float64)))
    hot = np.concatenate([np.flatnonzero(row == 500)[:1], top[:n_hot]])
    return np.unique(np.concatenate([rng.integers(0, row.size, n_random), hot]))


# name → (regime, I, K, kind[, base]); regimes: "wave" nc <= 64, "lists" 65..2048 with a thread
# owning >= 2 candidates, "deep" the same with nc > 256 (a thread's register list holds >= 2
# entries of the LDS list: list_insert bubbles, list_pop repeats), "overflow" nc > 2048.
TOPK_CASES = {
    # overflow, once per template instance KM = 64 / 64 / 32 / 16 / 8
    "overflow_8448_64": ("overflow", 8448, 64, "hot"),
    "overflow_27278_64": ("overflow", 27278, 64, "hot"),
    "overflow_16640_33": ("overflow", 16640, 33, "hot"),
    "overflow_33024_17": ("overflow", 33024, 17, "hot"),
    "overflow_70000_9": ("overflow", 70000, 9, "hot"),
    "overflow_80000_8": ("overflow", 80000, 8, "hot"),
    "overflow_wave3_8448_64": ("overflow", 8448, 64, "hot", 192),
    # the same with the whole top K in one thread's register list (K pops of one lane)
    "overflow_one_thread_16640_33": ("overflow", 16640, 33, "hot1"),
    "overflow_one_thread_33024_17": ("overflow", 33024, 17, "hot1"),
    "overflow_one_thread_70000_9": ("overflow", 70000, 9, "hot1"),
    "overflow_one_thread_80000_8": ("overflow", 80000, 8, "hot1"),
    # lists inside LDS
    "lists_5000_10": ("lists", 5000, 10, "hot"),
    "deep_70000_8": ("deep", 70000, 8, "hot"),
    "deep_140000_4": ("deep", 140000, 4, "hot"),
    "deep_3000_33": ("deep", 3000, 33, "hot"),
    "deep_40000_10": ("deep", 40000, 10, "hot"),
    "deep_20000_20": ("deep", 20000, 20, "hot"),
    "deep_wave3_5000_64": ("deep", 5000, 64, "hot", 192),
    # one wave
    "wave_flat_3000_10": ("wave", 3000, 10, "flat"),
    "wave_flat_300_64": ("wave", 300, 64, "flat"),
    "wave_descending_3000_10": ("wave", 3000, 10, "descending"),
    "wave_ascending_3000_10": ("wave", 3000, 10, "ascending"),
    "wave_all_items_37": ("wave", 37, 37, "random"),
    "wave_all_items_64": ("wave", 64, 64, "random"),
    "wave_three_left_300_10": ("wave", 300, 10, "three_left"),
    # exclusion bitmap past 32 KB (dynamic LDS attribute), items in its last word excluded
    "wave_bitmap_300001_10": ("wave", 300001, 10, "bitmap"),
    "wave_bitmap_1048576_10": ("wave", 1 << 20, 10, "bitmap"),
}


def topk_case(name):
    """(scores [R, I] float32, K, plain rows, (indptr, items) of the other rows). The first
    `plain` rows run without an exclusion CSR, the rest with one (CSR row r ↔ scores[plain + r])."""
    regime, I, K, kind, *rest = TOPK_CASES[name]
    seed = sum(name.encode()) * 7919 + I
    rng = np.random.default_rng(seed)
    if kind in ("hot", "hot1"):
        rows = [hot_row(I, K, rng, *rest) for _ in range(4)]
        if kind == "hot1":  # the best items all belong to thread 0: its list is popped K times
            for r in rows:
                r[::TOPK_THREADS] += 1000
        excl = [_excl_some(r, rng) for r in rows[2:]]
        return np.stack(rows), K, 2, _csr(excl)
    if kind == "bitmap":
        rows = rng.integers(-20, 20, (2, I)).astype(np.float32)
        rows[:, I - 6:] = 100 + np.arange(6, dtype=np.float32)  # the best items: the last six
        last_word = np.arange((I - 1) // 32 * 32, I)
        excl = [np.unique(np.concatenate([rng.integers(0, I, 40), [I - 1, I - 3, 0, 31, 32]])),
                np.unique(np.concatenate([rng.integers(0, I, 40), last_word[-4:]]))]
        return rows, K, 0, _csr(excl)
    if kind == "three_left":
        rows = rng.integers(-20, 20, (2, I)).astype(np.float32)
        keep = [np.array([7, 150, 299]), np.array([0, 255, 256])]
        return rows, K, 0, _csr([np.setdiff1d(np.arange(I), k) for k in keep])
    if kind == "flat":
        rows = np.full((4, I), 3.0, np.float32)
    elif kind == "descending":
        rows = np.tile(-np.arange(I, dtype=np.float32), (4, 1))
    elif kind == "ascending":
        rows = np.tile(np.arange(I, dtype=np.float32), (4, 1))
    else:
        rows = rng.integers(-20, 20, (4, I)).astype(np.float32)
    excl = [np.unique(rng.integers(0, I, min(I // 2, 30))) for _ in range(2)]
    return rows, K, 2, _csr(excl)


def topk_case_rows(name):
    """Every row of the case as the kernel ranks it (exclusions applied), with K."""
    scores, K, plain, (ip, it) = topk_case(name)
    out = [scores[r] for r in range(plain)]
    for r in range(plain, scores.shape[0]):
        out.append(masked_row(scores[r], it[ip[r - plain]:ip[r - plain + 1]]))
    return out, K


def topk_regime(row, K):
    nc = topk_candidates(row, K)
    if nc <= TOPK_WAVE:
        return "wave"
    if nc > TOPK_CAND:
        return "overflow"
    if topk_candidate_owners(row, K).max() < 2:
        return "lists_shallow"
    return "deep" if nc > TOPK_THREADS else "lists"


# ---------------------------------------------------------------------------------------------
# csrc/hashtab.hpp
# ---------------------------------------------------------------------------------------------
U64 = np.uint64
EMPTY = U64(0xFFFFFFFFFFFFFFFF)
MIN_COUNT = 10  # the vocabulary keeps count > 10


def table_key(h):
    """A stored key never equals the empty marker: ~0 → ~0 - 1 (array or scalar, uint64)."""
    h = np.asarray(h, U64)
    return np.where(h == EMPTY, EMPTY - U64(1), h)


def vslot(key, mask):
    """((key · 0x9E3779B97F4A7C15 mod 2^64) >> 32) & mask."""
    with np.errstate(over="ignore"):
        p = np.asarray(key, U64) * U64(0x9E3779B97F4A7C15)
    return ((p >> U64(32)) & U64(mask)).astype(np.int64)


def probe_table(keys, capacity):
    """Sequential linear probing of `keys` (table_key applied) into `capacity` slots:
    (slot of every distinct key that found one, keys left without a slot, whether some key's
    chain wrapped past the last slot). Which slots end up occupied, and how many keys cross the
    table's end, do not depend on the insertion order."""
    mask = capacity - 1
    table = {}
    slot_of, dropped, wrapped = {}, [], False
    for k in table_key(keys).tolist():
        if k in slot_of or k in dropped:
            continue
        h = int(vslot(U64(k), mask))
        for probe in range(capacity):
            s = (h + probe) & mask
            if s not in table:
                table[s] = k
                slot_of[k] = s
                wrapped |= s < h
                break
        else:
            dropped.append(k)
    return slot_of, dropped, wrapped


def _keys_with_home(rng, mask, lo, n, taken):
    """n fresh keys whose home slot is >= lo (rejection)."""
    out = []
    while len(out) < n:
        c = rng.integers(0, 1 << 63, 4096, dtype=np.int64).astype(U64) * U64(2) + U64(1)
        for k in c[vslot(c, mask) >= lo].tolist():
            if k not in taken and len(out) < n:
                taken.add(k)
                out.append(k)
    return out


def hash_keys(capacity, n_distinct, seed):
    """n_distinct distinct table keys: 0, ~0 - 1 (which the hash ~0 shares), six keys at home
    in the last four slots (at least two of their chains wrap), the rest uniform."""
    rng = np.random.default_rng(seed)
    taken = {0, int(EMPTY) - 1, int(EMPTY)}
    keys = [0, int(EMPTY) - 1]
    keys += _keys_with_home(rng, capacity - 1, capacity - 4, 6, taken)
    keys += _keys_with_home(rng, capacity - 1, 0, n_distinct - len(keys), taken)
    return np.array(keys, U64)


def hash_stream(keys, seed):
    """A token stream over `keys` (hashes: the key ~0 - 1 appears as both ~0 - 1 and ~0).
    keys[8], keys[9] occur exactly 10 times and keys[10], keys[11] exactly 11 (min_count's two
    sides); keys[12..15] form runs: 30 equal hashes over a wave boundary (50..79), 20 over a
    block boundary (250..269), one whole wave (320..383) and 200 from 400 (two whole waves, a
    block boundary at 512); the length is no multiple of 64."""
    rng = np.random.default_rng(seed)
    reps = rng.integers(1, 25, keys.size)
    reps[8:10] = 10
    reps[10:12] = 11
    reps[12:16] = 0
    reps[:2] = 12
    base = np.repeat(keys, reps)
    base[np.flatnonzero(base == EMPTY - U64(1))[::2]] = EMPTY  # ~0 and ~0 - 1: one key
    rng.shuffle(base)
    assert base.size >= 300
    run = lambda j, n: np.full(n, keys[j], U64)
    s = np.concatenate([base[:50], run(12, 30), base[50:220], run(13, 20), base[220:270],
                        run(14, 64), base[270:286], run(15, 200), base[286:]])
    if s.size % 64 == 0:
        s = np.concatenate([s, keys[16:17]])
    return s


def hash_counts(stream, present=None, pos_base=0):
    """The reference dict: table key → [count, first position]."""
    d = {}
    for i, k in enumerate(table_key(stream).tolist()):
        if present is not None and not present[i]:
            continue
        e = d.setdefault(k, [0, pos_base + i])
        e[0] += 1
    return d


# name → (capacity, distinct table keys)
HASH_CASES = {
    "cap64_load09": (64, 58),
    "cap64_full": (64, 64),
    "cap1024_load09": (1024, 922),
    "cap1024_full": (1024, 1024),
}
HASH_OVERFULL = (64, 80)


def hash_case(name):
    cap, nd = HASH_OVERFULL if name == "overfull" else HASH_CASES[name]
    keys = hash_keys(cap, nd, seed=cap * 131 + nd)
    return cap, keys, hash_stream(keys, seed=cap * 17 + nd)


def absent_hashes(keys, capacity, n, seed):
    """Hashes of no key in `keys` (even: hash_keys' random keys are odd), a quarter of them at
    home in the last four slots."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 1 << 62, 64 * n, dtype=np.int64).astype(U64) * U64(2)
    c = c[~np.isin(c, keys)]
    end = c[vslot(c, capacity - 1) >= capacity - 4][: n // 4]
    return np.concatenate([end, c[: n - end.size]])
