"""The texts of tests/ingest_edges.py have the properties their names claim (line lengths on
both sides of the 4,096-byte staging limit, separators on the 64-byte ballot edges, newlines on
the block and wave-quarter edges, counts of exactly 10 and 11, ...): without this, a GPU test
that passes says nothing about the path it took. Also the oracle's answers on the small cases
that can be checked by hand."""
import re

import numpy as np
import pytest

from oracle import criteo as OC
from oracle import textpipe as O
from tests import ingest_edges as E
from tests.criteo_text import make_tsv
from tests.textpipe_text import make_aliccp, make_amazon

COLS = O.ALICCP_COLUMNS


def test_old_generators_stay_under_the_staging_limit():
    """Documents the gap: no line of the generated texts reaches 4,096 bytes, so the in-place
    path of kv_parse_kernel / dien_parse_kernel (len > kStage) never ran under test."""
    sk, cm = make_aliccp(np.random.default_rng(0), 600, 40)
    am = make_amazon(np.random.default_rng(0), 600)
    tsv = make_tsv(np.random.default_rng(0), 400)
    longest = [max(E.stripped_lengths(t)) for t in (am, sk, cm, tsv)]
    assert max(longest) < 1024 < E.STAGE, longest


def test_no_forbidden_bytes():
    c, a, z = E.criteo_edges(), E.aliccp_edges(), E.amazon_edges()
    texts = [c["train"], c["train_empty_c26"], c["test"], a["skeleton"], a["common"], z["train"],
             z["test"], E.amazon_edges(unequal=False)["train"], E.amazon_partnerless(),
             E.ALICCP_TOO_FEW_COMMAS, *E.criteo_malformed().values()]
    for t in texts:
        assert not E.forbidden_bytes(t)
        assert t.replace("\r\n", "\n").splitlines() == E.lines_of(t)  # the oracles see the same lines
    assert all(not E.forbidden_bytes(b) for _, b in E.line_index_cases())
    assert E.forbidden_bytes("a\rb") and E.forbidden_bytes("a\x0bb") and E.forbidden_bytes("a\r")


# ---- line index ---------------------------------------------------------------------------
def test_line_index_cases():
    cases = dict(E.line_index_cases())
    assert len(cases) == 4 * len(E.LINE_INDEX_SIZES) - 1 + 1  # no all-'\n' layout at 3·4096+5
    for size in E.LINE_INDEX_SIZES:
        nl = {lay: np.flatnonzero(np.frombuffer(cases[f"{lay}_{size}"], np.uint8) == 10)
              for lay in ("none", "last", "edges")}
        assert len(cases[f"none_{size}"]) == size and nl["none"].size == 0
        assert nl["last"].tolist() == [size - 1]
        assert ("all_%d" % size in cases) == (size <= 8192)
        if size <= 8192:
            assert cases[f"all_{size}"] == b"\n" * size
        e = nl["edges"]
        assert e.tolist() == E.edge_offsets(size)
        assert set((e % E.QUARTER).tolist()) <= {0, E.QUARTER - 1}
        if size >= 4097:  # both sides of a wave quarter and of a block
            assert {0, 1023} == set((e % 1024).tolist()) and {0, 4095} <= set((e % 4096).tolist())
    assert E.edge_offsets(4097) == [0, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096]
    rnd = np.frombuffer(cases["random_20000"], np.uint8)
    assert rnd.size == 20000 and 400 < (rnd == 10).sum() < 600


# ---- Criteo -------------------------------------------------------------------------------
def _criteo_rows(text):
    return [ln.split("\t") for ln in text.replace("\r\n", "\n").splitlines(keepends=True)]


def test_criteo_edges_properties():
    c = E.criteo_edges()
    train, f = c["train"], c["facts"]
    rows = _criteo_rows(train)
    assert all(len(r) == 40 for r in rows) and all(len(r) == 40 for r in _criteo_rows(c["test"]))
    # I1 of every length 1..18; the edge integers; the 300-byte token
    assert {len(r[1]) for r in rows} >= set(range(1, 19))
    ints = {x for r in rows for x in r[1:14]}
    assert {str(v) for v in E.CRITEO_INTS} <= ints
    assert max(int(x) for x in ints if x) >= 10**17 and len(E.LONG_TOKEN) == 300
    assert any(E.LONG_TOKEN in r for r in rows)
    # counts on both sides of `count > 10`, as the oracle counts them (C26 keeps its '\n')
    counts = {}
    for r in rows:
        for v in OC._cats(r):
            counts[v] = counts.get(v, 0) + 1
    assert counts[f["t10"]] == 10 and counts[f["t11"]] == 11
    assert counts[f["same"]] > 10 and counts[f["same"] + "\n"] > 10  # two vocabulary entries
    vocab = OC.build_vocab(train)
    assert f["t10"] not in vocab and vocab[f["t11"]] > 0
    assert vocab[f["same"]] != vocab[f["same"] + "\n"]
    # the end of the file: a last line without '\n', C26 non-empty / empty
    assert rows[-1][39] == f["same"] and _criteo_rows(c["train_empty_c26"])[-1][39] == ""
    assert _criteo_rows(c["test"])[-1][39] == ""
    # '\n' on the last byte of a 4,096-byte block and on the first byte of the next
    a, b = f["nl_last_of_block"], f["nl_first_of_block"]
    assert train[a] == "\n" and a % 4096 == 4095 and train[b] == "\n" and b % 4096 == 0
    assert train[a - 1] != "\r" and b - a == 4097
    assert "\r\n" in train and re.search(r"[^\r]\n", train)
    # a tab in the last lane of a 64-byte chunk and a field starting in lane 0 of the next
    tab_lanes = set()
    for ln in E.lines_of(train):
        tab_lanes |= {i % 64 for i, ch in enumerate(ln) if ch == "\t"}
    assert tab_lanes == set(range(64))


def test_criteo_malformed_inputs():
    m = E.criteo_malformed()
    assert "" in E.lines_of(m["blank_line"])[1:-1]
    assert sorted({len(ln.split("\t")) for ln in E.lines_of(m["41_fields"])}) == [40, 41]


# ---- Ali-CCP ------------------------------------------------------------------------------
def _kv_of(line, field):
    return line.strip().split(",")[field]


def test_aliccp_edges_properties():
    a = E.aliccp_edges()
    sk, cm, at = E.lines_of(a["skeleton"]), E.lines_of(a["common"]), a["lines"]
    ls, lc = E.stripped_lengths(a["skeleton"]), E.stripped_lengths(a["common"])
    for lens in (ls, lc):  # both sides of kStage and well past it, in both files
        assert 4096 in lens and 4097 in lens and max(lens) > 6000
    assert ls[at["len_4096"]] == 4096 and ls[at["len_4097"]] == 4097
    assert [len(sk[at[f"p{p}"]].split(",")[0]) for p in range(130)] == list(range(130))
    # the ~400-triple line: wanted columns scattered, two of them in its last 64 bytes
    big = max(cm, key=len)
    toks = re.split("\x01|\x02|\x03", _kv_of(big, 2))
    assert len(toks) == 1200 and len(big) > 6000
    assert sum(k in COLS for k in toks[0::3]) == 6
    assert [k for k in re.split("\x01|\x02|\x03", big[-64:]) if k in COLS] == ["126", "127"]
    # a repeated wanted column whose winning occurrence starts beyond byte 4096 (both files)
    for line, kvf, col in ((cm[4], 2, "121"), (sk[at["repeat_beyond_4096"]], 5, "206")):
        occ = [m.start() for m in re.finditer(f"\x01{col}\x02|^{col}\x02", _kv_of(line, kvf))]
        assert len(occ) == 2 and line.index(_kv_of(line, kvf)) + occ[1] > 4096
    # separators of the kv field at offsets ≡ 63 and ≡ 0 (mod 64) from its start, over the lines
    lanes = {1: set(), 2: set(), 3: set()}
    key_start_lanes = set()
    for p in range(130):
        kv = _kv_of(sk[at[f"p{p}"]], 5)
        for i, ch in enumerate(kv):
            if ch in "\x01\x02\x03":
                lanes[ord(ch)].add(i % 64)
                if ch == "\x01":
                    key_start_lanes.add((i + 1) % 64)
    assert all(v == set(range(64)) for v in lanes.values()) and 0 in key_start_lanes
    # unwanted names that are a prefix / superstrings of wanted ones; 301 as value and weight
    keys = set()
    for line, kvf in [(x, 5) for x in sk] + [(x, 2) for x in cm]:
        keys |= set(re.split("\x01|\x02|\x03", _kv_of(line, kvf))[0::3])
    assert {"10", "1010", "3011"} <= keys and not {"10", "1010", "3011"} & set(COLS)
    t = re.split("\x01|\x02|\x03", _kv_of(sk[at["301_as_value_and_weight"]], 5))
    assert t[1] == "301" and t[2] == "301" and "301" not in t[0::3]
    # trailing key, empty last value, empty kv, strip(), labels
    assert sk[at["trailing_key"]].endswith("\x01216")
    assert sk[at["empty_last_value"]].endswith("\x01216\x02")
    assert sk[at["empty_kv"]].endswith(",") and _kv_of(sk[at["empty_kv"]], 5) == ""
    assert sk[at["spaces"]].startswith("  ") and sk[at["spaces"]].endswith(" \x1f ")
    assert any(x.startswith(" ") and x.endswith(" \x1f") for x in cm)
    assert sk[at["labels_00_01"]].split(",")[1:3] == ["00", "01"]
    assert sk[at["dropped"]].split(",")[1:3] == ["0", "1"]
    assert "\r\n" in a["skeleton"] and "\r\n" in a["common"]
    ids = [x.strip().split(",")[0] for x in cm]
    assert len(ids) == len(set(ids)) + 1 and ids[-1] == "c5"  # one duplicate id, last
    assert len(E.ALICCP_TOO_FEW_COMMAS.strip().split(",")) == 5


def test_aliccp_edges_oracle_answers():
    a = E.aliccp_edges()
    sk, at = E.lines_of(a["skeleton"]), a["lines"]
    rows = O.aliccp_join(a["skeleton"], a["common"])
    dropped = [x for x in sk if x.strip().split(",")[1:3] == ["0", "1"]]
    assert len(dropped) >= 2 and len(rows) == len(sk) - len(dropped)

    def row(name):
        got = O.aliccp_join(sk[at[name]] + "\n", a["common"])
        return got[0] if got else None

    c = COLS.index
    assert row("dropped") is None
    assert row("labels_00_01")[:2] == (0, 1)  # '00' / '01' are not '0' / '1': kept
    r = row("301_as_value_and_weight")
    assert r[2][c("301")] is None and r[2][c("205")] == "1000"
    assert row("trailing_key")[2][c("216")] is None
    assert row("empty_last_value")[2][c("216")] == ""
    assert row("empty_kv")[2][c("205")] is None and row("empty_kv")[2][c("127")] == "b127"
    assert row("spaces")[2][c("205")] == "1000" and row("spaces")[2][c("129")] == "v129c2"
    assert row("repeat_beyond_4096")[2][c("206")] == "2004"
    assert row("len_4096")[2][c("216")] == "late216" and row("len_4096")[2][c("121")] == "l121"
    # the duplicate common id: the later line wins as a whole (its 122 is gone)
    assert row("repeat_beyond_4096")[2][c("101")] == "new101"
    assert row("repeat_beyond_4096")[2][c("122")] is None
    # a literal '0' in 508 on at least 12 kept rows: an absent 508 encodes to its id
    v508 = [r[2][c("508")] for r in rows]
    assert v508.count("0") >= 12 and v508.count(None) >= 12 and set(v508) == {"0", None}
    vocab = O.aliccp_vocab(rows)
    assert vocab[c("508")] == {"0": 1}
    ids, _ = O.aliccp_encode(rows, vocab)
    assert (ids[:, c("508")] == 1).all()
    # the values whose order decides (first / last occurrence, old / new line) have their own ids
    assert {"e121", "l121"} <= set(vocab[c("121")]) and {"2000", "2004"} <= set(vocab[c("206")])
    assert "new101" in vocab[c("101")] and "5000" in vocab[c("301")]


# ---- Amazon -------------------------------------------------------------------------------
def test_amazon_edges_properties():
    z = E.amazon_edges()
    lines, at = E.lines_of(z["train"]), z["lines"]
    lens = E.stripped_lengths(z["train"])
    assert lens[at["len_4096"]] == 4096 and lens[at["len_4097"]] == 4097
    assert lens[at["hist_700"]] > 4096 and lens[at["chg_late"]] > 4096
    assert max(E.stripped_lengths(z["test"])) > 4096
    assert not z["train"].endswith("\n") and z["test"].endswith("\n") and "\r\n" in z["train"]
    f = [O._dien_fields(x) for x in lines]
    assert [len(lines[at[f"p{p}"]].strip().split("\t")[1]) for p in range(130)] == list(range(130))
    assert {x[0] for x in f} == {"0", "1", "1.0"}
    n_hi, n_hc = [len(x[3]) for x in f], [len(x[4]) for x in f]
    assert {1, 63, 64, 65, 200, 700} <= set(n_hi)
    assert f[at["hist_empty"]][3] == [""] and f[at["hist_empty"]][4] == ["C3"]  # one empty token
    assert any(a > b for a, b in zip(n_hi, n_hc)) and any(a < b for a, b in zip(n_hi, n_hc))
    assert lines[at["spaces"]].startswith(" ") and lines[at["spaces"]].endswith(" \x1f")
    # '\x02' on the last lane of a 64-byte chunk of the history field, a token on lane 0
    his = lines[at["hist_700"]].split("\t")[4]
    assert {i % 64 for i, ch in enumerate(his) if ch == "\x02"} == set(range(64))
    # partnerless items; the item whose cat changes (its last pair is the last of a long line)
    items, cats, i2c = O.dien_vocab(z["train"])
    lonely = [it for it in items if it not in i2c and it != "mask"]
    assert len(lonely) == 5 and all(it.startswith("P") for it in lonely)
    with pytest.raises(KeyError):
        O.dien_cat_of_item(items, cats, i2c)
    coi = O.dien_cat_of_item(items, cats, i2c, missing=-1)
    assert (coi == -1).sum() == 5 and all(coi[items[it]] == -1 for it in lonely)
    assert f[at["chg_early"]][1:3] == ("CHG0000001", "C1") and i2c["CHG0000001"] == "C5"
    assert f[at["chg_late"]][3][-1] == "CHG0000001" and f[at["chg_late"]][4][-1] == "C5"
    # the test text: unseen items, known cats
    ft = [O._dien_fields(x) for x in E.lines_of(z["test"])]
    assert any(it not in items for x in ft for it in x[3]) and any(x[1] not in items for x in ft)
    assert all(ct in cats for x in ft for ct in [x[2]] + x[4])
    assert {62, 63, 64, 65, 66, 128, 129, 130} <= {len(x[3]) for x in ft}
    # the well-formed variant has no partnerless item; the partnerless text has mostly such
    w = E.amazon_edges(unequal=False)
    wi, wc, w2c = O.dien_vocab(w["train"])
    assert (O.dien_cat_of_item(wi, wc, w2c) >= 0).all()
    assert all(len(x[3]) == len(x[4]) for x in map(O._dien_fields, E.lines_of(w["train"])))
    pi, pc, p2c = O.dien_vocab(E.amazon_partnerless())
    assert (O.dien_cat_of_item(pi, pc, p2c, missing=-1) == -1).mean() > 0.9


def test_dien_cat_of_item_missing_default_unchanged():
    text = "1\tu\tA\tc1\tB\x02C\tc2\n"  # C has no cat partner
    items, cats, i2c = O.dien_vocab(text)
    with pytest.raises(KeyError):
        O.dien_cat_of_item(items, cats, i2c)
    assert O.dien_cat_of_item(items, cats, i2c, missing=-1).tolist() == [0, 1, 2, -1, 3]


# ---- TFRecord -----------------------------------------------------------------------------
def test_tfrecord_padded_lengths():
    from oracle import tfrecord as OT

    ints, cats = np.arange(13, dtype=np.float32), np.arange(26, dtype=np.int64)
    for n in (E.STAGE, E.STAGE + 1):
        rec, ex = E.tfrecord_padded(ints, cats, 1, n)
        assert len(ex) == n and len(rec) == n + 16
        a, b, c = OT.read_records(rec)  # still a valid record of the same row
        np.testing.assert_array_equal(a[0], ints)
        np.testing.assert_array_equal(b[0], cats)
        assert c.tolist() == [1]
