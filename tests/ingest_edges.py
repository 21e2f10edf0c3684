"""Text that drives the ingestion scanners of csrc/criteo.hip and csrc/textpipe.hip over their
edges (not a test module): lines on both sides of the 4,096-byte LDS staging limit (kStage: a
longer line is scanned in place), separators on the last lane of one 64-byte ballot chunk and
token starts on lane 0 of the next, newlines on the last byte of a 4,096-byte block and of a
1,024-byte wave quarter of the line index, and the parsing rules no generated text exercises
(unequal histories, partnerless items, a literal '0' value, wanted names in value position,
strip(), integers past 2^24, counts of exactly 10 and 11).

Every builder is deterministic and returns the text with the facts about it that
tests/test_ingest_edges_cpu.py asserts, so that a passing GPU test says which path it took.
Expected outputs never come from here: the GPU tests compare with oracle/criteo.py,
oracle/textpipe.py and NumPy.

No builder emits a lone '\\r' or one of the bytes \\x0b \\x0c \\x1c \\x1d \\x1e \\x85: the oracles
split lines with str.splitlines(), which breaks on those, while the reference's file iteration
(and the kernels' line index) breaks on '\\n' only."""
import numpy as np

from oracle import tfrecord as OT

FORBIDDEN = (0x0b, 0x0c, 0x1c, 0x1d, 0x1e, 0x85)
STAGE = 4096   # kStage (csrc/textpipe.hip), kLineBlock (csrc/criteo.hip), kRecMax (csrc/tfrecord.hip)
QUARTER = 1024  # bytes per wave of nl_write_kernel


def forbidden_bytes(text) -> bool:
    """Whether `text` (str or bytes) holds a byte the oracles' splitlines() would split on but
    the reference would not: one of FORBIDDEN, or a '\\r' not followed by '\\n'."""
    b = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    a = np.frombuffer(b, np.uint8)
    if np.isin(a, FORBIDDEN).any():
        return True
    cr = np.flatnonzero(a == 13)
    return bool(((cr + 1 >= a.size) | (a[np.minimum(cr + 1, a.size - 1)] != 10)).any())


def lines_of(text: str):
    """The lines as the reference's file iteration yields them, terminators removed."""
    ls = text.replace("\r\n", "\n").split("\n")
    return ls[:-1] if ls[-1] == "" else ls


def stripped_lengths(text: str):
    """len(line.strip()) of every line: the length the kernels' stripped_line() scans."""
    return [len(ln.strip()) for ln in lines_of(text)]


# ---------------------------------------------------------------------------------------------
# rs_line_index
# ---------------------------------------------------------------------------------------------
LINE_INDEX_SIZES = [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 3 * 4096 + 5]


def edge_offsets(size):
    """Offsets {k·1024 - 1, k·1024, k·4096 - 1, k·4096} inside [0, size)."""
    offs = set()
    for unit in (QUARTER, STAGE):
        for k in range(size // unit + 2):
            offs.update((k * unit - 1, k * unit))
    return sorted(o for o in offs if 0 <= o < size)


def line_index_cases():
    """[(name, bytes)]: every size with no newline, one on the last byte, every byte a newline
    (sizes up to 8192) and newlines exactly on the block / wave-quarter edges; one 20,000-byte
    random text with newline density 1/40."""
    cases = []
    for size in LINE_INDEX_SIZES:
        base = np.full(size, ord("a"), np.uint8)
        cases.append((f"none_{size}", base.tobytes()))
        last = base.copy()
        last[-1] = 10
        cases.append((f"last_{size}", last.tobytes()))
        if size <= 8192:
            cases.append((f"all_{size}", np.full(size, 10, np.uint8).tobytes()))
        edges = base.copy()
        edges[edge_offsets(size)] = 10
        cases.append((f"edges_{size}", edges.tobytes()))
    rng = np.random.default_rng(20000)
    rnd = rng.integers(ord("a"), ord("z") + 1, 20000).astype(np.uint8)
    rnd[rng.random(20000) < 1 / 40] = 10
    cases.append(("random_20000", rnd.tobytes()))
    return cases


# ---------------------------------------------------------------------------------------------
# rs_criteo_parse (+ the vocabulary kernels behind CriteoVocab)
# ---------------------------------------------------------------------------------------------
CRITEO_INTS = [2**24 - 1, 2**24, 2**24 + 1, 2**31 - 1, 2**31, 10**12, "-0", "-7", ""]
_COMMON = ["a1b2c3d4", "0f0f0f0f", "deadbeef", "5eed5eed", "cafe0001"]
T10, T11, SAME = "7e4710aa", "7e4711bb", "5a5e5a5e"
LONG_TOKEN = "".join(f"{i % 16:x}" for i in range(300))


def _criteo_fields(k):
    ints = [str((k * 31 + j * 7) % 200) if (k + j) % 6 else "" for j in range(13)]
    cats = ["" if (k * 7 + c) % 13 == 0 else _COMMON[(k + c) % 5] for c in range(26)]
    return ints, cats


def _criteo_line(label, ints, cats):
    return "\t".join([str(label)] + [str(x) for x in ints] + list(cats))


class _Text:
    """Lines appended with their terminators; knows the byte offset of the next line."""

    def __init__(self):
        self.parts, self.off = [], 0

    def add(self, line, eol="\n"):
        self.parts.append(line + eol)
        self.off += len(line) + len(eol)

    def text(self):
        return "".join(self.parts)


def criteo_edges():
    """{'train', 'train_empty_c26', 'test', 'facts'}: 40-field Criteo lines.

    train: I1 of 1..18 digits (one line each: every later tab slides over the 64-byte chunk
    edges), the CRITEO_INTS values, a 300-byte token, two lines padded through C1 so that their
    '\\n' falls on the last byte of a 4,096-byte block and on the first byte of the next, CRLF
    and LF mixed, T10 exactly 10 and T11 exactly 11 times, SAME in C1 and in C26 (the trailing
    '\\n' makes those two keys), a last line without '\\n' whose C26 is SAME (no '\\n': the C1
    key). train_empty_c26: the same with that last C26 empty. test: unseen tokens, T10, T11,
    SAME on both sides, the big integers again, and an empty C26 at the end of the file."""
    def line(k, **over):
        ints, cats = _criteo_fields(k)
        for key, v in over.items():
            (ints if key[0] == "I" else cats)[int(key[1:]) - 1] = v
        return _criteo_line(k % 2, ints, cats)

    def build(first_k, overs, last_eol):
        t = _Text()
        for j, over in enumerate(overs):
            k = first_k + j
            pad = over.pop("pad_nl_to", None)
            if pad is not None:  # C1 sized so that this line's '\n' lands on offset ≡ pad (mod 4096)
                n = (pad - (t.off + len(line(k, C1="", **over)))) % STAGE or STAGE
                over["C1"] = "pq"[pad == 0] * n
            eol = "\r\n" if k % 5 == 2 and pad is None else "\n"
            t.add(line(k, **over), last_eol if j == len(overs) - 1 else eol)
        return t

    overs = [{}]  # the first vocabulary entries (ids 0, 1, ..) are common tokens
    overs += [{"I1": ("123456789" * 2)[:d]} for d in range(1, 19)]
    for r in range(3):  # the edge integers, rotated over the columns
        overs.append({f"I{2 + (j + 4 * r) % 12}": v for j, v in enumerate(CRITEO_INTS)})
    overs.append({"C5": LONG_TOKEN})
    overs += [{f"C{1 + (3 * j) % 25}": T10} for j in range(10)]
    overs += [{f"C{2 + (5 * j) % 24}": T11} for j in range(11)]
    overs += [{"C1": SAME} for j in range(12)]
    overs += [{"C26": SAME} for j in range(12)]  # hashed with its '\n' ('\r\n' folded)
    at = len(overs)
    overs += [{"pad_nl_to": STAGE - 1}, {"pad_nl_to": 0}]
    overs += [{} for j in range(4)]
    copy = lambda: [dict(o) for o in overs]
    train = build(0, copy() + [{"C26": SAME}], "")
    train_empty = build(0, copy() + [{"C26": ""}], "")
    starts = np.cumsum([0] + [len(x) for x in train.parts])
    test = build(1000, [
        {"C3": T10, "C4": T11, "C1": SAME, "C26": SAME},
        {"C1": "unseen01", "C26": "unseen02", "I1": "-7", "I2": 2**24 + 1, "I13": 10**17 + 3},
        {"C26": T11, "C2": LONG_TOKEN, "I5": "-0", "I6": 2**31, "I7": ""},
        *[{"I1": "9" * d, "I13": "9" * d} for d in (1, 9, 10, 18)],
        *[{} for j in range(6)],
        {"C26": ""}], "")
    facts = {"t10": T10, "t11": T11, "same": SAME, "nl_last_of_block": int(starts[at + 1]) - 1,
             "nl_first_of_block": int(starts[at + 2]) - 1}
    return {"train": train.text(), "train_empty_c26": train_empty.text(), "test": test.text(),
            "facts": facts}


def criteo_malformed():
    """{name: text} that must raise: a blank line in the middle, a 41-field line."""
    good = [_criteo_line(0, *_criteo_fields(k)) for k in range(6)]
    blank = "\n".join(good[:3] + [""] + good[3:]) + "\n"
    wide = "\n".join(good[:3] + [good[3] + "\textra"] + good[4:]) + "\n"
    return {"blank_line": blank, "41_fields": wide}


# ---------------------------------------------------------------------------------------------
# rs_kv_parse / rs_aliccp_join
# ---------------------------------------------------------------------------------------------
S1, S2, S3 = "\x01", "\x02", "\x03"
N_COMMON_IDS = 6  # c0 .. c5, each referenced by every sixth skeleton line


def _tri(field, value, weight="1.0"):
    return f"{field}{S2}{value}{S3}{weight}"


def _padded(make, target):
    """make(pad) with the pad that gives the line a stripped length of exactly `target`."""
    line = make(target - len(make(0).strip()))
    assert len(line.strip()) == target
    return line


def _unwanted(n, start=0):
    return [_tri(f"9{start + i:03d}_14", 10000 + i, "0.6931") for i in range(n)]


def aliccp_edges():
    """{'skeleton', 'common', 'lines': name → skeleton line number}: sample ids of 0..129 bytes
    with a leading unwanted value of the same length (every comma and every kv separator
    passes through two 64-byte chunks), common lines of ~400
    triples (> 6 KB) and lines of exactly 4096 / 4097 stripped bytes in both files, a repeated
    column whose last occurrence lies beyond byte 4096, unwanted names '10' '1010' '3011', '301'
    as a value and as a weight, a trailing key, an empty last value, an empty kv field, strip()
    of ' ' and '\\x1f', a literal '0' in 508, a dropped (0, 1) line, '00' / '01' labels, and a
    duplicate common id."""
    # ---- common_id,count,kv ---------------------------------------------------------------
    # 508 and 301 never appear here: a column absent from a skeleton line stays absent
    common = []
    common.append("c0,3," + S1.join([_tri("101", "e101"), _tri("121", "e121"), _tri("10", "bad10"),
                                     _tri("1010", "bad1010"), _tri("3011", "bad3011")]))
    big = _unwanted(400)
    for at, (f, v) in {0: ("101", "b101"), 57: ("122", "b122"), 133: ("124", "b124"),
                       250: ("125", "b125"), 398: ("126", "b126"), 399: ("127", "b127")}.items():
        big[at] = _tri(f, v)
    common.append("c1,400," + S1.join(big))
    for cid, target in (("c2", STAGE), ("c3", STAGE + 1)):
        common.append(_padded(lambda pad: f"{cid},3," + S1.join(
            [_tri("128", f"v128{cid}"), _tri("150_14", "x" * pad), _tri("129", f"v129{cid}")]), target))
    # 121 twice: the second (winning) one starts beyond byte 4096
    common.append("c4,302," + S1.join([_tri("121", "e121")] + _unwanted(300) + [_tri("121", "l121"),
                                                                               _tri("101", "e101")]))
    common.append("c5,2," + S1.join([_tri("101", "old101"), _tri("122", "old122")]))
    common.append(" c5,1," + _tri("101", "new101") + " \x1f")  # duplicate id: the later line wins
    # ---- sample_id,click,purchase,common_id,count,kv --------------------------------------
    skel, names = [], {}

    def add(name, line):
        names[name] = len(skel)
        skel.append(line)

    for p in range(130):
        click, buy = [(0, 0), (1, 0), (1, 1)][p % 3]
        if p % 17 == 5:
            click, buy = 0, 1  # dropped
        tris = [_tri("999", "v" * p), _tri("205", 1000 + p % 3), _tri("206", 2000 + p % 5)]
        if p % 4 == 0:
            tris.append(_tri("508", "0"))  # the literal value '0'
        if p % 2:
            tris.append(_tri("3011", "bad3011"))
        if p % 5 == 0:
            tris.append(_tri("301", 5000))
        tris.append(_tri("207", 3000 + p % 2))
        add(f"p{p}", f"{'s' * p},{click},{buy},c{p % N_COMMON_IDS},{len(tris)},{S1.join(tris)}")
    add("301_as_value_and_weight",
        "v301,1,0,c0,2," + S1.join([_tri("999", "301", "301"), _tri("205", 1000)]))
    add("trailing_key", "tk,1,0,c0,2," + S1.join([_tri("205", 1001), _tri("206", 2001)]) + S1 + "216")
    add("empty_last_value", "ev,1,0,c0,2," + _tri("205", 1002) + S1 + "216" + S2)
    add("empty_kv", "ek,1,1,c1,0,")
    add("spaces", "  sp,1,0,c2,1," + _tri("205", 1000) + " \x1f ")
    add("labels_00_01", "zz,00,01,c3,1," + _tri("205", 1001))
    add("dropped", "dd,0,1,c0,1," + _tri("205", 1002))
    for name, target in (("len_4096", STAGE), ("len_4097", STAGE + 1)):
        add(name, _padded(lambda pad: f"{name},1,0,c4,3," + S1.join(
            [_tri("205", 1001), _tri("109_14", "y" * pad), _tri("216", "late216")]), target))
    add("repeat_beyond_4096", "rp,1,0,c5,303," + S1.join(
        [_tri("206", 2000)] + _unwanted(300, 500) + [_tri("206", 2004), _tri("207", 3001)]))

    def join(lines):
        return "".join(ln + ("\r\n" if i % 9 == 4 else "\n") for i, ln in enumerate(lines))

    return {"skeleton": join(skel), "common": join(common), "lines": names}


ALICCP_TOO_FEW_COMMAS = "s,1,0,c0,1\n"  # five fields: ll[5] raises IndexError in the reference


# ---------------------------------------------------------------------------------------------
# rs_dien_parse / rs_dien_item_cat / rs_dien_encode
# ---------------------------------------------------------------------------------------------
N_ITEMS, N_CATS = 900, 7


def _item(i, unseen=False):
    return f"{'Z' if unseen else 'B'}{i:09d}"  # 10 characters, as an ASIN


def _cat(i):
    return f"C{i % N_CATS}"


def _dien_line(label, user, item, cat, his_items, his_cats):
    return "\t".join([label, user, item, cat, S2.join(his_items), S2.join(his_cats)])


def _hist(start, n, unseen=False):
    idx = [(start + 3 * j) % N_ITEMS for j in range(n)]
    return [_item(i, unseen) for i in idx], [_cat(i) for i in idx]


def amazon_edges(unequal=True):
    """{'train', 'test', 'lines': name → train line number}. Users of 0..129 bytes, histories
    of 1 (also the empty one), 63, 64, 65, 200 and 700 tokens (10-character items: the 700-token line is over 4 KB), stripped
    lengths of exactly 4096 and 4097, labels '0' '1' '1.0', strip() of ' ' and '\\x1f', an item
    whose cat changes with its last pair on a line over 4 KB, no trailing newline; with
    `unequal` also n_hi > n_hc (partnerless items P*) and n_hi < n_hc. The test text has unseen
    items and known cats."""
    labels = ["0", "1", "1.0"]
    lines, names = [], {}

    def add(name, line):
        names[name] = len(lines)
        lines.append(line)

    for p in range(130):
        hi, hc = _hist(p, 3)
        add(f"p{p}", _dien_line(labels[p % 3], "u" * p, _item(p), _cat(p), hi, hc))
    hi, hc = _hist(7, 1)
    add("hist_1", _dien_line("1", "u1", _item(1), _cat(1), hi, hc))
    add("hist_empty", "0\tu2\t" + _item(2) + "\t" + _cat(2) + "\t\tC3")
    for n in (63, 64, 65, 200, 700):
        hi, hc = _hist(n, n)
        add(f"hist_{n}", _dien_line("1", f"u{n}", _item(n), _cat(n), hi, hc))
    for name, target in (("len_4096", STAGE), ("len_4097", STAGE + 1)):
        hi, hc = _hist(11, 280)
        add(name, _padded(lambda pad: _dien_line("0", "w" * pad, _item(5), _cat(5), hi, hc), target))
    add("spaces", " 1.0\tu3\t" + _item(3) + "\t" + _cat(3) + "\t" + _item(4) + "\t" + _cat(4) + " \x1f")
    if unequal:
        hi, hc = _hist(20, 70)
        add("more_items", _dien_line("1", "u4", _item(6), _cat(6),
                                     hi + [f"P{j:09d}" for j in range(5)], hc))
        hi, hc = _hist(30, 3)
        add("more_cats", _dien_line("0", "u5", _item(8), _cat(8), hi, hc + ["C1", "C2", "C5"]))
        add("one_item_many_cats", _dien_line("0", "u6", _item(9), _cat(9), [_item(10)],
                                             ["C4", "C5", "C6"]))
    # CHG is paired with C1 early and with C5 as the last pair of a line over 4 KB (the target
    # pair comes first in the stream, the history pairs after it)
    add("chg_early", _dien_line("1", "u7", "CHG0000001", "C1", ["CHG0000001"], ["C1"]))
    hi, hc = _hist(40, 400)
    add("chg_late", _dien_line("1", "u8", "CHG0000001", "C2", hi + ["CHG0000001"], hc + ["C5"]))
    train = "".join(ln + ("\r\n" if i % 9 == 4 else "\n") for i, ln in enumerate(lines[:-1]))
    train += lines[-1]  # no trailing newline
    # ---- test -------------------------------------------------------------------------------
    tl = []
    for n in (1, 62, 63, 64, 65, 66, 128, 129, 130, 450):
        hi, hc = _hist(n + 1, n)
        hz, _ = _hist(n + 1, n, unseen=True)
        mixed = [z if j % 4 == 1 else h for j, (h, z) in enumerate(zip(hi, hz))]
        tl.append(_dien_line(labels[n % 3], f"t{n}", _item(n, unseen=n % 2 == 0), _cat(n), mixed, hc))
    tl.append("0\tt\t" + _item(2) + "\tC3\t\tC3")
    tl.append(" 1\tt\t" + _item(3) + "\tC0\t" + _item(4) + "\tC1 \x1f")
    if unequal:
        hi, hc = _hist(3, 80)
        tl.append(_dien_line("1", "t", _item(1), "C1", hi, hc[:30]))
        tl.append(_dien_line("1", "t", _item(1), "C1", hi[:2], hc))
    test = "".join(ln + "\n" for ln in tl)
    return {"train": train, "test": test, "lines": names}


def amazon_partnerless():
    """A train text in which most items have no cat partner (40 history items against one
    history cat per line): a negative draw lands on one of them with near certainty."""
    lines = []
    for k in range(20):
        lines.append(_dien_line("1", f"u{k}", _item(k), _cat(k),
                                [f"Q{k:04d}{j:05d}" for j in range(40)], [_cat(k)]))
    return "".join(ln + "\n" for ln in lines)


# ---------------------------------------------------------------------------------------------
# rs_tfrecord_parse_criteo: kRecMax
# ---------------------------------------------------------------------------------------------
def tfrecord_padded(ints, cats, label, payload_len):
    """One framed record: the canonical Example plus an unknown bytes feature sized so that the
    Example is exactly `payload_len` bytes."""
    F = OT.field

    def entry(key, feature):
        return F(1, 2, F(1, 2, key) + F(2, 2, feature))

    def example(key, pad):
        feats = (entry(b"int_features", F(1, 2, F(1, 2, OT.tensor_proto(np.asarray(ints, np.float32)))))
                 + entry(key, F(1, 2, F(1, 2, b"\xab" * pad)))
                 + entry(b"cat_features", F(1, 2, F(1, 2, OT.tensor_proto(np.asarray(cats, np.int64)))))
                 + entry(b"label", F(3, 2, F(1, 2, OT.varint(int(label))))))
        return F(1, 2, feats)

    for key in (b"pad", b"padd", b"paddi"):  # a varint length growing a byte can skip a size
        pad = payload_len - len(example(key, 0))
        for p in range(max(pad - 12, 0), pad + 1):
            ex = example(key, p)
            if len(ex) == payload_len:
                return OT.frame(ex), ex
    raise AssertionError(f"no padding gives a payload of {payload_len} bytes")
