"""GPU parity of the text scanners (rs_line_index, rs_criteo_parse, rs_kv_parse, rs_dien_parse,
rs_dien_item_cat, rs_dien_encode) and of the TFRecord staging limit on the texts of
tests/ingest_edges.py: lines longer than the 4,096-byte LDS stage (scanned in place), lines of
exactly 4,096 and 4,097 bytes, separators on the 64-byte ballot edges, newlines on the block and
wave-quarter edges of the line index, and the parsing rules the generated texts never reach.
tests/test_ingest_edges_cpu.py asserts that the texts have those properties. Everything is
bit-exact against oracle/criteo.py, oracle/textpipe.py and NumPy, except the Criteo dense
features (log(x + 1) in fp32: rtol 2e-7 as in tests/test_criteo_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import criteo as OC
from oracle import textpipe as O
from oracle import tfrecord as OT
from recommender_amd.data import AliCCPVocab, CriteoVocab, DienVocab, aliccp_join, read_tfrecord
from recommender_amd.data.aliccp import parse_kv_csv
from recommender_amd.data.criteo import read_criteo_tsv
from recommender_amd.data.text import fnv1a64, line_index, text_to_device
from tests import ingest_edges as E

pytestmark = pytest.mark.gpu

# ---- line index ---------------------------------------------------------------------------
LINE_CASES = dict(E.line_index_cases())


@pytest.mark.parametrize("name", list(LINE_CASES))
def test_line_index_matches_numpy(name):
    data = np.frombuffer(LINE_CASES[name], np.uint8)
    nl = np.flatnonzero(data == 10)
    ref = np.concatenate([[0], nl + 1]).astype(np.int64)
    starts, n_lines = line_index(text_to_device(LINE_CASES[name], "cuda"))
    assert n_lines == (nl.size if data[-1] == 10 else nl.size + 1)
    assert starts.numel() == nl.size + 1
    np.testing.assert_array_equal(starts.cpu().numpy()[:nl.size + 1], ref)


# ---- Criteo -------------------------------------------------------------------------------
@functools.lru_cache(None)
def _criteo():
    return E.criteo_edges()


@pytest.mark.parametrize("which", ["train", "train_empty_c26"])
def test_criteo_edges_match_oracle(which):
    c = _criteo()
    train, f = c[which], c["facts"]
    vocab = OC.build_vocab(train)
    v = CriteoVocab.build(train.encode())
    assert v.size == len(vocab)
    for text in (train, c["test"]):
        cat, dense, label = v.encode(text.encode())
        rc, rd, rl = OC.encode(text, vocab)
        np.testing.assert_array_equal(cat.cpu().numpy(), rc)
        np.testing.assert_array_equal(label.cpu().numpy(), rl)
        got = dense.cpu().numpy()
        nz = rd != 0
        rel = np.abs(got[nz].astype(np.float64) - rd[nz]) / np.abs(rd[nz].astype(np.float64))
        print(f"criteo dense ({which}): max relative error {rel.max():.3g}")
        np.testing.assert_allclose(got, rd, rtol=2e-7, atol=0)
    # the first test line carries T10 in C3, T11 in C4 and SAME in C1 and C26 (with its '\n')
    ids = cat.cpu().numpy()[0]
    assert f["t10"] not in vocab and ids[2] == 0          # seen 10 times: OOV → 0
    assert ids[3] == vocab[f["t11"]] and ids[3] != 0      # seen 11 times: its own id
    assert ids[0] == vocab[f["same"]] and ids[25] == vocab[f["same"] + "\n"] and ids[0] != ids[25]


@pytest.mark.parametrize("name", ["blank_line", "41_fields"])
def test_criteo_malformed_raises(name):
    with pytest.raises(ValueError):
        read_criteo_tsv(E.criteo_malformed()[name].encode())


# ---- Ali-CCP ------------------------------------------------------------------------------
@functools.lru_cache(None)
def _aliccp():
    a = E.aliccp_edges()
    rows = O.aliccp_join(a["skeleton"], a["common"])
    return a, rows, O.aliccp_vocab(rows)


def test_aliccp_edges_match_oracle():
    a, rows, vocab = _aliccp()
    g_rows = aliccp_join(a["skeleton"].encode(), a["common"].encode())
    assert g_rows.n == len(rows)
    v = AliCCPVocab.build(g_rows)
    assert v.sizes == [len(m) for m in vocab]
    feats, lab = v.encode(g_rows)
    ids, rl = O.aliccp_encode(rows, vocab)
    got = torch.cat([feats[c] for c in O.ALICCP_COLUMNS], 1).cpu().numpy()
    np.testing.assert_array_equal(got, ids)
    np.testing.assert_array_equal(lab.cpu().numpy(), rl)
    np.testing.assert_array_equal(
        g_rows.present.cpu().numpy().astype(bool), [[x is not None for x in r[2]] for r in rows])


@pytest.mark.parametrize("which,key_field,kv_field", [("skeleton", 3, 5), ("common", 0, 2)])
def test_kv_parse_per_line_matches_re_split(which, key_field, kv_field):
    """present and the value hash of every (line, column) against dict(zip(...)) of re.split:
    the vocabulary threshold cannot mask a wrongly matched key or a wrong occurrence."""
    a, _, _ = _aliccp()
    lines = [ln.strip().split(",") for ln in E.lines_of(a[which])]
    with_labels = which == "skeleton"
    kv = parse_kv_csv(a[which].encode(), key_field, kv_field, with_labels)
    dicts = [O._kv(ll[kv_field]) for ll in lines]
    present = np.array([[c in d for c in O.ALICCP_COLUMNS] for d in dicts])
    np.testing.assert_array_equal(kv.present.cpu().numpy().astype(bool), present)
    vals = np.array([[fnv1a64(d[c].encode()) if c in d else 0 for c in O.ALICCP_COLUMNS]
                     for d in dicts], np.int64)
    np.testing.assert_array_equal(kv.vals.cpu().numpy(), vals)
    np.testing.assert_array_equal(kv.key_hash.cpu().numpy(),
                                  np.array([fnv1a64(ll[key_field].encode()) for ll in lines], np.int64))
    if with_labels:
        np.testing.assert_array_equal(kv.labels.cpu().numpy(),
                                      [[int(ll[1]), int(ll[2])] for ll in lines])
        np.testing.assert_array_equal(kv.keep.cpu().numpy(),
                                      [not (ll[1] == "0" and ll[2] == "1") for ll in lines])


def test_aliccp_too_few_commas_raises():
    a, _, _ = _aliccp()
    with pytest.raises(ValueError):
        parse_kv_csv(E.ALICCP_TOO_FEW_COMMAS.encode(), 3, 5, True)
    with pytest.raises(ValueError):
        aliccp_join((a["skeleton"] + E.ALICCP_TOO_FEW_COMMAS).encode(), a["common"].encode())


# ---- Amazon -------------------------------------------------------------------------------
@functools.lru_cache(None)
def _amazon(unequal=True):
    z = E.amazon_edges(unequal)
    items, cats, i2c = O.dien_vocab(z["train"])
    return z, items, cats, O.dien_cat_of_item(items, cats, i2c, missing=-1)


@pytest.mark.parametrize("maxlen", [1, 63, 64, 65, 129])
def test_amazon_edges_match_oracle(maxlen):
    z, items, cats, coi = _amazon()
    v = DienVocab.build(z["train"].encode())
    assert v.n_item_ids == len(items) and v.n_cat_ids == len(cats)
    assert (coi == -1).sum() == 5  # the partnerless items
    np.testing.assert_array_equal(v.cat_of_item.cpu().numpy(), coi)
    for text in (z["train"], z["test"]):
        feats, lab = v.encode(text.encode(), maxlen=maxlen)
        rf, rl = O.dien_encode(text, items, cats, maxlen)
        for k in rf:
            np.testing.assert_array_equal(feats[k].cpu().numpy(), rf[k], err_msg=k)
        np.testing.assert_array_equal(lab.cpu().numpy(), rl)
    assert (rf["target_item"] == items["unk"]).any() and (rf["pos_his_item"] == items["unk"]).any()


def test_amazon_negative_on_partnerless_item_raises():
    text = E.amazon_partnerless()
    v = DienVocab.build(text.encode())
    assert (v.cat_of_item == -1).float().mean().item() > 0.9
    v.encode(text.encode(), maxlen=100)  # without negatives the text encodes
    with pytest.raises(KeyError):
        v.encode(text.encode(), maxlen=100, sample_negative=True, seed=4)


def test_amazon_negatives_follow_cat_of_item():
    z, items, cats, coi = _amazon(False)
    assert (coi >= 0).all()
    v = DienVocab.build(z["train"].encode())
    np.testing.assert_array_equal(v.cat_of_item.cpu().numpy(), coi)
    for text in (z["train"], z["test"]):
        f, _ = v.encode(text.encode(), maxlen=65, sample_negative=True, seed=4)
        ni, nc = f["neg_his_item"].cpu().numpy(), f["neg_his_cat"].cpu().numpy()
        assert ni.min() >= 1 and ni.max() <= len(items) - 1
        np.testing.assert_array_equal(nc, coi[ni])
        rf, _ = O.dien_encode(text, items, cats, 65)
        np.testing.assert_array_equal(f["pos_his_item"].cpu().numpy(), rf["pos_his_item"])


# ---- TFRecord staging limit (kRecMax = 4096) -----------------------------------------------
def _tf_arrays():
    rng = np.random.default_rng(4096)
    ints = np.log1p(rng.geometric(0.01, (3, 13))).astype(np.float32)
    cats = rng.integers(0, 1 << 40, (3, 26)).astype(np.int64)
    return ints, cats, np.array([1, 0, -1], np.int64)


@pytest.mark.parametrize("verify_crc", [True, False])
def test_tfrecord_payload_of_exactly_4096_bytes_parses(verify_crc):
    ints, cats, labels = _tf_arrays()
    big, ex = E.tfrecord_padded(ints[1], cats[1], labels[1], E.STAGE)
    assert len(ex) == 4096
    data = (OT.frame(OT.example(ints[0], cats[0], labels[0])) + big
            + OT.frame(OT.example(ints[2], cats[2], labels[2])))
    for src, rows in ((big, [1]), (data, [0, 1, 2])):
        feats, lab = read_tfrecord(src, verify_crc=verify_crc)
        np.testing.assert_array_equal(feats["int_features"].cpu().numpy(), ints[rows])
        np.testing.assert_array_equal(feats["cat_features"].cpu().numpy(), cats[rows])
        np.testing.assert_array_equal(lab.cpu().numpy(), labels[rows])


@pytest.mark.parametrize("verify_crc", [True, False])
def test_tfrecord_payload_of_4097_bytes_raises(verify_crc):
    ints, cats, labels = _tf_arrays()
    big, ex = E.tfrecord_padded(ints[1], cats[1], labels[1], E.STAGE + 1)
    assert len(ex) == 4097
    for src in (big, OT.frame(OT.example(ints[0], cats[0], labels[0])) + big):
        with pytest.raises(ValueError):
            read_tfrecord(src, verify_crc=verify_crc)
