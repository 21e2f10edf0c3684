"""rs_dien_users / data.amazon.read_dien_users against text.fnv1a64 of each line's user field on a
small hand-made file, the malformed-line flag, and the file → GroupAUC path end to end."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from recommender_amd.data.amazon import read_dien_text, read_dien_users
from recommender_amd.data.text import FNV_BASIS, fnv1a64, line_index, text_to_device
from tests import group_auc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
FILL = 0x5A5A5A5A5A5A5A5A

LONG_USER = bytes(65 + i % 26 for i in range(300))  # longer than a wave's 64-byte staging stride
USERS = [b"A1", b"", b"u", LONG_USER, "用户é".encode(), b"A1", b"B\xff\x80", b"u", b"last", b"A1"]
LABELS = [1, 0, 1, 0, 1, 0, 0, 1, 1, 0]


def make_file(users=USERS, labels=LABELS):
    """label \\t user \\t item \\t cat \\t his_items \\t his_cats; every third line ends in CRLF, the
    last line has no newline."""
    lines = []
    for i, (u, y) in enumerate(zip(users, labels)):
        line = b"\t".join([str(y).encode(), u, b"i%d" % (i % 4), b"c%d" % (i % 2),
                           b"\x02".join(b"i%d" % k for k in range(1 + i % 3)),
                           b"\x02".join(b"c%d" % (k % 2) for k in range(1 + i % 3))])
        lines.append(line + (b"" if i == len(users) - 1 else b"\r\n" if i % 3 == 0 else b"\n"))
    return b"".join(lines)


def raw_users(data):
    """rs_dien_users through the C entry point → (hashes, error flag); guards checked."""
    text = text_to_device(data, torch.device(DEV))
    starts, n = line_index(text)
    out = torch.full((n + GUARD,), FILL, dtype=torch.int64, device=DEV)
    err = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    st = L.lib().rs_dien_users(L.ptr(text), text.numel(), L.ptr(starts), n, L.ptr(out), L.ptr(err),
                               L.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert st == 0, L.lib().rs_last_error()
    out, err = out.cpu().numpy(), err.cpu().numpy()
    assert (out[n:] == FILL).all() and (err[1:] == 0).all()
    return out[:n], int(err[0])


def test_user_hashes_are_fnv1a64_of_the_user_bytes():
    data = make_file()
    assert not data.endswith(b"\n") and b"\r\n" in data
    want = np.array([fnv1a64(u) for u in USERS], np.int64)
    got, err = raw_users(data)
    np.testing.assert_array_equal(got, want)
    assert err == 0
    assert got[0] == got[5] == got[9] and got[2] == got[7]  # the same user on non-adjacent lines
    assert got[1] == fnv1a64(b"")  # the empty user field hashes to the basis
    np.testing.assert_array_equal(read_dien_users(data, DEV).cpu().numpy(), want)
    assert read_dien_users(b"", DEV).numel() == 0


def test_a_five_field_line_sets_the_flag_and_raises():
    lines = make_file().split(b"\n")
    lines[4] = b"1\tuser\titem\tcat\thist"  # five fields
    data = b"\n".join(lines)
    got, err = raw_users(data)
    assert err == L.RS_ERRBIT_OOB
    basis = FNV_BASIS - (1 << 64) if FNV_BASIS >= (1 << 63) else FNV_BASIS
    assert got[4] == basis
    ok = [i for i in range(len(USERS)) if i != 4]
    np.testing.assert_array_equal(got[ok], [fnv1a64(USERS[i]) for i in ok])
    with pytest.raises(ValueError):
        read_dien_users(data, DEV)


def test_file_to_gauc_end_to_end():
    from recommender_amd.metrics import GroupAUC

    rng = np.random.default_rng(21)
    names = [b"user%d" % i for i in range(12)] + [b"", LONG_USER]
    users = [names[i] for i in rng.integers(0, len(names), 400)]
    labels = rng.integers(0, 2, 400).tolist()
    data = make_file(users, labels)
    pred = (rng.integers(0, 40, 400) / 40).astype(np.float32)  # the fixed scores, with ties
    toks = read_dien_text(data, DEV)
    group = read_dien_users(data, DEV)
    np.testing.assert_array_equal(toks.label.cpu().numpy(), labels)
    # users grouped by their byte strings in Python
    index = {u: i for i, u in enumerate(sorted(set(users)))}
    by_bytes = R.counts_fast(pred, np.array(labels, np.float32), np.array([index[u] for u in users]))
    by_hash = R.counts_fast(pred, np.array(labels, np.float32), np.array([fnv1a64(u) for u in users]))
    for weight in R.WEIGHTS:
        m = GroupAUC(weight=weight)
        m.update_state(toks.label, torch.from_numpy(pred).to(DEV), group)
        for a, b in zip(m.groups(), by_hash):
            np.testing.assert_array_equal(a, b)
        assert m.result() == float(R.gauc_exact(*by_bytes, weight))
