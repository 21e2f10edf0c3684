"""The reference side of the layer-wise PinSage inference tests, checked without a GPU
(tests/pinsage_infer_ref.py):
  * the float64 restatement equals a literal join / group-by / divide / append / normalise loop
    written from pinsage/inference/inference.py:8-41;
  * a float32 NumPy form of the kernel's arithmetic stays within the GPU tests' tolerance on
    every GPU test input — the bound is reachable in fp32 before any GPU run;
  * those inputs have the properties the GPU tests rely on."""
import numpy as np
import pytest

from tests import pinsage_infer_ref as R


def test_restatement_equals_the_spark_loop():
    rng = np.random.default_rng(0)
    n, d_in, hidden, d_out = 6, 4, 3, 5
    feats = rng.normal(size=(n, d_in))
    w1, b1 = rng.normal(size=(d_in, hidden)), rng.normal(size=hidden)
    w2_hn, b2 = rng.normal(size=(d_in + hidden, d_out)), rng.normal(size=d_out)
    # item 3 has no neighbour (the inner join drops it); item 4 lists itself and one id twice
    nbr = np.array([[1, 2, -1], [0, 5, 3], [-1, 4, 0], [-1, -1, -1], [4, 1, 1], [2, -1, -1]], np.int32)
    cnt = np.array([[3, 1, 0], [2, 2, 7], [0, 5, 1], [0, 0, 0], [1, 4, 2], [6, 0, 0]], np.int32)
    edges = [(i, int(nbr[i, j]), int(cnt[i, j])) for i in range(n) for j in range(3)
             if nbr[i, j] >= 0]
    loop = R.spark_convolve_loop({i: feats[i].tolist() for i in range(n)}, edges, w1, b1, w2_hn, b2)
    assert sorted(loop) == [0, 1, 2, 4, 5]
    # the trained model's order is [nv ; h]: the demo's [h ; nv] kernel with its rows permuted
    w2 = np.concatenate([w2_hn[d_in:], w2_hn[:d_in]], 0)
    u = feats @ w1 + b1  # the demo's fc has no relu (activation=None)
    ref = R.layer_ref(feats, u, nbr, cnt, w2, b2, relu=False, norm="row")
    for it, row in loop.items():
        np.testing.assert_allclose(ref["out"][it], row, rtol=1e-12, atol=1e-14)
    # the dropped item keeps a row here: nv = 0, the weight sum clipped to 1
    y3 = feats[3] @ w2_hn[:d_in] + b2
    np.testing.assert_allclose(ref["out"][3], y3 / np.linalg.norm(y3), rtol=1e-12)


CASES = [(n, s, k) for n in R.N_ITEMS for s in R.SHAPES for k in R.KS]


@pytest.mark.parametrize("n,shape,k", CASES)
def test_fp32_form_within_tolerance_and_input_properties(n, shape, k):
    c = R.make_case(n, *shape, k)
    ok, oob = R.valid_slots(c["nbr"], c["cnt"], n)
    assert not oob.any()
    # the row patterns the GPU tests count on
    rows = np.arange(n)
    assert not ok[rows % 10 == 4].any(), "pattern 4 rows are entirely empty"
    assert (c["cnt"][rows % 10 == 7, k - 1] == 512).all()
    p8 = rows % 10 == 8
    assert (c["cnt"][p8, 0] == 0).all() and (c["nbr"][p8, 0] >= 0).all()
    p9 = rows % 10 == 9
    assert (c["nbr"][p9, k - 1] == n - 1).all() and (k == 1 or (c["nbr"][p9, 0] == 0).all())
    assert (c["nbr"][rows % 10 == 5, 0] == rows[rows % 10 == 5]).all()
    if k >= 2:
        p6 = rows % 10 == 6
        assert (c["nbr"][p6, 0] == c["nbr"][p6, 1]).all()
    for relu in (False, True):
        for norm in R.NORMS:
            ref = R.layer_ref(c["h"], c["u"], c["nbr"], c["cnt"], c["w2"], c["b2"], relu, norm)
            got = R.layer_f32(c["h"], c["u"], c["nbr"], c["cnt"], c["w2"], c["b2"], relu, norm)
            # includes: at most 1 % of the rows fall under the small-norm threshold
            R.assert_layer_close(got, ref, f"n {n} {shape} k {k} relu {relu} norm {norm}")


def test_negative_row_case_properties():
    c = R.negative_row_case()
    ref = R.layer_ref(c["h"], c["u"], c["nbr"], c["cnt"], c["w2"], c["b2"], True, "row")
    r = c["neg_row"]
    assert (ref["pre"][r] < -1e-3 * ref["M"][r]).all(), "every pre-activation of the row is negative"
    assert (ref["out"][r] == 0).all() and not ref["check"][r]
    others = np.arange(c["n"]) != r
    assert ref["check"][others].all(), "the built row is the only one under the threshold"
    got = R.layer_f32(c["h"], c["u"], c["nbr"], c["cnt"], c["w2"], c["b2"], True, "row")
    assert (got[r] == 0).all()
    R.assert_layer_close(got, ref, "negative row case")


def test_bad_id_inputs_are_flagged_by_the_reference():
    c = R.make_case(R.T + 1, 24, 32, 16, 3)
    nbr = c["nbr"].copy()
    nbr[2, 0], nbr[9, 1], nbr[40, 2] = c["n"], 2**31 - 1, -7
    ok, oob = R.valid_slots(nbr, c["cnt"], c["n"])
    assert oob.sum() == 3 and not ok[oob].any()
