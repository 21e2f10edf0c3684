"""tests/item_softmax_ref.py against torch float64 autograd of the materialised formula, every case
generator having the property it is named for, and rho32 (the float32 restatement's error, which
sets the GPU suite's tolerance) — all without a GPU."""
import numpy as np
import pytest
import torch

from tests import item_softmax_ref as R


def torch_eval(c):
    """loss and both gradients by torch float64 autograd over the [B, M] logits."""
    q = torch.tensor(c["q"], dtype=torch.float64, requires_grad=True)
    v = torch.tensor(c["v"], dtype=torch.float64, requires_grad=True)
    B, M = q.shape[0], v.shape[0]
    t = torch.arange(B) if c["targets"] is None else torch.tensor(c["targets"], dtype=torch.int64)
    z = (q @ v.T) * c["inv_temp"]
    if c["bias"] is not None:
        z = z - torch.tensor(c["bias"], dtype=torch.float64)[None]
    if c["ids"] is not None:
        ids = torch.tensor(c["ids"])
        drop = (ids[None, :] == ids[t][:, None]) & (torch.arange(M)[None, :] != t[:, None])
        z = z.masked_fill(drop, float("-inf"))
    lse = torch.logsumexp(z, 1)
    loss = lse - z[torch.arange(B), t]
    g = torch.tensor(c["g"], dtype=torch.float64)
    (loss * g).sum().backward()
    return {"loss": loss.detach().numpy(), "lse": lse.detach().numpy(), "dq": q.grad.numpy(),
            "dv": v.grad.numpy()}


@pytest.mark.parametrize("name", ["B33", "M1", "M129", "dim3", "dim65", "targets_None",
                                  "targets_reversed", "targets_same", "ids_None", "ids_equal",
                                  "ids_extreme", "dup_31_32", "mag_1_20.0", "zero_g", "splits2"])
def test_float64_restatement_is_torch_autograd(name):
    c, r64, _ = R.case(name)
    t = torch_eval(c)
    for n in R.OUT:
        np.testing.assert_allclose(r64[n], t[n], rtol=1e-11, atol=1e-12, err_msg=n)


def test_case_list_covers_the_sizes_and_paths():
    cs = {n: R.case(n)[0] for n in list(R.CASES) + list(R.MAG_CASES)}
    assert {c["q"].shape[0] for c in cs.values()} >= set(R.B_SIZES)
    assert {c["v"].shape[0] for c in cs.values()} >= set(R.M_SIZES)
    assert {c["q"].shape[1] for c in cs.values()} >= set(R.DIMS)
    assert {c["n_splits"] for c in cs.values()} >= set(R.SPLITS)
    assert {c["inv_temp"] for c in cs.values()} >= {1.0, 20.0}
    assert any(c["targets"] is None for c in cs.values())
    assert any(c["bias"] is not None and (c["bias"] > 0).any() and (c["bias"] < 0).any()
               for c in cs.values())
    for c in cs.values():  # every pooled case is finite
        assert all(np.isfinite(r).all() for r in R.evaluate(c).values())


def test_target_kinds():
    c = R.case("targets_identity")[0]
    assert (c["targets"] == np.arange(33)).all()
    c = R.case("targets_reversed")[0]
    assert (c["targets"] == 39 - np.arange(33)).all()
    assert len(set(R.case("targets_same")[0]["targets"])) == 1
    assert (R.case("targets_last")[0]["targets"] == 39).all()


def test_dominant_cases_dominate_by_30():
    n = 0
    for name in R.CASES:
        if not name.startswith("dom_"):
            continue
        n += 1
        c, r64, _ = R.case(name)
        _, ns, as_t, col = name.split("_")
        z = c["q"].astype(np.float64) @ c["v"].astype(np.float64).T
        others = np.delete(z, int(col), 1)
        assert (z[:, int(col)] >= others.max(1) + 30).all()
        assert (c["targets"] == int(col)).all() == bool(int(as_t))
        if not int(as_t):
            assert (c["targets"] != int(col)).all()
        # a kernel that dropped the column would be off by 30 or more in lse
        d = dict(c, v=np.delete(c["v"], int(col), 0),
                 targets=np.zeros_like(c["targets"]))
        assert (r64["lse"] - R.evaluate(d)["lse"] >= 30).all()
    assert n >= 100


def test_edge_columns_sit_on_every_boundary():
    assert R.edge_columns(300, 1) == [0, 31, 32, 127, 128, 159, 160, 299]
    e2 = R.edge_columns(300, 2)
    assert {149, 150, 150 + 31, 150 + 32, 150 + 127, 150 + 128, 299} <= set(e2)
    e7 = R.edge_columns(300, 7)
    assert {41, 42, 83, 84, 251, 252, 252 + 31, 252 + 32, 299} <= set(e7)


def test_duplicate_cases_contain_accidental_hits():
    for name in ("dup_31_32", "dup_32_31", "dup_127_128", "dup_128_127"):
        c, r64, _ = R.case(name)
        t, d = (int(x) for x in name.split("_")[1:])
        assert t // R.TILE != d // R.TILE and abs(t - d) == 1  # the two sides of a tile edge
        assert c["ids"][t] == c["ids"][d] and (c["targets"] == t).all()
        kept, valid, _ = R.kept_mask(5, 200, c["targets"].astype(np.int64), c["ids"])
        assert valid.all() and not kept[:, d].any() and kept.sum() == 5 * 199
        # keeping the duplicate (the row's largest logit) would move lse by 30 or more
        assert (R.evaluate(dict(c, ids=None))["lse"] - r64["lse"] >= 30).all()
    c = R.case("ids_some" if "ids_some" in R.CASES else "B33")[0]
    kept, _, _ = R.kept_mask(c["q"].shape[0], c["v"].shape[0], c["targets"].astype(np.int64),
                             c["ids"])
    assert not kept.all()
    c = R.case("ids_distinct")[0]
    assert len(set(c["ids"])) == 70
    c = R.case("ids_extreme")[0]
    assert {np.iinfo(np.int64).min, np.iinfo(np.int64).max} <= set(c["ids"])


def test_every_id_equal_keeps_the_target_only():
    c, r64, _ = R.case("ids_equal")
    assert (r64["loss"] == 0).all() and (r64["dq"] == 0).all() and (r64["dv"] == 0).all()


def test_magnitude_cases_reach_1e4_and_stay_finite():
    for sign in (1, -1):
        for it in (1.0, 20.0):
            c, r64, _ = R.case(f"mag_{sign}_{it}")
            z = it * (c["q"].astype(np.float64) @ c["v"].astype(np.float64).T)
            assert np.abs(z).max() >= 9.9e3 and (np.sign(z) == sign).all()
            assert all(np.isfinite(r).all() for r in r64.values())


def test_grad_loss_spans_six_decades_and_has_zero_rows():
    c, r64, _ = R.case("zero_g")
    assert (c["g"][[1, 7, 33, 38]] == 0).all()
    assert (r64["dq"][[1, 7, 33, 38]] == 0).all() and (r64["dq"][2] != 0).any()
    nz = np.abs(c["g"][c["g"] != 0])
    assert nz.max() >= 1e3 * 0.999 and nz.min() <= 1e-3 * 1.001
    assert (c["g"] > 0).any() and (c["g"] < 0).any()


def test_inf_bias_is_the_column_left_out():
    c, d, keep = R.inf_bias_case()
    rc, rd = R.evaluate(c), R.evaluate(d)
    assert all(np.isfinite(r).all() for r in rc.values())
    np.testing.assert_allclose(rc["loss"], rd["loss"], rtol=1e-13)
    np.testing.assert_allclose(rc["dq"], rd["dq"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(rc["dv"][keep], rd["dv"], rtol=1e-12, atol=1e-15)
    assert (rc["dv"][~keep] == 0).all()


def test_nan_query_row_poisons_what_the_contract_says():
    r = R.evaluate(R.nan_query_case(3))
    for n in ("loss", "lse"):
        assert np.isnan(r[n][3]) and np.isfinite(np.delete(r[n], 3)).all()
    assert np.isnan(r["dq"][3]).all() and np.isfinite(np.delete(r["dq"], 3, 0)).all()
    assert np.isnan(r["dv"]).all()  # every column has a term c(3, j) · queries[3]


def test_bad_target_rows_are_nan_and_add_nothing():
    c = R.random_case(3, 6, 9, 4)
    c["targets"][[1, 4]] = [-1, 9]
    r = R.evaluate(c)
    assert np.isnan(r["loss"][[1, 4]]).all() and np.isnan(r["lse"][[1, 4]]).all()
    assert (r["dq"][[1, 4]] == 0).all() and np.isfinite(r["dv"]).all()
    keep = np.array([0, 2, 3, 5])
    d = dict(c, q=c["q"][keep], targets=c["targets"][keep], g=c["g"][keep])
    np.testing.assert_allclose(r["dv"], R.evaluate(d)["dv"], rtol=1e-13, atol=1e-18)


def test_infinite_logits_follow_ieee():
    c = R.random_case(4, 3, 5, 4, ids=None)
    c["bias"][:] = [np.inf, 0, 0, 0, -np.inf]
    c["targets"][:] = [1, 0, 4]
    r = R.evaluate(c)
    assert r["lse"][0] == np.inf and r["loss"][1] == np.inf and np.isnan(r["loss"][2])
    assert R.same_pattern(R.evaluate(c, np.float32)["dq"], r["dq"])


def test_measures():
    ref = {"loss": np.array([1.0, np.nan]), "lse": np.array([2.0, 3.0]),
           "dq": np.array([[1.0, -4.0], [0.0, 0.0]]), "dv": np.array([[0.5, 0.25]])}
    got = {"loss": np.array([1.5, np.nan]), "lse": np.array([2.0, 3.0]),
           "dq": np.array([[1.0, -3.0], [0.0, 0.0]]), "dv": np.array([[0.5, 0.25]])}
    r = R.ratios(got, ref)
    assert r == {"loss": 0.5, "lse": 0.0, "dq": 1.0 / 8.0, "dv": 0.0}
    got["dq"] = np.array([[1.0, -4.0], [1e-30, 0.0]])
    assert R.ratios(got, ref)["dq"] == np.inf
    assert R.same_pattern(got["loss"], ref["loss"]) and not R.same_pattern(got["lse"], ref["loss"])
    assert not R.same_pattern(np.array([np.inf]), np.array([-np.inf]))


def test_rho32_is_finite_and_the_structural_cases_are_1000_times_it():
    rho = R.rho32()
    print("\n  rho32 over %d cases: %s" % (len(R.CASES), " ".join(f"{n}={r:.3g}" for n, r in rho.items())))
    assert all(0 < r < np.inf for r in rho.values())
    for name in R.CASES:
        assert all(R.case(name)[2][n] <= rho[n] for n in R.OUT)
    assert 30 >= 1000 * 4 * rho["lse"] and 30 >= 1000 * 4 * rho["loss"]
    assert max(rho.values()) < 1e-4  # the pool is well conditioned: the figure means something
    mag = R.rho32(mag=True)
    print("  rho32 over the %d magnitude cases: %s"
          % (len(R.MAG_CASES), " ".join(f"{n}={r:.3g}" for n, r in mag.items())))
    assert all(rho[n] < mag[n] < np.inf for n in R.OUT)
