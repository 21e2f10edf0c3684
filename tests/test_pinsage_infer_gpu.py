"""GPU tests of the layer-wise PinSage inference (recommender_amd/pinsage/inference.py,
rs_pinsage_infer_layer) against the float64 restatement and the tolerances of
tests/pinsage_infer_ref.py: one layer at every tile edge, width and slot count; bit-exact
invariances (run to run, truncated table, chunked neighbour table); agreement with the trained
model's own Convolve and with the unfused composition; the whole chain stage by stage, each
reference stage fed the GPU's previous stage; out-of-range neighbour ids."""
import numpy as np
import pytest
import torch

from oracle import pinsage as O
from recommender_amd import _lib as L
from recommender_amd.pinsage import (PinSageModel, PinSageSampler, convolve, infer_item_reprs,
                                     item_neighbors)
from recommender_amd.pinsage import inference as I
from recommender_amd.pinsage.evaluation import hit_rate_eval, recommend
from recommender_amd.pinsage.graph import HeteroGraph
from tests import pinsage_infer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_kernel(c, relu, norm, n=None, nbr=None):
    """rs_pinsage_infer_layer on the first n items of case c: (out [n, d_out] NumPy, err flag)."""
    n = c["n"] if n is None else n
    h, u = dev(c["h"][:n]), dev(c["u"][:n])
    nb, ct = dev((c["nbr"] if nbr is None else nbr)[:n]), dev(c["cnt"][:n])
    w2, b2 = dev(c["w2"]), dev(c["b2"])
    out = torch.full((n, c["d_out"]), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("rs_pinsage_infer_layer", L.ptr(h), n, c["d_in"], L.ptr(u), c["hidden"], L.ptr(nb),
           L.ptr(ct), c["k"], L.ptr(w2), L.ptr(b2), c["d_out"], int(relu), int(norm), L.ptr(out),
           L.ptr(flag), L.stream_ptr(DEV))
    return out.cpu().numpy(), int(flag.item())


def run_layer(c, relu, norm, fused):
    """inference.layer_from_u on case c (every norm, fused or composed): (out NumPy, flag)."""
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        out = I.layer_from_u(dev(c["h"]), dev(c["u"]), dev(c["nbr"]), dev(c["cnt"]), dev(c["w2"]),
                             dev(c["b2"]), int(relu), norm, fused, flag)
    return out.cpu().numpy(), int(flag.item())


def ref_of(c, relu, norm, nbr=None, **kw):
    return R.layer_ref(c["h"], c["u"], c["nbr"] if nbr is None else nbr, c["cnt"], c["w2"], c["b2"],
                       relu, norm, **kw)


# ---- 1. one layer against float64 ---------------------------------------------------------------
CASES = [(n, s, k) for n in R.N_ITEMS for s in R.SHAPES for k in R.KS]


@pytest.mark.parametrize("n,shape,k", CASES)
def test_layer_matches_float64(n, shape, k):
    c = R.make_case(n, *shape, k)
    for relu in (False, True):
        for norm in R.NORMS:
            got, flag = run_layer(c, relu, norm, True)
            assert flag == 0
            R.assert_layer_close(got, ref_of(c, relu, norm), f"relu {relu} norm {norm}")


def test_all_negative_row_is_exact_zeros():
    c = R.negative_row_case()
    got, flag = run_layer(c, True, "row", True)
    assert flag == 0
    assert (got[c["neg_row"]] == 0).all() and not np.signbit(got[c["neg_row"]]).any()
    R.assert_layer_close(got, ref_of(c, True, "row"), "negative row case")


def test_entry_point_refuses_shapes_past_its_limits():
    c = R.make_case(5, 8, 8, 65, 3)
    with pytest.raises(L.RecsysError, match="d_out <= 64"):
        run_kernel(c, 1, 1)
    t = torch.zeros(4, device=DEV)
    st = L.lib().rs_pinsage_infer_layer(L.ptr(t), 1, 1, L.ptr(t), 1, L.ptr(t), L.ptr(t), 33,
                                        L.ptr(t), L.ptr(t), 1, 0, 0, L.ptr(t), None,
                                        L.stream_ptr(DEV))
    assert st == L.RS_E_UNSUPPORTED


# ---- 2. bit-exact invariances -------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((24, 32, 16), 3), ((5, 3, 7), 10), ((192, 64, 64), 32)])
def test_two_runs_are_equal_and_rows_do_not_depend_on_the_table(shape, k):
    c = R.make_case(4 * R.T + 1, *shape, k)
    for norm in (0, 1):
        a, _ = run_kernel(c, 1, norm)
        b, _ = run_kernel(c, 1, norm)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        for i in (0, 1, R.T - 1, R.T, 2 * R.T + 5, 3 * R.T + 17):
            m = int(max([i] + c["nbr"][i].tolist())) + 1
            if m == c["n"]:
                continue
            # the table truncated just past the largest id row i uses; the rows kept drop the
            # slots that pointed past it (they are not the rows compared)
            nbr = c["nbr"].copy()
            nbr[nbr >= m] = -1
            nbr[i] = c["nbr"][i]
            t, flag = run_kernel(c, 1, norm, n=m, nbr=nbr)
            assert flag == 0
            np.testing.assert_array_equal(t[i].view(np.uint32), a[i].view(np.uint32),
                                          err_msg=f"row {i} over {m} of {c['n']} items")


def hand_graph():
    users, items, n_users, n_items = R.hand_graph_edges()
    g = HeteroGraph(users, items, n_users, n_items, device=DEV)
    return g, O.BipartiteGraph.from_edges(users, items, n_users, n_items)


def test_item_neighbors_chunking_and_oracle():
    g, og = hand_graph()
    smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=11)
    step0 = smp.step
    nbr, cnt = item_neighbors(smp, step=5)
    assert smp.step == step0 and nbr.shape == (g.n_items, 3) and nbr.dtype == torch.int32
    for bs in (1, 7, g.n_items):
        nb, ct = item_neighbors(smp, step=5, batch_size=bs)
        assert torch.equal(nb, nbr) and torch.equal(ct, cnt), f"chunks of {bs}"
    rn, rc = O.pinsage_neighbors(og, np.arange(g.n_items), 4, 2, 0.0, 3, 11, 5, 0)
    np.testing.assert_array_equal(nbr.cpu().numpy(), rn)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rc)
    assert (rn == -1).all(1).any() and (rn >= 0).all(1).any(), "dead-end and full rows both occur"


# ---- 3. against the existing modules ------------------------------------------------------------
def conv_ref(h, nbr, cnt, W1, b1, W2, b2, relu, norm):
    """float64 Convolve from h (fc_1 included); fc_1's own fp32 bound rides in the tolerance."""
    u, Mu = R.dense64(h, W1, b1, relu)
    return R.layer_ref(h, u, nbr, cnt, W2, b2, relu, norm, u_bound=Mu)


def params(*ts):
    return [t.detach().cpu().numpy() for t in ts]


def test_frobenius_equals_the_models_convolve_and_fused_equals_unfused():
    g, _ = hand_graph()
    n = g.n_items
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    model = PinSageModel(g_with_features(g), g.itype, 2, 8, 32, 16, generator=gen)
    conv = model.sagenet.convolves[0]
    with torch.no_grad():
        conv.fc_1.bias.uniform_(-0.2, 0.2, generator=gen)
        conv.fc_2.bias.uniform_(0.1, 0.5, generator=gen)
    smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=11)
    nbr, cnt = item_neighbors(smp)
    h = torch.rand(n, 24, device=DEV, generator=gen) * 2 - 1
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    block = smp.to_block(ids, nbr, cnt)
    assert torch.equal(block.src_nodes, ids), "the block's src order is the identity"
    with torch.no_grad():
        want = conv(block, (h, h)).cpu().numpy()
    ref = conv_ref(h.cpu().numpy(), nbr.cpu().numpy(), cnt.cpu().numpy(),
                   *params(conv.fc_1.kernel, conv.fc_1.bias, conv.fc_2.kernel, conv.fc_2.bias),
                   True, "frobenius")
    fused = convolve(h, nbr, cnt, conv.fc_1, conv.fc_2, "relu", "frobenius", fused=True).cpu().numpy()
    unfused = convolve(h, nbr, cnt, conv.fc_1, conv.fc_2, "relu", "frobenius", fused=False).cpu().numpy()
    for name, a, b in (("fused vs Convolve", fused, want), ("fused vs unfused", fused, unfused)):
        ratio = float((np.abs(a.astype(np.float64) - b) / (2 * ref["tol"])).max())
        assert ratio <= 1.0, f"{name}: max err / (2 tol) = {ratio:.3g}"
    for name, a in (("fused", fused), ("unfused", unfused), ("Convolve", want)):
        R.assert_layer_close(a, ref, name)
    # every norm and both activations, fused against unfused, each within one bound of float64
    for act in ("relu", None):
        for norm in R.NORMS:
            r = conv_ref(h.cpu().numpy(), nbr.cpu().numpy(), cnt.cpu().numpy(),
                         *params(conv.fc_1.kernel, conv.fc_1.bias, conv.fc_2.kernel, conv.fc_2.bias),
                         act == "relu", norm)
            pair = (conv.fc_2.kernel, conv.fc_2.bias)  # a (kernel, bias) pair is accepted too
            a = convolve(h, nbr, cnt, conv.fc_1, pair, act, norm, fused=True).cpu().numpy()
            b = convolve(h, nbr, cnt, conv.fc_1, conv.fc_2, act, norm, fused=False).cpu().numpy()
            R.assert_layer_close(a, r, f"fused {act} {norm}")
            R.assert_layer_close(b, r, f"unfused {act} {norm}")


def g_with_features(g, seed=2):
    """The same edges with the item features PinSageModel's projector reads."""
    rng = np.random.default_rng(seed)
    g.nodes[g.itype].data["year"] = torch.from_numpy(rng.integers(0, 12, g.n_items)).to(DEV)
    g.nodes[g.itype].data["genre"] = torch.from_numpy(
        (rng.random((g.n_items, 6)) < 0.3).astype(np.int8)).to(DEV)
    return g


def test_shape_past_the_limits_takes_the_unfused_path(monkeypatch):
    c = R.make_case(R.T + 1, 24, 32, 65, 3)
    calls = []
    real = I._convolve_unfused
    monkeypatch.setattr(I, "_convolve_unfused", lambda *a, **k: calls.append(1) or real(*a, **k))
    rng = np.random.default_rng(5)
    W1 = (rng.uniform(-1, 1, (24, 32)) / 5).astype(np.float32)
    b1 = rng.uniform(-0.2, 0.2, 32).astype(np.float32)
    for norm in R.NORMS:
        got = convolve(dev(c["h"]), dev(c["nbr"]), dev(c["cnt"]), (dev(W1), dev(b1)),
                       (dev(c["w2"]), dev(c["b2"])), "relu", norm, fused=True)
        ref = conv_ref(c["h"], c["nbr"], c["cnt"], W1, b1, c["w2"], c["b2"], True, norm)
        R.assert_layer_close(got.cpu().numpy(), ref, f"d_out 65 norm {norm}")
    assert len(calls) == 3


# ---- 4. the chain -------------------------------------------------------------------------------
def chain_setup():
    rng = np.random.default_rng(9)
    n_users, n_items = 120, 300
    users = np.concatenate([np.arange(n_users), rng.integers(0, n_users, 2400)])
    items = np.concatenate([rng.integers(0, n_items, n_users), rng.integers(0, n_items - 9, 2400)])
    key = np.unique(users * n_items + items)
    users, items = key // n_items, key % n_items
    ts = rng.integers(0, 10**9, users.size)
    year = rng.integers(0, 12, n_items)
    genre = (rng.random((n_items, 6)) < 0.3).astype(np.int8)
    g = HeteroGraph(users, items, n_users, n_items, device=DEV,
                    item_data={"year": year, "genre": genre}, edge_data={"timestamp": ts})
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    model = PinSageModel(g, g.itype, 2, 8, 32, 16, generator=gen)
    with torch.no_grad():
        for d in [m for c in model.sagenet.convolves for m in (c.fc_1, c.fc_2)] + \
                [model.sagenet.fc_1, model.sagenet.fc_2]:
            d.bias.uniform_(0.05, 0.3, generator=gen)
    smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=9)
    return g, model, smp, year, genre, (users, items)


def check_chain(model, smp, year, genre, fused):
    """infer_item_reprs stage by stage: each float64 stage is fed the GPU's previous stage."""
    out, stages, (nbr, cnt) = infer_item_reprs(model, smp, fused=fused, return_stages=True)
    assert out.shape == (300, 16) and len(stages) == 4 and out is stages[-1]
    st = [s.cpu().numpy() for s in stages]
    nb, ct = nbr.cpu().numpy(), cnt.cpu().numpy()
    fp = model.feature_projector
    tabs = {k: t.weight.detach().cpu().numpy().astype(np.float64)
            for k, t in (("year", fp.year_embedding), ("genre", fp.genre_embedding),
                         ("id", fp.id_embedding))}
    ids = np.arange(300)
    rows = (tabs["year"][year[ids]], tabs["genre"][genre[ids].astype(np.int64)], tabs["id"][ids])
    f64 = np.concatenate([rows[0], rows[1].mean(1), rows[2]], 1)
    fM = np.concatenate([np.abs(rows[0]), np.abs(rows[1]).mean(1), np.abs(rows[2])], 1)
    assert (np.abs(st[0] - f64) <= R.RTOL * fM).all(), "features"
    net = model.sagenet
    for l, conv in enumerate(net.convolves):
        ref = conv_ref(st[l], nb, ct, *params(conv.fc_1.kernel, conv.fc_1.bias, conv.fc_2.kernel,
                                              conv.fc_2.bias), True, "row")
        R.assert_layer_close(st[l + 1], ref, f"layer {l + 1} (fused={fused})")
    W1, b1, W2, b2 = params(net.fc_1.kernel, net.fc_1.bias, net.fc_2.kernel, net.fc_2.bias)
    a, Ma = R.dense64(st[2], W1, b1, True)
    y, My = R.dense64(a, W2, b2, False)
    My = My + Ma @ np.abs(W2.astype(np.float64))  # fc_1's own bound through fc_2
    assert (np.abs(st[3] - y) <= R.RTOL * My).all(), "head"
    return out


def test_chain_matches_float64_stage_by_stage_and_feeds_the_evaluation():
    from scipy import sparse as ssp

    g, model, smp, year, genre, (users, items) = chain_setup()
    out = check_chain(model, smp, year, genre, None)
    check_chain(model, smp, year, genre, False)
    assert torch.isfinite(infer_item_reprs(model, smp, norm="frobenius")).all()
    recs = recommend(g, 10, out, None, g.utype, "timestamp", 32)
    assert recs.shape == (g.n_users, 10)
    truth = ssp.coo_matrix((np.ones(users.size), (users, items)), (g.n_users, g.n_items))
    assert 0.0 <= hit_rate_eval(recs, truth.tocsr()) <= 1.0


def test_train_main_evaluates_with_layerwise_reprs(capsys):
    from recommender_amd.pinsage.train import main

    main(["--steps", "1", "--eval_every", "1", "--eval-reprs", "layerwise"])
    assert "hit_rate" in capsys.readouterr().out


def test_command_line_writes_the_representations(tmp_path):
    path = tmp_path / "reprs.npy"
    reprs = I.main(["--out", str(path)])
    saved = np.load(path)
    assert saved.shape == (3706, 16) and np.isfinite(saved).all()
    np.testing.assert_array_equal(saved, reprs.cpu().numpy())


# ---- 5. bad ids -----------------------------------------------------------------------------------
def test_out_of_range_ids_are_skipped_flagged_and_raise():
    c = R.make_case(R.T + 1, 24, 32, 16, 3)
    nbr = c["nbr"].copy()
    nbr[2, 0], nbr[9, 1], nbr[40, 2] = c["n"], 2**31 - 1, -7
    for norm in (0, 1):
        got, flag = run_kernel(c, 1, norm, nbr=nbr)
        assert flag & L.RS_ERRBIT_OOB
        # the reference skips the flagged slots; every row, the three included, equals it
        R.assert_layer_close(got, ref_of(c, True, "row" if norm else None, nbr=nbr), f"norm {norm}")
        clean, flag0 = run_kernel(c, 1, norm)
        assert flag0 == 0
        keep = np.ones(c["n"], bool)
        keep[[2, 9, 40]] = False
        np.testing.assert_array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    rng = np.random.default_rng(6)
    fc1 = (dev((rng.uniform(-1, 1, (24, 32)) / 5).astype(np.float32)), None)
    for fused in (True, False):
        with pytest.raises(L.RecsysError, match="outside"):
            convolve(dev(c["h"]), dev(nbr), dev(c["cnt"]), fc1, (dev(c["w2"]), dev(c["b2"])),
                     fused=fused)
    convolve(dev(c["h"]), dev(c["nbr"]), dev(c["cnt"]), fc1, (dev(c["w2"]), dev(c["b2"])))
