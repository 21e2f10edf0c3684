"""Per-kernel roofline table for the secondary paths (DIEN attention + GRU/AUGRU,
PinSage sampling + mean-pool, EGES, ESMM-shaped embedding) at their BASELINE config shapes.

Every kernel is called through the C ABI on device-resident inputs, timed with HIP events
over `--iters` launches on the stream it runs on, and reported with its ALGORITHMIC bytes per
launch (each input byte read once, each output byte written once; the formulas are next to
each case and in DESIGN.md §4), achieved GB/s and the fraction of the 8 TB/s HBM peak.
The recurrent DIEN kernels carry L dependent steps per example, so they are latency-bound by
construction ("DIEN is really latency-bound"); their fraction says how far.

Usage: python benchmarks/bench_kernels.py [--iters 20] > profiles/rNN_kernel_roofline.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recommender_amd import _lib as L  # noqa: E402

PEAK = 8000.0  # GB/s, MI355X HBM3E spec
DEV = "cuda"


def timed(fn, iters):
    s = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def report(name, cfg, us, nbytes, out):
    gbs = nbytes / (us * 1e-6) / 1e9
    line = {"kernel": name, "config": cfg, "avg_us": round(us, 2), "algorithmic_bytes": int(nbytes),
            "achieved_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / PEAK, 4)}
    out.append(line)
    print(json.dumps(line), flush=True)


def dien(iters, out):
    B, T, H = 4096, 100, 36
    g = torch.Generator(device=DEV).manual_seed(0)
    xw = torch.randn(B, T, 3 * H, device=DEV, generator=g)
    U = torch.randn(H, 3 * H, device=DEV, generator=g) * 0.1
    rb = torch.zeros(3 * H, device=DEV)
    lens = torch.randint(2, T + 1, (B,), device=DEV, generator=g)
    mask = (torch.arange(T, device=DEV)[None] < lens[:, None]).to(torch.uint8).contiguous()
    outp = torch.empty(B, T, H, device=DEV)
    saved = torch.empty(B, T, 4 * H, device=DEV)
    st = L.stream_ptr(DEV)
    cfg = {"B": B, "L": T, "H": H}
    us = timed(lambda: L.call("rs_gru_fwd", L.ptr(xw), L.ptr(U), L.ptr(rb), L.ptr(mask), B, T, H,
                              L.ptr(outp), L.ptr(saved), st), iters)
    report("rs_gru_fwd", cfg, us, B * T * (12 * H + 1 + 4 * H + 16 * H), out)
    dout = torch.randn(B, T, H, device=DEV, generator=g)
    dxw = torch.empty(B, T, 3 * H, device=DEV)
    din = torch.empty(B, T, 3 * H, device=DEV)
    us = timed(lambda: L.call("rs_gru_bwd", L.ptr(dout), L.ptr(outp), L.ptr(saved), L.ptr(U),
                              L.ptr(mask), B, T, H, L.ptr(dxw), L.ptr(din), 0, st), iters)
    report("rs_gru_bwd", cfg, us, B * T * (4 * H + 4 * H + 16 * H + 1 + 12 * H + 12 * H), out)
    att = torch.rand(B, T, device=DEV, generator=g)
    kuh = torch.randn(H, H, device=DEV, generator=g) * 0.1
    final = torch.empty(B, H, device=DEV)
    states = torch.empty(B, T, H, device=DEV)
    us = timed(lambda: L.call("rs_augru_fwd", L.ptr(xw), L.ptr(att), L.ptr(kuh), L.ptr(kuh),
                              L.ptr(kuh), L.ptr(mask), B, T, H, L.ptr(final), L.ptr(states),
                              L.ptr(saved), 0, st), iters)
    report("rs_augru_fwd", cfg, us, B * T * (12 * H + 4 + 1 + 4 * H + 16 * H) + 4 * B * H, out)
    dfinal = torch.randn(B, H, device=DEV, generator=g)
    datt = torch.empty(B, T, device=DEV)
    us = timed(lambda: L.call("rs_augru_bwd", L.ptr(dfinal), L.ptr(att), L.ptr(states),
                              L.ptr(saved), L.ptr(kuh), L.ptr(kuh), L.ptr(kuh), L.ptr(mask), B, T,
                              H, L.ptr(dxw), L.ptr(datt), 0, st), iters)
    report("rs_augru_bwd", cfg, us, B * T * (4 + 4 * H + 16 * H + 1 + 12 * H + 4) + 4 * B * H, out)
    hs = torch.randn(B, T, H, device=DEV, generator=g)
    q = torch.randn(B, H, device=DEV, generator=g)
    a = torch.empty(B, T, device=DEV)
    us = timed(lambda: L.call("rs_dien_attention_fwd", L.ptr(hs), L.ptr(q), L.ptr(mask), B, T, H,
                              L.ptr(a), st), iters)
    report("rs_dien_attention_fwd", cfg, us, B * T * (4 * H + 1 + 4) + 4 * B * H, out)
    da = torch.randn(B, T, device=DEV, generator=g)
    dhs = torch.empty_like(hs)
    dq = torch.empty_like(q)
    us = timed(lambda: L.call("rs_dien_attention_bwd", L.ptr(hs), L.ptr(q), L.ptr(a), L.ptr(da), B,
                              T, H, L.ptr(dhs), L.ptr(dq), st), iters)
    report("rs_dien_attention_bwd", cfg, us, B * T * (4 * H + 4 + 4 + 4 * H) + 8 * B * H, out)


def pinsage(iters, out):
    from recommender_amd.pinsage import PinSageSampler
    from recommender_amd.pinsage.layers import weighted_mean_agg  # noqa: F401
    from recommender_amd.pinsage.sampler import item_pairs
    from recommender_amd.pinsage.train import ML20M, build_graph

    g = build_graph(ML20M, 4)
    smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=4)
    h, p, n = item_pairs(g, 4096, 4, 0)
    seeds, _, ns = smp.unique_first(torch.cat([h, p, n]), g.n_items)
    seeds = seeds[: int(ns.item())].contiguous()
    S = seeds.numel()
    cfg = {"graph": "ml20m_shaped", "edges": g.n_edges, "seeds": S, "walks": 4, "traversals": 2,
           "k": 3}
    # 4 walks x 4 hops, each hop: indptr pair (16 B) + one neighbour id (4 B); out 3 x (4 + 4) B
    us = timed(lambda: smp.neighbors(seeds, 0, None, 0), iters)
    report("rs_pinsage_neighbors", cfg, us, S * (4 + 4 * 4 * 20 + 3 * 8), out)
    nbr, cnt = smp.neighbors(seeds, 0, None, 0)
    ids = torch.cat([seeds, nbr.reshape(-1)])
    us = timed(lambda: smp.unique_first(ids, g.n_items), iters)
    report("rs_unique_first", {"n": ids.numel(), "n_nodes": g.n_items}, us,
           ids.numel() * (4 + 4 + 4 + 4) + g.n_items * 4, out)
    blk = smp.to_block(seeds, nbr, cnt)
    E = int(blk.n_edges.item())
    Hh = 32
    u = torch.randn(blk.n_src, Hh, device=DEV)
    nv = torch.empty(blk.n_dst, Hh, device=DEV)
    wsum = torch.empty(blk.n_dst, device=DEV)
    st = L.stream_ptr(DEV)
    acfg = {"n_dst": blk.n_dst, "n_src": blk.n_src, "edges": E, "H": Hh}
    us = timed(lambda: L.call("rs_weighted_mean_agg_fwd", L.ptr(u), blk.n_src, Hh, L.ptr(blk.indptr),
                              L.ptr(blk.edge_src), L.ptr(blk.edge_w), blk.n_dst, L.ptr(nv),
                              L.ptr(wsum), st), iters)
    report("rs_weighted_mean_agg_fwd", acfg, us, E * (4 + 4 + 4 * Hh) + blk.n_dst * (8 + 4 * Hh), out)
    gu = torch.empty_like(u)
    us = timed(lambda: L.call("rs_weighted_mean_agg_bwd", L.ptr(nv), Hh, L.ptr(blk.t_indptr),
                              L.ptr(blk.t_edge), L.ptr(blk.edge_dst), L.ptr(blk.edge_w), L.ptr(wsum),
                              blk.n_src, L.ptr(gu), st), iters)
    report("rs_weighted_mean_agg_bwd", acfg, us,
           E * (4 + 4 + 4 + 4 + 4 * Hh) + blk.n_src * (4 + 4 * Hh), out)


def eges(iters, out):
    from recommender_amd.embedding import Embedding

    B, M, D, V = 1024, 6, 160, 63001
    t = Embedding(V, D, device=DEV)
    ids = torch.randint(0, V, (B, M), device=DEV, dtype=torch.int32)
    h = torch.randn(B, D, device=DEV)
    logits = torch.empty(B, M, device=DEV)
    st = L.stream_ptr(DEV)
    cfg = {"B": B, "M": M, "D": D}
    us = timed(lambda: L.call("rs_match_logits_fwd", L.ptr(t.weight), V, D, L.ptr(ids), 0, M, L.ptr(h),
                              B, L.ptr(logits), L.ptr(t.err_flag), st), iters)
    report("rs_match_logits_fwd", cfg, us, B * M * (4 + 4 * D) + B * 4 * D + B * M * 4, out)
    rows = torch.empty(B * M, D, device=DEV)
    gh = torch.empty(B, D, device=DEV)
    us = timed(lambda: L.call("rs_match_logits_bwd", L.ptr(t.weight), V, D, L.ptr(ids), 0, M, L.ptr(h),
                              L.ptr(logits), B, L.ptr(rows), L.ptr(gh), st), iters)
    report("rs_match_logits_bwd", cfg, us,
           B * M * (4 + 4 * D + 4) + B * 4 * D + B * M * 4 * D + B * 4 * D, out)


def eges_sampler(iters, out):
    """EGES pair pipeline on a 63001-item weighted graph, 65536 walks of
    length 10 per refill. Bytes: traces written + per hop indptr pair / log2(deg) prefix probes
    / one index (random reads, latency-bound); skipgrams: traces read, flag + offset per slot,
    pairs written; negatives: ids written (the CDF table is L2-resident; the kernel is ALU-bound)."""
    from recommender_amd.eges.sampler import EGESPairSampler, skipgram_slots
    from tests.eges_graph import make_graph

    V, W, Lw = 63001, 65536, 10
    indptr, indices, w = make_graph(np.random.default_rng(4), V, 1_000_000, 50)
    s = EGESPairSampler(indptr, indices, w, V, device=DEV, walks_per_refill=W)
    deg = max(1.0, indices.size / V)
    probes = int(np.ceil(np.log2(deg + 1)))
    cfg = {"items": V, "edges": int(indices.size), "walks": W, "length": Lw}
    us = timed(lambda: s.walks(W, 1), iters)
    report("rs_eges_walks", cfg, us, W * (Lw + 1) * 4 + W * Lw * (16 + 4 + 8 * probes), out)
    tr = s.walks(W, 1)
    slots = skipgram_slots(Lw + 1, 5)
    us = timed(lambda: s.skipgrams(tr), iters)
    tgt, _ = s.skipgrams(tr)
    P = tgt.numel()
    report("rs_skipgram_pairs(+1 sync)", dict(cfg, pairs=P), us,
           W * (Lw + 1) * 4 * 2 + W * slots * 16 + P * 8, out)
    us = timed(lambda: s.negatives(P, 1), iters)
    report("rs_log_uniform_sample(ALU-bound: Philox + CDF walk)", {"pairs": P, "num_ns": 5,
                                                                 "range": V}, us, P * 5 * 4, out)
    def refill():
        s._target, s._context = s._target[:0], s._context[:0]
        s.refill()

    us = timed(refill, max(3, iters // 4))
    line = {"kernel": "eges_refill(walks+skipgrams+negatives)", "config": dict(cfg, pairs=P),
            "avg_us": round(us, 2), "pairs_per_s": round(P / (us * 1e-6))}
    out.append(line)
    print(json.dumps(line), flush=True)


def pinsage_eval(iters, out):
    """PinSage evaluation at ML-1M / ML-20M shapes: rs_masked_topk bytes =
    the score rows read once + the exclusion CSR + the top-k written; plus the whole
    get_item_reprs → recommend → hit_rate pass on ML-1M, wall clock."""
    import time

    from recommender_amd.pinsage import PinSageModel, PinSageSampler
    from recommender_amd.pinsage.evaluation import (get_item_reprs, hit_rate_eval, masked_topk,
                                                    recommend)
    from recommender_amd.pinsage.train import ML1M, build_dataset
    from recommender_amd.synthetic import ML20M

    for name, shape in (("ml1m", ML1M), ("ml20m", ML20M)):
        g, val, _ = build_dataset(shape, 4, DEV)
        R = min(g.n_users, 8192)
        scores = torch.randn(R, g.n_items, device=DEV)
        nb = R * g.n_items * 4 + int(g.u2i_indptr[R]) * 4 + R * 8 + R * 10 * 4
        us = timed(lambda: masked_topk(scores, 10, 0, g), iters)
        report("rs_masked_topk", {"graph": name, "rows": R, "items": g.n_items, "k": 10}, us, nb,
               out)
        if name != "ml1m":
            continue
        torch.manual_seed(0)
        model = PinSageModel(g, g.itype, 2, 8, 32, 16)
        smp = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0.0, 3, seed=4)
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reprs = get_item_reprs(model, smp, g, g.itype, 32)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            recs = recommend(g, 10, reprs, None, g.utype, "timestamp", 32)
            hr = hit_rate_eval(recs, val.tocsr())
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        line = {"kernel": "pinsage_eval(get_item_reprs bs32 + recommend + hit_rate)",
                "config": {"graph": name, "users": g.n_users, "items": g.n_items, "k": 10},
                "item_reprs_ms": round((t1 - t0) * 1e3, 2),
                "recommend_hit_rate_ms": round((t2 - t1) * 1e3, 3), "hit_rate": hr}
        out.append(line)
        print(json.dumps(line), flush=True)


def topk_ip(iters, out, rounds=5):
    """Fused top-k inner-product retrieval (rs_topk_ip) against the path it replaces, recommend's
    chunked torch.matmul (≤ 1 GiB of fp32 scores per chunk) + rs_masked_topk, interleaved in one
    process: `rounds` rounds of both, each timed with events over its launches; medians reported
    with every round's time next to them, and the fused call's fraction of the 157.3 TF fp32
    MFMA peak (2·Q·N·D flop).
    (a) ML-20M-shaped PinSage: every user's latest item against all items, D 16, k 10, the u2i
        CSR as the exclusion. (b) EGES-like: 65 536 queries x 2^20 items, D 160, k 10, no
        exclusion; one launch per round."""
    from recommender_amd.functional import topk_inner_product
    from recommender_amd.pinsage import evaluation as E
    from recommender_amd.pinsage.train import build_dataset
    from recommender_amd.synthetic import ML20M

    peak_tf = 157.3

    def bench(name, q, x, k, excl_graph, n_iter):
        Q, N, D = q.shape[0], x.shape[0], x.shape[1]
        rows = max(32, min(Q, E._SCORE_CHUNK_BYTES // (4 * N)))
        recs = torch.empty(Q, k, dtype=torch.int32, device=DEV)
        xt = x.t()

        def base():
            for b0 in range(0, Q, rows):
                b1 = min(Q, b0 + rows)
                recs[b0:b1] = E.masked_topk(torch.matmul(q[b0:b1], xt), k, b0, excl_graph)
            return recs

        excl = None if excl_graph is None else (excl_graph.u2i_indptr, excl_graph.u2i)

        def fused():
            return topk_inner_product(q, x, k, exclude=excl, with_scores=False)[0]

        a, b = base().clone(), fused()
        same = float((a == b).all(1).float().mean())
        times = {"base": [], "fused": []}
        s = torch.cuda.current_stream()
        for _ in range(rounds):
            for label, fn in (("base", base), ("fused", fused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s)
                for _ in range(n_iter):
                    fn()
                e1.record(s)
                torch.cuda.synchronize()
                times[label].append(e0.elapsed_time(e1) / n_iter)
        mb, mf = float(np.median(times["base"])), float(np.median(times["fused"]))
        line = {"kernel": "rs_topk_ip vs matmul + rs_masked_topk",
                "config": {"shape": name, "queries": Q, "items": N, "D": D, "k": k,
                           "exclusion": excl is not None, "chunk_rows": rows},
                "base_ms": round(mb, 3), "fused_ms": round(mf, 3), "speedup": round(mb / mf, 2),
                "fused_frac_of_fp32_mfma_peak": round(2.0 * Q * N * D / (mf * 1e-3) / 1e12 / peak_tf, 4),
                "rows_identical_to_base": round(same, 5),
                "base_rounds_ms": [round(t, 3) for t in times["base"]],
                "fused_rounds_ms": [round(t, 3) for t in times["fused"]]}
        out.append(line)
        print(json.dumps(line), flush=True)

    gen = torch.Generator(device=DEV).manual_seed(4)
    g, _, _ = build_dataset(ML20M, 4, DEV)
    reprs = torch.randn(g.n_items, 16, device=DEV, generator=gen)
    latest = E.latest_items(g, "timestamp")
    bench("pinsage_ml20m", reprs[latest.long()].contiguous(), reprs, 10, g, max(1, iters // 4))
    del g
    x = torch.randn(1 << 20, 160, device=DEV, generator=gen)
    q = x[torch.randint(0, 1 << 20, (65536,), device=DEV, generator=gen)].contiguous()
    bench("eges_like", q, x, 10, None, 1)


def topk_i8(iters, out, rounds=5):
    """Two-stage retrieval (rs_topk_ip_i8, then rs_rerank_ip) against the exhaustive rs_topk_ip,
    interleaved in one process: `rounds` rounds of the exact call, the int8 scan and the re-rank,
    one launch each, timed with events; medians reported with every round next to them. The
    quantisation of the catalogue (done once) is timed on its own. Per line: recall@10 of the
    re-ranked result against the exact one, the bytes of codes + scales against the fp32
    catalogue, and the scan's fraction of the 8 TB/s HBM peak counting one read of codes + scales
    (its traffic floor: every 32-query row of blocks reads the catalogue again, mostly from cache).
    Shapes: 65 536 queries x 2^20 items, k 10, kc 64, at D 64, 128 and 160; at D 160 also 256
    queries (a serving batch) and kc 16. Data: a 4096-centre Gaussian mixture with unit-norm rows,
    and unstructured normal rows. Queries are catalogue rows."""
    from recommender_amd.functional import (quantize_rows_i8, rerank_inner_product,
                                            topk_inner_product, topk_inner_product_i8)

    N, k, kc = 1 << 20, 10, 64
    hbm_bytes_per_s = 8.0e12
    gen = torch.Generator(device=DEV).manual_seed(4)
    s = torch.cuda.current_stream()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        r = fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def bench(name, x, Q, kc=kc):
        D = x.shape[1]
        q = x[torch.randint(0, N, (Q,), device=DEV, generator=gen)].contiguous()
        quantize_rows_i8(x)  # warm-up
        quant_ms, (codes, scales) = once(lambda: quantize_rows_i8(x))
        cand = topk_inner_product_i8(q, codes, scales, kc, with_keys=False)[0]
        fns = {"exact": lambda: topk_inner_product(q, x, k, with_scores=False)[0],
               "scan": lambda: topk_inner_product_i8(q, codes, scales, kc, with_keys=False)[0],
               "rerank": lambda: rerank_inner_product(q, x, cand, k, with_scores=False)[0]}
        exact, got = fns["exact"](), fns["rerank"]()
        recall = float((got[:, :, None] == exact[:, None, :]).any(1).float().mean())
        times = {label: [] for label in fns}
        for _ in range(rounds):
            for label, fn in fns.items():
                times[label].append(once(fn)[0])
        me, ms, mr = (float(np.median(times[label])) for label in ("exact", "scan", "rerank"))
        coded = codes.numel() + 4 * scales.numel()
        line = {"kernel": "rs_topk_ip_i8 + rs_rerank_ip vs rs_topk_ip",
                "config": {"data": name, "queries": Q, "items": N, "D": D, "k": k, "kc": kc},
                "exact_ms": round(me, 3), "scan_ms": round(ms, 3), "rerank_ms": round(mr, 3),
                "quantize_once_ms": round(quant_ms, 3),
                "speedup": round(me / (ms + mr), 2),
                "two_stage_below_fastest_exact_round": bool(ms + mr < min(times["exact"])),
                "recall_at_10": round(recall, 4),
                "coded_bytes": coded, "fp32_bytes": 4 * x.numel(),
                "coded_fraction": round(coded / (4 * x.numel()), 4),
                "scan_frac_of_hbm_peak_one_catalogue_read":
                    round(coded / (ms * 1e-3) / hbm_bytes_per_s, 5),
                "scan_int8_TOPS": round(2.0 * Q * N * D / (ms * 1e-3) / 1e12, 1),
                "exact_rounds_ms": [round(t, 3) for t in times["exact"]],
                "scan_rounds_ms": [round(t, 3) for t in times["scan"]],
                "rerank_rounds_ms": [round(t, 3) for t in times["rerank"]]}
        out.append(line)
        print(json.dumps(line), flush=True)

    for D in (64, 128, 160):
        centres = torch.nn.functional.normalize(torch.randn(4096, D, device=DEV, generator=gen))
        member = torch.randint(0, 4096, (N,), device=DEV, generator=gen)
        x = centres[member] + 0.05 * torch.randn(N, D, device=DEV, generator=gen)
        x = torch.nn.functional.normalize(x).contiguous()
        del centres, member
        bench("gaussian_mixture_4096", x, 65536)
        if D == 160:
            bench("gaussian_mixture_4096", x, 256)
            bench("gaussian_mixture_4096", x, 65536, kc=16)  # fewer candidates: fewer compactions
        del x
        x = torch.randn(N, D, device=DEV, generator=gen)
        bench("normal", x, 65536)
        if D == 160:
            bench("normal", x, 256)
            bench("normal", x, 65536, kc=16)
        del x


def item_softmax(iters, out, rounds=3):
    """functional.item_softmax_loss (rs_item_softmax_fwd + _bwd, no [B, M] matrix) against the
    torch composition logsumexp(q @ v.T * inv_temp - log_q, 1) - diagonal under autograd, forward
    + backward, interleaved in one process: `rounds` rounds of both, each timed with events over
    its launches; medians and every round's time, and each side's peak memory over the inputs
    (torch.cuda.max_memory_allocated). A torch side that cannot allocate is reported as such and
    skipped. B = M = 8 192; B = M = 32 768; B = 4 096 over M = 2^20; all at D = 128."""
    from recommender_amd.functional import item_softmax_loss

    inv_temp = 10.0
    gen = torch.Generator(device=DEV).manual_seed(4)

    def bench(B, M, D, n_iter):
        q = (torch.randn(B, D, device=DEV, generator=gen) / D ** 0.5).requires_grad_()
        v = (torch.randn(M, D, device=DEV, generator=gen) / D ** 0.5).requires_grad_()
        log_q = torch.randn(M, device=DEV, generator=gen)
        t = torch.randint(0, M, (B,), device=DEV, generator=gen, dtype=torch.int32)
        tl = t.long()
        rows = torch.arange(B, device=DEV)

        def fused():
            q.grad = v.grad = None
            loss = item_softmax_loss(q, v, t, temperature=1.0 / inv_temp, log_q=log_q)
            loss.backward()
            return loss.detach()

        def base():
            q.grad = v.grad = None
            z = torch.matmul(q, v.t()) * inv_temp - log_q[None]
            loss = (torch.logsumexp(z, 1) - z[rows, tl]).mean()
            loss.backward()
            return loss.detach()

        def peak(fn):
            q.grad = v.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            r = fn()
            torch.cuda.synchronize()
            return r, torch.cuda.max_memory_allocated() - m0

        lf, peak_f = peak(fused)
        gq = q.grad.clone()
        try:
            lb, peak_b = peak(base)
            diff = {"loss_diff": abs(float(lf) - float(lb)),
                    "dq_max_diff": float((gq - q.grad).abs().max())}
            sides = (("base", base), ("fused", fused))
        except torch.OutOfMemoryError:
            q.grad = v.grad = None
            torch.cuda.empty_cache()
            peak_b, diff, sides = None, {}, (("fused", fused),)
        times = {"base": [], "fused": []}
        s = torch.cuda.current_stream()
        for _ in range(rounds):
            for label, fn in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s)
                for _ in range(n_iter):
                    fn()
                e1.record(s)
                torch.cuda.synchronize()
                times[label].append(e0.elapsed_time(e1) / n_iter)
        mf = float(np.median(times["fused"]))
        line = {"kernel": "item_softmax_loss fwd+bwd vs torch logsumexp(q @ v.T) autograd",
                "config": {"B": B, "M": M, "D": D, "inv_temp": inv_temp},
                "fused_ms": round(mf, 3), "fused_peak_MiB": round(peak_f / 2 ** 20, 1),
                "fused_rounds_ms": [round(x, 3) for x in times["fused"]],
                # five tile GEMMs of 2·B·M·D flop each
                "fused_TF": round(10.0 * B * M * D / (mf * 1e-3) / 1e12, 2)}
        if peak_b is None:
            line["base"] = "torch side could not allocate its [B, M] tensors: skipped"
        else:
            mb = float(np.median(times["base"]))
            line.update({"base_ms": round(mb, 3), "base_peak_MiB": round(peak_b / 2 ** 20, 1),
                         "base_rounds_ms": [round(x, 3) for x in times["base"]],
                         "speedup": round(mb / mf, 2), **diff})
        out.append(line)
        print(json.dumps(line), flush=True)
        q.grad = v.grad = None

    bench(8192, 8192, 128, max(1, iters // 4))
    bench(32768, 32768, 128, 1)
    bench(4096, 1 << 20, 128, 1)


def ivf_topk(iters, out, rounds=5):
    """IVF retrieval (retrieval.IVFIndex.search: coarse rs_topk_ip over the centroids, then
    rs_ivf_topk_ip) against the exhaustive rs_topk_ip at the EGES-like shape of topk_ip():
    65 536 queries x 2^20 items, D 160, k 10, nlist 1024, nprobe 1, 4, 16, 64. Interleaved in one
    process: `rounds` rounds of the exact call and every nprobe, one launch each, timed with
    events; medians reported with every round next to them. Per line: recall@10 against the exact
    result, the mean fraction of the catalogue a query scans, the index build time (one build,
    10 Lloyd iterations, host-timed after a synchronise).
    Data: (a) a Gaussian mixture, 4096 centres, unit-norm rows; (b) unstructured normal rows.
    Queries are catalogue rows."""
    from recommender_amd.functional import topk_inner_product
    from recommender_amd.retrieval import IVFIndex
    import time

    N, Q, D, k, nlist = 1 << 20, 65536, 160, 10, 1024
    gen = torch.Generator(device=DEV).manual_seed(4)
    s = torch.cuda.current_stream()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        r = fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def bench(name, x):
        q = x[torch.randint(0, N, (Q,), device=DEV, generator=gen)].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = IVFIndex.build(x, nlist)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        sizes = index.list_sizes
        fns = {"exact": lambda: topk_inner_product(q, x, k, with_scores=False)[0]}
        for nprobe in (1, 4, 16, 64):
            fns[nprobe] = lambda nprobe=nprobe: index.search(q, k, nprobe, with_scores=False)[0]
        exact = fns["exact"]()
        stats = {}
        for nprobe in (1, 4, 16, 64):
            got = fns[nprobe]()
            recall = float((got[:, :, None] == exact[:, None, :]).any(1).float().mean())
            scanned = float(sizes[index.probes(q, nprobe).long()].sum(1).float().mean()) / N
            stats[nprobe] = (recall, scanned)
        times = {label: [] for label in fns}
        for _ in range(rounds):
            for label, fn in fns.items():
                times[label].append(once(fn)[0])
        me = float(np.median(times["exact"]))
        for nprobe in (1, 4, 16, 64):
            mi = float(np.median(times[nprobe]))
            line = {"kernel": "IVFIndex.search vs rs_topk_ip",
                    "config": {"data": name, "queries": Q, "items": N, "D": D, "k": k,
                               "nlist": nlist, "nprobe": nprobe},
                    "exact_ms": round(me, 3), "ivf_ms": round(mi, 3), "speedup": round(me / mi, 2),
                    "ivf_below_fastest_exact_round": bool(mi < min(times["exact"])),
                    "recall_at_10": round(stats[nprobe][0], 4),
                    "scanned_fraction": round(stats[nprobe][1], 5),
                    "build_ms": round(build_ms, 1),
                    "largest_list": int(sizes.max()), "empty_lists": int((sizes == 0).sum()),
                    "exact_rounds_ms": [round(t, 3) for t in times["exact"]],
                    "ivf_rounds_ms": [round(t, 3) for t in times[nprobe]]}
            out.append(line)
            print(json.dumps(line), flush=True)

    centres = torch.nn.functional.normalize(torch.randn(4096, D, device=DEV, generator=gen))
    member = torch.randint(0, 4096, (N,), device=DEV, generator=gen)
    x = centres[member] + 0.05 * torch.randn(N, D, device=DEV, generator=gen)
    bench("gaussian_mixture_4096", torch.nn.functional.normalize(x).contiguous())
    del x, centres, member
    bench("normal", torch.randn(N, D, device=DEV, generator=gen))


def din_activation(iters, out, rounds=5):
    """DIN's LocalActivationUnit fused (csrc/din_activation.hip) against the unfused torch unit
    with the same weights, at the cfg3 shape (B 4096, L 100, D 36), with synthetic_batch history
    lengths (2 + Geometric(0.1)) and with full histories; forward alone and forward + backward,
    interleaved in one process: `rounds` rounds of both paths, each timed with events over its
    launches, medians reported with every round next to them. Roofline line: the `his` read
    (forward) and the `his` reads + `dhis` write (forward + backward: his is read by both passes)
    over the fused time. Also torch.cuda.max_memory_allocated around one forward + backward of
    each path, above the memory held before it."""
    from recommender_amd.dien.layers import LocalActivationUnit

    B, T, D = 4096, 100, 36
    units = []
    for fused in (True, False):
        g = torch.Generator(device=DEV).manual_seed(3)
        units.append(LocalActivationUnit(D, device=DEV, generator=g, fused=fused))
    gen = torch.Generator(device=DEV).manual_seed(4)
    rng = np.random.default_rng(4)
    tgt = (torch.randn(B, 1, D, device=DEV, generator=gen) * 0.5).requires_grad_(True)
    his = (torch.randn(B, T, D, device=DEV, generator=gen) * 0.5).requires_grad_(True)
    drep = torch.randn(B, D, device=DEV, generator=gen)
    lens = np.clip(2 + rng.geometric(0.1, B), 2, T)
    masks = {"synthetic": torch.from_numpy(np.arange(T)[None, :] < lens[:, None]).to(DEV),
             "full": torch.ones(B, T, dtype=torch.bool, device=DEV)}
    s = torch.cuda.current_stream()
    for mname, mask in masks.items():
        def fwd(u):
            with torch.no_grad():
                return u((tgt, his), mask=mask)

        def fwd_bwd(u):
            for p in (tgt, his, *u.parameters()):
                p.grad = None
            u((tgt, his), mask=mask).backward(drep)

        peak = []
        for u in units:
            fwd_bwd(u)
            for p in (tgt, his, *u.parameters()):
                p.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fwd_bwd(u)
            torch.cuda.synchronize()
            peak.append(torch.cuda.max_memory_allocated() - base)
        for what, fn, nbytes in (("fwd", fwd, B * T * D * 4), ("fwd+bwd", fwd_bwd, 3 * B * T * D * 4)):
            times = {"fused": [], "unfused": []}
            for u in units:
                fn(u)
            for _ in range(rounds):
                for label, u in zip(("fused", "unfused"), units):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(s)
                    for _ in range(iters):
                        fn(u)
                    e1.record(s)
                    torch.cuda.synchronize()
                    times[label].append(e0.elapsed_time(e1) / iters * 1e3)
            mf, mu = float(np.median(times["fused"])), float(np.median(times["unfused"]))
            gbs = nbytes / (mf * 1e-6) / 1e9
            line = {"kernel": f"din_activation {what}",
                    "config": {"B": B, "L": T, "D": D, "mask": mname,
                               "valid_steps": int(mask.sum())},
                    "fused_us": round(mf, 1), "unfused_us": round(mu, 1),
                    "speedup": round(mu / mf, 2), "his_dhis_bytes": int(nbytes),
                    "fused_achieved_GBs": round(gbs, 1), "fused_frac_of_hbm_peak": round(gbs / PEAK, 4),
                    "fwd_bwd_peak_alloc_MB": {"fused": round(peak[0] / 2 ** 20, 1),
                                              "unfused": round(peak[1] / 2 ** 20, 1)},
                    "fused_rounds_us": [round(t, 1) for t in times["fused"]],
                    "unfused_rounds_us": [round(t, 1) for t in times["unfused"]]}
            out.append(line)
            print(json.dumps(line), flush=True)


def embedding(iters, out):
    from recommender_amd.esmm import FEAT_VOCAB
    from recommender_amd.synthetic import aliccp_batch, scaled_vocab

    vocab = scaled_vocab(FEAT_VOCAB, 40_000_000)
    card = torch.tensor(list(vocab.values()), dtype=torch.int64)
    so = torch.zeros(card.numel() + 1, dtype=torch.int64)
    so[1:] = torch.cumsum(card, 0)
    V, D, B, S = int(so[-1]), 18, 65536, card.numel()
    table = torch.empty(V, D, device=DEV).uniform_(-0.05, 0.05)
    feats, _ = aliccp_batch(np.random.default_rng(4), B, vocab)
    ids = torch.from_numpy(np.concatenate(list(feats.values()), 1)).to(DEV).contiguous()
    so = so.to(DEV)
    outp = torch.empty(B, S, D, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = L.stream_ptr(DEV)
    cfg = {"tables": S, "rows": V, "D": D, "B": B}
    us = timed(lambda: L.call("rs_embedding_fwd", L.ptr(table), V, D, L.ptr(ids), 0, ids.numel(),
                              L.ptr(so), S, L.ptr(outp), L.ptr(err), st), iters)
    report("rs_embedding_fwd", cfg, us, ids.numel() * (4 + 2 * 4 * D), out)


def embedding_bag(iters, out, rounds=5):
    """EmbeddingBag against what it replaces, interleaved in one process (`rounds` rounds of every
    variant, each timed over `iters` launches; medians reported, every round's time next to them).

    (a) DIEN BASE history mean: B 4096, L 100, D 18, lengths U[1, 100], 63 001 items, [B, L] ids
        with a valid mask. (b) multi-hot DLRM: 26 slots x B 8192 CSR bags, D 64, lengths
        Geometric(1/8) capped at 64, over the cfg2 slab (26 x 10M rows).
    Forward: rs_embedding_bag_fwd against rs_embedding_fwd + torch's masked pooling. Backward
    (sort + apply, SGD and row-wise Adagrad, lr 0 so the table stays put): the sort remapped to
    bags reading dout [n_bags, D], against torch expanding dout to [n_ids, D] rows for the
    ordinary apply. Bytes, forward: live ids x (4 D + id bytes) + n_bags x 4 D. Backward: dout
    once, 8 bytes of sorted key + position per id, each touched row read and written."""
    rng = np.random.default_rng(4)
    st = L.stream_ptr(torch.device(DEV))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    shapes = []
    # (a)
    B, Lh, D, V = 4096, 100, 18, 63001
    lens = rng.integers(1, Lh + 1, B)
    valid = np.arange(Lh)[None, :] < lens[:, None]
    ids = np.where(valid, rng.integers(1, V, (B, Lh)), 0).astype(np.int32)
    shapes.append(dict(name="dien_base", V=V, D=D, n_bags=B, bag_len=Lh, ids=ids.reshape(-1),
                       offsets=None, valid=valid.reshape(-1).astype(np.uint8), so=None,
                       bag_of_pos=np.repeat(np.arange(B), Lh), lens=lens))
    # (b)
    S, B2, D2, per = 26, 8192, 64, 10_000_000
    nb = S * B2
    lens = np.minimum(rng.geometric(1 / 8, nb), 64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, per, offs[-1]).astype(np.int32)
    shapes.append(dict(name="multihot_cfg2", V=S * per, D=D2, n_bags=nb, bag_len=0, ids=ids,
                       offsets=offs, valid=None, so=np.arange(S + 1, dtype=np.int64) * per,
                       bag_of_pos=np.repeat(np.arange(nb), lens), lens=lens))
    for sh in shapes:
        V, D, nb, bl = sh["V"], sh["D"], sh["n_bags"], sh["bag_len"]
        n = sh["ids"].size
        table = torch.empty(V, D, device=DEV).uniform_(-0.05, 0.05)
        ids = torch.from_numpy(sh["ids"]).to(DEV)
        offs = None if sh["offsets"] is None else torch.from_numpy(sh["offsets"]).to(DEV)
        valid = None if sh["valid"] is None else torch.from_numpy(sh["valid"]).to(DEV)
        so = None if sh["so"] is None else torch.from_numpy(sh["so"]).to(DEV)
        n_slots = 1 if so is None else so.numel() - 1
        bag_of_pos = torch.from_numpy(sh["bag_of_pos"]).to(DEV)
        # the baseline and both sorts take global rows (a slab bag's slot is bag % n_slots)
        slot_lo = 0 if so is None else so[bag_of_pos % n_slots]
        rows64 = (ids.long() + slot_lo).contiguous()
        live = n if valid is None else int(valid.sum())
        cfg = {"shape": sh["name"], "rows": V, "D": D, "n_bags": nb, "n_ids": n, "live_ids": live}
        pooled = torch.empty(nb, D, device=DEV)
        scale = torch.empty(nb, device=DEV)
        gathered = torch.empty(n, D, device=DEV)
        m = None if valid is None else valid.view(nb, bl, 1).float()

        def bag_fwd():
            L.call("rs_embedding_bag_fwd", L.ptr(table), V, D, L.ptr(ids), 0, n, L.ptr(offs), nb,
                   bl, L.ptr(valid), None, L.RS_BAG_MEAN, L.ptr(so), n_slots, L.ptr(pooled), D,
                   L.ptr(scale), L.ptr(err), st)

        def base_fwd():
            L.call("rs_embedding_fwd", L.ptr(table), V, D, L.ptr(rows64), 1, n, None, 1,
                   L.ptr(gathered), L.ptr(err), st)
            if m is not None:  # dien/layers.py compute_his_average
                return (gathered.view(nb, bl, D) * m).sum(1) / m.sum(1)
            return torch.zeros(nb, D, device=DEV).index_add_(0, bag_of_pos, gathered) * scale[:, None]

        bag_fwd()
        # backward
        dout = torch.randn(nb, D, device=DEV)
        s_rows = torch.empty(n, dtype=torch.int32, device=DEV)
        s_pos = torch.empty(n, dtype=torch.int32, device=DEV)
        bag_pos = torch.empty(n, dtype=torch.int32, device=DEV)
        sws = torch.empty(L.lib().rs_sort_ids_workspace_size(n), dtype=torch.uint8, device=DEV)
        aws = torch.empty(L.lib().rs_apply_workspace_size(n, D), dtype=torch.uint8, device=DEV)
        acc_row = torch.full((V,), 0.1, device=DEV)
        prm = L.AdamParams(0.0, 0.0, 0.0, 0.0, 0.0, 1e-7)

        def sort():
            L.call("rs_sort_ids_slots", L.ptr(rows64), 1, n, L.ptr(valid), None, 1, V, V,
                   L.ptr(s_rows), L.ptr(s_pos), None, L.ptr(err), L.ptr(sws), sws.numel(), st)

        def bag_bwd(opt, acc):
            sort()
            L.call("rs_embedding_bag_remap_pos", L.ptr(s_pos), n, L.ptr(offs), nb, bl,
                   L.ptr(bag_pos), st)
            L.call("rs_embedding_apply_scaled", opt, L.ptr(table), L.ptr(acc), None, V, D,
                   L.ptr(s_rows), L.ptr(bag_pos), n, L.ptr(dout), L.ptr(scale), 1, prm, None,
                   L.ptr(aws), aws.numel(), st)

        def base_bwd(opt, acc):
            g = (dout * scale[:, None])
            if m is not None:   # the masked mean's backward: [B, L, D] rows, zero where masked
                rows = (g.unsqueeze(1) * m).reshape(n, D)
            else:               # index_add_'s backward: a gather of the pooled gradient
                rows = g[bag_of_pos]
            sort()
            L.call("rs_embedding_apply", opt, L.ptr(table), L.ptr(acc), None, V, D, L.ptr(s_rows),
                   L.ptr(s_pos), n, L.ptr(rows), prm, None, L.ptr(aws), aws.numel(), st)

        variants = [("fwd", "bag", bag_fwd), ("fwd", "lookup+torch pool", base_fwd)]
        for oname, opt, acc in (("sgd", L.RS_OPT_SGD, None),
                                ("rowwise_adagrad", L.RS_OPT_ROWWISE_ADAGRAD, acc_row)):
            variants.append((f"bwd[{oname}]", "bag", lambda o=opt, a=acc: bag_bwd(o, a)))
            variants.append((f"bwd[{oname}]", "expanded", lambda o=opt, a=acc: base_bwd(o, a)))
        variants.append(("sort", "shared by both backward paths", sort))
        times = {v[:2]: [] for v in variants}
        for _ in range(rounds):
            for what, side, fn in variants:
                times[(what, side)].append(timed(fn, iters))
        uniq = int(torch.unique(rows64 if valid is None else rows64[valid != 0]).numel())
        fwd_bytes = live * (4 * D + 4) + nb * 4 * D
        bwd_bytes = nb * 4 * D + n * 8 + uniq * 8 * D
        med = {k: float(np.median(v)) for k, v in times.items()}
        for what, side, _ in variants:
            us = med[(what, side)]
            extra = {"rounds_us": [round(t, 1) for t in times[(what, side)]]}
            if side != "bag" and (what, "bag") in med:
                extra["bag_over_this"] = round(med[(what, "bag")] / us, 3)
            nbytes = fwd_bytes if what == "fwd" else (n * 16 if what == "sort" else bwd_bytes)
            report(f"embedding_bag {what}: {side} (interleaved, median of {rounds})",
                   dict(cfg, **extra), us, nbytes, out)
        del table, gathered, acc_row
        torch.cuda.empty_cache()


def embedding_q8(iters, out, rounds=5):
    """Row-wise int8 tables against the fp32 ones, interleaved in one process (`rounds` rounds of
    every variant, each timed over `iters` launches; medians reported, every round's time next to
    them). One table of 8M rows, D = 128 and 64 (fp32 4 / 2 GB, q8 1.15 GB / 640 MB: all well past
    the 256 MB Infinity Cache), 2M int32 ids, uniform and the bench's Zipf(1.05) spread over the
    table; both sides read the same ids. Lookup: rs_embedding_q8_fwd against rs_embedding_fwd.
    Bag (mean, fixed length 1, 10, 100): rs_embedding_bag_q8_fwd against rs_embedding_bag_fwd.
    Bytes: every id 4, every row read once (4 D fp32, q_ld quantised), every output row 4 D."""
    from recommender_amd.synthetic import _spread, bounded_zipf

    rng = np.random.default_rng(4)
    st = L.stream_ptr(torch.device(DEV))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    V, n = 8_000_000, 2_097_152
    id_sets = {"uniform": rng.integers(0, V, n).astype(np.int32),
               "zipf1.05": _spread(bounded_zipf(rng, n, V), V).astype(np.int32)}
    for D in (128, 64):
        table = torch.empty(V, D, device=DEV).uniform_(-0.05, 0.05)
        q_ld = int(L.lib().rs_q8_row_bytes(D))
        qt = torch.empty(V, q_ld, dtype=torch.uint8, device=DEV)

        def quant():
            L.call("rs_quantize_rows_q8", L.ptr(table), D, V, D, L.ptr(qt), q_ld, L.ptr(err), st)

        report("rs_quantize_rows_q8", {"rows": V, "D": D, "q_ld": q_ld}, timed(quant, 3),
               V * (4 * D + q_ld), out)
        outp = torch.empty(n, D, device=DEV)
        for dist, ids_np in id_sets.items():
            ids = torch.from_numpy(ids_np).to(DEV)

            def lookup_f():
                L.call("rs_embedding_fwd", L.ptr(table), V, D, L.ptr(ids), 0, n, None, 1,
                       L.ptr(outp), L.ptr(err), st)

            def lookup_q():
                L.call("rs_embedding_q8_fwd", L.ptr(qt), V, D, q_ld, L.ptr(ids), 0, n, None, 1,
                       L.ptr(outp), D, L.ptr(err), st)

            def bag_f(nb, bl):
                L.call("rs_embedding_bag_fwd", L.ptr(table), V, D, L.ptr(ids), 0, nb * bl, None,
                       nb, bl, None, None, L.RS_BAG_MEAN, None, 1, L.ptr(outp), D, None,
                       L.ptr(err), st)

            def bag_q(nb, bl):
                L.call("rs_embedding_bag_q8_fwd", L.ptr(qt), q_ld, V, D, L.ptr(ids), 0, nb * bl,
                       None, nb, bl, None, None, L.RS_BAG_MEAN, None, 1, L.ptr(outp), D, None,
                       L.ptr(err), st)

            variants = [("lookup", "fp32", lookup_f, n * (8 * D + 4)),
                        ("lookup", "q8", lookup_q, n * (q_ld + 4 * D + 4))]
            for bl in (1, 10, 100):
                nb = n // bl
                variants.append((f"bag L={bl}", "fp32", lambda nb=nb, bl=bl: bag_f(nb, bl),
                                 nb * bl * (4 * D + 4) + nb * 4 * D))
                variants.append((f"bag L={bl}", "q8", lambda nb=nb, bl=bl: bag_q(nb, bl),
                                 nb * bl * (q_ld + 4) + nb * 4 * D))
            times = {v[:2]: [] for v in variants}
            for _ in range(rounds):
                for what, side, fn, _ in variants:
                    times[(what, side)].append(timed(fn, iters))
            med = {k: float(np.median(v)) for k, v in times.items()}
            for what, side, _, nbytes in variants:
                cfg = {"rows": V, "D": D, "q_ld": q_ld, "n_ids": n, "ids": dist,
                       "rounds_us": [round(t, 1) for t in times[(what, side)]]}
                if side == "q8":
                    cfg["fp32_over_q8_time"] = round(med[(what, "fp32")] / med[(what, "q8")], 3)
                report(f"embedding_q8 {what}: {side} (interleaved, median of {rounds})", cfg,
                       med[(what, side)], nbytes, out)
        assert int(err.item()) == 0
        del table, qt, outp
        torch.cuda.empty_cache()


def dlrm_score(iters, out, rounds=5):
    """DLRM scoring for serving against the parent's fastest forward, interleaved in one process
    (`rounds` rounds of every variant, each timed over `iters` launches; medians reported, every
    round's time next to them). One table of 8M rows (fp32 4 GB at D = 128: past the Infinity
    Cache), 26 slots laid out as slab offsets over it, B = 65 536, int32 ids, uniform and the
    bench's Zipf(1.05) per slot, D = 128 and 64. Bytes per example, S = 26, nz = 351:
      rs_dlrm_interaction_fwd_head (D = 128 only)  read S·4D + 4D + 4S, written 4(nz + D) + 4
      rs_dlrm_score                                 read S·4D + 4D + 4S, written 4
      rs_dlrm_score_q8 (16-byte and 4-byte reads)   read S·q_ld + 4D + 4S, written 4
    The 4-byte read form is reached by the same table placed 4 bytes off its allocation. Module
    level (uniform ids): DLRM.forward under no_grad (the parent's route: interaction row to HBM,
    top MLP as three GEMMs) against DLRM.score and against the quantised model's forward; their
    bytes are the kernel's above (the MLPs' weights are not counted)."""
    from recommender_amd.ctr.train import build_model
    from recommender_amd.quantized import QuantizedEmbedding
    from recommender_amd.synthetic import _spread, bounded_zipf

    rng = np.random.default_rng(4)
    dev = torch.device(DEV, 0)
    st = L.stream_ptr(dev)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    S, B = 26, 65536
    card = 8_000_000 // S
    V = card * S
    so = torch.arange(S + 1, dtype=torch.int64, device=DEV) * card
    id_sets = {"uniform": rng.integers(0, card, (B, S)).astype(np.int32),
               "zipf1.05": _spread(bounded_zipf(rng, B * S, card), card).astype(np.int32)
               .reshape(B, S)}
    nz = S * (S + 1) // 2
    for D in (128, 64):
        g = torch.Generator(device=DEV)
        g.manual_seed(4)
        model = build_model("DLRM", D, V, S, 13, dev, slot_cardinalities=[card] * S, generator=g)
        table = model.embedding_layer.weight.detach()
        q_ld = int(L.lib().rs_q8_row_bytes(D))
        bufs = [torch.zeros(V * q_ld + 16, dtype=torch.uint8, device=DEV) for _ in range(2)]
        qts = [b[sh:sh + V * q_ld].view(V, q_ld) for b, sh in zip(bufs, (0, 4))]
        for qt in qts:
            L.call("rs_quantize_rows_q8", L.ptr(table), D, V, D, L.ptr(qt), q_ld, L.ptr(err), st)
        width = (nz + D + 15) // 16 * 16
        q = torch.randn(width, device=DEV) * 0.05
        c = torch.full((1,), 0.1, device=DEV)
        dense = torch.relu(torch.randn(B, D, device=DEV))
        row = torch.empty(B, width, device=DEV)
        y = torch.empty(B, device=DEV)
        qmodel = build_model("DLRM", D, S, S, 13, dev, slot_cardinalities=[1] * S)
        qmodel.bottom_mlp, qmodel.top_mlp = model.bottom_mlp, model.top_mlp
        qmodel.embedding_layer = QuantizedEmbedding(V, D, device=dev, slot_offsets=so, q_ld=q_ld,
                                                    qweight=qts[0])
        rd = S * 4 * D + 4 * D + 4 * S
        rq = S * q_ld + 4 * D + 4 * S
        for dist, ids_np in id_sets.items():
            ids = torch.from_numpy(ids_np).to(DEV)
            x = {"cat_features": ids, "int_features": torch.rand(B, 13, device=DEV)}

            def head():
                L.call("rs_dlrm_interaction_fwd_head", L.ptr(table), V, D, L.ptr(ids), 0, S,
                       L.ptr(so), L.ptr(dense), B, L.ptr(row), width, L.ptr(q), L.ptr(c), 2,
                       L.ptr(y), L.ptr(err), st)

            def score():
                L.call("rs_dlrm_score", L.ptr(table), V, D, L.ptr(ids), 0, S, L.ptr(so),
                       L.ptr(dense), B, L.ptr(q), L.ptr(c), 2, L.ptr(y), L.ptr(err), st)

            def score_q8(qt):
                L.call("rs_dlrm_score_q8", L.ptr(qt), q_ld, V, D, L.ptr(ids), 0, S, L.ptr(so),
                       L.ptr(dense), B, L.ptr(q), L.ptr(c), 2, L.ptr(y), L.ptr(err), st)

            def no_grad(m, fn):
                def run():
                    with torch.no_grad():
                        fn(m)
                return run

            variants = []
            if D == 128:
                variants.append(("rs_dlrm_interaction_fwd_head fp32", head,
                                 B * (rd + 4 * (nz + D) + 4)))
            variants += [("rs_dlrm_score fp32", score, B * (rd + 4)),
                         ("rs_dlrm_score_q8 16-byte reads", lambda: score_q8(qts[0]), B * (rq + 4)),
                         ("rs_dlrm_score_q8 4-byte reads", lambda: score_q8(qts[1]), B * (rq + 4))]
            if dist == "uniform":
                variants += [
                    ("DLRM.forward no_grad fp32", no_grad(model, lambda m: m(x)),
                     B * (rd + 4 * (nz + D) + 4)),
                    ("DLRM.score fp32", no_grad(model, lambda m: m.score(x)), B * (rd + 4)),
                    ("DLRM.forward quantised", no_grad(qmodel, lambda m: m(x)), B * (rq + 4))]
            times = {v[0]: [] for v in variants}
            for _ in range(rounds):
                for name, fn, _ in variants:
                    times[name].append(timed(fn, iters))
            med = {k: float(np.median(v)) for k, v in times.items()}
            base = "rs_dlrm_interaction_fwd_head fp32" if D == 128 else "rs_dlrm_score fp32"
            for name, _, nbytes in variants:
                cfg = {"rows": V, "D": D, "q_ld": q_ld, "slots": S, "batch": B, "ids": dist,
                       "rounds_us": [round(t, 1) for t in times[name]]}
                ref = "DLRM.forward no_grad fp32" if name.startswith("DLRM.") else base
                cfg[f"time_of_{ref.split()[0]}_over_this"] = round(med[ref] / med[name], 3)
                report(f"dlrm_score {name} (interleaved, median of {rounds})", cfg, med[name],
                       nbytes, out)
        assert int(err.item()) == 0
        del model, qmodel, table, qts, bufs, row
        torch.cuda.empty_cache()


def group_auc(iters, out, rounds=5):
    """rs_group_auc against the same counts from torch ops on the GPU (a two-key stable torch.sort,
    cumsum and index_add_), interleaved in one process: `rounds` rounds of both, each timed with
    events over `iters` calls; medians reported, every round's time next to them. n = 2^22
    predictions (512 distinct levels: ties) over 2^16 users with Zipf(1.05) and with uniform
    membership (int64 user ids), and one group of 2^22 (group = NULL; the torch side then sorts
    once) with the same 512 levels and with continuous predictions (about 3.7M tie runs). Both sides are checked equal before timing. Bytes: pred, label 4 + 4 and the id 8 per
    example read, 24 per group written."""
    from recommender_amd.synthetic import bounded_zipf

    rng = np.random.default_rng(4)
    dev = torch.device(DEV)
    st = L.stream_ptr(dev)
    n, U = 1 << 22, 1 << 16
    pred = torch.from_numpy((rng.integers(0, 512, n) / 512).astype(np.float32)).to(dev)
    label = torch.from_numpy((rng.random(n) < 0.3).astype(np.float32)).to(dev)
    ids = rng.permutation(U).astype(np.int64) * 1_000_003 - (1 << 35)
    distinct = torch.from_numpy(rng.random(n).astype(np.float32)).to(dev)  # nearly every run of one
    groups = {"zipf1.05": (torch.from_numpy(ids[bounded_zipf(rng, n, U) % U]).to(dev), pred),
              "uniform": (torch.from_numpy(ids[rng.integers(0, U, n)]).to(dev), pred),
              "one group": (None, pred),
              "one group, continuous predictions": (None, distinct)}
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    w2 = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = L.scratch(L.lib().rs_group_auc_workspace_size(n), dev)

    def fused(g, pred):
        L.call("rs_group_auc", L.ptr(pred), L.ptr(label), L.ptr(g), L.RS_ID_I64, n, L.ptr(keys),
               L.ptr(cnt), L.ptr(pos), L.ptr(w2), L.ptr(info), L.ptr(info[1:]), L.ptr(ws),
               ws.numel(), st)

    def torch_counts(g, pred):
        p, perm = torch.sort(pred, stable=True)
        if g is not None:
            gs, i2 = torch.sort(g[perm], stable=True)
            p, perm = p[i2], perm[i2]
        else:
            gs = torch.zeros(n, dtype=torch.int64, device=dev)
        neg = (label[perm] == 0).to(torch.int64)
        negcum = torch.cat([neg.new_zeros(1), torch.cumsum(neg, 0)])
        one = torch.ones(1, dtype=torch.bool, device=dev)
        ghead = torch.cat([one, gs[1:] != gs[:-1]])
        rhead = ghead | torch.cat([one, p[1:] != p[:-1]])
        g0 = torch.nonzero(ghead).view(-1)
        r0 = torch.nonzero(rhead).view(-1)
        end = torch.full((1,), n, dtype=torch.int64, device=dev)
        r1, g1 = torch.cat([r0[1:], end]), torch.cat([g0[1:], end])
        g_of_run = torch.cumsum(ghead.to(torch.int64), 0)[r0] - 1
        neg_before = negcum[r0] - negcum[g0[g_of_run]]
        neg_in = negcum[r1] - negcum[r0]
        contrib = ((r1 - r0) - neg_in) * (2 * neg_before + neg_in)
        w = torch.zeros(g0.numel(), dtype=torch.int64, device=dev).index_add_(0, g_of_run, contrib)
        c = g1 - g0
        return gs[g0], c, c - (negcum[g1] - negcum[g0]), w, r0.numel()

    for what, (g, pred) in groups.items():
        fused(g, pred)
        G = int(info[0])
        *ref, runs = torch_counts(g, pred)
        assert int(info[1]) == 0 and G == ref[0].numel()
        for a, b in zip((keys, cnt, pos, w2), ref):
            assert torch.equal(a[:G].to(torch.int64), b), what
        variants = [("rs_group_auc", lambda g=g, p=pred: fused(g, p)),
                    ("torch sort + cumsum", lambda g=g, p=pred: torch_counts(g, p))]
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, fn in variants:
                times[name].append(timed(fn, iters))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, _ in variants:
            cfg = {"n": n, "groups": G, "membership": what, "tie_runs": runs,
                   "rounds_us": [round(t, 1) for t in times[name]]}
            if name == "rs_group_auc":
                cfg["torch_over_fused_time"] = round(med["torch sort + cumsum"] / med[name], 3)
            report(f"group_auc {what}: {name} (interleaved, median of {rounds})", cfg, med[name],
                   n * (8 + (8 if g is not None else 0)) + 24 * G, out)


def criteo(iters, out):
    """Criteo TSV ingestion: line index + parse + vocab lookup over a ~45 MB synthetic text
    (algorithmic bytes: text read once, outputs written once)."""
    from recommender_amd.data import CriteoVocab, read_criteo_tsv
    from tests.criteo_text import make_tsv

    text = make_tsv(np.random.default_rng(4), 200_000, vocab=5000).encode()
    vocab = CriteoVocab.build(text)
    n = text.count(b"\n") + 1
    out_bytes = n * (26 * 8 + 13 * 4 + 4)
    us = timed(lambda: vocab.encode(text), max(3, iters // 4))
    cfg = {"lines": n, "text_MB": round(len(text) / 1e6, 1), "vocab": vocab.size,
           "includes": "pinned host->device copy of the text + 3 host syncs"}
    report("criteo_encode(host tsv->device ids)", cfg, us, len(text) + out_bytes, out)
    dtext = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV)
    us = timed(lambda: vocab.encode(dtext), iters)
    cfg = dict(cfg, includes="text already in HBM; line index + parse + lookup + 3 host syncs")
    report("criteo_encode(device tsv->ids)", cfg, us, len(text) + out_bytes, out)
    _, _, hashes, _ = read_criteo_tsv(dtext)
    us = timed(lambda: vocab.lookup(hashes), iters)
    report("rs_vocab_lookup", {"tokens": hashes.numel(), "capacity": vocab.capacity}, us,
           hashes.numel() * 16, out)


def textpipe(iters, out):
    """Ali-CCP join + vocab + encode and Amazon (DIEN) vocab + encode on
    synthetic text already in HBM, beside the oracle's CPU time for the same text. Algorithmic
    bytes: every text byte read once + the id / label outputs written once."""
    import time

    from oracle import textpipe as O
    from recommender_amd.data import AliCCPVocab, DienVocab, aliccp_join
    from recommender_amd.data.aliccp import parse_kv_csv
    from tests.textpipe_text import make_aliccp, make_amazon

    rng = np.random.default_rng(4)
    sk, cm = make_aliccp(rng, 100_000, 5_000, n_vals=3000)
    dsk = torch.frombuffer(bytearray(sk.encode()), dtype=torch.uint8).to(DEV)
    dcm = torch.frombuffer(bytearray(cm.encode()), dtype=torch.uint8).to(DEV)
    rows = aliccp_join(dsk, dcm)
    vocab = AliCCPVocab.build(rows)

    def full():
        r = aliccp_join(dsk, dcm)
        v = AliCCPVocab.build(r)
        return v.encode(r)

    us = timed(full, max(3, iters // 4))
    t0 = time.perf_counter()
    orows = O.aliccp_join(sk, cm)
    O.aliccp_encode(orows, O.aliccp_vocab(orows))
    cpu_s = time.perf_counter() - t0
    nbytes = dsk.numel() + dcm.numel() + rows.n * (18 * 4 + 8)
    cfg = {"skeleton_lines": sk.count("\n"), "common_lines": cm.count("\n"), "kept": rows.n,
           "text_MB": round((dsk.numel() + dcm.numel()) / 1e6, 1), "vocab": sum(vocab.sizes),
           "oracle_cpu_s": round(cpu_s, 3),
           "includes": "parse both files, map, join, count, collect, sort, assign, encode; 6 host syncs"}
    report("aliccp_pipeline(device csv->ids)", cfg, us, nbytes, out)
    us = timed(lambda: parse_kv_csv(dsk, 3, 5, True), iters)
    report("rs_kv_parse(skeleton, incl. line index)", {"lines": cfg["skeleton_lines"]}, us,
           dsk.numel() + rows.n * 18 * 9, out)

    text = make_amazon(rng, 100_000, n_items=60_000, n_cats=800, max_hist=100)
    dt = torch.frombuffer(bytearray(text.encode()), dtype=torch.uint8).to(DEV)
    v = DienVocab.build(dt)

    def dien_full():
        vv = DienVocab.build(dt)
        return vv.encode(dt, 100, sample_negative=True, seed=4)

    us = timed(dien_full, max(3, iters // 4))
    t0 = time.perf_counter()
    items, cats, i2c = O.dien_vocab(text)
    O.dien_encode(text, items, cats, 100)
    cpu_s = time.perf_counter() - t0
    n = text.count("\n")
    nbytes = dt.numel() + n * (4 * 100 * 4 + 12)
    cfg = {"lines": n, "maxlen": 100, "text_MB": round(dt.numel() / 1e6, 1),
           "items": v.items.size, "cats": v.cats.size, "oracle_cpu_s_without_negatives": round(cpu_s, 3),
           "includes": "parse (2 passes), 2 vocab builds, item->cat map, encode + negatives; 5 host syncs"}
    report("dien_pipeline(device text->ids)", cfg, us, nbytes, out)
    us = timed(lambda: v.encode(dt, 100, sample_negative=True, seed=4), iters)
    report("dien_encode(device text->ids, vocab built)", {"lines": n}, us, nbytes, out)


def dlrm_path(iters, out):
    """The north-star embedding path's four launches run alone and back to back on one stream
    (no co-running GEMMs), at the bench config: 26 slots over a 40M x 128 fp32 slab, batch
    65 536, Zipf ids. SGD with lr 0 so repeated applies move the same bytes without drifting.
    Bytes: SURVEY §8(d) per-kernel formulas (bench.py kernel_bytes); path = §8(d) whole-path."""
    from bench import kernel_bytes
    from recommender_amd.optim import SortedIds
    from recommender_amd.synthetic import criteo_batch, criteo_cardinalities

    S, D, B, V = 26, 128, 65536, 40_000_000
    cards = criteo_cardinalities(V, S)
    so = torch.tensor(np.concatenate([[0], np.cumsum(cards)]), dtype=torch.int64, device=DEV)
    table = torch.empty(V, D, device=DEV)
    table.uniform_(-0.05, 0.05)
    cat, _, _ = criteo_batch(np.random.default_rng(4), B, cards)
    ids = torch.from_numpy(cat).to(DEV)
    dense = torch.randn(B, D, device=DEV)
    Z = 27 * 26 // 2 + D
    inter = torch.empty(B, 512, device=DEV)
    gout = torch.randn(B, 512, device=DEV) * 1e-3
    gemb = torch.empty(B * S, D, device=DEV)
    gden = torch.empty(B, D, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = L.stream_ptr(torch.device(DEV))
    s0 = SortedIds(ids, V, so, err, count_unique=True)
    U = int(s0.n_unique.item())
    ws = torch.empty(L.lib().rs_apply_workspace_size(B * S, D), dtype=torch.uint8, device=DEV)
    prm = L.AdamParams(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)

    def fwd():
        L.call("rs_dlrm_interaction_fwd", L.ptr(table), V, D, L.ptr(ids), 1, S, L.ptr(so),
               L.ptr(dense), B, 1, L.ptr(inter), 512, L.ptr(err), st)

    srows = torch.empty(B * S, dtype=torch.int32, device=DEV)
    spos = torch.empty(B * S, dtype=torch.int32, device=DEV)
    sws = torch.empty(L.lib().rs_sort_ids_workspace_size(B * S), dtype=torch.uint8, device=DEV)

    def srt():  # raw C call on preallocated buffers (no per-call Python allocation)
        L.call("rs_sort_ids", L.ptr(ids), 1, B * S, L.ptr(so), S, V, L.ptr(srows), L.ptr(spos),
               None, L.ptr(err), L.ptr(sws), sws.numel(), st)

    def bwd():
        L.call("rs_dlrm_interaction_bwd", L.ptr(table), V, D, L.ptr(ids), 1, S, L.ptr(so),
               L.ptr(dense), B, 1, L.ptr(gout), 512, L.ptr(gemb), L.ptr(gden), st)

    def apply():
        L.call("rs_embedding_apply", L.RS_OPT_SGD, L.ptr(table), None, None, V, D, L.ptr(s0.rows),
               L.ptr(s0.pos), B * S, L.ptr(gemb), prm, None, L.ptr(ws), ws.numel(), st)

    # the production path (fused forward + unit backward, sort, scaled apply)
    q = torch.randn(480, device=DEV) * 0.05
    cc = torch.zeros(1, device=DEV)
    yv = torch.empty(B, 1, device=DEV)
    G = torch.randn(B, device=DEV) * 1e-3

    xin = torch.rand(B, 13, device=DEV)
    lab = (torch.rand(B, device=DEV) < 0.25).float()
    sums = torch.empty(512 + 2 + 14 * 128, device=DEV)
    tws = torch.empty(L.lib().rs_dlrm_train_workspace_size(B), dtype=torch.uint8, device=DEV)
    yb = torch.empty(B, device=DEV)

    gb = torch.empty(B, device=DEV)

    def train_unit():
        L.call("rs_dlrm_train_step_fwd_unit", L.ptr(table), V, D, L.ptr(ids), 1, S, L.ptr(so),
               L.ptr(dense), L.ptr(xin), 13, L.ptr(lab), B, L.ptr(q), L.ptr(cc), 1e-7, 1.0 / B,
               L.ptr(yb), L.ptr(gemb), L.ptr(gb), L.ptr(sums), L.ptr(tws), tws.numel(), L.ptr(err),
               st)

    def apply_unit():
        L.call("rs_embedding_apply_scaled", L.RS_OPT_SGD, L.ptr(table), None, None, V, D,
               L.ptr(s0.rows), L.ptr(s0.pos), B * S, L.ptr(gemb), L.ptr(gb), S, prm, None,
               L.ptr(ws), ws.numel(), st)

    def fwd_dx():
        L.call("rs_dlrm_interaction_fwd_head_dx", L.ptr(table), V, D, L.ptr(ids), 1, S, L.ptr(so),
               L.ptr(dense), B, L.ptr(inter), 480, L.ptr(q), L.ptr(cc), 2, L.ptr(yv), L.ptr(gemb),
               L.ptr(gden), L.ptr(err), st)

    def apply_scaled():
        L.call("rs_embedding_apply_scaled", L.RS_OPT_SGD, L.ptr(table), None, None, V, D,
               L.ptr(s0.rows), L.ptr(s0.pos), B * S, L.ptr(gemb), L.ptr(G), S, prm, None,
               L.ptr(ws), ws.numel(), st)

    def apply_final():
        L.call("rs_embedding_apply_scaled", L.RS_OPT_SGD, L.ptr(table), None, None, V, D,
               L.ptr(s0.rows), L.ptr(s0.pos), B * S, L.ptr(gemb), None, 1, prm, None,
               L.ptr(ws), ws.numel(), st)

    bwd()
    cfg = {"B": B, "S": S, "D": D, "rows": V, "unique": U}
    per_ex = S * (8 + 8 * D) + S * (8 + 4 * D) + (U / B) * 8 * D
    # the chunked train kernel (unit rows + G, scaled apply)
    tot = 0.0
    for name, fn in (("rs_dlrm_train_step_fwd_unit", train_unit), ("rs_sort_ids", srt),
                     ("rs_embedding_apply_scaled", apply_unit)):
        us = timed(fn, iters)
        tot += us
        report(name + " (alone)", cfg, us, kernel_bytes(name, B, S, D, 8, U), out)
    report("embedding_path (chunked train kernel, sort, scaled apply; alone)",
           dict(cfg, bytes_per_example=round(per_ex, 1)), tot, per_ex * B, out)
    # the previous production path (fused forward + unit backward, scaled apply)
    tot = 0.0
    for name, fn in (("rs_dlrm_interaction_fwd_head_dx", fwd_dx), ("rs_sort_ids", srt),
                     ("rs_embedding_apply_scaled", apply_scaled)):
        us = timed(fn, iters)
        tot += us
        report(name + " (alone)", cfg, us, kernel_bytes(name, B, S, D, 8, U), out)
    report("embedding_path (fwd + unit bwd, scaled apply: 3 launches back to back, alone)",
           dict(cfg, bytes_per_example=round(per_ex, 1)), tot, per_ex * B, out)
    # the previous path (separate re-gathering backward), for the record
    tot = 0.0
    for name, fn in (("rs_dlrm_interaction_fwd", fwd), ("rs_sort_ids", srt),
                     ("rs_dlrm_interaction_bwd", bwd), ("rs_embedding_apply", apply)):
        us = timed(fn, iters)
        tot += us
        report(name + " (alone)", cfg, us, kernel_bytes(name, B, S, D, 8, U), out)
    report("embedding_path (fwd + re-gathering bwd: 4 launches back to back, alone)",
           dict(cfg, bytes_per_example=round(per_ex, 1)), tot, per_ex * B, out)
    apply_kinds(iters, out, table, s0, gemb, ws, cfg, U)


def apply_kinds(iters, out, table, s0, gemb, ws, cfg, U, rounds=5):
    """The sparse apply's three update rules — SGD (the yardstick), element-wise Adagrad and
    row-wise Adagrad — over the same sorted ids and gradient rows, interleaved: `rounds` rounds of
    SGD, Adagrad, row-wise, each timed over `iters` launches; the median round is reported with
    every round's time next to it. lr 0, so the table stays put; the Adagrad accumulators grow by
    g² per launch from 0.1 (no effect on the bytes moved). Bytes: the SGD apply's, plus the
    accumulator read and written per touched row: 8·D bytes element-wise, 8 bytes row-wise."""
    from bench import kernel_bytes

    V, D = table.shape
    n = s0.n
    B, S = cfg["B"], cfg["S"]
    st = L.stream_ptr(torch.device(DEV))
    prm = L.AdamParams(0.0, 0.0, 0.0, 0.0, 0.0, 1e-7)
    acc_el = torch.full((V, D), 0.1, device=DEV)
    acc_row = torch.full((V,), 0.1, device=DEV)
    base = kernel_bytes("rs_embedding_apply", B, S, D, 8, U)
    kinds = (("sgd", L.RS_OPT_SGD, None, base),
             ("adagrad", L.RS_OPT_ADAGRAD, acc_el, base + U * 8 * D),
             ("rowwise_adagrad", L.RS_OPT_ROWWISE_ADAGRAD, acc_row, base + U * 8))
    times = {k[0]: [] for k in kinds}
    for _ in range(rounds):
        for name, opt, acc, _ in kinds:
            times[name].append(timed(lambda: L.call(
                "rs_embedding_apply", opt, L.ptr(table), L.ptr(acc), None, V, D, L.ptr(s0.rows),
                L.ptr(s0.pos), n, L.ptr(gemb), prm, None, L.ptr(ws), ws.numel(), st), iters))
    sgd = float(np.median(times["sgd"]))
    for name, _, _, nbytes in kinds:
        us = float(np.median(times[name]))
        report(f"rs_embedding_apply[{name}] (interleaved, median of {rounds})",
               dict(cfg, rounds_us=[round(t, 1) for t in times[name]],
                    ratio_to_sgd=round(us / sgd, 3)), us, nbytes, out)


def sort_only(iters, out):
    """rs_sort_ids alone at the north-star batch (26 x 65 536 int64 ids over the 40M-row slab),
    called straight through the C ABI on preallocated buffers (no Python allocation per call)."""
    from recommender_amd.synthetic import criteo_batch, criteo_cardinalities

    S, B, V = 26, 65536, 40_000_000
    cards = criteo_cardinalities(V, S)
    so = torch.tensor(np.concatenate([[0], np.cumsum(cards)]), dtype=torch.int64, device=DEV)
    ids = torch.from_numpy(criteo_batch(np.random.default_rng(4), B, cards)[0]).to(DEV)
    n = ids.numel()
    rows = torch.empty(n, dtype=torch.int32, device=DEV)
    pos = torch.empty(n, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.lib().rs_sort_ids_workspace_size(n), dtype=torch.uint8, device=DEV)
    st = L.stream_ptr(torch.device(DEV))
    fn = lambda: L.call("rs_sort_ids", L.ptr(ids), 1, n, L.ptr(so), S, V, L.ptr(rows), L.ptr(pos),
                        None, L.ptr(err), L.ptr(ws), ws.numel(), st)
    us = timed(fn, iters)
    report("rs_sort_ids (raw C call)", {"n_ids": n, "rows": V}, us, n * 8 + n * 8, out)


def chain(iters, out):
    """rs_chain_reduce at the DLRM MLP shapes (factored backward): the top MLP's GEMV over the
    compact interaction row (n0 480, nl 1, sigmoid) and the bottom MLP's 13 x 128 outer
    reduction (relu). Bytes: x, dy, y read once (+ G written for the top)."""
    B = 65536
    for n0, nl, act, gout in ((480, 1, 2, True), (13, 128, 1, False)):
        x = torch.randn(B, n0, device=DEV)
        dy = torch.randn(B, nl, device=DEV)
        y = torch.rand(B, nl, device=DEV)
        o = torch.empty(n0 * nl + nl, device=DEV)
        g = torch.empty(B, nl, device=DEV) if gout else None
        nb = L.lib().rs_chain_reduce_workspace_size(B, n0, nl)
        ws = torch.empty(nb // 4 + 1, device=DEV)
        st = L.stream_ptr(torch.device(DEV))
        fn = lambda: L.call("rs_chain_reduce", L.ptr(x), n0, n0, L.ptr(dy), L.ptr(y), nl, act, B,
                            L.ptr(o), L.ptr(g), L.ptr(ws), ws.numel() * 4, st)
        us = timed(fn, iters)
        by = B * (n0 * 4 + 2 * nl * 4 + (nl * 4 if gout else 0))
        report("rs_chain_reduce", {"B": B, "n0": n0, "nl": nl, "act": act}, us, by, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="dien,pinsage,pinsage_eval,eges,eges_sampler,embedding,criteo,textpipe")
    args = ap.parse_args()
    L.load()
    out = []
    for name in args.only.split(","):
        globals()[name](args.iters, out)


if __name__ == "__main__":
    main()
