"""PinSage whole-catalogue inference, layer by layer (reference pinsage/inference/).

item_neighbors    data_prepare.py:28-43   every item's neighbour table [n_items, k] (ids, visit
                  counts; -1 / 0 = empty slot) from PinSageSampler.neighbors. Draws are keyed by
                  (seed, step, item, walk, layer), so chunking changes no bit.
item_features     data_prepare.py:45-56   the projected features [n_items, 3E] of every item.
convolve          inference.py:8-41       one Convolve layer over all items: fc_1 through the
                  Dense forward, then rs_pinsage_infer_layer (weighted mean of the neighbours'
                  rows, concat, fc_2, activation and the per-row L2 norm of
                  spark_function.py:29-34 in one pass). fused=False, or shapes past the kernel's
                  limits, compose the existing kernels instead (_convolve_unfused).
infer_item_reprs  the features, every model.sagenet.convolves[l] over the same neighbour table,
                  then the head fc_2(fc_1(·)) as SageNet.forward; feeds evaluation.recommend.

Unlike evaluation.get_item_reprs (seeds pushed through the sampler and the model 32 at a time,
two blocks and several host reads per batch, a result that depends on batch_size), this embeds
each layer once for every item and needs no block: the dst nodes are the items in order, the
src nodes the same items.

Differences from the Spark demo:
  * the concat order is the trained model's [nv, h] (layers.py:26); the demo's [h, nv] is a row
    permutation of fc_2's kernel;
  * an item with no neighbour keeps a row, with nv = 0 (the weight sum clipped to 1 as
    layers.py:23); the demo's inner join drops it;
  * a row whose norm is 0 stays zero (the demo's l2norm gives NaN).
norm: "row" is the reference's inference norm; "frobenius" divides by one norm over all items —
what the trained model's own Convolve computes with every item in one batch (it was trained
under that global norm, layers.py:28-29); None leaves fc_2's output as it is.

`python -m recommender_amd.pinsage.inference [--graph ml1m|ml20m] [--out reprs.npy]` runs it on
the synthetic MovieLens graph of pinsage/train.py; `--neighbors K --neighbors-out nbrs.npy` adds
each item's K nearest items by inner product (rs_topk_ip, the item itself excluded);
`--neighbors-nlist N --neighbors-nprobe P` searches them through an IVF index (retrieval.py),
`--neighbors-int8 KC` through the int8 candidate scan with an exact re-rank (retrieval.Int8Index).
"""
from __future__ import annotations

import argparse
import time

import torch

from .. import _lib as L
from ..nn import Dense, _affine
from .layers import frobenius_normalize

_NORMS = ("row", "frobenius", None)


def item_neighbors(sampler, step: int | None = None, batch_size: int | None = None):
    """(nbr, cnt) [n_items, k] int32 for every item: PinSageSampler.neighbors(arange(n_items),
    layer 0, no exclusion) at RNG step `step` (default: the sampler's current step, which is not
    advanced), optionally batch_size items at a time — bit-equal however it is chunked."""
    n, dev = sampler.g.n_items, sampler.g.device
    bs = n if not batch_size else int(batch_size)
    parts = []
    for b0 in range(0, n, max(bs, 1)):
        ids = torch.arange(b0, min(n, b0 + bs), dtype=torch.int32, device=dev)
        parts.append(sampler.neighbors(ids, 0, None, step))
    if len(parts) == 1:
        return parts[0]
    return (torch.cat([p[0] for p in parts]).contiguous(),
            torch.cat([p[1] for p in parts]).contiguous())


def item_features(model, batch_size: int | None = None) -> torch.Tensor:
    """model.feature_projector over every item, [n_items, 3E], without gradients."""
    fp = model.feature_projector
    n, dev = fp.item_id.numel(), fp.item_id.device
    bs = n if not batch_size else int(batch_size)
    with torch.no_grad():
        parts = [fp(torch.arange(b0, min(n, b0 + bs), dtype=torch.int32, device=dev))
                 for b0 in range(0, n, max(bs, 1))]
        return parts[0] if len(parts) == 1 else torch.cat(parts)


def _kernel_bias(fc):
    """(kernel [in, out], bias [out]) of a Dense module or a (kernel, bias) pair."""
    k, b = (fc.kernel, fc.bias) if isinstance(fc, Dense) else fc
    k = k.detach().float().contiguous()
    b = torch.zeros(k.shape[1], device=k.device) if b is None else b.detach().float().contiguous()
    return k, b


def fused_supported(d_in: int, hidden: int, d_out: int, k: int) -> bool:
    """The shapes rs_pinsage_infer_layer takes (the entry point refuses the others)."""
    return (1 <= d_in <= L.RS_PINSAGE_INFER_MAX_DIN and 1 <= hidden <= L.RS_PINSAGE_INFER_MAX_HIDDEN
            and 1 <= d_out <= L.RS_PINSAGE_INFER_MAX_DOUT and 1 <= k <= L.RS_PINSAGE_INFER_MAX_K)


def neighbor_csr(nbr: torch.Tensor, cnt: torch.Tensor, err_flag: torch.Tensor | None = None):
    """(indptr [n+1] int32, edge_src int32, edge_w float32) of the neighbour table, edges in
    slot order: the CSR rs_weighted_mean_agg_fwd reads. Empty slots (-1, or a zero count) carry
    no edge; any other id outside [0, n_items) carries none either and sets RS_ERRBIT_OOB."""
    n = nbr.shape[0]
    if nbr.numel() >= 2**31:
        raise ValueError("neighbor_csr: n_items * k must stay below 2^31 (int32 edge offsets)")
    inside = (nbr >= 0) & (nbr < n)
    if err_flag is not None:
        err_flag |= ((nbr != -1) & ~inside).any().to(torch.int32) * L.RS_ERRBIT_OOB
    valid = inside & (cnt != 0)
    indptr = torch.zeros(n + 1, dtype=torch.int32, device=nbr.device)
    indptr[1:] = torch.cumsum(valid.sum(1), 0)
    edge_src = nbr[valid].contiguous()
    edge_w = cnt[valid].float().contiguous()
    if edge_src.numel() == 0:  # a pointer to read from, never dereferenced
        edge_src = torch.zeros(1, dtype=torch.int32, device=nbr.device)
        edge_w = torch.zeros(1, device=nbr.device)
    return indptr, edge_src, edge_w


def _row_normalize(z: torch.Tensor) -> torch.Tensor:
    nrm = torch.linalg.vector_norm(z, dim=1, keepdim=True)
    return torch.where(nrm > 0, z / nrm, torch.zeros_like(z))


def _convolve_unfused(h, u, nbr, cnt, k2, b2, act, norm, err_flag, csr=None):
    """The layer from the existing kernels: rs_weighted_mean_agg_fwd on the table's CSR, cat,
    the Dense forward, then the norm. The fallback past the fused kernel's limits, the
    benchmark's baseline and the tests' cross-check."""
    n, H = u.shape
    dev = h.device
    indptr, edge_src, edge_w = csr if csr is not None else neighbor_csr(nbr, cnt, err_flag)
    nv = torch.empty(n, H, device=dev)
    L.call("rs_weighted_mean_agg_fwd", L.ptr(u), n, H, L.ptr(indptr), L.ptr(edge_src),
           L.ptr(edge_w), n, L.ptr(nv), None, L.stream_ptr(dev))
    z = _affine(torch.cat([nv, h], dim=-1), k2, b2, act)
    if norm == "row":
        return _row_normalize(z)
    return frobenius_normalize(z) if norm == "frobenius" else z


def layer_from_u(h, u, nbr, cnt, k2, b2, act: int, norm, fused, err_flag, csr=None):
    """The layer after fc_1 (u = fc_1(h) given; contiguous fp32 / int32 device tensors, act 0 / 1):
    rs_pinsage_infer_layer when fused is not False and the shapes fit, else _convolve_unfused.
    Out-of-range ids set RS_ERRBIT_OOB in err_flag ([1] int32 device); nothing is raised here."""
    n, d_in = h.shape
    hidden, d_out, k = u.shape[1], k2.shape[1], nbr.shape[1]
    if fused is False or n == 0 or not fused_supported(d_in, hidden, d_out, k):
        return _convolve_unfused(h, u, nbr, cnt, k2, b2, act, norm, err_flag, csr)
    out = torch.empty(n, d_out, device=h.device)
    L.call("rs_pinsage_infer_layer", L.ptr(h), n, d_in, L.ptr(u), hidden, L.ptr(nbr), L.ptr(cnt),
           k, L.ptr(k2), L.ptr(b2), d_out, act, 1 if norm == "row" else 0, L.ptr(out),
           L.ptr(err_flag), L.stream_ptr(h.device))
    return frobenius_normalize(out) if norm == "frobenius" else out


def convolve(h: torch.Tensor, nbr: torch.Tensor, cnt: torch.Tensor, fc1, fc2,
             activation: str | None = "relu", norm: str | None = "row",
             fused: bool | None = None, csr=None) -> torch.Tensor:
    """One Convolve layer over all items (inference.py:8-41): h [n_items, d_in] → [n_items,
    d_out]. fc1 / fc2: nn.Dense modules or (kernel, bias) pairs, fc2's kernel with rows [nv ; h].
    activation: "relu" (the trained model) or None (the Spark demo's fc). norm: "row",
    "frobenius" or None. fused: None / True = rs_pinsage_infer_layer when the shapes fit, False =
    the composition of the existing kernels (csr: its neighbor_csr, when the caller keeps one).
    Raises RecsysError at the end if a slot held an id other than -1 outside [0, n_items)."""
    if activation not in ("relu", None, "linear"):
        raise ValueError(f"convolve: activation must be 'relu' or None, got {activation!r}")
    if norm not in _NORMS:
        raise ValueError(f"convolve: norm must be one of {_NORMS}, got {norm!r}")
    L.require_device(h, "h")
    act = 1 if activation == "relu" else 0
    dev = h.device
    with torch.no_grad():
        h = h.detach().float().contiguous()
        nbr = nbr.to(torch.int32).contiguous()
        cnt = cnt.to(torch.int32).contiguous()
        n, d_in = h.shape
        if nbr.shape != cnt.shape or nbr.dim() != 2 or nbr.shape[0] != n:
            raise ValueError("convolve: nbr and cnt must both be [n_items, k]")
        k = nbr.shape[1]
        k1, b1 = _kernel_bias(fc1)
        k2, b2 = _kernel_bias(fc2)
        hidden, d_out = k1.shape[1], k2.shape[1]
        if k1.shape[0] != d_in or k2.shape[0] != hidden + d_in:
            raise ValueError(f"convolve: fc1 must be [{d_in}, hidden] and fc2 [hidden + {d_in}, "
                             f"d_out], got {tuple(k1.shape)} and {tuple(k2.shape)}")
        err_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        u = _affine(h, k1, b1, act)
        out = layer_from_u(h, u, nbr, cnt, k2, b2, act, norm, fused, err_flag, csr)
    if int(err_flag.item()) & L.RS_ERRBIT_OOB:
        raise L.RecsysError("pinsage convolve: a neighbour id outside [0, n_items) (its slot "
                            "was skipped)")
    return out


def infer_item_reprs(model, sampler, norm: str | None = "row", step: int | None = None,
                     fused: bool | None = None, return_stages: bool = False):
    """Every item's representation [n_items, conv_output_size], layer-wise: item_features, each
    model.sagenet.convolves[l] over one neighbour table (item_neighbors at `step`), then the head
    fc_2(fc_1(·)) as SageNet.forward. return_stages: also the list [features, layer 1, ...,
    layer L, head output] and the table (nbr, cnt)."""
    net = model.sagenet
    h = item_features(model)
    nbr, cnt = item_neighbors(sampler, step)
    csr = neighbor_csr(nbr, cnt) if fused is False else None
    stages = [h]
    for conv in net.convolves:
        h = convolve(h, nbr, cnt, conv.fc_1, conv.fc_2, "relu", norm, fused, csr)
        stages.append(h)
    with torch.no_grad():
        out = net.fc_2(net.fc_1(h))
    stages.append(out)
    return (out, stages, (nbr, cnt)) if return_stages else out


def main(argv=None):
    from ..synthetic import ML20M
    from .model import PinSageModel
    from .sampler import PinSageSampler
    from .train import ML1M, build_dataset

    ap = argparse.ArgumentParser(description="PinSage layer-wise inference on the synthetic "
                                             "MovieLens graph")
    ap.add_argument("--graph", choices=["ml1m", "ml20m"], default="ml1m")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--norm", choices=["row", "frobenius", "none"], default="row")
    ap.add_argument("--fused", type=int, default=1, help="0: compose the existing kernels")
    ap.add_argument("--out", default=None, help="write the representations to this .npy file")
    ap.add_argument("--neighbors", type=int, default=0, metavar="K",
                    help="with --neighbors-out: each item's K nearest items by inner product")
    ap.add_argument("--neighbors-out", default=None, metavar="FILE",
                    help="write the [n_items, K] int32 neighbour ids (best first, the item "
                         "itself excluded, -1 = none left) to this .npy file")
    ap.add_argument("--neighbors-nlist", type=int, default=0, metavar="N",
                    help="search the neighbours through an IVF index of N lists (0: exact)")
    ap.add_argument("--neighbors-nprobe", type=int, default=8, metavar="P",
                    help="lists searched per item with --neighbors-nlist")
    ap.add_argument("--neighbors-int8", type=int, default=0, metavar="KC",
                    help="search the neighbours in two stages: an int8 scan keeps KC candidates "
                         "per item, the exact fp32 re-rank keeps K (0: exact)")
    args = ap.parse_args(argv)
    if bool(args.neighbors) != bool(args.neighbors_out):
        ap.error("--neighbors K and --neighbors-out FILE go together")
    if args.neighbors_int8 and (args.neighbors_nlist > 0 or args.neighbors_int8 < args.neighbors):
        ap.error("--neighbors-int8 KC needs KC >= K and excludes --neighbors-nlist")
    torch.manual_seed(args.seed)
    g, _, _ = build_dataset(ML1M if args.graph == "ml1m" else ML20M, args.seed)
    model = PinSageModel(g, g.itype, 2, 8, 32, 16)
    sampler = PinSageSampler(g, g.itype, g.utype, 2, 2, 4, 0, 3, seed=args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reprs = infer_item_reprs(model, sampler, None if args.norm == "none" else args.norm,
                             fused=None if args.fused else False)
    torch.cuda.synchronize()
    print(f"{tuple(reprs.shape)} item representations in {(time.perf_counter() - t0) * 1e3:.1f} ms "
          f"(first call: includes library and kernel loading)")
    if args.out:
        import numpy as np

        np.save(args.out, reprs.cpu().numpy())
        print(f"wrote {args.out}")
    if args.neighbors_out:
        import numpy as np

        from ..functional import topk_inner_product

        own = torch.arange(reprs.shape[0], dtype=torch.int32, device=reprs.device)
        if args.neighbors_nlist > 0:
            from ..retrieval import IVFIndex

            index = IVFIndex.build(reprs, args.neighbors_nlist)
            nbrs, _ = index.search(reprs, args.neighbors, args.neighbors_nprobe, exclude_one=own,
                                   with_scores=False)
        elif args.neighbors_int8 > 0:
            from ..retrieval import Int8Index

            nbrs, _ = Int8Index.from_float(reprs).search(reprs, args.neighbors,
                                                         args.neighbors_int8, exclude_one=own,
                                                         with_scores=False)
        else:
            nbrs, _ = topk_inner_product(reprs, reprs, args.neighbors, exclude_one=own,
                                         with_scores=False)
        np.save(args.neighbors_out, nbrs.cpu().numpy())
        print(f"wrote {args.neighbors_out}")
    return reprs


if __name__ == "__main__":
    main()
