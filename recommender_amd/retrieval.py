"""IVF (inverted-file) approximate top-k inner-product retrieval: the catalogue clustered once by
k-means, every query scored only against the lists whose centroids it scores highest with
(include/recsys_hip.h, "IVF top-k inner-product retrieval").

IVFIndex.build            Lloyd's k-means by Euclidean distance out of three existing kernels:
                          assignment is rs_topk_ip with k = 1 over [x, 1] · [c, -½‖c‖²]
                          (argmin ‖x - c‖², ties to the lower list), the centroid mean is
                          rs_embedding_bag_fwd in RS_BAG_MEAN over the members in ascending id
                          order, grouping is a stable sort. Every step is deterministic: two
                          builds are bit-identical.
IVFIndex.from_assignment  the index of a given (centroids, assignment): how build finishes and
                          how tests hand-build indexes.
IVFIndex.search           coarse step topk_inner_product(queries, centroids, nprobe), then the
                          list scan rs_ivf_topk_ip. The result equals the exhaustive result
                          restricted to the probed lists, bit for bit; with nprobe = nlist it is
                          topk_inner_product's.

Int8Index                 the other approximate form, with nothing to train: an
                          int8 MFMA scan of the whole catalogue keeps n_candidates items per
                          query (rs_topk_ip_i8), the exact fp32 re-rank keeps k (rs_rerank_ip).
search_index              one search call for either index type.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .functional import (ivf_topk_inner_product, quantize_rows_i8, rerank_inner_product,
                         topk_inner_product, topk_inner_product_i8)

_KEYS = ("centroids", "centroid_bias", "list_offsets", "item_ids", "vectors")


def _items_2d(items: torch.Tensor, fn: str) -> torch.Tensor:
    L.require_device(items, "items")
    if items.dim() != 2 or items.shape[1] < 1:
        raise ValueError(f"{fn}: items must be [n, dim] with dim >= 1, got {tuple(items.shape)}")
    return items.detach().float().contiguous()


def centroid_bias(centroids: torch.Tensor) -> torch.Tensor:
    """-½‖c‖² per centroid, summed in float64 and rounded once to fp32."""
    return (-0.5 * centroids.double().square().sum(dim=1)).float()


def _assign(items1: torch.Tensor, centroids: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """int32 [n]: argmin ‖x - c‖² as argmax x · c - ½‖c‖² through rs_topk_ip (k = 1)."""
    cb = torch.cat([centroids, bias[:, None]], dim=1)
    return topk_inner_product(items1, cb, 1, with_scores=False)[0][:, 0]


def _group(assign: torch.Tensor, nlist: int):
    """(order int64 [n]: ids grouped by list, ascending inside a list; offsets int64 [nlist+1])."""
    order = torch.sort(assign, stable=True)[1]
    counts = torch.bincount(assign.long(), minlength=nlist)
    offsets = torch.zeros(nlist + 1, dtype=torch.int64, device=assign.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order, offsets


class IVFIndex:
    """centroids fp32 [nlist, dim], centroid_bias fp32 [nlist], list_offsets int64 [nlist + 1],
    item_ids int32 [n], vectors fp32 [n, dim]: a list-major bitwise copy of the item rows, list l
    being rows list_offsets[l] .. list_offsets[l+1] with ids ascending."""

    def __init__(self, centroids, centroid_bias, list_offsets, item_ids, vectors):
        self.centroids = centroids
        self.centroid_bias = centroid_bias
        self.list_offsets = list_offsets
        self.item_ids = item_ids
        self.vectors = vectors

    # ---- construction ----------------------------------------------------------------
    @classmethod
    def from_assignment(cls, items: torch.Tensor, centroids: torch.Tensor,
                        assign: torch.Tensor) -> "IVFIndex":
        """The index whose list assign[i] (in [0, nlist)) holds item i."""
        x = _items_2d(items, "IVFIndex.from_assignment")
        c = centroids.detach().to(x.device, torch.float32).contiguous()
        if c.dim() != 2 or c.shape[1] != x.shape[1] or c.shape[0] < 1:
            raise ValueError("IVFIndex.from_assignment: centroids must be [nlist >= 1, dim]")
        a = torch.as_tensor(assign).to(x.device).reshape(-1)
        if a.numel() != x.shape[0]:
            raise ValueError("IVFIndex.from_assignment: one list per item is needed")
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= c.shape[0]):
            raise ValueError("IVFIndex.from_assignment: a list id outside [0, nlist)")
        order, offsets = _group(a, c.shape[0])
        return cls(c, centroid_bias(c), offsets, order.to(torch.int32), x[order].contiguous())

    @classmethod
    def build(cls, items: torch.Tensor, nlist: int, n_iter: int = 10,
              init: torch.Tensor | None = None) -> "IVFIndex":
        """Lloyd's k-means, n_iter updates. Centroids start from init ([nlist, dim]) or from the
        item rows floor(c · n / nlist); a list that empties keeps its centroid. A final
        assignment against the final centroids makes the stored lists agree with them."""
        x = _items_2d(items, "IVFIndex.build")
        n, dim = x.shape
        if dim > 255:
            raise ValueError("IVFIndex.build: the assignment takes one extra column, so dim <= 255;"
                             " cluster elsewhere and use IVFIndex.from_assignment")
        if not 1 <= nlist <= n:
            raise ValueError(f"IVFIndex.build: need 1 <= nlist <= n, got nlist {nlist}, n {n}")
        dev = x.device
        if init is not None:
            c = init.detach().to(dev, torch.float32).contiguous().clone()
            if tuple(c.shape) != (nlist, dim):
                raise ValueError(f"IVFIndex.build: init must be [{nlist}, {dim}]")
        else:
            rows = (torch.arange(nlist, dtype=torch.int64, device=dev) * n) // nlist
            c = x[rows].contiguous()
        x1 = torch.cat([x, torch.ones(n, 1, device=dev)], dim=1)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        mean = torch.empty(nlist, dim, device=dev)
        for _ in range(n_iter):
            assign = _assign(x1, c, centroid_bias(c))
            order, offsets = _group(assign, nlist)
            L.call("rs_embedding_bag_fwd", L.ptr(x), n, dim, L.ptr(order), L.RS_ID_I64, n,
                   L.ptr(offsets), nlist, 0, None, None, L.RS_BAG_MEAN, None, 1, L.ptr(mean), dim,
                   None, L.ptr(err), L.stream_ptr(dev))
            empty = (offsets[1:] == offsets[:-1])[:, None]
            c = torch.where(empty, c, mean)
        return cls.from_assignment(x, c, _assign(x1, c, centroid_bias(c)))

    # ---- search ----------------------------------------------------------------------
    def probes(self, queries: torch.Tensor, nprobe: int) -> torch.Tensor:
        """int32 [Q, nprobe]: the lists whose centroids score highest by inner product, -1 past
        nlist."""
        return topk_inner_product(queries, self.centroids, nprobe, with_scores=False)[0]

    def search(self, queries, k: int, nprobe: int, exclude=None, exclude_base: int = 0,
               exclude_one=None, with_scores: bool = True, list_splits: int = 0):
        """(idx int32 [Q, k], scores fp32 [Q, k]) like topk_inner_product, over the nprobe lists
        of every query only."""
        return ivf_topk_inner_product(queries, self.probes(queries, nprobe), self.list_offsets,
                                      self.item_ids, self.vectors, k, exclude=exclude,
                                      exclude_base=exclude_base, exclude_one=exclude_one,
                                      with_scores=with_scores, list_splits=list_splits)

    # ---- persistence and shape -------------------------------------------------------
    def state_dict(self) -> dict:
        return {k: getattr(self, k) for k in _KEYS}

    @classmethod
    def from_state_dict(cls, sd: dict) -> "IVFIndex":
        missing = [k for k in _KEYS if k not in sd]
        if missing:
            raise KeyError(f"IVFIndex.from_state_dict: missing {missing}")
        return cls(*(sd[k] for k in _KEYS))

    @property
    def nlist(self) -> int:
        return self.centroids.shape[0]

    @property
    def n_items(self) -> int:
        return self.vectors.shape[0]

    @property
    def dim(self) -> int:
        return self.vectors.shape[1]

    @property
    def list_sizes(self) -> torch.Tensor:
        return self.list_offsets[1:] - self.list_offsets[:-1]


_I8_KEYS = ("codes", "scales", "vectors")


class Int8Index:
    """Two-stage search over the whole catalogue with no index to train: codes
    int8 [n, c_ld] and scales fp32 [n] (quantize_rows_i8 of the item rows) for the int8 MFMA
    candidate scan, vectors fp32 [n, dim] (the item rows themselves) for the exact re-rank."""

    def __init__(self, codes, scales, vectors):
        self.codes = codes
        self.scales = scales
        self.vectors = vectors

    @classmethod
    def from_float(cls, items: torch.Tensor) -> "Int8Index":
        x = _items_2d(items, "Int8Index.from_float")
        codes, scales = quantize_rows_i8(x)
        return cls(codes, scales, x)

    def search(self, queries, k: int, n_candidates: int = 64, exclude=None, exclude_base: int = 0,
               exclude_one=None, with_scores: bool = True):
        """(idx int32 [Q, k], scores fp32 [Q, k]) like topk_inner_product: the n_candidates best
        items of every query by the int8 key (exclusions applied there), re-ranked to k by the
        exact fp32 score. The scores are topk_inner_product's bits; the set is exact whenever the
        true top k lie among the candidates."""
        if not 1 <= k <= n_candidates:
            raise ValueError(f"Int8Index.search: need 1 <= k <= n_candidates, got {k}, "
                             f"{n_candidates}")
        cand, _ = topk_inner_product_i8(queries, self.codes, self.scales, n_candidates,
                                        exclude=exclude, exclude_base=exclude_base,
                                        exclude_one=exclude_one, with_keys=False)
        return rerank_inner_product(queries, self.vectors, cand, k, with_scores=with_scores)

    def state_dict(self) -> dict:
        return {k: getattr(self, k) for k in _I8_KEYS}

    @classmethod
    def from_state_dict(cls, sd: dict) -> "Int8Index":
        missing = [k for k in _I8_KEYS if k not in sd]
        if missing:
            raise KeyError(f"Int8Index.from_state_dict: missing {missing}")
        return cls(*(sd[k] for k in _I8_KEYS))

    @property
    def n_items(self) -> int:
        return self.vectors.shape[0]

    @property
    def dim(self) -> int:
        return self.vectors.shape[1]


def search_index(index, queries, k: int, nprobe: int = 8, n_candidates: int = 64, **kw):
    """index.search for either index type: an IVFIndex takes nprobe, an Int8Index n_candidates
    (at least k) and ignores nprobe."""
    if isinstance(index, Int8Index):
        return index.search(queries, k, max(n_candidates, k), **kw)
    return index.search(queries, k, nprobe, **kw)
