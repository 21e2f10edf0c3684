"""Item-to-item recall over the EGES hidden vectors (what eges/model.py:82-88 get_hidden exists
for): every item's vector, then the k nearest items by inner product through rs_topk_ip.

item_hidden    [n_items, D]: model.get_hidden over every item id, in chunks, without gradients.
               GES / EGES take the items' category and brand ids; DeepWalk takes ids only.
similar_items  (idx int32 [Q, k], scores fp32 [Q, k]): per query item its k best other items
               (the query item itself is excluded). Inner product: normalise the rows first for
               cosine similarity. index= (retrieval.IVFIndex.build(hidden, nlist)) searches
               the nprobe nearest lists instead of the whole catalogue.
"""
from __future__ import annotations

import torch

from ..functional import topk_inner_product
from .model import DeepWalk


def item_hidden(model, item2cat=None, item2brand=None, batch: int = 65536) -> torch.Tensor:
    table = model.input_embedding if isinstance(model, DeepWalk) else model.id_embedding
    n, dev = table.input_dim, table.weight.device
    side = None
    if not isinstance(model, DeepWalk):
        if item2cat is None or item2brand is None:
            raise ValueError("item_hidden: GES / EGES need item2cat and item2brand")
        side = [torch.as_tensor(t).to(dev, torch.int32).reshape(-1, 1) for t in (item2cat, item2brand)]
        if any(t.shape[0] != n for t in side):
            raise ValueError(f"item_hidden: item2cat and item2brand must hold {n} ids")
    out = torch.empty(n, table.output_dim, device=dev)
    with torch.no_grad():
        for b0 in range(0, n, max(int(batch), 1)):
            b1 = min(n, b0 + max(int(batch), 1))
            ids = torch.arange(b0, b1, dtype=torch.int32, device=dev).reshape(-1, 1)
            inp = ids if side is None else (ids, side[0][b0:b1], side[1][b0:b1])
            out[b0:b1] = model.get_hidden(inp).reshape(b1 - b0, -1)
    return out


def similar_items(hidden: torch.Tensor, query_items: torch.Tensor, k: int, index=None,
                  nprobe: int = 8, n_candidates: int = 64):
    """index: a retrieval.IVFIndex over `hidden`: the search covers the nprobe lists nearest to
    each query only (approximate; nprobe = index.nlist is exact). A retrieval.Int8Index: an int8
    scan of every item keeps n_candidates per query, re-ranked exactly to k (nprobe is ignored).
    None: exhaustive."""
    query_items = torch.as_tensor(query_items).to(hidden.device)
    if index is not None:
        from ..retrieval import search_index

        return search_index(index, hidden[query_items.long()], k, nprobe, n_candidates,
                            exclude_one=query_items)
    return topk_inner_product(hidden[query_items.long()], hidden, k, exclude_one=query_items)
