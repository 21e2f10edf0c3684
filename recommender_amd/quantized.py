"""Row-wise int8 embedding tables for serving (RS_Q8, include/recsys_hip.h a-1c).

A trained fp32 table [n_rows, dim] is held as uint8 [n_rows, q_ld]: per row a float32 scale, a
float32 bias and one 8-bit code per column (144 bytes instead of 512 at dim = 128), so a model can
be scored, or its rows pooled, beside a training job without a second fp32 copy of its slab.

`QuantizedEmbedding` / `QuantizedEmbeddingBag` are the forward-only counterparts of `Embedding` /
`SlabEmbedding` and `EmbeddingBag`; `from_float` builds one from a trained table and
`quantize_embeddings(model)` swaps a model's tables in place. DLRM reads a quantised table through
its scoring kernel (`DLRM.score`, `functional.dlrm_score`: rs_dlrm_score_q8), the other models
through the lookup. Nothing here joins autograd.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .embedding import Embedding, EmbeddingBag, check_err_flag
from .functional import (dequantize_rows, embedding_bag_q8, embedding_lookup_q8, q8_row_bytes,
                         quantize_rows)


class QuantizedEmbedding(nn.Module):
    """Embedding's lookup surface over an RS_Q8 table. Buffers: qweight (uint8 [n_rows, q_ld]),
    slot_offsets (None for one shared table), err_flag. Built empty (every row dequantises to
    zeros) for load_state_dict, or from a trained table by from_float."""

    fused_optimizer = None  # never trained: the hooks that ask find no optimizer

    def __init__(self, input_dim: int, output_dim: int, mask_zero: bool = False, device=None,
                 slot_offsets: torch.Tensor | None = None, q_ld: int | None = None,
                 qweight: torch.Tensor | None = None):
        super().__init__()
        device = torch.device(device) if device is not None else torch.device("cuda")
        self.input_dim = int(input_dim)
        self.output_dim = int(output_dim)
        self.mask_zero = bool(mask_zero)
        self.q_ld = q8_row_bytes(self.output_dim) if q_ld is None else int(q_ld)
        if self.q_ld < 8 + self.output_dim or self.q_ld % 4:
            raise ValueError("q_ld must be a multiple of 4 and >= 8 + output_dim")
        if qweight is None:
            qweight = torch.zeros(self.input_dim, self.q_ld, dtype=torch.uint8, device=device)
        elif tuple(qweight.shape) != (self.input_dim, self.q_ld) or qweight.dtype != torch.uint8:
            raise ValueError(f"qweight must be uint8 [{self.input_dim}, {self.q_ld}]")
        self.register_buffer("qweight", qweight.to(device).contiguous())
        self.register_buffer("slot_offsets",
                             None if slot_offsets is None else slot_offsets.to(device, torch.int64))
        self.register_buffer("err_flag", torch.zeros(1, dtype=torch.int32, device=device))

    @classmethod
    def from_float(cls, emb: Embedding, q_ld: int | None = None, **kw):
        """The quantised copy of a trained Embedding / SlabEmbedding / EmbeddingBag: ordered after
        a pending sparse update of it, quantised straight from emb.weight. Raises ValueError when
        a row holds a NaN or an infinity, or its range overflows (RS_ERRBIT_NONFINITE)."""
        if not isinstance(emb, Embedding):
            raise TypeError(f"from_float: an Embedding, SlabEmbedding or EmbeddingBag, "
                            f"not {type(emb).__name__}")
        emb.wait_update()
        err = torch.zeros(1, dtype=torch.int32, device=emb.weight.device)
        q = quantize_rows(emb.weight, q_ld, err_flag=err)
        if int(err.item()) & L.RS_ERRBIT_NONFINITE:
            raise ValueError("from_float: the table holds a row that cannot be quantised (a NaN, "
                             "an infinity, or a range that overflows fp32)")
        return cls(emb.input_dim, emb.output_dim, mask_zero=emb.mask_zero,
                   device=emb.weight.device, slot_offsets=emb.slot_offsets, q_ld=q.shape[1],
                   qweight=q, **kw)

    @property
    def n_slots(self) -> int:
        return 1 if self.slot_offsets is None else self.slot_offsets.numel() - 1

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        return embedding_lookup_q8(self, ids)

    def compute_mask(self, ids: torch.Tensor):
        return ids != 0 if self.mask_zero else None

    def dequantize(self) -> torch.Tensor:
        """The fp32 [n_rows, dim] table the codes stand for (rs_dequantize_rows_q8)."""
        return dequantize_rows(self.qweight, self.output_dim)

    def check_errors(self) -> int:
        return check_err_flag(self.err_flag)

    def oob_detected(self) -> bool:
        return bool(self.check_errors() & L.RS_ERRBIT_OOB)

    def reset_oob(self):
        self.err_flag.zero_()

    def extra_repr(self):
        return (f"{self.input_dim}, {self.output_dim}, mask_zero={self.mask_zero}, "
                f"slots={self.n_slots}, q_ld={self.q_ld}")


class QuantizedEmbeddingBag(QuantizedEmbedding):
    """EmbeddingBag's forward over an RS_Q8 table: the result equals, bit for bit, EmbeddingBag
    over dequantize()."""

    def __init__(self, input_dim: int, output_dim: int, mode: str = "mean", **kw):
        super().__init__(input_dim, output_dim, **kw)
        if mode not in ("sum", "mean"):
            raise ValueError("mode must be 'sum' or 'mean'")
        self.mode = mode

    @classmethod
    def from_float(cls, emb: Embedding, q_ld: int | None = None, mode: str | None = None):
        return super().from_float(emb, q_ld, mode=mode or getattr(emb, "mode", "mean"))

    def forward(self, ids: torch.Tensor, offsets=None, valid=None, per_sample_weights=None):
        return embedding_bag_q8(self, ids, offsets, mode=self.mode, valid=valid,
                                per_sample_weights=per_sample_weights)

    def extra_repr(self):
        return f"{super().extra_repr()}, mode={self.mode}"


def from_float(emb: Embedding, q_ld: int | None = None):
    """QuantizedEmbeddingBag of an EmbeddingBag, QuantizedEmbedding of any other table."""
    cls = QuantizedEmbeddingBag if isinstance(emb, EmbeddingBag) else QuantizedEmbedding
    return cls.from_float(emb, q_ld)


def _forward_only_owners():
    """The modules known to read their tables through the tables' forward alone."""
    from .ctr.model import DeepFM
    from .esmm.tables import FeatureTables

    return (DeepFM, FeatureTables)


def _dlrm_unservable(model) -> str | None:
    """Which limit of rs_dlrm_score_q8 a DLRM is outside of (None: it can be served)."""
    from .nn import vec_chain_ready

    D, S = model.embedding_size, model.num_cat_fea
    if not model.compact:
        return "compact=False (the kernel forms the compact interaction row)"
    if D not in (64, 128):
        return f"embedding size {D} is not 64 or 128"
    if not 1 <= S <= 31:
        return f"{S} slots; the kernel takes 1 to 31"
    layers = list(model.top_mlp.mlp)
    if not (vec_chain_ready(layers, model.compact_rows.numel())
            and all(l.act_code == 0 for l in layers[:-1]) and layers[-1].act_code in (0, 1, 2)):
        return "the top MLP is not three layers with biases ending in one unit"
    return None


def quantize_embeddings(model: nn.Module, forward_only: tuple = ()) -> nn.Module:
    """Swap, in place, every Embedding / SlabEmbedding / EmbeddingBag of `model` for its
    quantised copy and return the model, for use under torch.no_grad(). Only tables whose rows
    are read through their forward alone can be swapped: those of DeepFM (embedding_layer) and of
    FeatureTables (the slab of ESMM / MMOE / BASE), and of the module classes the caller vouches
    for in forward_only; and DLRM's, whose forward then runs DLRM.score (rs_dlrm_score_q8: lookup,
    interaction and top MLP in one kernel over the quantised rows) when that kernel can serve it:
    compact=True, embedding size 64 or 128, at most 31 slots, a three-layer top MLP with biases
    ending in one unit. Everything is checked before anything is swapped. TypeError for any other
    DLRM (its other kernels read weight as fp32), a row-sharded slab, a table with a fused
    optimizer still attached, and a table held by a module of any other class."""
    from .ctr.model import DLRM
    from .sharded import ShardedSlabEmbedding

    owners = _forward_only_owners() + (DLRM,) + tuple(forward_only)
    swaps = []
    for owner in model.modules():
        if isinstance(owner, DLRM):
            why = _dlrm_unservable(owner)
            if why:
                raise TypeError(f"quantize_embeddings: DLRM's scoring kernel (rs_dlrm_score_q8) "
                                f"cannot serve this model: {why}")
        for name, child in owner.named_children():
            if isinstance(child, ShardedSlabEmbedding):
                raise TypeError(f"quantize_embeddings: {name} is a row-sharded slab; its rows are "
                                "exchanged between ranks as fp32")
            if not isinstance(child, Embedding):
                continue
            if child.fused_optimizer is not None:
                raise TypeError(f"quantize_embeddings: {name} still has a fused optimizer "
                                "attached; a quantised table is not trained")
            if not isinstance(owner, owners):
                raise TypeError(f"quantize_embeddings: {type(owner).__name__} is not known to read "
                                f"{name} through its forward alone (pass forward_only=)")
            swaps.append((owner, name, child))
    if isinstance(model, Embedding):
        raise TypeError("quantize_embeddings: a bare table has no owner to swap it in; "
                        "use from_float")
    for owner, name, child in swaps:
        setattr(owner, name, from_float(child))
    return model
