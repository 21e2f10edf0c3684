"""Training counterpart of eges/train.py (loop :14-24: sigmoid CE on the 1+num_ns skip-gram
logits, reduce_mean, Keras Adam on every table — IndexedSlices → SparseAdam(mode='keras')).

Data: the reference's pair pipeline (eges/data_loader.py:28-62: weighted walk → skipgrams →
log-uniform negatives) runs on the device (eges/sampler.py, EGESPairSampler) over a synthetic
weighted item graph (the JD session data is not available offline); `synthetic_batch` keeps
the i.i.d. batches of the same shapes for the model benchmarks.
Hyper-parameters from eges/train.py:45-54,75-92 (emb 160, num_ns 5, batch 1024, seed 4)."""
from __future__ import annotations

import argparse
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..functional import item_softmax_loss
from ..optim import SparseAdam
from ..steps import StaticKerasAdam
from .model import EGES, GES, DeepWalk
from .sampler import EGESPairSampler


def log_uniform(rng, n, range_max):
    """tf.random.log_uniform_candidate_sampler's distribution P(k) = log((k+2)/(k+1)) /
    log(range_max+1), by inverse CDF (without its uniqueness rejection)."""
    u = rng.random(n)
    return np.minimum((np.exp(u * np.log(range_max + 1.0)) - 1.0).astype(np.int64), range_max - 1)


def synthetic_item_graph(rng, n_items, n_edges):
    """Symmetric weighted co-occurrence CSR over items 1..n_items-1 (0 = OOV, no edges):
    popularity-skewed endpoints, integer session-count weights."""
    pop = rng.zipf(1.3, 2 * n_edges) % (n_items - 1) + 1
    src, dst = pop[:n_edges], pop[n_edges:]
    keep = src != dst
    s = np.concatenate([src[keep], dst[keep]])
    d = np.concatenate([dst[keep], src[keep]])
    w = rng.integers(1, 10, s.size).astype(np.float32)
    order = np.argsort(s, kind="stable")
    s, d, w = s[order], d[order], w[order]
    indptr = np.zeros(n_items + 1, np.int64)
    np.add.at(indptr, s + 1, 1)
    return np.cumsum(indptr), d.astype(np.int32), w


def synthetic_batch(rng, batch, n_items, n_cat, n_brand, num_ns=5):
    target = rng.integers(1, n_items, (batch, 1))
    pos = rng.integers(1, n_items, (batch, 1))
    neg = log_uniform(rng, batch * num_ns, n_items).reshape(batch, num_ns)
    context = np.concatenate([pos, neg], 1)
    item2cat = (np.arange(n_items) * 2654435761) % n_cat
    item2brand = (np.arange(n_items) * 40503) % n_brand
    label = np.zeros((batch, 1 + num_ns), np.float32)
    label[:, 0] = 1
    return (target.astype(np.int32), item2cat[target].astype(np.int32),
            item2brand[target].astype(np.int32), context.astype(np.int32), label)


class EGESStep:
    _static = None  # steps.StaticKerasAdam, built by the first static_step

    def __init__(self, model, lr=1e-3, loss="sigmoid", temperature=1.0, log_q=None):
        """loss: "sigmoid" (the reference's sigmoid CE over 1 + num_ns sampled logits) or
        "inbatch" (softmax CE of every query against the batch's positives, by
        functional.item_softmax_loss; the sampled negatives and the labels are not used).
        log_q: optional float tensor [n_items], the log sampling probability of every item,
        subtracted from the logits of the columns that hold it (the logQ correction)."""
        if loss not in ("sigmoid", "inbatch"):
            raise ValueError(f"EGESStep: loss must be sigmoid or inbatch, got {loss!r}")
        self.model = model
        self.opt = SparseAdam(model.tables(), lr=lr, mode="keras")
        self.loss = loss
        self.temperature = float(temperature)
        self.log_q = log_q

    def _loss(self, inputs, labels):
        if self.loss == "sigmoid":
            logits = self.model(inputs)
            return F.binary_cross_entropy_with_logits(logits, labels)  # sigmoid CE, reduce_mean
        *query, match = inputs
        hidden = self.model.get_hidden(query[0] if len(query) == 1 else tuple(query))  # [B, 1, D]
        pos = match[:, :1]
        rows = self.model.output_embedding(pos)  # [B, 1, D]; its gradient: the sparse apply
        ids = pos.reshape(-1)
        B = hidden.shape[0]
        log_q = None if self.log_q is None else self.log_q.index_select(0, ids.long())
        return item_softmax_loss(hidden.reshape(B, -1), rows.reshape(B, -1), None,
                                 temperature=self.temperature, log_q=log_q, item_ids=ids,
                                 reduction="mean")

    def __call__(self, inputs, labels):
        loss = self._loss(inputs, labels)
        loss.backward()
        self.opt.step()
        return loss.detach()

    # -- graph-capturable step --------------------------------------------------------------
    def static_step(self, inputs, labels):
        """The same step as a Keras-Adam step that can sit in a HIP graph
        (steps.StaticKerasAdam over the tables). Its Adam state is its own: do not interleave
        with __call__."""
        if self._static is None:
            self._static = StaticKerasAdam([], self.opt.tables, self.opt, self.opt.lr)
            self.opt_graph = self._static.opt
        loss = self._loss(inputs, labels)
        loss.backward()
        self._static.step()
        return loss.detach()

    def capture(self, inputs, labels):
        """Record one static_step on (inputs, labels) — static device tensors the caller
        refills before each replay — into a HIP graph; returns replay() -> loss tensor. Run at
        least one eager static_step first."""
        return self._static.capture(lambda: self.static_step(inputs, labels))


def build(model_type, n_items, n_cat, n_brand, embedding_size=160, device="cuda", generator=None):
    if model_type == "BGE":
        return DeepWalk(n_items, embedding_size, device=device, generator=generator)
    if model_type == "GES":
        return GES(n_items, n_cat, n_brand, embedding_size, device=device, generator=generator)
    if model_type == "EGES":
        return EGES(n_items, n_cat, n_brand, embedding_size, 3, device=device, generator=generator)
    raise ValueError(model_type)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_type", default="BGE", choices=["BGE", "GES", "EGES"])
    ap.add_argument("--train_batch_size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--n_items", type=int, default=63001)
    ap.add_argument("--loss", default="sigmoid", choices=["sigmoid", "inbatch"])
    ap.add_argument("--temperature", type=float, default=1.0)
    args = ap.parse_args(argv)
    rng = np.random.default_rng(args.seed)
    n_cat, n_brand = 801, 3000
    indptr, indices, weights = synthetic_item_graph(rng, args.n_items, 16 * args.n_items)
    items = np.arange(args.n_items)
    sampler = EGESPairSampler(indptr, indices, weights, args.n_items,
                              item2cat=(items * 2654435761) % n_cat,
                              item2brand=(items * 40503) % n_brand, seed=args.seed)
    model = build(args.model_type, args.n_items, n_cat, n_brand)
    step = EGESStep(model, loss=args.loss, temperature=args.temperature)
    t0 = time.perf_counter()
    for s in range(args.steps):
        *inp, lab = sampler.next_batch(args.train_batch_size, args.model_type)
        loss = step(tuple(inp), lab)
        if s % 50 == 0:
            print(f"step {s} loss {float(loss):.4f}")
    torch.cuda.synchronize()
    print(f"{args.steps * args.train_batch_size / (time.perf_counter() - t0):.0f} examples/s")


if __name__ == "__main__":
    main()
