"""What the model trainers' steps share: the dense-parameter list, the bucketed gradient
all-reduce, HIP-graph capture, and the sync-free Keras-Adam step that can sit in a graph
(TrainStep / DIENStep / EGESStep / PinSageStep.static_step)."""
from __future__ import annotations

import torch

from ._lib import Workspace
from .nn import invalidate_compose_cache
from .optim import GraphKerasAdam, densify_grad


def dense_parameters(model):
    """The model's autograd parameters without the tables' zero-size grad handles."""
    return [p for n, p in model.named_parameters() if not n.endswith("grad_handle")]


def allreduce_mean_(comm, tensors):
    """One bucketed all-reduce of `tensors`, averaged over the ranks, in place (the
    MirroredStrategy gradient sync). A single tensor is its own bucket."""
    flat = tensors[0] if len(tensors) == 1 else torch._utils._flatten_dense_tensors(tensors)
    comm.all_reduce_(flat)
    flat.mul_(1.0 / comm.world)
    if flat is not tensors[0]:
        torch._foreach_copy_(tensors, list(torch._utils._unflatten_dense_tensors(flat, tensors)))


def capture_graph(body):
    """Record body() into a HIP graph; returns replay() -> what body() returned. A replay moves
    the parameters in place without bumping their version counters, so the composed MLP chains
    (nn.invalidate_compose_cache) are dropped before the capture (the graph must record the
    compositions it reads), after it, and after every replay (eager steps recompose). That
    clears a dict which stays empty unless composed chains are in use, so every model's
    capture goes through here."""
    g = torch.cuda.CUDAGraph()
    invalidate_compose_cache()
    with torch.cuda.graph(g):
        out = body()
    invalidate_compose_cache()

    def replay():
        g.replay()
        invalidate_compose_cache()
        return out
    return replay


class StaticKerasAdam:
    """A trainer's Keras-Adam step with no host-side per-step scalars, so it can sit in a HIP
    graph: each table's IndexedSlices gradient is densified (densify_grad: the sort + tiled
    segmented sum of the sparse apply, no sync) straight into the flat gradient buffer, and
    Keras Adam runs over every variable with lr_t from device memory (GraphKerasAdam; a variable
    without a gradient is skipped as Keras skips it). Keras' sparse Adam decays m / v and moves
    every row each step anyway (_resource_apply_sparse [3p TF 2.2]), so this dense step is the
    same update as KerasAdam + SparseAdam(mode="keras"). Its Adam state is its own (sparse_opt's
    is released): do not interleave with the trainer's __call__.

    The flat buffer holds `dense` without table weights and empty tensors, in order, then the
    tables in order. comm (a sharded.Comm whose collectives are live): the flat gradient buffer
    is all-reduced and averaged over the ranks before the Adam launch — one collective, RCCL
    under nccl, so the sharded step captures too. The layout is fixed, so every parameter must
    then have a gradient on every rank."""

    def __init__(self, dense, tables, sparse_opt, lr, comm=None):
        self.tables = list(tables)
        tw = {id(t.weight) for t in self.tables}
        self.dense = [p for p in dense if id(p) not in tw and p.numel() > 0]
        self.opt = GraphKerasAdam(self.dense + [t.weight for t in self.tables], lr=lr)
        self.ws = Workspace()
        self.comm = comm
        sparse_opt.release_state()  # the graph path's Adam state is self.opt's

    def zero_grad(self):
        for p in self.dense:
            p.grad = None

    def step(self):
        """After backward(): densify, (all-reduce,) Keras Adam. Outside a capture it also rolls
        the lr_t window and counts the step; a capture records the step and replay() counts."""
        opt = self.opt
        grads = [p.grad for p in self.dense]  # None: Keras skips the variable
        nd = len(self.dense)
        for i, t in enumerate(self.tables):
            got = t.take_grad(with_valid=True, segments=True)
            grads.append(densify_grad(t, got[0], got[1], self.ws, valid=got[2],
                                      out=opt.grad_view(nd + i)) if got is not None else None)
        if self.comm is not None and self.comm.collective:
            if any(g is None for g in grads):
                raise ValueError("sharded static_step: a parameter has no gradient on this rank; "
                                 "the all-reduce needs the same flat layout on every rank")
            opt.collect(grads)
            allreduce_mean_(self.comm, [opt.grad_flat])
            grads = [opt.grad_view(i) for i in range(len(grads))]
        if not torch.cuda.is_current_stream_capturing():
            opt.prepare()
            opt.iterations += 1
        opt.apply(grads)

    def capture(self, body, after_replay=None):
        """Record body() — a static step on static device tensors the caller refills before each
        replay — into a HIP graph; returns replay() -> what body() returned. Run at least one
        eager step first (it builds the library handles and workspaces the graph reads).
        after_replay: host-side bookkeeping to run after each replay."""
        opt = self.opt
        opt.prepare()
        torch.cuda.synchronize()
        run = capture_graph(body)

        def replay():
            opt.prepare()
            out = run()
            opt.iterations += 1
            if after_replay is not None:
                after_replay()
            return out
        return replay
