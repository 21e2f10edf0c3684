"""NumPy restatement of the two sparse Adagrad update rules (include/recsys_hip.h RS_OPT_ADAGRAD /
RS_OPT_ROWWISE_ADAGRAD), fp32 with every operation rounded on its own, and float64 evaluations
of the same formulas to judge them against. The gradient of a row is the kernel's segment sum:
oracle.embedding.sort_ids + segment_sum_tiled over the (masked, scaled) gradient rows.

tests/test_adagrad_cpu.py checks the helper itself; tests/test_adagrad_gpu.py compares the
kernels with it."""
from __future__ import annotations

import numpy as np

from oracle import embedding as O

f32 = np.float32


def segment_grads(ids, grad, n_rows, slot_offsets=None, valid=None, row_scale=None, scale_group=1):
    """(uniq_rows, uniq_grad): the deduplicated fp32 gradient in the kernel's tiled order.
    valid (per position, optional): positions flagged 0 are left out. row_scale (optional): the
    gradient row of position p is row_scale[p // scale_group] * grad[p], one rounded fp32
    multiply before the sum. Ids outside their table are dropped."""
    ids = np.asarray(ids).astype(np.int64)
    shape = ids.shape
    flat = ids.reshape(-1)
    g = np.asarray(grad, f32).reshape(flat.size, -1)
    if valid is not None:
        flat = np.where(np.asarray(valid).reshape(-1) != 0, flat, -1)
    if row_scale is not None:
        sc = np.asarray(row_scale, f32)[np.arange(flat.size) // int(scale_group)]
        g = (sc[:, None] * g).astype(f32)
    sr, sp, _ = O.sort_ids(flat.reshape(shape), n_rows, slot_offsets)
    return O.segment_sum_tiled(sr, sp, g, n_rows)


def apply_adagrad(w, acc, uniq_rows, uniq_grad, lr, epsilon):
    """Element-wise: a = acc + g*g; w -= (lr*g) / (sqrt(a) + eps); acc = a. Returns (w, acc)."""
    w, acc = np.array(w, f32), np.array(acc, f32)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, f32)
    a = acc[u] + g * g
    w[u] = w[u] - (f32(lr) * g) / (np.sqrt(a, dtype=f32) + f32(epsilon))
    acc[u] = a
    return w, acc


def rowwise_accumulator(acc, uniq_rows, uniq_grad):
    """fp32 row-wise accumulator after the step: acc[r] + (sum_d g[d]*g[d]) / D, the squares
    added in column order (the kernel's order differs: compare with the derived bound)."""
    acc = np.array(acc, f32)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, f32)
    s = np.zeros(g.shape[0], f32)
    for d in range(g.shape[1]):
        s = s + g[:, d] * g[:, d]
    acc[u] = acc[u] + s / f32(g.shape[1])
    return acc


def rowwise_update(w, new_acc, uniq_rows, uniq_grad, lr, epsilon):
    """Row-wise weights given the rows' NEW accumulator values (new_acc [n_rows]):
    w[d] -= (lr*g[d]) / (sqrt(a) + eps), the same a for every d of the row."""
    w = np.array(w, f32)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, f32)
    den = np.sqrt(np.asarray(new_acc, f32)[u], dtype=f32) + f32(epsilon)
    w[u] = w[u] - (f32(lr) * g) / den[:, None]
    return w


def apply_rowwise_adagrad(w, acc, uniq_rows, uniq_grad, lr, epsilon):
    """Row-wise, all in fp32. Returns (w, acc)."""
    a = rowwise_accumulator(acc, uniq_rows, uniq_grad)
    return rowwise_update(w, a, uniq_rows, uniq_grad, lr, epsilon), a


# ---- float64 evaluations of the same formulas (inputs exactly the fp32 values) ----------------
def apply_adagrad_f64(w, acc, uniq_rows, uniq_grad, lr, epsilon):
    w, acc = np.array(w, np.float64), np.array(acc, np.float64)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, np.float64)
    a = acc[u] + g * g
    w[u] = w[u] - (float(f32(lr)) * g) / (np.sqrt(a) + float(f32(epsilon)))
    acc[u] = a
    return w, acc


def rowwise_accumulator_f64(acc, uniq_rows, uniq_grad):
    acc = np.array(acc, np.float64)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, np.float64)
    acc[u] = acc[u] + (g * g).sum(1) / g.shape[1]
    return acc


def apply_rowwise_adagrad_f64(w, acc, uniq_rows, uniq_grad, lr, epsilon):
    a = rowwise_accumulator_f64(acc, uniq_rows, uniq_grad)
    w = np.array(w, np.float64)
    u = np.asarray(uniq_rows, np.int64)
    g = np.asarray(uniq_grad, np.float64)
    w[u] = w[u] - (float(f32(lr)) * g) / (np.sqrt(a[u]) + float(f32(epsilon)))[:, None]
    return w, a


def rowwise_acc_rtol(dim: int) -> float:
    """Worst-case relative error of the fp32 row-wise accumulator against float64: D rounded
    squares summed in fp32 in ANY order (each partial sum of non-negative terms carries at most
    one rounding per level it passes: <= D roundings in all), the division by D and the add to
    the old accumulator — every term non-negative, so nothing cancels: (D + 3) * 2^-24."""
    return (dim + 3) * 2.0 ** -24
