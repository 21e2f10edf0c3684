"""Device metrics: Keras' thresholded AUC, and the exact per-group AUC.

AUC(num_thresholds=200, curve='ROC', summation_method='interpolation') mirrors
keras.metrics.AUC [3p TF 2.2] as the reference uses it (ctr/train.py:86 default 200,
dien/train.py:43-44 20000, esmm/train.py:164 10000): update_state(y_true, y_pred) on device
(rs_auc_update: one bucket histogram pass), result() from the exact int64 counts, reset_states().
Curves: ROC (interpolation / minoring / majoring) and PR (interpolation, Davis & Goadrich).

GroupAUC / ExactAUC: the exact Mann-Whitney AUC per group (GAUC, per user) or pooled, from
rs_group_auc's integer pair counts; the ratios and their weighted mean are formed on the host."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L

EPSILON = 1e-7  # keras backend epsilon


def keras_thresholds(num_thresholds: int) -> np.ndarray:
    """metrics.AUC.__init__: [0 - eps] + [(i + 1) / (T - 1) for i in range(T - 2)] + [1 + eps],
    stored as float32."""
    t = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
    return np.array([0.0 - EPSILON] + t + [1.0 + EPSILON], dtype=np.float32)


def auc_from_counts(neg: np.ndarray, pos: np.ndarray, curve: str = "ROC",
                    summation_method: str = "interpolation") -> float:
    """AUC.result() from per-bucket counts (bucket b = #thresholds < prediction)."""
    T = neg.size - 1
    # TP_i = Σ_{b > i} pos[b] (prediction above threshold i)
    tp = np.cumsum(pos[::-1])[::-1][1:].astype(np.float64)
    fp = np.cumsum(neg[::-1])[::-1][1:].astype(np.float64)
    fn = pos.sum() - tp
    tn = neg.sum() - fp

    def div(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)

    if curve == "PR" and summation_method == "interpolation":
        dtp = tp[: T - 1] - tp[1:]
        p = tp + fp
        dp = p[: T - 1] - p[1:]
        prec_slope = div(dtp, np.maximum(dp, 0))
        intercept = tp[1:] - prec_slope * p[1:]
        safe_p_ratio = np.where((p[: T - 1] > 0) & (p[1:] > 0), div(p[: T - 1], np.maximum(p[1:], 0)),
                                np.ones_like(p[1:]))
        pr_auc_increment = div(prec_slope * (dtp + intercept * np.log(safe_p_ratio)),
                               np.maximum(tp[1:] + fn[1:], 0))
        return float(np.sum(pr_auc_increment))
    recall = div(tp, tp + fn)
    if curve == "ROC":
        x, y = div(fp, fp + tn), recall
    else:  # PR with riemann sums
        x, y = recall, div(tp, tp + fp)
    if summation_method == "interpolation":
        heights = (y[: T - 1] + y[1:]) / 2.0
    elif summation_method == "minoring":
        heights = np.minimum(y[: T - 1], y[1:])
    else:
        heights = np.maximum(y[: T - 1], y[1:])
    return float(np.sum((x[: T - 1] - x[1:]) * heights))


class AUC:
    def __init__(self, num_thresholds: int = 200, curve: str = "ROC",
                 summation_method: str = "interpolation", name: str | None = None, device="cuda"):
        if num_thresholds <= 1:
            raise ValueError("num_thresholds must be > 1")
        self.num_thresholds = num_thresholds
        self.curve = curve.upper()
        self.summation_method = summation_method.lower()
        self.name = name
        self.device = torch.device(device)
        self.thresholds = torch.from_numpy(keras_thresholds(num_thresholds)).to(self.device)
        self.counts = torch.zeros(2, num_thresholds + 1, dtype=torch.int64, device=self.device)
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)

    def update_state(self, y_true, y_pred, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not used by the reference")
        p = torch.as_tensor(y_pred, device=self.device).reshape(-1).float().contiguous()
        y = torch.as_tensor(y_true, device=self.device).reshape(-1).float().contiguous()
        if p.numel() != y.numel():
            raise ValueError("y_true and y_pred sizes differ")
        L.call("rs_auc_update", L.ptr(p), L.ptr(y), p.numel(), L.ptr(self.thresholds),
               self.num_thresholds, L.ptr(self.counts), L.ptr(self.err_flag),
               L.stream_ptr(self.device))

    def result(self) -> float:
        c = self.counts.cpu().numpy()
        if int(self.err_flag.item()):
            raise ValueError("predictions must be in [0, 1] (keras.metrics.AUC asserts this)")
        return auc_from_counts(c[0], c[1], self.curve, self.summation_method)

    def reset_states(self):
        self.counts.zero_()
        self.err_flag.zero_()


def gauc_from_counts(n: np.ndarray, pos: np.ndarray, w2: np.ndarray, weight: str = "impressions") -> float:
    """Σ_u w_u·AUC_u / Σ_u w_u over the groups with 0 < pos < n, AUC_u = w2 / (2·pos·(n − pos))
    and w_u = n ("impressions"), pos ("positives") or 1 ("uniform"), in float64 from the exact
    integers; 0.0 when no group qualifies (auc_from_counts' empty-ratio convention). The value is
    the exact rational rounded once: every term enters math.fsum as its correctly rounded
    quotient plus that quotient's remainder, the sum is kept as two floats, and the only
    rounding that counts is the last division."""
    if weight not in GroupAUC.WEIGHTS:
        raise ValueError(f"weight must be one of {GroupAUC.WEIGHTS}, got {weight!r}")
    parts, den = [], 0
    for nu, pu, wu in zip(n.tolist(), pos.tolist(), w2.tolist()):
        if 0 < pu < nu:
            w = nu if weight == "impressions" else pu if weight == "positives" else 1
            t, d = w * wu, 2 * pu * (nu - pu)
            q = t / d  # int / int: correctly rounded
            qn, qd = q.as_integer_ratio()
            parts += [q, (t * qd - qn * d) / (d * qd)]
            den += w
    if not den:
        return 0.0
    hi = math.fsum(parts)
    lo = math.fsum(parts + [-hi])
    return float((Fraction(hi) + Fraction(lo)) / den)


class GroupAUC:
    """GAUC, the per-user AUC DIN / DIEN are judged by: every group's exact Mann-Whitney AUC
    (ties ½; rs_group_auc's integer counts) averaged with weight n, pos or 1; groups whose examples
    are all of one label are left out. update_state(y_true, y_pred, group) appends to device
    buffers (capacity doubles, nothing moves to the host); a group's examples may come in any
    number of calls and any order. groups() -> (keys, n, pos, w2) as NumPy; result() -> float."""
    WEIGHTS = ("impressions", "positives", "uniform")

    def __init__(self, weight: str = "impressions", name: str | None = None, device="cuda"):
        if weight not in self.WEIGHTS:
            raise ValueError(f"weight must be one of {self.WEIGHTS}, got {weight!r}")
        self.weight = weight
        self.name = name
        self.device = torch.device(device)
        self.reset_states()

    def reset_states(self):
        self.size = 0
        self._pred = torch.empty(0, dtype=torch.float32, device=self.device)
        self._label = torch.empty(0, dtype=torch.float32, device=self.device)
        self._group = torch.empty(0, dtype=torch.int64, device=self.device)

    def _append(self, cols):
        k = cols[0].numel()
        if self.size + k > self._pred.numel():
            cap = max(2 * self._pred.numel(), self.size + k, 1024)
            for name in ("_pred", "_label", "_group"):
                old = getattr(self, name)
                new = torch.empty(cap, dtype=old.dtype, device=self.device)
                new[:self.size] = old[:self.size]
                setattr(self, name, new)
        for buf, c in zip((self._pred, self._label, self._group), cols):
            buf[self.size:self.size + k] = c
        self.size += k

    def update_state(self, y_true, y_pred, group):
        p = torch.as_tensor(y_pred, device=self.device).detach().reshape(-1).float()
        y = torch.as_tensor(y_true, device=self.device).detach().reshape(-1).float()
        g = torch.as_tensor(group, device=self.device).reshape(-1).to(torch.int64)
        if not p.numel() == y.numel() == g.numel():
            raise ValueError("y_true, y_pred and group sizes differ")
        self._append((p, y, g))

    def _counts(self):
        from .functional import group_auc_counts

        s = self.size
        return group_auc_counts(self._pred[:s], self._label[:s], self._group[:s])

    def groups(self):
        return tuple(t.cpu().numpy() for t in self._counts())

    def result(self) -> float:
        _, n, pos, w2 = self.groups()
        return gauc_from_counts(n, pos, w2, self.weight)


class ExactAUC(GroupAUC):
    """The exact pooled AUC (Mann-Whitney, ties ½; no threshold grid): GroupAUC's one-group case,
    update_state(y_true, y_pred). 0.0 while either label is absent."""

    def __init__(self, name: str | None = None, device="cuda"):
        super().__init__("uniform", name, device)

    def update_state(self, y_true, y_pred):
        p = torch.as_tensor(y_pred, device=self.device).reshape(-1)
        super().update_state(y_true, p, torch.zeros(p.numel(), dtype=torch.int64, device=self.device))

    def _counts(self):
        from .functional import group_auc_counts

        s = self.size
        return group_auc_counts(self._pred[:s], self._label[:s], None)
