"""Drop-in counterpart of the reference's metrics.py: the training metrics `er_score`, `f1_score`, `cos_sim`
(metrics.py:217-299), the scoring helpers `Challenge_Metric`, `extract_middle`, `output_to_metric`, `get_er` (:95-214) and
`evaluate` / `eval_callback` (:14-87).

On GPU tensors the training metrics are ONE HIP launch (iris_event_metrics, challenge_amd/csrc/k_metrics.h): no host sync,
capturable into the training step's hipGraph.  On CPU tensors they take a vectorised torch path with the same arithmetic
(`er` bitwise equal).  `MetricSet` serves a compiled metric list with one launch per batch and keeps the epoch accumulators
`fit` reads once per epoch.

Reference semantics kept on purpose:
  * er_score(smoothing=True) pools the predictions with AveragePooling1D(31, padding='same') - stride 31, Keras' default -
    and compares the pooled run middles, as indices, with full-rate label frames.
  * f1_score() wraps ONE stateful F1Score: its counts are never reset, so the value logged per batch is the F1 of everything
    counted since the callable was made, training and validation batches alike; Keras then averages those values over the
    epoch's batches.
The scoring helpers run on the host, once per file."""
from __future__ import annotations

import json
import math
import os
from glob import glob
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as N
from .trainer import cos_sim  # noqa: F401  (metrics.py:277-288; the CPU path of the `cos_sim` metric)

SMOOTHING_POOL = int(0.5 * 16000) // 256   # metrics.py:222: 31 frames


def _first(x):
    return x[0] if isinstance(x, tuple) else x


def _device(device) -> torch.device:
    """The key of a per-device state: a bare 'cuda' is the current device."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def _pool_same_strided(y: torch.Tensor, k: int) -> torch.Tensor:
    """Keras AveragePooling1D(k, padding='same') (stride = k) on [B, T, K]: ceil(T / k) windows, the padding split floor /
    ceil before / after, each window the mean of its in-range frames summed in frame order (as the kernel sums)."""
    b, t, c = y.shape
    n = -(-t // k)
    pad0 = (n * k - t) // 2
    yp = y.new_zeros(b, n * k, c)
    yp[:, pad0:pad0 + t] = y
    yr = yp.view(b, n, k, c)
    acc = torch.zeros_like(yr[:, :, 0])
    for j in range(k):   # sequential fp32 sum (the zero padding adds exactly nothing)
        acc = acc + yr[:, :, j]
    lo = (torch.arange(n) * k - pad0).clamp(min=0)
    hi = (torch.arange(n) * k - pad0 + k).clamp(max=t)
    return acc / (hi - lo).to(y.dtype)[None, :, None]


def _runs(x: torch.Tensor):
    """x bool [B, K, T] -> (starts, ends) as index rows (b, k, t) in (clip, class, time) order."""
    xi = x.to(torch.int8)
    prev = torch.nn.functional.pad(xi, (1, 0))[..., :-1]
    nxt = torch.nn.functional.pad(xi, (0, 1))[..., 1:]
    return (x & (prev == 0)).nonzero(), (x & (nxt == 0)).nonzero()


def er_host(y_true: torch.Tensor, y_pred: torch.Tensor, threshold: float = 0.5, pool: int = 0) -> torch.Tensor:
    """The reference's er_score on CPU tensors [B, T, K] / [B, T', K] -> [B] fp32 (see k_metrics.h for the restatement)."""
    y_true = y_true.to(torch.float32)
    y_pred = y_pred.to(torch.float32)
    if pool > 1:
        y_pred = _pool_same_strided(y_pred, pool)
    thr = torch.tensor(threshold, dtype=torch.float32)
    yt = (y_true >= thr).transpose(1, 2)
    yp = (y_pred >= thr).transpose(1, 2)
    b, k, t = yt.shape
    ts, te = _runs(yt)
    ps, pe = _runs(yp)
    mid = (ps[:, 2] + pe[:, 2]) // 2
    keep = mid < t
    hit = torch.zeros(b, k, t, dtype=torch.int32)
    hit[ps[keep, 0], ps[keep, 1], mid[keep]] = 1
    cum = torch.nn.functional.pad(hit.cumsum(-1), (1, 0))   # cum[..., i] = middles in [0, i)
    correct = (cum[ts[:, 0], ts[:, 1], te[:, 2] + 1] - cum[ts[:, 0], ts[:, 1], ts[:, 2]]) > 0
    n_true = torch.bincount(ts[:, 0], minlength=b).to(torch.float32)
    n_pred = torch.bincount(ps[:, 0], minlength=b).to(torch.float32)
    n_corr = torch.bincount(ts[:, 0], weights=correct.to(torch.float64), minlength=b).to(torch.float32)
    return (n_true + n_pred - 2 * n_corr) / torch.clamp(n_true, min=1)


def f1_counts_host(y_true: torch.Tensor, y_pred: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    p = (y_pred > threshold).to(torch.float64)
    y = y_true.to(torch.float64)
    return torch.stack([(p * y).sum(), (p * (1 - y)).sum(), ((1 - p) * y).sum()])


def f1_from_counts(c: torch.Tensor) -> torch.Tensor:
    """Micro F1 of fp64 (tp, fp, fn) with div-no-nan precision / recall (tfa FBetaScore.result, beta 1) -> fp32 scalar."""
    tp, fp, fn = c[0], c[1], c[2]
    zero = torch.zeros((), dtype=torch.float64, device=c.device)
    prec = torch.where(tp + fp != 0, tp / torch.where(tp + fp != 0, tp + fp, 1.0), zero)
    rec = torch.where(tp + fn != 0, tp / torch.where(tp + fn != 0, tp + fn, 1.0), zero)
    ps = prec + rec
    return (torch.where(ps != 0, prec * rec / torch.where(ps != 0, ps, 1.0), zero) * 2.0).to(torch.float32)


class _Workspace:
    """Slab + ticket of iris_event_metrics, one pair per (device, batch size); never freed while this object lives (a
    captured graph holds the addresses).  Made by an eager call: a capture needs its warm-up call first (torch's recipe)."""

    def __init__(self):
        self._ws = {}

    def get(self, device, batch):
        key = (device, batch)
        if key not in self._ws:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("event_metrics: the first call for a batch size must be eager (warm up before the capture)")
            self._ws[key] = (torch.zeros(3 * batch, dtype=torch.float64, device=device),
                             torch.zeros(1, dtype=torch.int32, device=device))
        return self._ws[key]


def event_metrics(y_true: torch.Tensor, y_pred: torch.Tensor, threshold: float = 0.5, pool: int = 0, want_cos: bool = False,
                  f1_state: Optional[torch.Tensor] = None, f1_threshold: float = 0.5, accum: Optional[torch.Tensor] = None,
                  workspace: Optional[_Workspace] = None) -> Dict[str, torch.Tensor]:
    """One iris_event_metrics launch on the current stream: {'er': [B], 'cos_sim': [B] (want_cos), 'f1_score': [] (f1_state)}.
    `f1_state` (fp64 [3], cumulative) and `accum` (fp64 [5]: sum er, sum cos, sum f1, clips, batches) are updated in place."""
    if y_true.dim() != 3 or y_pred.dim() != 3 or y_true.shape[0] != y_pred.shape[0] or y_true.shape[2] != y_pred.shape[2]:
        raise ValueError(f"event_metrics: y_true [B, T, K] and y_pred [B, T', K], got {tuple(y_true.shape)} / {tuple(y_pred.shape)}")
    if not (y_true.is_cuda and y_pred.is_cuda):
        raise ValueError("event_metrics: GPU tensors (the CPU path is er_host / f1_counts_host / cos_sim)")
    dev = y_true.device
    yt = y_true.detach().to(torch.float32).contiguous()
    yp = y_pred.detach().to(torch.float32).contiguous()
    b, t, k = yt.shape
    er = torch.empty(b, dtype=torch.float32, device=dev)
    cos = torch.empty(b, dtype=torch.float32, device=dev) if want_cos else None
    f1 = torch.empty((), dtype=torch.float32, device=dev) if f1_state is not None else None
    for name, s, n in (("f1_state", f1_state, 3), ("accum", accum, 5)):
        if s is not None and (s.dtype != torch.float64 or s.device != dev or s.numel() != n or not s.is_contiguous()):
            raise ValueError(f"event_metrics: {name} must be a contiguous fp64 [{n}] tensor on {dev}")
    slab = ticket = None
    if f1_state is not None or accum is not None:
        slab, ticket = (workspace or _WS).get(dev, b)

    def ptr(x):
        return x.data_ptr() if x is not None else None
    N.check(N.lib().iris_event_metrics(ptr(yt), ptr(yp), b, t, yp.shape[1], k, float(threshold), int(pool), float(f1_threshold),
                                       ptr(er), ptr(cos), ptr(f1_state), ptr(f1), ptr(accum), ptr(slab), ptr(ticket),
                                       torch.cuda.current_stream(dev).cuda_stream), "iris_event_metrics")
    out = {'er': er}
    if cos is not None:
        out['cos_sim'] = cos
    if f1 is not None:
        out['f1_score'] = f1
    return out


_WS = _Workspace()


class _ErScore:
    def __init__(self, threshold=0.5, smoothing=True):
        self.threshold, self.smoothing = float(threshold), bool(smoothing)
        self.pool = SMOOTHING_POOL if smoothing else 0
        self.__name__ = 'er'   # Keras logs the inner function's name (metrics.py:220)

    def __call__(self, y_true, y_pred):
        y_true, y_pred = _first(y_true), _first(y_pred)
        if y_pred.is_cuda:
            return event_metrics(y_true, y_pred, self.threshold, self.pool)['er']
        return er_host(y_true, y_pred, self.threshold, self.pool)


def er_score(threshold=0.5, smoothing=True):
    """metrics.py:217-274: per-clip error rate [B] of the thresholded frame predictions."""
    return _ErScore(threshold, smoothing)


class _F1Score:
    """tfa F1Score(num_classes=3, threshold=0.5, average='micro') behind a plain function (metrics.py:291-299): the counts
    (fp64 tp, fp, fn) live as long as this object, one state per device."""

    def __init__(self, threshold=0.5):
        self.threshold = float(threshold)
        self.states: Dict[torch.device, torch.Tensor] = {}
        self.__name__ = 'f1_score'

    def state(self, device) -> torch.Tensor:
        device = _device(device)
        if device not in self.states:
            self.states[device] = torch.zeros(3, dtype=torch.float64, device=device)
        return self.states[device]

    def __call__(self, y_true, y_pred):
        y_true, y_pred = _first(y_true), _first(y_pred)
        st = self.state(y_pred.device)
        if y_pred.is_cuda:
            return event_metrics(y_true, y_pred, f1_state=st, f1_threshold=self.threshold)['f1_score']
        st += f1_counts_host(y_true, y_pred, self.threshold)
        return f1_from_counts(st)


def f1_score():
    return _F1Score(0.5)


def _cos_sim_metric(y_true, y_pred):
    """metrics.py:277-288 (== trainer.cos_sim); one launch on GPU tensors."""
    y_true, y_pred = _first(y_true), _first(y_pred)
    if y_pred.is_cuda:
        return event_metrics(y_true, y_pred, want_cos=True)['cos_sim']
    return cos_sim(y_true, y_pred)


_cos_sim_metric.__name__ = 'cos_sim'


# ---------------------------------------------------------------------------
# integer count states of the validation pass: what ScoreHistogram, SedEval and Psds share
# ---------------------------------------------------------------------------
def _workspace_query(name: str, *args) -> int:
    """The byte count the library's query `name` gives for these arguments; what it refuses (0) is a ValueError."""
    n_bytes = int(getattr(N.lib(), name)(*args))
    if n_bytes <= 0:
        N.check(-1, name)
    return n_bytes


class _CountState:
    """Integer counts of everything `update` has seen: one int64 tensor of shape `_shape` per device (as `_F1Score` keeps its
    states).  On GPU tensors an update is the subclass's launches on the current stream - integer adds: exact, independent of the
    order, no host sync - on CPU tensors its host rule, the same arithmetic with torch ops.  A subclass checks its parameters,
    sets `_shape`, and gives the four things that differ:
      _host(y_true, y_pred)               the counts of one batch, on the host
      _workspace_bytes(b, t, k)           what its launches need as scratch memory (0: none, the default)
      _launch(yt, yp, ws, state, stream)  its iris_* call on fp32 contiguous tensors; `ws` an int64 tensor of at least that size, or None
      metrics(counts)                     the host arithmetic on counts (one rank's or the sum over ranks)
    MAX_CLASSES bounds n_classes; MAX_FRAMES, where set, bounds T, and B * T then stays below 2^31."""
    MAX_CLASSES = 16
    MAX_FRAMES = None

    def __init__(self, n_classes: int):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= self.MAX_CLASSES:
            raise ValueError(f"{type(self).__name__}: n_classes in [1, {self.MAX_CLASSES}], got {n_classes}")
        self.states: Dict[torch.device, torch.Tensor] = {}
        self._workspaces: Dict[tuple, torch.Tensor] = {}
        self._retired: List[torch.Tensor] = []

    def _workspace_bytes(self, b: int, t: int, k: int) -> int:
        return 0

    def state(self, device) -> torch.Tensor:
        device = _device(device)
        if device not in self.states:
            self.states[device] = torch.zeros(*self._shape, dtype=torch.int64, device=device)
        return self.states[device]

    def _workspace(self, device, stream: int, n_bytes: int) -> torch.Tensor:
        """The workspace of (device, stream), at least n_bytes in 8-byte words: the launches of one stream are ordered, those of
        two streams get a workspace each.  A larger one replaces it; the old one is kept while this object lives (launches or a
        captured graph may still hold its address)."""
        ws = self._workspaces.get((device, stream))
        if ws is None or ws.numel() * 8 < n_bytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}.update: the first call for a shape must be eager (warm up before the capture)")
            if ws is not None:
                self._retired.append(ws)
            ws = self._workspaces[(device, stream)] = torch.empty((n_bytes + 7) // 8, dtype=torch.int64, device=device)
        return ws

    @torch.no_grad()
    def update(self, y_true: torch.Tensor, y_pred: torch.Tensor) -> None:
        name = type(self).__name__
        y_true, y_pred = _first(y_true), _first(y_pred)
        if y_true.dim() != 3 or y_pred.dim() != 3 or y_true.shape != y_pred.shape:
            raise ValueError(f"{name}.update: y_true and y_pred [B, T, K] at the same frame rate, got {tuple(y_true.shape)} "
                             f"/ {tuple(y_pred.shape)}")
        if y_pred.shape[2] != self.n_classes:
            raise ValueError(f"{name}.update: {y_pred.shape[2]} classes, made for {self.n_classes}")
        if not (y_true.is_floating_point() and y_pred.is_floating_point()):
            raise ValueError(f"{name}.update: floating-point tensors, got {y_true.dtype} / {y_pred.dtype}")
        if y_true.device != y_pred.device:
            raise ValueError(f"{name}.update: y_true on {y_true.device}, y_pred on {y_pred.device}")
        if y_pred.numel() == 0:
            return
        b, t, k = y_pred.shape
        if self.MAX_FRAMES and (t > self.MAX_FRAMES or b * t > 2 ** 31 - 1):
            raise ValueError(f"{name}.update: T {t} (<= 2^{self.MAX_FRAMES.bit_length() - 1}) and B * T {b * t} (<= 2^31 - 1)")
        st = self.state(y_pred.device)
        if not y_pred.is_cuda:
            st += self._host(y_true, y_pred)
            return
        yt = y_true.detach().to(torch.float32).contiguous()
        yp = y_pred.detach().to(torch.float32).contiguous()
        stream = torch.cuda.current_stream(yp.device).cuda_stream
        n_bytes = self._workspace_bytes(b, t, k)
        self._launch(yt, yp, self._workspace(yp.device, stream, n_bytes) if n_bytes else None, st, stream)

    def reset(self) -> None:
        for s in self.states.values():
            s.zero_()

    def counts(self) -> torch.Tensor:
        """The counts on the host, summed over this object's devices."""
        out = torch.zeros(*self._shape, dtype=torch.int64)
        for s in self.states.values():
            out += s.cpu()
        return out

    def total(self, all_reduce: bool = False) -> torch.Tensor:
        """The counts summed over this object's devices (at least one update has made a state), on the first one's device, and
        with `all_reduce` over the ranks (int64 SUM: exact, every rank gets the same values).  The sums are formed in a clone: the
        live states are never modified.  The caller's `.cpu()` is the one copy to the host."""
        states = list(self.states.values())
        total = states[0].clone() if all_reduce or len(states) > 1 else states[0]
        for s in states[1:]:
            total += s.to(total.device)
        if all_reduce:
            torch.distributed.all_reduce(total)
        return total

    def compute(self) -> dict:
        return self.metrics(self.counts())


class _CompiledCounts:
    """What score_curves(), sed_eval() and psds() return: a `_CountState` subclass behind a compiled metric.  A `MetricSet` feeds
    it in the 'val' phase only and returns no per-step value for it; `counter` is made by the first batch (its class count).
    `names` are the row entries it adds, `row` the function from the counter's `metrics(counts)` to their values."""

    def __init__(self, name: str, cls, names: tuple, row, **kwargs):
        cls(1, **kwargs)   # (refuses bad arguments now, not at the first validation batch)
        self.cls, self.kwargs, self.names, self.row = cls, kwargs, names, row
        self.counter: Optional[_CountState] = None
        self.__name__ = name

    def update(self, y_true, y_pred) -> None:
        y_pred = _first(y_pred)
        if self.counter is None:
            self.counter = self.cls(y_pred.shape[-1], **self.kwargs)
        self.counter.update(y_true, y_pred)

    def reset(self) -> None:
        if self.counter is not None:
            self.counter.reset()

    def values(self, prefix: str = '', all_reduce: bool = False) -> Dict[str, float]:
        """{prefix + name: value} for `names` from the validation counts (NaN before the first batch), summed over the ranks first
        with `all_reduce`, in one copy to the host.  Every rank must have seen a validation batch, or none."""
        c = self.counter
        if c is None or not c.states:
            return {prefix + n: float('nan') for n in self.names}
        return {prefix + n: v for n, v in zip(self.names, self.row(c.metrics(c.total(all_reduce).cpu())))}

    def __call__(self, y_true, y_pred):
        raise TypeError(f"{self.__name__}() has no per-batch value: compile it (model.compile(metrics=[...])) and read "
                        "MetricSet.val_values after the validation pass")


# ---------------------------------------------------------------------------
# threshold-free validation numbers from a score histogram (no counterpart in the reference)
# ---------------------------------------------------------------------------
CURVE_MIN_BINS, CURVE_MAX_BINS, CURVE_MAX_CLASSES = 16, 4096, 16


def check_curve_bins(bins) -> int:
    bins = int(bins)
    if bins < CURVE_MIN_BINS or bins > CURVE_MAX_BINS or bins & (bins - 1):
        raise ValueError(f"score histogram: bins must be a power of two in [{CURVE_MIN_BINS}, {CURVE_MAX_BINS}], got {bins}")
    return bins


def score_hist_host(y_true: torch.Tensor, y_pred: torch.Tensor, bins: int) -> torch.Tensor:
    """The counts [K, 2, bins + 1] (int64) of one batch with torch ops, on the tensors' device - the CPU path of
    `ScoreHistogram.update`, and the rule iris_score_hist restates: label = y_true >= 0.5 (NaN: negative), slot =
    min(bins - 1, max(0, floor(p * bins))) in fp32 (p * bins is exact: bins is a power of two), slot `bins` for a NaN p."""
    yt = y_true.detach().to(torch.float32)
    yp = y_pred.detach().to(torch.float32)
    k = yp.shape[-1]
    label = (yt >= 0.5).to(torch.int64)
    slot = torch.clamp(torch.floor(yp * float(bins)), 0.0, float(bins - 1))
    slot = torch.where(torch.isnan(yp), torch.full_like(slot, float(bins)), slot).to(torch.int64)
    cls = torch.arange(k, device=yp.device, dtype=torch.int64).expand_as(slot)
    idx = (cls * 2 + label) * (bins + 1) + slot
    return torch.bincount(idx.reshape(-1), minlength=k * 2 * (bins + 1)).view(k, 2, bins + 1)


def _nanmean(values) -> float:
    kept = [v for v in values if v == v]
    return sum(kept) / len(kept) if kept else float('nan')


def curve_metrics(counts) -> dict:
    """Host arithmetic on a score histogram [K, 2, bins + 1] of integers (NumPy or a tensor; one rank's or the sum over ranks):
    counts[k, 0] the negative frames, counts[k, 1] the positive ones, slot `bins` the NaN predictions (excluded from every curve).
    With pos[b], neg[b] the counts of a class, P, N their sums over the real bins, TP_b = sum_{j >= b} pos[j], FP_b likewise:
      auroc          sum_b pos[b] (2 sum_{j < b} neg[j] + neg[b]) / (2 P N): ties inside a bin count half; NaN if P or N is 0
      ap             sum_b (pos[b] / P) TP_b / (TP_b + FP_b): sklearn's step-wise average precision on the binned scores; NaN if P = 0
      best_f1        max_b 2 TP_b / (TP_b + FP_b + P), best_threshold = b / bins for the smallest such b; NaN if P = 0
      ece            sum_b (n_b / n) |pos[b] / n_b - (b + 0.5) / bins| over the non-empty bins, n_b = pos[b] + neg[b]; NaN if n = 0
    The sums are formed in Python integers (exact); each quotient is rounded once.  Returns {'per_class': {name: [K values]} with
    the names above and the integer fields n_pos, n_neg, n_nan; 'auc', 'map', 'best_f1': the means over the classes where the
    value is defined (NaN if there is none); 'bins'}."""
    c = np.asarray(counts.detach().cpu() if torch.is_tensor(counts) else counts)
    if c.ndim != 3 or c.shape[1] != 2 or c.shape[2] < 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"curve_metrics: integer counts [K, 2, bins + 1], got {c.dtype} {tuple(c.shape)}")
    bins = c.shape[2] - 1
    nan = float('nan')
    per = {n: [] for n in ('auroc', 'ap', 'best_f1', 'best_threshold', 'ece', 'n_pos', 'n_neg', 'n_nan')}
    for k in range(c.shape[0]):
        neg = [int(v) for v in c[k, 0, :bins]]
        pos = [int(v) for v in c[k, 1, :bins]]
        p_all, n_all = sum(pos), sum(neg)
        per['n_pos'].append(p_all)
        per['n_neg'].append(n_all)
        per['n_nan'].append(int(c[k, 0, bins]) + int(c[k, 1, bins]))
        below, num = 0, 0
        for b in range(bins):
            num += pos[b] * (2 * below + neg[b])
            below += neg[b]
        per['auroc'].append(num / (2 * p_all * n_all) if p_all and n_all else nan)
        ap, clean, tp, fp = 0.0, 0, 0, 0
        best_num, best_den, best_b = -1, 1, 0
        for b in range(bins - 1, -1, -1):   # thresholds from the top: TP_b, FP_b as running sums
            tp += pos[b]
            fp += neg[b]
            if pos[b] and not fp:
                clean += pos[b]             # precision exactly 1: summed as integers (perfect separation gives exactly 1.0)
            elif pos[b]:
                ap += (pos[b] * tp) / (p_all * (tp + fp))
            # F1_b = 2 TP_b / (TP_b + FP_b + P), compared exactly by cross-multiplication; `>=` on the way down keeps the smallest b
            if p_all and 2 * tp * best_den >= best_num * (tp + fp + p_all):
                best_num, best_den, best_b = 2 * tp, tp + fp + p_all, b
        per['ap'].append(clean / p_all + ap if p_all else nan)
        per['best_f1'].append(best_num / best_den if p_all else nan)
        per['best_threshold'].append(best_b / bins if p_all else nan)
        n = p_all + n_all
        ece = 0.0
        for b in range(bins):
            nb = pos[b] + neg[b]
            if nb:
                ece += (nb / n) * abs(pos[b] / nb - (b + 0.5) / bins)
        per['ece'].append(ece if n else nan)
    return {'per_class': per, 'auc': _nanmean(per['auroc']), 'map': _nanmean(per['ap']), 'best_f1': _nanmean(per['best_f1']),
            'bins': bins}


class ScoreHistogram(_CountState):
    """The score histogram per (class, label), a `_CountState` of int64 [K, 2, bins + 1].  On GPU tensors an update is ONE
    iris_score_hist launch, no workspace; on CPU tensors `score_hist_host`.  `compute` is `curve_metrics` on the counts."""
    MAX_CLASSES = CURVE_MAX_CLASSES

    def __init__(self, n_classes: int, bins: int = 1024):
        self.bins = check_curve_bins(bins)
        super().__init__(n_classes)
        self._shape = (self.n_classes, 2, self.bins + 1)

    def _host(self, y_true, y_pred):
        return score_hist_host(y_true, y_pred, self.bins)

    def _launch(self, yt, yp, ws, st, stream):
        b, t, k = yp.shape
        N.check(N.lib().iris_score_hist(yt.data_ptr(), yp.data_ptr(), b, t, k, self.bins, st.data_ptr(), stream), "iris_score_hist")

    def metrics(self, counts) -> dict:
        return curve_metrics(counts)


CURVE_NAMES = ('auc', 'map', 'best_f1')   # what a compiled score_curves() adds to a row (macro means); `fit` MAXIMISES such a monitor


def score_curves(bins=1024):
    """A metric for `compile(metrics=[...])`: ROC-AUC, average precision and the best frame F1 of the validation pass, from an
    on-device score histogram with `bins` bins (`fit` logs val_auc, val_map, val_best_f1)."""
    return _CompiledCounts('score_curves', ScoreHistogram, CURVE_NAMES, lambda m: [m[n] for n in CURVE_NAMES], bins=bins)


# ---------------------------------------------------------------------------
# segment- and event-based detection measures (Mesaros, Heittola & Virtanen 2016; no counterpart in the reference)
# ---------------------------------------------------------------------------
SED_MAX_THRESHOLDS, SED_MAX_CLASSES, SED_MAX_FRAMES = 16, 16, 1 << 20


def check_sed_params(thresholds=(0.5,), segment=1.0, collar=0.2, offset_pct=50, sr=16000, hop=256):
    """-> (thresholds as a tuple of fp32 values, hop, seg_samples, collar_samples, offset_pct), or ValueError: what
    iris_sed_counts refuses, refused alike for both paths."""
    try:
        thr = tuple(float(np.float32(h)) for h in thresholds)
    except TypeError:
        raise ValueError(f"sed_eval: thresholds must be a sequence of numbers, got {thresholds!r}") from None
    if not 1 <= len(thr) <= SED_MAX_THRESHOLDS:
        raise ValueError(f"sed_eval: 1 .. {SED_MAX_THRESHOLDS} thresholds, got {len(thr)}")
    if not all(np.isfinite(h) for h in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError(f"sed_eval: thresholds must be finite and strictly increasing (as fp32), got {thresholds!r}")
    if int(offset_pct) != offset_pct or not 0 <= int(offset_pct) <= 100:
        raise ValueError(f"sed_eval: offset_pct must be an integer in [0, 100], got {offset_pct!r}")
    hop_i, seg_samples, collar_samples = int(hop), int(round(segment * sr)), int(round(collar * sr))
    if hop_i != hop or hop_i < 1 or seg_samples < hop_i or collar_samples < 0 or max(seg_samples, collar_samples, hop_i) >= 2 ** 31:
        raise ValueError(f"sed_eval: hop {hop!r} (an integer >= 1), segment {segment!r} s = {seg_samples} samples (>= hop), collar "
                         f"{collar!r} s = {collar_samples} samples (>= 0)")
    return thr, hop_i, seg_samples, collar_samples, int(offset_pct)


def _greedy_matches(ref_on, ref_off, pred_on, pred_off, collar_samples, offset_pct) -> int:
    """Matches of one row's events (onsets / offsets in samples, in time order): every reference event takes the earliest free
    predicted event within both collars."""
    taken = [False] * len(pred_on)
    lo = n = 0
    for on_r, off_r in zip(ref_on, ref_off):
        tol = max(100 * collar_samples, offset_pct * (off_r - on_r))
        while lo < len(pred_on) and (taken[lo] or pred_on[lo] < on_r - collar_samples):
            lo += 1
        for q in range(lo, len(pred_on)):
            if pred_on[q] > on_r + collar_samples:
                break
            if not taken[q] and 100 * abs(pred_off[q] - off_r) <= tol:
                taken[q] = True
                n += 1
                break
    return n


def sed_counts_host(y_true: torch.Tensor, y_pred: torch.Tensor, thresholds=(0.5,), segment=1.0, collar=0.2, offset_pct=50,
                    sr=16000, hop=256) -> torch.Tensor:
    """The counts [n_thr, K + 1, 6] (int64, on the host) of one batch [B, T, K]: rows k < K hold (seg_tp, seg_fp, seg_fn, ev_tp,
    ev_fp, ev_fn), row K holds (S, D, I, n_segments, 0, 0) - the CPU path of `SedEval.update` and the rule iris_sed_counts
    restates (include/iris_frontend.h).  Activities, segments and run ends are torch ops on the tensors' device; the events then
    go to the host in one copy and are matched there, row by row."""
    thr, hop, seg_samples, collar_samples, offset_pct = check_sed_params(thresholds, segment, collar, offset_pct, sr, hop)
    yt = y_true.detach().to(torch.float32)
    yp = y_pred.detach().to(torch.float32)
    dev = yp.device
    b, t, k = yp.shape
    n = len(thr)
    levels = torch.tensor(thr, dtype=torch.float32, device=dev)
    act = torch.cat([(yt >= 0.5)[None], yp[None] >= levels[:, None, None, None]])          # [1 + n, B, T, K]; NaN: False
    seg = (torch.arange(t, device=dev, dtype=torch.int64) * hop) // seg_samples
    n_seg = ((t - 1) * hop) // seg_samples + 1
    seg_act = torch.zeros(1 + n, b, n_seg, k, dtype=torch.int32, device=dev).index_add_(2, seg, act.to(torch.int32)) > 0
    ref, pred = seg_act[:1], seg_act[1:]
    out = torch.zeros(n, k + 1, 6, dtype=torch.int64, device=dev)
    out[:, :k, 0] = (ref & pred).sum((1, 2))
    out[:, :k, 1] = (~ref & pred).sum((1, 2))
    out[:, :k, 2] = (ref & ~pred).sum((1, 2))
    n_fn, n_fp = (ref & ~pred).sum(-1), (~ref & pred).sum(-1)                               # [n, B, n_seg]
    out[:, k, 0] = torch.minimum(n_fn, n_fp).sum((1, 2))
    out[:, k, 1] = (n_fn - n_fp).clamp(min=0).sum((1, 2))
    out[:, k, 2] = (n_fp - n_fn).clamp(min=0).sum((1, 2))
    out[:, k, 3] = b * n_seg
    rows = act.permute(0, 1, 3, 2)                                                          # [1 + n, B, K, T]
    starts, ends = _runs(rows.reshape(1 + n, b * k, t))                                     # (list, row, frame), sorted alike
    row_id = (starts[:, 0] * (b * k) + starts[:, 1]).cpu().numpy()
    on = (starts[:, 2] * hop).cpu().tolist()
    off = ((ends[:, 2] + 1) * hop).cpu().tolist()
    edge = np.searchsorted(row_id, np.arange((1 + n) * b * k + 1)).tolist()                 # events of (list, row): edge[i] .. edge[i + 1]
    ev = np.zeros((n, k, 3), np.int64)
    for r in range(b * k):
        r0, r1 = edge[r], edge[r + 1]
        for j in range(n):
            p0, p1 = edge[(1 + j) * b * k + r], edge[(1 + j) * b * k + r + 1]
            tp = _greedy_matches(on[r0:r1], off[r0:r1], on[p0:p1], off[p0:p1], collar_samples, offset_pct) if r1 > r0 and p1 > p0 else 0
            ev[j, r % k] += (tp, p1 - p0 - tp, r1 - r0 - tp)
    out = out.cpu()
    out[:, :k, 3:] = torch.from_numpy(ev)
    return out


def _ratio(num, den) -> float:
    return num / den if den else float('nan')


def _prf(tp, fp, fn) -> tuple:
    return _ratio(tp, tp + fp), _ratio(tp, tp + fn), _ratio(2 * tp, 2 * tp + fp + fn)


def sed_metrics(counts, thresholds) -> dict:
    """Host arithmetic on the counts [n_thr, K + 1, 6] of `SedEval` (integers: NumPy or a tensor; one rank's or the sum over
    ranks), float64, a zero denominator giving NaN as in `curve_metrics`.  Returns {'thresholds', 'per_threshold': one dict per
    threshold, 'best_event_f1_threshold', 'best_segment_f1_threshold' (the first threshold with the largest micro F1; NaN if
    none is defined)}.  Each per-threshold dict holds
      'segment': micro 'f1' = 2 TP / (2 TP + FP + FN) over the classes with 'precision' and 'recall', 'macro_f1' (the mean over
                 the classes where F1 is defined), 'er' = (S + D + I) / Nref with Nref = sum_k (seg_tp + seg_fn) and its parts
                 'substitution_rate', 'deletion_rate', 'insertion_rate', the integers 'n_ref' and 'n_segments', and 'per_class'
                 {'f1', 'precision', 'recall': [K values]};
      'event':   micro 'f1', 'precision', 'recall', 'macro_f1', 'er' = (FN + FP) / n_ref, the integers 'n_ref', 'n_pred', and
                 'per_class' likewise.  Classes are scored independently: no substitutions across classes at event level."""
    c = np.asarray(counts.detach().cpu() if torch.is_tensor(counts) else counts)
    if c.ndim != 3 or c.shape[1] < 2 or c.shape[2] != 6 or not np.issubdtype(c.dtype, np.integer) or c.shape[0] != len(thresholds):
        raise ValueError(f"sed_metrics: integer counts [n_thr = {len(thresholds)}, K + 1, 6], got {c.dtype} {tuple(c.shape)}")
    k = c.shape[1] - 1
    per_thr = []
    for j in range(c.shape[0]):
        v = [[int(x) for x in row] for row in c[j]]
        res = {}
        for name, o in (('segment', 0), ('event', 3)):
            cls = [_prf(v[i][o], v[i][o + 1], v[i][o + 2]) for i in range(k)]
            tp, fp, fn = (sum(v[i][o + d] for i in range(k)) for d in range(3))
            prec, rec, f1 = _prf(tp, fp, fn)
            res[name] = {'f1': f1, 'precision': prec, 'recall': rec, 'macro_f1': _nanmean([x[2] for x in cls]), 'n_ref': tp + fn,
                         'per_class': {'precision': [x[0] for x in cls], 'recall': [x[1] for x in cls], 'f1': [x[2] for x in cls]}}
            if name == 'segment':
                s, d, i, n_segments = v[k][:4]
                res[name].update(er=_ratio(s + d + i, tp + fn), substitution_rate=_ratio(s, tp + fn), deletion_rate=_ratio(d, tp + fn),
                                 insertion_rate=_ratio(i, tp + fn), n_segments=n_segments)
            else:
                res[name].update(er=_ratio(fn + fp, tp + fn), n_pred=tp + fp)
        per_thr.append(res)

    def best(kind):
        vals = [r[kind]['f1'] for r in per_thr]
        kept = [x for x in vals if x == x]
        return float(thresholds[vals.index(max(kept))]) if kept else float('nan')
    return {'thresholds': [float(h) for h in thresholds], 'per_threshold': per_thr, 'best_event_f1_threshold': best('event'),
            'best_segment_f1_threshold': best('segment')}


class SedEval(_CountState):
    """Segment-based (1 s segments: ER, F1) and event-based (200 ms onset collar, offset collar max(200 ms, 50 % of the event):
    F1, ER) detection counts at every threshold of `thresholds`, a `_CountState` of int64 [n_thr, K + 1, 6].  On GPU tensors an
    update is iris_sed_counts - two launches, with a workspace - on CPU tensors `sed_counts_host`.  Event matching is greedy in
    time order and per class; `compute` is `sed_metrics` on the counts."""
    MAX_CLASSES, MAX_FRAMES = SED_MAX_CLASSES, SED_MAX_FRAMES

    def __init__(self, n_classes: int, thresholds=(0.5,), segment=1.0, collar=0.2, offset_pct=50, sr=16000, hop=256):
        super().__init__(n_classes)
        self.thresholds, self.hop, self.seg_samples, self.collar_samples, self.offset_pct = \
            check_sed_params(thresholds, segment, collar, offset_pct, sr, hop)
        self._host_args = dict(thresholds=self.thresholds, segment=segment, collar=collar, offset_pct=offset_pct, sr=sr, hop=hop)
        self._levels = (N.C.c_float * len(self.thresholds))(*self.thresholds)
        self._shape = (len(self.thresholds), self.n_classes + 1, 6)

    def _host(self, y_true, y_pred):
        return sed_counts_host(y_true, y_pred, **self._host_args)

    def _workspace_bytes(self, b, t, k):
        return _workspace_query("iris_sed_workspace_bytes", b, t, k, len(self.thresholds), self.hop, self.seg_samples)

    def _launch(self, yt, yp, ws, st, stream):
        b, t, k = yp.shape
        N.check(N.lib().iris_sed_counts(yt.data_ptr(), yp.data_ptr(), b, t, k, self._levels, len(self.thresholds), self.hop,
                                        self.seg_samples, self.collar_samples, self.offset_pct, ws.data_ptr(), ws.numel() * 8,
                                        st.data_ptr(), stream), "iris_sed_counts")

    def metrics(self, counts) -> dict:
        return sed_metrics(counts, self.thresholds)


SED_NAMES = ('seg_f1', 'seg_er', 'event_f1')   # what a compiled sed_eval() adds to a row; `fit` MAXIMISES the two F1, minimises seg_er


def _sed_row(m: dict) -> list:
    first = m['per_threshold'][0]
    return [first['segment']['f1'], first['segment']['er'], first['event']['f1']]


def sed_eval(thresholds=(0.5,), segment=1.0, collar=0.2, offset_pct=50, sr=16000, hop=256):
    """A metric for `compile(metrics=[...])`: segment-based F1 / ER and event-based F1 of the validation pass at the FIRST
    threshold of the list, from on-device integer counts (`fit` logs val_seg_f1, val_seg_er, val_event_f1).  `hop` is the hop of
    the frames the metric sees - the model's output frames - in samples."""
    return _CompiledCounts('sed_eval', SedEval, SED_NAMES, _sed_row, thresholds=thresholds, segment=segment, collar=collar,
                           offset_pct=offset_pct, sr=sr, hop=hop)


# ---------------------------------------------------------------------------
# polyphonic sound detection score (Bilen et al., ICASSP 2020; no counterpart in the reference)
# ---------------------------------------------------------------------------
PSDS_MAX_THRESHOLDS, PSDS_MAX_CLASSES, PSDS_MAX_FRAMES = 64, 16, 1 << 20
PSDS_SCENARIOS = {   # the two DCASE Task 4 settings
    1: dict(dtc_pct=70, gtc_pct=70, cttc_pct=None, alpha_ct=0.0, alpha_st=1.0),
    2: dict(dtc_pct=10, gtc_pct=10, cttc_pct=30, alpha_ct=0.5, alpha_st=1.0),
}


def psds_default_thresholds() -> tuple:
    return tuple(float(h) for h in np.linspace(0.01, 0.99, 50).astype(np.float32))


def check_psds_params(thresholds=None, dtc_pct=70, gtc_pct=70, cttc_pct=None):
    """-> (thresholds as a tuple of fp32 values, dtc_pct, gtc_pct, cttc_pct or None), or ValueError: what iris_psds_counts
    refuses, refused alike for both paths.  `thresholds` None: the 50 values of np.linspace(0.01, 0.99, 50) as fp32; `cttc_pct`
    None (or 0, as in the C ABI): no cross-triggers are counted."""
    if thresholds is None:
        thresholds = psds_default_thresholds()
    try:
        thr = tuple(float(np.float32(h)) for h in thresholds)
    except TypeError:
        raise ValueError(f"psds: thresholds must be a sequence of numbers, got {thresholds!r}") from None
    if not 1 <= len(thr) <= PSDS_MAX_THRESHOLDS:
        raise ValueError(f"psds: 1 .. {PSDS_MAX_THRESHOLDS} thresholds, got {len(thr)}")
    if not all(np.isfinite(h) for h in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError(f"psds: thresholds must be finite and strictly increasing (as fp32), got {thresholds!r}")
    for name, v in (('dtc_pct', dtc_pct), ('gtc_pct', gtc_pct)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 100:
            raise ValueError(f"psds: {name} must be an integer in [1, 100], got {v!r}")
    if cttc_pct is not None and (isinstance(cttc_pct, bool) or not isinstance(cttc_pct, (int, np.integer)) or not 0 <= int(cttc_pct) <= 100):
        raise ValueError(f"psds: cttc_pct must be None or an integer in [1, 100], got {cttc_pct!r}")
    return thr, int(dtc_pct), int(gtc_pct), (int(cttc_pct) or None) if cttc_pct is not None else None


def _psds_frames_column(k: int) -> int:
    """The column of row 0 of the totals plane that holds n_frames: K - for K = 1, where that is the gt_frames column, 2."""
    return k if k > 1 else 2


def psds_counts_host(y_true: torch.Tensor, y_pred: torch.Tensor, thresholds=None, dtc_pct=70, gtc_pct=70, cttc_pct=None) -> torch.Tensor:
    """The counts [n_thr + 1, K, K + 2] (int64, on the host) of one batch [B, T, K] in the layout of include/iris_frontend.h
    (iris_psds_counts): plane j, row c holds TP in column c, the cross-triggers on class k in column k != c, FP in column K and
    the detections in column K + 1; the last plane holds n_gt, gt_frames per class and n_frames.  The CPU path of `Psds.update`
    and the rule the kernel restates: torch ops on the tensors' device, threshold after threshold, and one copy to the host."""
    thr, dtc, gtc, cttc = check_psds_params(thresholds, dtc_pct, gtc_pct, cttc_pct)
    yt = y_true.detach().to(torch.float32)
    yp = y_pred.detach().to(torch.float32)
    dev = yp.device
    b, t, k = yp.shape
    n = len(thr)
    out = torch.zeros(n + 1, k, k + 2, dtype=torch.int64, device=dev)
    ref = (yt >= 0.5).permute(0, 2, 1)                                                # [B, K, T]; NaN: False
    lab = torch.nn.functional.pad(ref.to(torch.int64).cumsum(-1), (1, 0))             # lab[..., x]: active label frames before x
    gs, ge = _runs(ref)
    g_b, g_k, g_s, g_e = gs[:, 0], gs[:, 1], gs[:, 2], ge[:, 2] + 1
    out[n, :, 0] = torch.bincount(g_k, minlength=k)
    out[n, :, 1] = ref.sum((0, 2))
    out[n, 0, _psds_frames_column(k)] = b * t
    classes = torch.arange(k, device=dev)
    levels = torch.tensor(thr, dtype=torch.float32, device=dev)
    for j in range(n):
        ds, de = _runs((yp >= levels[j]).permute(0, 2, 1))
        d_b, d_c, d_s, d_e = ds[:, 0], ds[:, 1], ds[:, 2], de[:, 2] + 1
        length = d_e - d_s
        inter = lab[d_b, :, d_e] - lab[d_b, :, d_s]                                   # [N, K]: I_k(d)
        passes = 100 * inter.gather(1, d_c[:, None])[:, 0] >= dtc * length
        out[j, :, k + 1] = torch.bincount(d_c, minlength=k)
        out[j, :, k] = torch.bincount(d_c[~passes], minlength=k)
        if cttc:
            ct = ~passes[:, None] & (100 * inter >= cttc * length[:, None]) & (classes[None] != d_c[:, None])
            out[j, :, :k] = torch.bincount((d_c[:, None] * k + classes[None])[ct], minlength=k * k).view(k, k)
        edge = torch.zeros(b, k, t + 1, dtype=torch.int64, device=dev)               # + 1 at a passing start, - 1 at its end
        one = torch.ones((), dtype=torch.int64, device=dev)
        edge.index_put_((d_b[passes], d_c[passes], d_s[passes]), one, accumulate=True)
        edge.index_put_((d_b[passes], d_c[passes], d_e[passes]), -one, accumulate=True)
        cover = torch.nn.functional.pad(edge.cumsum(-1)[..., :t].cumsum(-1), (1, 0))  # passing frames before x
        tp = 100 * (cover[g_b, g_k, g_e] - cover[g_b, g_k, g_s]) >= gtc * (g_e - g_s)
        out[j, classes, classes] = torch.bincount(g_k[tp], minlength=k)
    return out.cpu()


def _step_curve(points):
    """[(eFPR, TPR)] -> (x, y): sorted by eFPR, the largest TPR among equal eFPR, the running maximum of TPR."""
    best = {}
    for x, y in points:
        best[x] = max(y, best.get(x, 0.0))
    xs, ys, top = [], [], 0.0
    for x in sorted(best):
        top = max(top, best[x])
        xs.append(x)
        ys.append(top)
    return xs, ys


def _step_value(xs, ys, x) -> float:
    """The step function held from the left: the value of the last point at or before x, 0 before the first."""
    i = int(np.searchsorted(np.asarray(xs, np.float64), x, side='right'))
    return ys[i - 1] if i else 0.0


def psds_metrics(counts, thresholds, hop=256, sr=16000, alpha_ct=0.0, alpha_st=1.0, e_max=100.0) -> dict:
    """Host arithmetic on the counts [n_thr + 1, K, K + 2] of `Psds` (integers: NumPy or a tensor; one rank's or the sum over
    ranks), float64; one frame is hop / sr seconds.  Per class c with ground truth and per threshold: TPR = TP / n_gt[c],
    FPR = FP per hour of audio, CTR[c][k] = CT[c][k] per hour of label activity of class k (classes k != c with activity),
    eFPR = FPR + alpha_ct * mean_k CTR[c][k].  The class's curve is the points (eFPR, TPR) sorted by eFPR, the largest TPR among
    equal eFPR, the running maximum, read as a step function held from the left (0 before the first point);
    eTPR(x) = mean over the scored classes - alpha_st * their population standard deviation, not clipped; 'psds' is its mean
    over [0, e_max], summed exactly over the union of the breakpoints.  Classes without ground truth are left out
    ('classes_without_gt'); with none left the score is NaN.  Also: 'curves' {class: {'efpr', 'tpr'}}, 'tpr_at_e_max' (NaN for a
    class left out), 'cross_triggers' {'threshold': the one nearest 0.5, 'matrix': CT[c][k] there}, and the totals."""
    c = np.asarray(counts.detach().cpu() if torch.is_tensor(counts) else counts)
    n = len(thresholds)
    if c.ndim != 3 or c.shape[0] != n + 1 or c.shape[2] != c.shape[1] + 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"psds_metrics: integer counts [n_thr + 1 = {n + 1}, K, K + 2], got {c.dtype} {tuple(c.shape)}")
    if not (e_max > 0 and np.isfinite(e_max)) or hop < 1 or sr <= 0:
        raise ValueError(f"psds_metrics: e_max {e_max!r} (> 0), hop {hop!r} (>= 1), sr {sr!r} (> 0)")
    k = c.shape[1]
    n_gt = [int(c[n, i, 0]) for i in range(k)]
    gt_frames = [int(c[n, i, 1]) for i in range(k)]
    n_frames = int(c[n, 0, _psds_frames_column(k)])

    def hours(frames):
        return frames * hop / sr / 3600.0
    curves, scored = {}, [i for i in range(k) if n_gt[i] > 0]
    for i in scored:
        others = [o for o in range(k) if o != i and gt_frames[o] > 0]
        points = []
        for j in range(n):
            efpr = int(c[j, i, k]) / hours(n_frames)
            if others:
                efpr += alpha_ct * sum(int(c[j, i, o]) / hours(gt_frames[o]) for o in others) / len(others)
            points.append((efpr, int(c[j, i, i]) / n_gt[i]))
        curves[i] = _step_curve(points)
    if scored:
        knots = sorted({0.0, float(e_max)} | {x for xs, _ in curves.values() for x in xs if 0.0 < x < e_max})
        parts = []
        for lo, hi in zip(knots, knots[1:]):
            v = np.asarray([_step_value(*curves[i], lo) for i in scored], np.float64)
            parts.append((float(v.mean()) - alpha_st * float(v.std())) * (hi - lo))
        score = math.fsum(parts) / float(e_max)
    else:
        score = float('nan')
    near = int(np.argmin([abs(float(h) - 0.5) for h in thresholds]))
    return {'psds': score, 'thresholds': [float(h) for h in thresholds], 'alpha_ct': float(alpha_ct), 'alpha_st': float(alpha_st),
            'e_max': float(e_max), 'classes_scored': scored, 'classes_without_gt': [i for i in range(k) if n_gt[i] == 0],
            'curves': {i: {'efpr': list(xs), 'tpr': list(ys)} for i, (xs, ys) in curves.items()},
            'tpr_at_e_max': [_step_value(*curves[i], float(e_max)) if i in curves else float('nan') for i in range(k)],
            'cross_triggers': {'threshold': float(thresholds[near]),
                               'matrix': [[int(c[near, i, o]) if o != i else 0 for o in range(k)] for i in range(k)]},
            'n_gt': n_gt, 'gt_frames': gt_frames, 'n_frames': n_frames}


class Psds(_CountState):
    """Intersection-based detection counts at every threshold (default: 50 from 0.01 to 0.99) under one criteria set - scenario
    1 or 2 of DCASE Task 4 (PSDS_SCENARIOS), or a dict with dtc_pct, gtc_pct, cttc_pct and optionally alpha_ct, alpha_st - a
    `_CountState` of int64 [n_thr + 1, K, K + 2].  On GPU tensors an update is iris_psds_counts - two launches, with a workspace -
    on CPU tensors `psds_counts_host`.  `compute` is `psds_metrics` on the counts."""
    MAX_CLASSES, MAX_FRAMES = PSDS_MAX_CLASSES, PSDS_MAX_FRAMES

    def __init__(self, n_classes: int, scenario=1, thresholds=None, sr=16000, hop=256, e_max=100.0):
        super().__init__(n_classes)
        if isinstance(scenario, dict):
            unknown = set(scenario) - {'dtc_pct', 'gtc_pct', 'cttc_pct', 'alpha_ct', 'alpha_st'}
            if unknown or not {'dtc_pct', 'gtc_pct'} <= set(scenario):
                raise ValueError(f"Psds: a scenario dict holds dtc_pct, gtc_pct and optionally cttc_pct, alpha_ct, alpha_st, got {scenario!r}")
            sc = dict(cttc_pct=None, alpha_ct=0.0, alpha_st=1.0)
            sc.update(scenario)
        elif scenario in PSDS_SCENARIOS and not isinstance(scenario, bool):
            sc = dict(PSDS_SCENARIOS[scenario])
        else:
            raise ValueError(f"Psds: scenario 1, 2 or a dict, got {scenario!r}")
        self.thresholds, self.dtc_pct, self.gtc_pct, self.cttc_pct = \
            check_psds_params(thresholds, sc['dtc_pct'], sc['gtc_pct'], sc['cttc_pct'])
        self.alpha_ct, self.alpha_st = float(sc['alpha_ct']), float(sc['alpha_st'])
        if int(hop) != hop or hop < 1 or not sr > 0 or not (e_max > 0 and np.isfinite(e_max)):
            raise ValueError(f"Psds: hop {hop!r} (an integer >= 1), sr {sr!r} (> 0), e_max {e_max!r} (> 0)")
        self.hop, self.sr, self.e_max = int(hop), sr, float(e_max)
        self._levels = (N.C.c_float * len(self.thresholds))(*self.thresholds)
        self._shape = (len(self.thresholds) + 1, self.n_classes, self.n_classes + 2)

    def _host(self, y_true, y_pred):
        return psds_counts_host(y_true, y_pred, self.thresholds, self.dtc_pct, self.gtc_pct, self.cttc_pct)

    def _workspace_bytes(self, b, t, k):
        return _workspace_query("iris_psds_workspace_bytes", b, t, k, len(self.thresholds))

    def _launch(self, yt, yp, ws, st, stream):
        b, t, k = yp.shape
        N.check(N.lib().iris_psds_counts(yt.data_ptr(), yp.data_ptr(), b, t, k, self._levels, len(self.thresholds), self.dtc_pct,
                                         self.gtc_pct, self.cttc_pct or 0, ws.data_ptr(), ws.numel() * 8, st.data_ptr(), stream),
                "iris_psds_counts")

    def metrics(self, counts) -> dict:
        return psds_metrics(counts, self.thresholds, self.hop, self.sr, self.alpha_ct, self.alpha_st, self.e_max)


PSDS_NAMES = ('psds',)   # what a compiled psds() adds to a row; `fit` MAXIMISES such a monitor


def psds(scenario=1, thresholds=None, sr=16000, hop=256, e_max=100.0):
    """A metric for `compile(metrics=[...])`: the polyphonic sound detection score of the validation pass under DCASE scenario
    1 or 2 (or a criteria dict, see `Psds`), from on-device integer counts at 50 thresholds (`fit` logs val_psds).  `hop` is the
    hop of the frames the metric sees - the model's output frames - in samples."""
    return _CompiledCounts('psds', Psds, PSDS_NAMES, lambda m: [m['psds']], scenario=scenario, thresholds=thresholds, sr=sr,
                           hop=hop, e_max=e_max)


VAL_MAXIMISED = tuple(n for n in CURVE_NAMES + SED_NAMES + PSDS_NAMES if n != 'seg_er')   # larger is better, but for the one error rate


def _is_cos(m):
    return m is cos_sim or m is _cos_sim_metric


def metric_name(m) -> str:
    return 'cos_sim' if _is_cos(m) else getattr(m, '__name__', type(m).__name__)


class MetricSet:
    """A compiled metric list (`CustomModel.compile(metrics=...)`).  Any of er_score / f1_score / cos_sim are served by ONE
    iris_event_metrics launch per batch on a GPU (at most one of each kind; other callables are called as they are).  Each call
    adds to the epoch accumulator of its phase ('train' / 'val'): fp64 [5] = sum er, sum cos, sum f1, clips, batches - zeroed by
    `reset`, read once per epoch by `fit` (Keras' means: per-clip metrics weighted by clips, the scalar F1 by batches).
    The count metrics score_curves(), sed_eval() and psds() (at most one of each) are fed in the 'val' phase only - the launches
    of their counters: one, two and two more - and read with `val_values`; a 'train'-phase call launches nothing for them, so the
    captured training step is what it is without them.  `counted` holds them in the fixed order curves, sed, psds, whatever their
    order in the list: the order of their row entries, and the order in which every rank all-reduces their counts."""

    def __init__(self, metrics):
        self.metrics = list(metrics)
        self.er = next((m for m in self.metrics if isinstance(m, _ErScore)), None)
        self.f1 = next((m for m in self.metrics if isinstance(m, _F1Score)), None)
        self.cos = any(_is_cos(m) for m in self.metrics)
        compiled = [m for m in self.metrics if isinstance(m, _CompiledCounts)]
        self.counted: List[_CompiledCounts] = []
        for attr, kind in (('curves', 'score_curves'), ('sed', 'sed_eval'), ('psds', 'psds')):
            same = [m for m in compiled if m.__name__ == kind]
            if len(same) > 1:
                raise ValueError(f"MetricSet: at most one {kind}() in a metric list")
            setattr(self, attr, same[0] if same else None)
            self.counted += same
        fused = {id(self.er), id(self.f1)} | {id(m) for m in compiled}
        self.others = [m for m in self.metrics if id(m) not in fused and not _is_cos(m)]
        self.names = [metric_name(m) for m in self.metrics]
        dup = sorted({n for n in self.names if self.names.count(n) > 1})
        if dup:   # (one result per name: a second er_score or f1_score would overwrite the first in the step's outputs)
            raise ValueError(f"MetricSet: metric names must be unique, {dup} appear more than once")
        self.accums: Dict[tuple, torch.Tensor] = {}
        self.workspace = _Workspace()

    def accum(self, device, phase: str) -> torch.Tensor:
        key = (torch.device(device), phase)
        if key not in self.accums:
            self.accums[key] = torch.zeros(5, dtype=torch.float64, device=key[0])
        return self.accums[key]

    def state_tensors(self) -> List[torch.Tensor]:
        """Everything a call advances (F1 counts, accumulators): GraphedTrainStep saves / restores them around its warm-up."""
        return list(self.accums.values()) + (list(self.f1.states.values()) if self.f1 is not None else [])

    def reset(self, phase: Optional[str] = None) -> None:
        for (_, ph), a in self.accums.items():
            if phase is None or ph == phase:
                a.zero_()
        if phase in (None, 'val'):
            for m in self.counted:
                m.reset()

    @torch.no_grad()
    def __call__(self, y_true, y_pred, phase: str = 'train') -> Dict[str, torch.Tensor]:
        y_true, y_pred = _first(y_true), _first(y_pred).detach()
        dev = y_pred.device
        acc = self.accum(dev, phase)
        fused = self.er is not None or self.f1 is not None or self.cos
        res: Dict[str, torch.Tensor] = {}
        if fused and y_pred.is_cuda:
            er = self.er or _ErScore(0.5, False)
            r = event_metrics(y_true, y_pred, er.threshold, er.pool, want_cos=self.cos,
                              f1_state=self.f1.state(dev) if self.f1 is not None else None,
                              f1_threshold=self.f1.threshold if self.f1 is not None else 0.5, accum=acc,
                              workspace=self.workspace)
            if self.er is not None:
                res['er'] = r['er']
            for key in ('cos_sim', 'f1_score'):
                if key in r:
                    res[key] = r[key]
        elif fused:
            er = cs = f1 = None
            if self.er is not None:
                er = res['er'] = self.er(y_true, y_pred)
            if self.cos:
                cs = res['cos_sim'] = cos_sim(y_true, y_pred)
            if self.f1 is not None:
                f1 = res['f1_score'] = self.f1(y_true, y_pred)
            b = y_pred.shape[0]
            acc += torch.stack([er.double().sum() if er is not None else acc.new_zeros(()),
                                cs.double().sum() if cs is not None else acc.new_zeros(()),
                                f1.double() if f1 is not None else acc.new_zeros(()),
                                acc.new_tensor(float(b)), acc.new_tensor(1.0)])
        for m in self.others:
            res[metric_name(m)] = m(y_true, y_pred)
        if phase == 'val':   # the counters' launches on a GPU; the train phase launches nothing
            for m in self.counted:
                m.update(y_true, y_pred)
        return {n: res[n] for n in self.names if n in res}

    @staticmethod
    def _rows(compiled, prefix: str, all_reduce: bool) -> Dict[str, float]:
        out: Dict[str, float] = {}
        for m in compiled:
            if m is not None:
                out.update(m.values(prefix, all_reduce))
        return out

    def val_values(self, prefix: str = '', all_reduce: bool = False) -> Dict[str, float]:
        """The row entries of the compiled count metrics (`_CompiledCounts.values`, in the order of `counted`); {} without any."""
        return self._rows(self.counted, prefix, all_reduce)

    def curve_values(self, prefix: str = '', all_reduce: bool = False) -> Dict[str, float]:
        """`val_values` of the compiled score_curves() alone."""
        return self._rows([self.curves], prefix, all_reduce)

    def sed_values(self, prefix: str = '', all_reduce: bool = False) -> Dict[str, float]:
        """`val_values` of the compiled sed_eval() alone."""
        return self._rows([self.sed], prefix, all_reduce)

    def psds_values(self, prefix: str = '', all_reduce: bool = False) -> Dict[str, float]:
        """`val_values` of the compiled psds() alone."""
        return self._rows([self.psds], prefix, all_reduce)

    def epoch_values(self, sums: torch.Tensor, prefix: str = '') -> Dict[str, float]:
        """Row entries from an accumulator's (possibly all-reduced) host values."""
        s = [float(v) for v in sums]
        out = {}
        for n in self.names:
            if n == 'er' and self.er is not None:
                out[prefix + n] = s[0] / s[3] if s[3] else float('nan')
            elif n == 'cos_sim' and self.cos:
                out[prefix + n] = s[1] / s[3] if s[3] else float('nan')
            elif n == 'f1_score' and self.f1 is not None:
                out[prefix + n] = s[2] / s[4] if s[4] else float('nan')
        return out


# ---------------------------------------------------------------------------
# scoring helpers (host; once per file)                        metrics.py:95-214
# ---------------------------------------------------------------------------
class Challenge_Metric:
    def __init__(self, sr=16000, hop=256) -> None:
        self.sr = sr
        self.hop = hop

    def get_start_end_time(self, data):
        out = []
        for cls in self.get_start_end_frame(data):
            sec = np.round(cls * self.hop / self.sr).astype(np.int32)   # tf.round: half to even, as np.round
            out.append(np.unique(sec, axis=0) if len(sec) else sec)    # gather(unique(..., True)[1]): sorted unique rows
        return tuple(out)

    def get_start_end_frame(self, data):
        """[T, 3] frame decisions -> per class [n, 2] (first, last frame) of each event; an event still open at the end
        closes at the last frame (metrics.py:111-137)."""
        data = np.asarray(data.detach().cpu() if torch.is_tensor(data) else data)
        prev = np.concatenate([np.zeros([1, 3], data.dtype), data[:-1, :]], 0)
        diff = np.argwhere(prev != data)
        out = []
        for c in range(3):
            idx = diff[diff[:, 1] == c][:, 0].astype(np.int64)
            if idx.shape[0] % 2 != 0:
                idx = np.concatenate([idx, np.array([len(data)], np.int64)])
            idx = idx.reshape(-1, 2)
            out.append(np.stack([idx[:, 0], idx[:, 1] - 1], 1))
        return tuple(out)


def extract_middle(y_pred):
    """metrics.py:165-179: [B, T, K] binary -> [N, 3] int64 (clip, middle frame, class) in (clip, class, time) order."""
    y = np.asarray(y_pred.detach().cpu() if torch.is_tensor(y_pred) else y_pred)
    prev = np.pad(y, [[0, 0], [1, 0], [0, 0]])[:, :-1]
    nxt = np.pad(y, [[0, 0], [0, 1], [0, 0]])[:, 1:]
    starts = np.argwhere(np.clip(y - prev, 0, 1))
    ends = np.argwhere(np.clip(y - nxt, 0, 1))

    def order(a):
        a = a[np.argsort(a[:, -1], kind='stable')]
        return a[np.argsort(a[:, 0], kind='stable')]
    return ((order(starts) + order(ends)) / 2).astype(np.int64)


def get_er(gt, predict):
    """metrics.py:182-198: greedy matching - ground-truth events by start time, each takes the first remaining prediction of
    its class (by time) inside [start, end]; (N - 2 matched) / len(gt).  An empty gt raises ZeroDivisionError, as there."""
    gt = np.asarray(gt).reshape(-1, 3)
    pred = np.asarray(predict).reshape(-1, 2)
    pred = pred[np.argsort(pred[:, 1], kind='stable')]
    gt = gt[np.argsort(gt[:, 1], kind='stable')]
    n = len(pred) + len(gt)
    answer = 0
    for g in gt:
        for i, p in enumerate(pred):
            if g[1] <= p[1] <= g[2] and g[0] == p[0]:
                answer += 2
                pred = np.concatenate([pred[:i], pred[i + 1:]], 0)
                break
    return (n - answer) / len(gt)


def output_to_metric(hop, sr):
    """metrics.py:201-214: per class [n, 2] frame events -> [N, 2] int32 (class, int(((s + e) / 2) * hop / sr))."""
    def output_to_metric_(cls0, cls1, cls2):
        rows = []
        for c, cls in enumerate((cls0, cls1, cls2)):
            for item in np.asarray(cls).reshape(-1, 2):
                rows.append([c, int(((int(item[0]) + int(item[1])) / 2) * hop / sr)])
        return np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return output_to_metric_


# ---------------------------------------------------------------------------
# challenge score                                              metrics.py:14-87
# ---------------------------------------------------------------------------
def evaluate(config, model, overlap_hop=512, verbose: bool = False, *, wav_dir: str = '.',
             answer_path: str = 'sample_answer.json', device=None, curves: Optional["ScoreHistogram"] = None,
             sed: Optional["SedEval"] = None, psds: Optional["Psds"] = None):
    """Per-file ER of `model` on sorted(glob(wav_dir/*.wav)) against answer_path's 'task2_answer' (metrics.py:31-87): the
    frame decisions of inference.predict_frames (smoothed, >= 0.5), then get_start_end_frame -> output_to_metric -> get_er.
    `curves`: a ScoreHistogram that is also fed every file's frame posteriors (the smoothed probabilities, before the 0.5
    decision) against the `second2frame` labels of the file's answer; the decisions and the scores are what they are without it.
    `sed`: a SedEval (made for 3 classes at hop 256) fed the same two tensors, one [1, T, K] update per file.
    `psds`: a Psds (made for 3 classes at hop 256) likewise."""
    from . import data_utils as D
    from .inference import features_for_eval, predict_frames
    with open(answer_path) as f:
        answer_gt = json.load(f)['task2_answer']
    sr, hop = 16000, 256
    metric = Challenge_Metric()
    if device is None:
        device = next(model.parameters()).device if hasattr(model, 'parameters') else None
    final_score = []
    counters = [c for c in (curves, sed, psds) if c is not None]
    for path in sorted(glob(os.path.join(wav_dir, '*.wav'))):
        spec = D.load_wav(path, device)
        name = os.path.basename(path)[:-4]
        if not counters:
            preds = predict_frames(model, features_for_eval(spec, config), config, overlap_hop)
        else:
            from .eval import second2frame
            post = predict_frames(model, features_for_eval(spec, config), config, overlap_hop, threshold=False)
            labels = second2frame(answer_gt[name], post.shape[0], sr / hop).to(post.device)
            for counter in counters:
                counter.update(labels[None], post.to(torch.float32)[None])
            preds = (post >= 0.5).to(torch.float32)   # (predict_frames' own decision)
        cls0, cls1, cls2 = metric.get_start_end_frame(preds.cpu().numpy())
        predict = output_to_metric(hop, sr)(cls0, cls1, cls2)
        final_score.append(get_er(answer_gt[name], predict))
    if verbose:
        print('FINAL SCORE:', np.mean(final_score))
    return final_score


class eval_callback:
    """metrics.py:14-28: on epochs with epoch % 5 == 2, a copy of the model loaded from the checkpoint `name` is scored with
    `evaluate`; when its mean ER is not worse than the best so far the copy is saved as <name>_sample.pt.  Same
    `on_epoch_end(epoch, model)` shape as swa.SWA."""

    def __init__(self, config, name, **evaluate_kwargs):
        self.config, self.name, self.score = config, name, np.inf
        self.kwargs = evaluate_kwargs

    def on_epoch_end(self, epoch, model):
        if epoch % 5 != 2:
            return
        from .model import get_model
        ckpt = os.path.splitext(self.name)[0] + '.pt'
        dev = next(model.parameters()).device
        clone = get_model(self.config).to(dev)   # (tf.keras.models.clone_model + load_weights(NAME))
        if dev.type == 'cuda':
            clone = clone.to(memory_format=torch.channels_last)
        clone.load_state_dict(torch.load(ckpt, map_location=dev) if os.path.exists(ckpt) else model.state_dict())
        score = float(np.mean(evaluate(self.config, clone, verbose=True, **self.kwargs)))
        if score <= self.score:
            self.score = score
            torch.save(clone.state_dict(), os.path.splitext(self.name)[0] + '_sample.pt')
