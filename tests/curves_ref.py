"""The definitions behind metrics.curve_metrics / ScoreHistogram, from scratch and WITHOUT a histogram: the bin rule per element
in NumPy float32, ROC-AUC by counting (positive, negative) pairs, average precision and the best F1 by sweeping thresholds over
the sorted quantised scores.  Everything is exact integer / rational arithmetic until the one final division (fractions), so
this side carries no rounding of its own beyond that of a correctly rounded quotient or a sum of K <= bins such terms."""
from fractions import Fraction

import numpy as np


def quantise(p, bins):
    """Slot of every prediction: min(bins - 1, max(0, floor(p * bins))) in float32, `bins` for NaN.  Element by element."""
    p = np.asarray(p, np.float32).reshape(-1)
    out = np.empty(p.shape, np.int64)
    fb = np.float32(bins)
    for i, v in enumerate(p):
        if v != v:
            out[i] = bins
            continue
        with np.errstate(over='ignore', invalid='ignore'):
            x = np.floor(np.float32(v * fb))
        if x == np.inf:
            out[i] = bins - 1
        elif x == -np.inf:
            out[i] = 0
        else:
            out[i] = min(bins - 1, max(0, int(x)))
    return out


def labels(y):
    """y_true >= 0.5 in float32; NaN is negative."""
    y = np.asarray(y, np.float32).reshape(-1)
    return np.array([bool(v >= np.float32(0.5)) for v in y])


def counts(y_true, y_pred, bins):
    """[K, 2, bins + 1] by a plain loop over the elements of [..., K] arrays (the thing the kernel and the torch path must equal)."""
    y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    k = y_pred.shape[-1]
    out = np.zeros((k, 2, bins + 1), np.int64)
    q = quantise(y_pred, bins).reshape(-1, k)
    lab = labels(y_true).reshape(-1, k)
    for c in range(k):
        for s, pos in zip(q[:, c], lab[:, c]):
            out[c, int(pos), s] += 1
    return out


def class_metrics(y_true, y_pred, bins):
    """One class: y_true, y_pred flat.  NaN predictions are dropped.  Returns a dict of auroc, ap, best_f1, best_threshold, ece
    (floats, NaN where undefined) and n_pos, n_neg, n_nan."""
    q = quantise(y_pred, bins)
    lab = labels(y_true)
    keep = q < bins
    n_nan = int((~keep).sum())
    q, lab = q[keep], lab[keep]
    pos, neg = np.sort(q[lab]), np.sort(q[~lab])
    n_pos, n_neg = len(pos), len(neg)
    nan = float('nan')
    out = {'n_pos': n_pos, 'n_neg': n_neg, 'n_nan': n_nan}
    # ROC-AUC: pairs (positive, negative) with the positive ranked higher count 1, ties 1/2 - counted, in twice-units
    if n_pos and n_neg:
        twice = 0
        for s in pos:
            twice += 2 * int(np.searchsorted(neg, s, 'left')) + int(np.searchsorted(neg, s, 'right') - np.searchsorted(neg, s, 'left'))
        out['auroc'] = float(Fraction(twice, 2 * n_pos * n_neg))
    else:
        out['auroc'] = nan
    # thresholds: the distinct quantised scores, descending (sklearn's precision_recall_curve on these scores)
    if n_pos:
        ap = Fraction(0)
        best, best_slot = Fraction(-1), None
        prev_tp = 0
        for s in sorted(set(q.tolist()), reverse=True):
            tp = int((pos >= s).sum())
            fp = int((neg >= s).sum())
            ap += Fraction(tp - prev_tp, n_pos) * Fraction(tp, tp + fp)
            prev_tp = tp
        # best F1 over EVERY threshold b / bins (not only the occupied ones): ties take the smallest b
        for b in range(bins):
            tp = int((pos >= b).sum())
            fp = int((neg >= b).sum())
            f1 = Fraction(2 * tp, 2 * tp + fp + (n_pos - tp))
            if f1 > best:
                best, best_slot = f1, b
        out['ap'] = float(ap)
        out['best_f1'] = float(best)
        out['best_threshold'] = best_slot / bins
    else:
        out['ap'] = out['best_f1'] = out['best_threshold'] = nan
    n = n_pos + n_neg
    if n:
        ece = Fraction(0)
        for s in set(q.tolist()):
            nb = int((q == s).sum())
            pb = int((pos == s).sum())
            ece += Fraction(nb, n) * abs(Fraction(pb, nb) - Fraction(2 * s + 1, 2 * bins))
        out['ece'] = float(ece)
    else:
        out['ece'] = nan
    return out


def _nanmean(v):
    v = [x for x in v if x == x]
    return sum(v) / len(v) if v else float('nan')


def metrics(y_true, y_pred, bins):
    """[..., K] arrays -> {'per_class': {name: [K]}, 'auc', 'map', 'best_f1'} (macro means over the defined classes)."""
    y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    k = y_pred.shape[-1]
    rows = [class_metrics(y_true.reshape(-1, k)[:, c], y_pred.reshape(-1, k)[:, c], bins) for c in range(k)]
    per = {n: [r[n] for r in rows] for n in rows[0]}
    return {'per_class': per, 'auc': _nanmean(per['auroc']), 'map': _nanmean(per['ap']), 'best_f1': _nanmean(per['best_f1'])}
