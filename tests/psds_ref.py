"""The intersection-based counts behind the polyphonic sound detection score (Bilen et al., ICASSP 2020) as plain loops over
explicit event lists and interval intersections: the reference of metrics.psds_counts_host and of iris_psds_counts.  It shares no
formulation with either (no prefix counts, no bit masks): every |d ∩ g| is min(ends) - max(starts) of two listed events.

Label activity is y_true >= 0.5f, predicted activity at threshold h is y_pred >= h in fp32, a NaN is inactive; events are the
maximal runs [s, e) of one (clip, class) row.  For a detection d of class c, I_k(d) = sum of |d ∩ g| over the events g of label
k of its clip.  d passes if 100 I_c(d) >= dtc_pct len(d); else it is a false positive, and a cross-trigger on every k != c with
100 I_k(d) >= cttc_pct len(d) (cttc_pct given).  A ground-truth event g is a true positive if 100 cov(g) >= gtc_pct len(g), cov(g)
the sum of |g ∩ d| over the PASSING detections d of its class and clip.

counts [n_thr + 1, K, K + 2] int64: plane j, row c: TP in column c, CT[c][k] in column k != c, FP in column K, detections in
column K + 1; plane n_thr: row k holds (n_gt[k], gt_frames[k]) in columns 0, 1, row 0 holds n_frames in column K (K = 1: 2)."""
import bisect

import numpy as np

F32 = np.float32


def events(active):
    """A row of booleans -> [(s, e)], e exclusive, in time order."""
    step = np.diff(np.concatenate(([0], np.asarray(active, np.int8), [0])))   # + 1 at a first frame, - 1 behind a last one
    return list(zip(np.flatnonzero(step == 1).tolist(), np.flatnonzero(step == -1).tolist()))


def overlap(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


def intersection(d, evs):
    """sum of |d ∩ g| over the events g of `evs` (in time order, disjoint): those that end at or before d begins are skipped
    by bisection, the walk stops at the first that begins at or after d ends."""
    i = bisect.bisect_right([g[1] for g in evs], d[0]) if len(evs) > 8 else 0
    total = 0
    while i < len(evs) and evs[i][0] < d[1]:
        total += overlap(d, evs[i])
        i += 1
    return total


def frames_column(k):
    return k if k > 1 else 2


def counts(y_true, y_pred, thresholds, dtc_pct=70, gtc_pct=70, cttc_pct=None):
    yt, yp = np.asarray(y_true, F32), np.asarray(y_pred, F32)
    b_n, t_n, k_n = yp.shape
    n = len(thresholds)
    out = np.zeros((n + 1, k_n, k_n + 2), np.int64)
    with np.errstate(invalid='ignore'):
        ref = yt >= F32(0.5)
        acts = [yp >= F32(h) for h in thresholds]
    for b in range(b_n):
        gts = [events(ref[b, :, k]) for k in range(k_n)]
        for k in range(k_n):
            out[n, k, 0] += len(gts[k])
            out[n, k, 1] += sum(e - s for s, e in gts[k])
        for j in range(n):
            for c in range(k_n):
                passing = []
                for d in events(acts[j][b, :, c]):
                    length = d[1] - d[0]
                    out[j, c, k_n + 1] += 1
                    if 100 * intersection(d, gts[c]) >= dtc_pct * length:
                        passing.append(d)
                        continue
                    out[j, c, k_n] += 1
                    if cttc_pct:
                        for k in range(k_n):
                            if k != c and 100 * intersection(d, gts[k]) >= cttc_pct * length:
                                out[j, c, k] += 1
                for g in gts[c]:
                    if 100 * intersection(g, passing) >= gtc_pct * (g[1] - g[0]):
                        out[j, c, c] += 1
    out[n, 0, frames_column(k_n)] += b_n * t_n
    return out
