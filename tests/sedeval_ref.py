"""The definition of the segment- and event-based detection counts (Mesaros, Heittola & Virtanen 2016, as written out for
metrics.SedEval / iris_sed_counts), as plain Python loops over rows, frames and events: no vectorisation, nothing shared with
the product code.  Everything else is compared with `counts` for EQUALITY."""
import numpy as np

F32 = np.float32


def params(sr=16000, hop=256, segment=1.0, collar=0.2, offset_pct=50):
    return int(hop), int(round(segment * sr)), int(round(collar * sr)), int(offset_pct)


def active(value, level):
    """value >= level in fp32; a NaN is inactive."""
    value, level = F32(value), F32(level)
    if value != value:
        return False
    return bool(value >= level)


def runs(row):
    """Maximal runs [s, e] of True in a list of booleans; a run open at the end closes at the last frame."""
    out, start = [], None
    for f, a in enumerate(row):
        if a and start is None:
            start = f
        if not a and start is not None:
            out.append((start, f - 1))
            start = None
    if start is not None:
        out.append((start, len(row) - 1))
    return out


def may_match(p, r, hop, collar_samples, offset_pct):
    on_p, off_p = p[0] * hop, (p[1] + 1) * hop
    on_r, off_r = r[0] * hop, (r[1] + 1) * hop
    len_r = (r[1] + 1 - r[0]) * hop
    return abs(on_p - on_r) <= collar_samples and 100 * abs(off_p - off_r) <= max(100 * collar_samples, offset_pct * len_r)


def greedy_matches(ref, pred, hop, collar_samples, offset_pct):
    """Reference events by increasing onset; each takes the earliest predicted event that is still free and may match."""
    free = [True] * len(pred)
    n = 0
    for r in sorted(ref):
        for i, p in enumerate(pred):
            if free[i] and may_match(p, r, hop, collar_samples, offset_pct):
                free[i] = False
                n += 1
                break
    return n


def counts(y_true, y_pred, thresholds, sr=16000, hop=256, segment=1.0, collar=0.2, offset_pct=50):
    """int64 [n_thr, K + 1, 6]: rows k < K (seg_tp, seg_fp, seg_fn, ev_tp, ev_fp, ev_fn), row K (S, D, I, n_segments, 0, 0)."""
    hop, seg_samples, collar_samples, offset_pct = params(sr, hop, segment, collar, offset_pct)
    y_true, y_pred = np.asarray(y_true, F32), np.asarray(y_pred, F32)
    n_b, n_t, n_k = y_true.shape
    out = np.zeros((len(thresholds), n_k + 1, 6), np.int64)
    n_seg = ((n_t - 1) * hop) // seg_samples + 1
    for j, h in enumerate(thresholds):
        for b in range(n_b):
            seg_ref = [[False] * n_k for _ in range(n_seg)]
            seg_pred = [[False] * n_k for _ in range(n_seg)]
            for k in range(n_k):
                ref_row = [active(y_true[b, f, k], 0.5) for f in range(n_t)]
                pred_row = [active(y_pred[b, f, k], h) for f in range(n_t)]
                for f in range(n_t):
                    s = (f * hop) // seg_samples
                    seg_ref[s][k] = seg_ref[s][k] or ref_row[f]
                    seg_pred[s][k] = seg_pred[s][k] or pred_row[f]
                ref_ev, pred_ev = runs(ref_row), runs(pred_row)
                tp = greedy_matches(ref_ev, pred_ev, hop, collar_samples, offset_pct)
                out[j, k, 3] += tp
                out[j, k, 4] += len(pred_ev) - tp
                out[j, k, 5] += len(ref_ev) - tp
            for s in range(n_seg):
                n_fn = n_fp = 0
                for k in range(n_k):
                    r, p = seg_ref[s][k], seg_pred[s][k]
                    out[j, k, 0] += 1 if r and p else 0
                    out[j, k, 1] += 1 if p and not r else 0
                    out[j, k, 2] += 1 if r and not p else 0
                    n_fn += 1 if r and not p else 0
                    n_fp += 1 if p and not r else 0
                out[j, n_k, 0] += min(n_fn, n_fp)
                out[j, n_k, 1] += max(0, n_fn - n_fp)
                out[j, n_k, 2] += max(0, n_fp - n_fn)
                out[j, n_k, 3] += 1
    return out
