"""NumPy restatement of `iris_filter_draw` (csrc/k_draw.h: the FilterAugment draws of a batch) on the oracle's Philox, and
the float64 gain definition it is held to."""
import numpy as np

from oracle.frontend_ref import draw_below, draw_unit, philox4x32_10

DRAW_FILTER = 7
_M32 = 0xFFFFFFFF


def gains64(bounds, db, n_mel, kind):
    """float64 [n_mel]: 10^(dB / 20) of the piecewise curve (the issue's definition), from boundaries and dB values."""
    bounds = np.asarray(bounds, np.int64)
    db = np.asarray(db, np.float64)
    m = np.arange(n_mel)
    j = np.searchsorted(bounds, m, side="right") - 1
    if kind == "step":
        curve = db[j]
    else:
        curve = db[j] + (db[j + 1] - db[j]) * (m - bounds[j]) / (bounds[j + 1] - bounds[j])
    return np.power(10.0, curve / 20.0)


def filter_draw_device(batch, n_mel, kind, n_lo, n_hi, min_bw, db_lo, db_hi, seed, state):
    """(bounds int32 [B, n_hi + 1], db float64 [B, n_hi + 1] - the exact value of db_lo + fl32(db_hi - db_lo) u -, n_band [B],
    gain float64 [B, n_mel] from the float32-rounded dB values); state = [call counter], advanced in place."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    c0, c1 = state[0] & _M32, (state[0] >> 32) & _M32
    bounds = np.full((batch, n_hi + 1), n_mel, np.int32)
    db = np.zeros((batch, n_hi + 1), np.float64)
    counts = np.zeros(batch, np.int32)
    gain = np.zeros((batch, n_mel), np.float64)
    span = np.float64(np.float32(db_hi) - np.float32(db_lo))
    for b in range(batch):
        n = n_lo + draw_below(philox4x32_10(c0, c1, b * 64, DRAW_FILTER, k0, k1)[0], n_hi - n_lo + 1)
        counts[b] = n
        slots = n_mel - n * min_bw + (n - 1)
        cuts = []
        for i in range(n - 1):
            v = draw_below(philox4x32_10(c0, c1, b * 64 + 1 + i // 4, DRAW_FILTER, k0, k1)[i % 4], slots - i)
            at = 0
            while at < len(cuts) and v >= cuts[at]:
                v += 1
                at += 1
            cuts.insert(at, v)
        bounds[b, 0] = 0
        for j in range(1, n):
            bounds[b, j] = j * min_bw + cuts[j - 1] - (j - 1)
        for i in range(n if kind == "step" else n + 1):
            u = draw_unit(philox4x32_10(c0, c1, b * 64 + 16 + i // 4, DRAW_FILTER, k0, k1)[i % 4])
            db[b, i] = np.float64(np.float32(db_lo)) + span * np.float64(u)
        db32 = db[b].astype(np.float32)
        gain[b] = gains64(bounds[b, :n + 1], db32[:n if kind == "step" else n + 1], n_mel, kind)
    state[0] += 1
    return bounds, db, counts, gain


def ulps(a32, ref64):
    """|a - ref| in units of the float32 spacing at ref."""
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(a32, np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
