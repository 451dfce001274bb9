"""NumPy restatement of `iris_crop_windows` and `iris_crop_draw` (csrc/k_crop.h: training windows cut from labelled
recordings), written from their definitions in include/iris_frontend.h, on the oracle's Philox (as tests/filtaug_ref.py)."""
import numpy as np

from oracle.frontend_ref import philox4x32_10

DRAW_CROP = 8
_M32 = 0xFFFFFFFF


def crop_windows_ref(waves, event_tables, draws, hop, n_frame, n_classes):
    """(wav float32 [B, C, (n_frame - 1) * hop], y float32 [B, n_frame, n_classes]) for draws [B, 2] of (recording, first
    frame): sample s of a window is the recording's sample q * hop + s where that exists and 0 otherwise; y[f, k] counts the
    recording's events (class, start, end) with class == k and start <= q + f < end.  `waves`: [C, len_i] arrays holding
    exactly the samples that exist."""
    draws = np.asarray(draws)
    length = (n_frame - 1) * hop
    chan = int(np.asarray(waves[0]).shape[0])
    wav = np.zeros((len(draws), chan, length), np.float32)
    y = np.zeros((len(draws), n_frame, n_classes), np.float32)
    for b, (i, q) in enumerate(draws):
        w = np.asarray(waves[i], np.float32)
        piece = w[:, q * hop:q * hop + length]
        wav[b, :, :piece.shape[1]] = piece
        for k, start, end in np.asarray(event_tables[i], np.int64).reshape(-1, 3):
            for f in range(n_frame):
                if start <= q + f < end:
                    y[b, f, k] += 1
    return wav, y


def positions(lens, hop, n_frame):
    """(n_pos [n], prefix int64 [n + 1]): n_pos = max((len - L) // hop, 0) + 1 and its prefix sums."""
    length = (n_frame - 1) * hop
    n_pos = np.maximum((np.asarray(lens, np.int64) - length) // hop, 0) + 1
    return n_pos, np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int64)


def crop_draw_ref(seed, call, batch, prefix):
    """int32 [batch, 2] of (recording, first frame) of call number `call` (0 = the first) under `seed`: the 64-bit word
    x << 32 | y of philox(call lo, call hi, b * 64, DRAW_CROP; key = seed lo, hi), u = (word * total) >> 64, the recording
    with prefix[i] <= u < prefix[i + 1], q = u - prefix[i]."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    c0, c1 = call & _M32, (call >> 32) & _M32
    prefix = [int(p) for p in prefix]
    total = prefix[-1]
    out = np.zeros((batch, 2), np.int32)
    for b in range(batch):
        r = philox4x32_10(c0, c1, b * 64, DRAW_CROP, k0, k1)
        u = (((int(r[0]) << 32) | int(r[1])) * total) >> 64
        i = max(j for j in range(len(prefix) - 1) if prefix[j] <= u)
        out[b] = (i, u - prefix[i])
    return out
