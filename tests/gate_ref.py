"""The activity gate (iris_activity_gate, include/iris_frontend.h) restated in float64 NumPy, run by run and sequentially, and
the inputs the tests share.

The energies of the kernel and of this file differ by the order of a sum of exact squares: about n 2^-53 relative.  The
decision E >= thr can therefore differ only on a frame whose energy lies that close to the threshold.  `near_threshold` names
the frames within 2^-40 thr - the only frames a comparison of masks may leave out - and the condition the tests rest on is
that on every input they name this set is EMPTY (asserted from this file alone in tests/test_gate_host.py, on a CPU), so
every mask comparison is an equality over all frames."""
import numpy as np

AMPS = (0.0, 1e-4, 0.01, 0.3)


def owner(length, hop):
    """owner(s) = min((s + hop // 2) // hop, T - 1) for s < length, T = 1 + length // hop."""
    return np.minimum((np.arange(length) + hop // 2) // hop, length // hop)


def frame_energy(x, hop):
    x = np.asarray(x)
    sq = (x.astype(np.float64) ** 2).sum(axis=0)
    return np.bincount(owner(x.shape[1], hop), weights=sq, minlength=1 + x.shape[1] // hop)


def threshold(E, range_db, floor):
    ok = E[~np.isnan(E)]
    P = ok.max() if ok.size else 0.0
    with np.errstate(invalid="ignore"):
        return max(P * 10.0 ** (-float(range_db) / 10.0), float(floor))


def runs(m):
    """[(value, first, one past last)] of the maximal runs of a boolean vector."""
    out, first = [], 0
    for t in range(1, len(m) + 1):
        if t == len(m) or m[t] != m[first]:
            out.append((bool(m[first]), first, t))
            first = t
    return out


def mask_steps(m0, min_gap, min_event, hang):
    T = len(m0)
    m1 = m0.copy()
    for value, a, b in runs(m0):
        if not value and b - a <= min_gap and a > 0 and b < T:   # a gap at the edge of the clip has a one on one side only
            m1[a:b] = True
    m2 = m1.copy()
    for value, a, b in runs(m1):
        if value and b - a < min_event:
            m2[a:b] = False
    m = np.zeros(T, bool)
    for value, a, b in runs(m2):
        if value:
            m[max(a - hang, 0):min(b + hang, T)] = True
    return m


def gate_ref(x, hop, range_db=40.0, floor=0.0, min_gap=12, min_event=6, hang=1):
    """(y, m, E, thr): the gated waveform, the mask (bool [T]), the energies (float64 [T]) and the threshold."""
    x = np.asarray(x, np.float32)
    E = frame_energy(x, hop)
    thr = threshold(E, range_db, floor)
    with np.errstate(invalid="ignore"):
        m0 = (E >= thr) & (E > 0)
    m = mask_steps(m0, int(min_gap), int(min_event), int(hang))
    y = np.where(m[owner(x.shape[1], hop)][None, :], x, np.float32(0.0))
    return y, m, E, thr


def near_threshold(E, thr):
    """The frames with |E - thr| <= 2^-40 thr.  A threshold of 0 (no energy anywhere: the decision is E > 0, and a sum of
    squares of floats is 0 only when every one is) or +inf (only +inf reaches it) leaves nothing to rounding."""
    if thr == 0.0 or not np.isfinite(thr):
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.abs(E - thr) <= 2.0 ** -40 * thr)


def build_input(chan, length, hop, seed, amps=AMPS, longest=8):
    """Gaussian segments of 1 .. `longest` frames at amplitudes drawn from `amps`; the segments meet at k hop + hop // 5 + 1,
    off the frames' own boundaries k hop - hop // 2."""
    rng = np.random.default_rng(seed)
    amp = np.empty(length, np.float32)
    pos = 0
    while pos < length:
        end = pos + int(rng.integers(1, longest + 1)) * hop + (hop // 5 + 1 if pos == 0 else 0)
        amp[pos:end] = amps[int(rng.integers(0, len(amps)))]
        pos = end
    return rng.standard_normal((chan, length)).astype(np.float32) * amp


# ---- the inputs of tests/test_gate_gpu.py: (name, x [C, L], hop, settings) ----
RAW_HOP, RAW_LENS = 64, (1, 31, 700, 960, 4133, 9001)
SETTINGS = (dict(range_db=40.0, floor=0.0, min_gap=3, min_event=4, hang=1),
            dict(range_db=20.0, floor=0.0, min_gap=0, min_event=1, hang=0),
            dict(range_db=40.0, floor=0.0, min_gap=12, min_event=6, hang=1),
            dict(range_db=60.0, floor=1e-3, min_gap=1, min_event=2, hang=3))
MANY, MANY_LEN, MANY_HOP = 70000, 3, 2
MANY_SETTINGS = dict(range_db=20.0, floor=0.0, min_gap=0, min_event=1, hang=0)
LABEL_HOP, LABEL_LENS = 256, (32000, 20011, 48000, 777)
DEFAULTS = dict(range_db=40.0, floor=0.0, min_gap=12, min_event=6, hang=1)
PLAIN = dict(range_db=40.0, floor=0.0, min_gap=0, min_event=1, hang=0)         # m = m0
# the long record: parameters beyond a 64-frame word (59 runs, the longest 198 frames; 3 runs, 210 active frames)
LONG_SETTINGS = (SETTINGS[0], dict(range_db=40.0, floor=0.0, min_gap=9, min_event=40, hang=3),
                 dict(range_db=20.0, floor=0.0, min_gap=10, min_event=66, hang=70))


def raw_waves(chan):
    return [build_input(chan, n, RAW_HOP, 100 * chan + i) for i, n in enumerate(RAW_LENS)]


def long_wave():
    """4,200 hops (4,201 frames) at hop 4: 66 mask words, more than the 4 waves of a workgroup take in one round."""
    return build_input(2, 16800, 4, 7)


def special_waves():
    """An all-zero record, one with a NaN sample and one with a +inf sample (hop 64, 40 frames)."""
    zero = np.zeros((2, 2560), np.float32)
    nan, inf = build_input(2, 2560, 64, 11), build_input(2, 2560, 64, 12)
    nan[1, 1000] = np.nan
    inf[0, 1500] = np.inf
    return [zero, nan, inf]


def many_buffer():
    """70,000 records of [1, 3] samples, back to back in one buffer: every third all zero, every third with a first frame 40 dB
    under its second."""
    buf = np.random.default_rng(5).standard_normal((MANY, 1, MANY_LEN)).astype(np.float32)
    buf[0::3] = 0.0
    buf[1::3, :, 0] *= np.float32(0.01)
    return buf


def many_ref(buf):
    """(E [n, 2], thr [n], m [n, 2]) of `many_buffer` under MANY_SETTINGS, all records at once: at hop 2 a record of three
    samples has the frames {0} and {1, 2}, and with min_gap 0, min_event 1 and hang 0 steps 3 - 5 change nothing, so m = m0.
    (tests/test_gate_host.py holds a sample of the records to `gate_ref`.)"""
    sq = buf[:, 0, :].astype(np.float64) ** 2
    E = np.stack([sq[:, 0], sq[:, 1] + sq[:, 2]], axis=1)
    thr = E.max(axis=1) * 10.0 ** (-MANY_SETTINGS["range_db"] / 10.0)
    return E, thr, (E >= thr[:, None]) & (E > 0)


def label_waves():
    """Stereo voices at hop 256 without the amplitude 0: every sample the gate keeps is non-zero."""
    return [build_input(2, n, LABEL_HOP, 40 + i, AMPS[1:], 40) for i, n in enumerate(LABEL_LENS)]


def gpu_inputs():
    """Every (name, x, hop, settings) a GPU test gates, the 70,000 records of `many_buffer` aside (`many_ref`)."""
    for chan in (1, 2):
        for k, settings in enumerate(SETTINGS):
            for x in raw_waves(chan):
                yield f"raw c{chan} s{k} L{x.shape[1]}", x, RAW_HOP, settings
    for k, settings in enumerate(LONG_SETTINGS):
        yield f"long s{k}", long_wave(), 4, settings
    for k, x in enumerate(special_waves()):
        yield f"special {k}", x, RAW_HOP, SETTINGS[0]
        yield f"special {k} plain", x, RAW_HOP, PLAIN
    for i, x in enumerate(label_waves()):
        yield f"label {i}", x, LABEL_HOP, DEFAULTS
