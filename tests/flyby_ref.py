"""Reference forms of the fly-by augmentation (iris_flyby), a helper beside the tests.

A static source at (0, 0, z_s) above the ground plane z = 0 and an array whose centre moves as p(t) = p0 + v t (constant velocity,
no rotation), microphone c at p(t) + m_c, t = n / fs, fs = 16000, sound speed 343 m/s.  A voice x [C, L] becomes y [C, L], channel
c from row c of the source:

    y[c, n] = sum_p g_{c,p}(n) * sum_s x[c, s] * cut * g(cut * (s - pos_{c,p}(n)))
    g(t)    = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,      cut = 0.99 / (1 + |v| / 343),   x = 0 outside [0, L)

over at most two paths: p = 0 the direct sound (a_0 = 1), p = 1 the ground reflection from the image source (0, 0, -z_s) with
a_1 = beta (beta == 0: one path).  With d_{c,p}(n) the distance from microphone c at sample n to the (image) source and r_ref the
smallest direct distance over the microphones and t in [0, (L - 1) / fs]:

    pos_{c,p}(n) = n - (d_{c,p}(n) - r_ref) * (fs / 343),        g_{c,p}(n) = a_p * r_ref / d_{c,p}(n)

d, pos, i0 = floor(pos) and frac = pos - i0 are float64.  A record without paths (geometry None) is the identity.

`flyby_ref`  : the definition in float64; also returns S[c, n] = cut * sum_p |g_{c,p}(n)| * sum over the support of |x[c, s]|,
               the scale of the error rule |y - y_ref| <= K u S.
`yardstick32`: the same loop in NumPy float32 (position, frac and gain from float64, everything after in float32, the taps by
               np.sin / np.cos directly, the sum in ascending s, path 0 before path 1).  K is derived from ITS error over the
               inputs of tests/test_flyby_gpu.py (`gpu_cases`), not from the kernel's: K = ceil(2 x its worst ratio), the factor
               2 covering the device's sinf / cosf against NumPy's, as for `speed_ref` (K = 8 with the same window).

Measured (tests/test_flyby_host.py::test_yardstick_sets_k recomputes it): the yardstick's worst |y32 - y_ref| / (u S) over
`gpu_cases()` is YARDSTICK_WORST = 1.650 below (receding, L = 1023, C = 3, beta = 0), so K = ceil(3.30) = 4."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
WIDTH = 6
FS = 16000.0
SOUND = 343.0
SCALE = FS / SOUND            # samples per metre
YARDSTICK_WORST = 1.650       # worst rule ratio of `yardstick32` over `gpu_cases()`
K = 4                         # ceil(2 * YARDSTICK_WORST)


def geometry(p0, v, z_s=1.5, beta=0.0, mics=((0.0, 0.0, 0.0),)):
    return {"p0": np.asarray(p0, np.float64), "v": np.asarray(v, np.float64), "z_s": float(z_s), "beta": float(beta),
            "mics": np.asarray(mics, np.float64).reshape(-1, 3)}


def line_mics(channels, spacing=0.1):
    m = np.zeros((channels, 3))
    m[:, 0] = spacing * (np.arange(channels) - 0.5 * (channels - 1))
    return m


def distance(geom, c, z_src, t):
    """|p0 + v t + m_c - (0, 0, z_src)| for t an array of seconds, in float64."""
    q = geom["p0"] + geom["mics"][c]
    dx, dy, dz = q[0] + geom["v"][0] * t, q[1] + geom["v"][1] * t, (q[2] - z_src) + geom["v"][2] * t
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def r_ref_closed(geom, length):
    """The smallest direct distance over the microphones and t in [0, (length - 1) / fs]: per microphone d^2(t) is a quadratic
    in t, whose vertex is clamped to the interval."""
    v, t_end = geom["v"], (int(length) - 1) / FS
    vv = float(np.dot(v, v))
    best = math.inf
    for c in range(geom["mics"].shape[0]):
        q = geom["p0"] + geom["mics"][c] - np.array([0.0, 0.0, geom["z_s"]])
        t = 0.0 if vv == 0.0 else min(max(-float(np.dot(q, v)) / vv, 0.0), t_end)
        best = min(best, float(distance(geom, c, geom["z_s"], np.float64(t))))
    return best


def cut_of(geom):
    return 0.99 / (1.0 + math.sqrt(float(np.dot(geom["v"], geom["v"]))) / SOUND)


def paths(geom, length, r_ref=None):
    """(pos [C, P, L], gain [C, P, L], cut, H) in float64; P = 1 at beta == 0, else 2."""
    r_ref = r_ref_closed(geom, length) if r_ref is None else float(r_ref)
    n = np.arange(int(length), dtype=np.float64)
    t = n / FS
    amps = [1.0] if geom["beta"] == 0.0 else [1.0, geom["beta"]]
    chan = geom["mics"].shape[0]
    pos, gain = np.empty((chan, len(amps), int(length))), np.empty((chan, len(amps), int(length)))
    for c in range(chan):
        for p, a in enumerate(amps):
            d = distance(geom, c, geom["z_s"] if p == 0 else -geom["z_s"], t)
            pos[c, p] = n - (d - r_ref) * SCALE
            gain[c, p] = a * r_ref / d
    cut = cut_of(geom)
    return pos, gain, cut, int(math.ceil(WIDTH / cut))


def _windows(row, i0, h):
    """row[i0[n] + k] for k = -h .. h + 1, zeros outside [0, L): [n, 2h + 2]."""
    length = row.shape[0]
    k = np.arange(-h, h + 2, dtype=np.int64)
    idx = i0[:, None] + k[None, :]
    ok = (idx >= 0) & (idx < length)
    return np.where(ok, row[np.clip(idx, 0, length - 1)], 0), k


def flyby_ref(x, geom, r_ref=None):
    """(y [C, L] float64, S [C, L] float64) by the definition, in float64.  geom None: the identity.  r_ref: the reference
    distance, when it is not the geometry's own (the linearity test refers two geometries to one)."""
    x = np.asarray(x, np.float64)
    if geom is None:
        return x.copy(), np.abs(x)
    chan, length = x.shape
    assert geom["mics"].shape[0] == chan
    pos, gain, cut, h = paths(geom, length, r_ref)
    y, s_abs = np.zeros((chan, length)), np.zeros((chan, length))
    for c in range(chan):
        for p in range(pos.shape[1]):
            i0 = np.floor(pos[c, p])
            frac = pos[c, p] - i0
            i0 = np.clip(i0, -4.0e9, 4.0e9).astype(np.int64)
            win, k = _windows(x[c], i0, h)
            t = cut * (k[None, :].astype(np.float64) - frac[:, None])
            inside = np.abs(t) < WIDTH
            pt = np.pi * t
            sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
            taps = np.where(inside, cut * sinc * np.cos(pt / (2 * WIDTH)) ** 2, 0.0)
            y[c] += gain[c, p] * np.einsum("nk,nk->n", win, taps)
            s_abs[c] += cut * np.abs(gain[c, p]) * np.einsum("nk,nk->n", np.abs(win), inside.astype(np.float64))
    return y, s_abs


def yardstick32(x, geom, r_ref=None):
    """y [C, L] float32: the definition with every operation after the float64 position rounded to float32."""
    x = np.asarray(x, F32)
    if geom is None:
        return x.copy()
    chan, length = x.shape
    pos, gain, cut, h = paths(geom, length, r_ref)
    cut32, pi32, six = F32(cut), F32(np.pi), F32(WIDTH)
    y = np.empty((chan, length), F32)
    for c in range(chan):
        for p in range(pos.shape[1]):
            i0 = np.floor(pos[c, p])
            frac = (pos[c, p] - i0).astype(F32)
            i0 = np.clip(i0, -4.0e9, 4.0e9).astype(np.int64)
            win, k = _windows(x[c], i0, h)
            d = (k[None, :].astype(F32) - frac[:, None]).astype(F32)
            t = (cut32 * d).astype(F32)
            pt = (pi32 * t).astype(F32)
            sinc = np.where(pt == 0, F32(1), (np.sin(pt).astype(F32) / np.where(pt == 0, F32(1), pt)).astype(F32)).astype(F32)
            cs = np.cos((pt / F32(2 * WIDTH)).astype(F32)).astype(F32)
            taps = np.where(np.abs(t) < six, ((cut32 * sinc).astype(F32) * (cs * cs).astype(F32)).astype(F32), F32(0)).astype(F32)
            acc = np.zeros(length, F32)
            for j in range(taps.shape[1]):   # ascending s, every product and every addition rounded
                acc = (acc + (win[:, j] * taps[:, j]).astype(F32)).astype(F32)
            term = (gain[c, p].astype(F32) * acc).astype(F32)
            y[c] = term if p == 0 else (y[c] + term).astype(F32)   # path 0 before path 1
    return y


def make_wave(shape, seed):
    """Noise [C, L] float32 whose trailing fifth is silent (as padded voices are)."""
    w = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    w[:, shape[1] - shape[1] // 5:] = 0
    return w


def rule_ratio(out, ref, s_abs):
    """Worst |out - ref| / (u S) over the elements with S > 0; elements with S == 0 must be exactly 0."""
    err = np.abs(np.asarray(out, np.float64) - ref)
    ok = s_abs > 0
    assert np.all(np.asarray(out)[~ok] == 0), "an output whose whole support is zero input must be exactly 0"
    return float((err[ok] / (U * s_abs[ok])).max()) if ok.any() else 0.0


# the inputs of tests/test_flyby_gpu.py: a tile edge on either side (1023 / 1024 / 1025), a second tile (4099), sources shorter
# than the tap support (1, 7), an odd channel count
LENGTHS = (1, 7, 255, 1023, 1024, 1025, 4099)
CHANNELS = (1, 2, 3)
BETAS = (0.0, 0.6)
SHAPES = ("hover", "overhead", "receding")


def case_geometry(shape, channels, length, beta):
    """hover: a still array 12 m up, 6 m to the side.  overhead: 15 m/s straight over the source at 5 m altitude, closest
    approach mid-clip (the largest rate swing).  receding: 15 m/s away from a start 40 m off at 5 m altitude (the largest
    delay, and a distance at which a float32 position would be 2e-4 samples off)."""
    mics = line_mics(channels)
    if shape == "hover":
        return geometry((6.0, -2.0, 12.0), (0.0, 0.0, 0.0), 1.5, beta, mics)
    if shape == "overhead":
        t_c = 0.5 * (length - 1) / FS
        return geometry((-15.0 * t_c, 0.0, 5.0), (15.0, 0.0, 0.0), 1.5, beta, mics)
    if shape == "receding":
        return geometry((40.0, 0.0, 5.0), (15.0 * 0.8, 15.0 * 0.6, 0.0), 1.5, beta, mics)
    raise ValueError(shape)


def gpu_cases():
    """[(name, x [C, L] float32, geometry)] - every length x channel count x flight x beta, one seed each."""
    cases = []
    for length in LENGTHS:
        for chan in CHANNELS:
            for shape in SHAPES:
                for beta in BETAS:
                    seed = 1000 + len(cases)
                    x = make_wave((chan, length), seed) if length > 1 else np.full((chan, 1), 0.7, F32)
                    cases.append((f"{shape} L={length} C={chan} beta={beta}", x, case_geometry(shape, chan, length, beta)))
    return cases
