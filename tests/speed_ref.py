"""Reference forms of speed perturbation (iris_speed_perturb), a helper beside the tests.

Speed perturbation of a waveform x [C, L] by rate > 0 (rate > 1 = faster and shorter): n = ceil(L / rate) samples and

    y[c, m] = sum_s x[c, s] * cut * g(cut * (s - m * rate)),      cut = 0.99 * min(1, 1 / rate),
    g(t)    = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,  x[c, s] = 0 outside [0, L)

with the position m * rate formed in float64: i0 = floor(m * rate), frac = m * rate - i0.  This is the Hann-windowed sinc of
torchaudio.functional.resample (width 6, rolloff 0.99) at a real-valued position; for a rational rate = o / n it is
`oracle.frontend_ref.resample_waveform(x, o, n)`.  rate == 1 returns the source itself.

`speed_ref`  : the definition in float64; also returns S[c, m] = cut * sum over the support of |x[c, s]|, the scale of the
               error rule |y - y_ref| <= K u S.
`yardstick32`: the same loop in NumPy float32 (position and frac from float64, everything after in float32, the taps by
               np.sin / np.cos directly, the sum in ascending s).  K is derived from its error, not from the kernel's."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
WIDTH = 6


def speed_len(length, rate):
    return int(math.ceil(float(length) / float(rate)))


def _grid(length, rate):
    """(n, i0 [n] int64, frac [n] float64, cut float64, H): output m sits at (double)m * rate; the taps of an output lie in
    s = i0 - H .. i0 + H + 1 with H = ceil(6 / cut)."""
    rate = float(rate)
    n = speed_len(length, rate)
    pos = np.arange(n, dtype=np.float64) * np.float64(rate)
    i0 = np.floor(pos)
    cut = 0.99 * min(1.0, 1.0 / rate)
    return n, i0.astype(np.int64), pos - i0, cut, int(math.ceil(WIDTH / cut))


def _windows(x, i0, h):
    """x[c, i0[m] + k] for k = -h .. h + 1, zeros outside [0, L): [C, n, 2h + 2]; the source is read only where it exists, so
    a rate far above L costs no memory."""
    c, length = x.shape
    k = np.arange(-h, h + 2, dtype=np.int64)
    idx = i0[:, None] + k[None, :]
    ok = (idx >= 0) & (idx < length)
    win = x[:, np.clip(idx, 0, length - 1)]
    return np.where(ok[None], win, 0), k


def speed_ref(x, rate, chunk=1 << 16):
    """(y [C, n] float64, S [C, n] float64) by the definition, in float64."""
    x = np.asarray(x, np.float64)
    if float(rate) == 1.0:
        return x.copy(), np.abs(x)
    n, i0, frac, cut, h = _grid(x.shape[1], rate)
    h = min(h, x.shape[1] + 1)   # beyond the source on both sides there are only zeros
    y, s_abs = np.empty((x.shape[0], n)), np.empty((x.shape[0], n))
    for a in range(0, n, chunk):
        win, k = _windows(x, i0[a:a + chunk], h)
        t = cut * (k[None, :].astype(np.float64) - frac[a:a + chunk, None])
        inside = np.abs(t) < WIDTH
        pt = np.pi * t
        sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
        taps = np.where(inside, cut * sinc * np.cos(pt / (2 * WIDTH)) ** 2, 0.0)
        y[:, a:a + chunk] = np.einsum("cmk,mk->cm", win, taps)
        s_abs[:, a:a + chunk] = cut * np.einsum("cmk,mk->cm", np.abs(win), inside.astype(np.float64))
    return y, s_abs


def yardstick32(x, rate, chunk=1 << 16):
    """y [C, n] float32: the definition with every operation after the float64 position rounded to float32."""
    x = np.asarray(x, F32)
    if float(rate) == 1.0:
        return x.copy()
    n, i0, frac, cut, h = _grid(x.shape[1], rate)
    h = min(h, x.shape[1] + 1)
    cut32, pi32, six = F32(cut), F32(np.pi), F32(WIDTH)
    y = np.empty((x.shape[0], n), F32)
    for a in range(0, n, chunk):
        win, k = _windows(x, i0[a:a + chunk], h)
        d = (k[None, :].astype(F32) - frac[a:a + chunk, None].astype(F32)).astype(F32)
        t = (cut32 * d).astype(F32)
        pt = (pi32 * t).astype(F32)
        sinc = np.where(pt == 0, F32(1), (np.sin(pt).astype(F32) / np.where(pt == 0, F32(1), pt)).astype(F32)).astype(F32)
        cs = np.cos((pt / F32(2 * WIDTH)).astype(F32)).astype(F32)
        taps = np.where(np.abs(t) < six, ((cut32 * sinc).astype(F32) * (cs * cs).astype(F32)).astype(F32), F32(0)).astype(F32)
        acc = np.zeros((x.shape[0], win.shape[1]), F32)
        for j in range(taps.shape[1]):   # ascending s, every product and every addition rounded
            acc = (acc + (win[:, :, j] * taps[None, :, j]).astype(F32)).astype(F32)
        y[:, a:a + chunk] = acc
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
