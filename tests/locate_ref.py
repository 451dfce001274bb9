"""The float64 definition of event localisation that `transforms.locate_events`, `FrontendPlan.locate` and the kernels of
k_locate.h are held to - NumPy, complex arithmetic, whitening every frame (the kernels scale the moments instead).

    spec [B, F, T, 4] = (re0, re1, im0, im1),  X0 = re0 + i im0,  X1 = re1 + i im1,  n_fft = 2 (F - 1)
    factors (a, b, c) per (sample, bin, block of `block` frames): whiten_ref.factors_ref, or a = b = 1, c = 0 in one block
    an event (sample, first, last) is cut at block boundaries into segments j = first // block .. last // block; per
    (segment, bin k) with a != 0, over the segment's frames:
        z0 = a X0, z1 = b (X1 - c X0), p00 = sum |z0|^2, p11 = sum |z1|^2, p10 = sum z1 conj(z0)
    per lag n of -N .. N (steps of 1 / q sample): e = exp(-i 2 pi k n / (n_fft q)), s1 = b (e - c),
        term = (a^2 p00 + |s1|^2 p11 + 2 a Re(conj(s1) p10)) / (a^2 + |s1|^2)
    curve = the sum of the terms, n_terms = the sum over contributing (segment, bin) pairs of the segment's frame count
"""
import math

import numpy as np

import whiten_ref as W

U = 2.0 ** -53
C_TERM = 72    # the kernels' roundings per term besides the two sums, counted in csrc/k_locate.h and DESIGN.md (K16)


def identity_factors(b, f):
    return np.ones((b, f, 1)), np.ones((b, f, 1)), np.zeros((b, f, 1), np.complex128)


def factors_of(fac):
    """(a, b, c) float64 / complex from a stored [B, F, J, 4] = (a, b, Re c, Im c) array (the device's fp32 factors)."""
    g = np.asarray(fac, np.float64)
    return g[..., 0], g[..., 1], g[..., 2] + 1j * g[..., 3]


def segments(first, last, block):
    """[(j, t0, t1)] with t0 .. t1 inclusive."""
    return [(j, max(first, j * block), min(last, (j + 1) * block - 1)) for j in range(first // block, last // block + 1)]


def steer(f, n_lag, q):
    """e[k, n] = exp(-i 2 pi k n / (n_fft q)) for k < f and n = -n_lag .. n_lag, the phase reduced in integers first."""
    period = 2 * (f - 1) * q
    m = (np.arange(f)[:, None] * np.arange(-n_lag, n_lag + 1)[None, :]) % period
    m = np.where(2 * m > period, m - period, m)   # |m| <= period / 2: the phase's rounding stays below 4 u
    return np.exp(-2j * np.pi * m / period)


def segment_curve(x0, x1, abc, k_lo, k_hi, n_lag, q, with_mag=False):
    """One segment: x0, x1 [F, n] complex, abc = (a [F], b [F], c [F]) -> (curve [2 N + 1], n_terms[, magnitude [2 N + 1]])."""
    f, n = x0.shape
    a, b, c = abc
    ks = np.arange(k_lo, k_hi)
    ks = ks[a[ks] != 0]
    if ks.size == 0:
        z = np.zeros(2 * n_lag + 1)
        return (z, 0, z) if with_mag else (z, 0)
    a, b, c = a[ks, None], b[ks, None], c[ks, None]
    z0, z1 = a * x0[ks], b * (x1[ks] - c * x0[ks])
    p00, p11 = (np.abs(z0) ** 2).sum(-1, keepdims=True), (np.abs(z1) ** 2).sum(-1, keepdims=True)
    p10 = (z1 * np.conj(z0)).sum(-1, keepdims=True)
    e = steer(f, n_lag, q)[ks]
    s1 = b * (e - c)
    den = a ** 2 + np.abs(s1) ** 2
    term = (a ** 2 * p00 + np.abs(s1) ** 2 * p11 + 2 * a * (np.conj(s1) * p10).real) / den
    curve = np.array([math.fsum(col) for col in term.T])
    if not with_mag:
        return curve, int(ks.size) * n
    # the magnitude the error bound is stated in: nothing cancelled, neither in X1 - c X0 nor in e - c nor in the three parts
    y = np.abs(x1[ks]) + np.abs(c) * np.abs(x0[ks])
    m00, m11 = p00, (b ** 2) * (y ** 2).sum(-1, keepdims=True)
    m10 = a * b * (np.abs(x0[ks]) * y).sum(-1, keepdims=True)
    s1m = b * (1 + np.abs(c))
    mag = (a ** 2 * m00 + s1m ** 2 * m11 + 2 * a * s1m * m10) * (a ** 2 + s1m ** 2) / den ** 2
    return curve, int(ks.size) * n, mag.sum(0)


def locate_ref(spec, events, abc=None, block=None, k_lo=0, k_hi=None, n_lag=40, q=8, with_bound=False):
    """-> (curve [E, 2 N + 1] float64, n_terms [E] int64); with_bound also the bound [E, 2 N + 1] of |kernel - this|:
    (2 n_l + 2 n_s + 2 C_TERM) u sum A - the kernels' derived (n_l + n_s + C_TERM) u sum A and as much again for this
    restatement's own roundings - n_l = ceil(longest segment / 64), n_s = segments x ceil((k_hi - k_lo) / 64)."""
    x0, x1 = W.channels(spec)
    bsz, f, t = x0.shape
    k_hi = f if k_hi is None else k_hi
    if abc is None:
        abc, block = identity_factors(bsz, f), max(t, 1)
    else:
        block, _ = W.block_of(t, block)
    events = np.asarray(events, np.int64).reshape(-1, 3)
    lags = 2 * n_lag + 1
    curve, n_terms, bound = np.zeros((len(events), lags)), np.zeros(len(events), np.int64), np.zeros((len(events), lags))
    for i, (s, first, last) in enumerate(events):
        segs = segments(int(first), int(last), block)
        n_l = max((t1 - t0 + 1 + 63) // 64 for _, t0, t1 in segs)
        n_s = len(segs) * ((k_hi - k_lo + 63) // 64)
        mag = np.zeros(lags)
        for j, t0, t1 in segs:
            r = segment_curve(x0[s, :, t0:t1 + 1], x1[s, :, t0:t1 + 1], tuple(v[s, :, j] for v in abc), k_lo, k_hi, n_lag, q, True)
            curve[i] += r[0]
            n_terms[i] += r[1]
            mag += r[2]
        bound[i] = (2 * n_l + 2 * n_s + 2 * C_TERM) * U * mag
    return (curve, n_terms, bound) if with_bound else (curve, n_terms)


def worst_fraction(got, ref, bound):
    """max |got - ref| / bound: <= 1 passes.  Where the bound is 0 the value must be exactly the reference's."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(frac.max()) if frac.size else 0.0


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def delayed(sig, delay):
    """A [F, T] spectrum delayed by `delay` samples: the FFT phase exp(-i 2 pi k delay / n_fft), float64."""
    f = sig.shape[0]
    return sig * np.exp(-2j * np.pi * np.arange(f)[:, None] * delay / (2 * (f - 1)))


def scene(seed, f=513, t=512, interferer_delay=2.5, source_delay=-3.0, source_db=-10.0, noise_db=-20.0, frames=(100, 160)):
    """The issue's scene: a white interferer at `interferer_delay`, sensor noise `noise_db` under it, and a white source
    `source_db` under the interferer at `source_delay` in frames[0] .. frames[1] (inclusive).  float64 [1, F, T, 4]."""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    v, g_n, g_s = cn(f, t), 10.0 ** (noise_db / 20.0), 10.0 ** (source_db / 20.0)
    x0, x1 = v + g_n * cn(f, t), delayed(v, interferer_delay) + g_n * cn(f, t)
    s = np.zeros((f, t), np.complex128)
    s[:, frames[0]:frames[1] + 1] = g_s * cn(f, frames[1] - frames[0] + 1)
    x0, x1 = x0 + s, x1 + delayed(s, source_delay)
    return np.stack([x0.real, x1.real, x0.imag, x1.imag], axis=-1)[None]
