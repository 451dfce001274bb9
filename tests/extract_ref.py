"""The float64 definition of event extraction that `transforms.extract_events`, `FrontendPlan.beamform` and the kernel of
k_beamform.h are held to - NumPy, complex arithmetic.

    spec [B, F, T, 4] = (re0, re1, im0, im1),  X0 = re0 + i im0,  X1 = re1 + i im1,  n_fft = 2 (F - 1)
    factors (a, b, c) per (sample, bin, block of `block` frames): whiten_ref.factors_ref, or a = b = 1, c = 0 in one block
    for event (sample, first, last) with delay tdoa, frame t in first .. last, block j = t // block, bin k:
        k outside [k_lo, k_hi), a == 0 or tdoa not finite:  Y = 0
        r = k tdoa / n_fft,  r -= rint(r),  e = cos(2 pi r) - i sin(2 pi r)
        s1 = b (e - c),  den = a^2 + |s1|^2,  g1 = b conj(s1) / den,  g0 = a^2 / den - g1 c,   Y = g0 X0 + g1 X1
"""
import numpy as np

import locate_ref as L
import whiten_ref as W

U = 2.0 ** -24
C_BEAM = 6     # the kernel's roundings per component, counted in csrc/k_beamform.h and DESIGN.md (K17)


def steering(f, tdoa):
    """e[k] = exp(-i 2 pi k tdoa / n_fft) for k < f, the phase reduced to |r| <= 1/2 turn first."""
    r = np.arange(f, dtype=np.float64) * np.float64(tdoa) / np.float64(2 * (f - 1))
    r = r - np.rint(r)
    return np.cos(2 * np.pi * r) - 1j * np.sin(2 * np.pi * r)


def coefficients(a, b, c, e):
    """(g0, g1) of Y = g0 X0 + g1 X1; arrays of one shape, a != 0."""
    s1 = b * (e - c)
    den = a ** 2 + np.abs(s1) ** 2
    g1 = b * np.conj(s1) / den
    return a ** 2 / den - g1 * c, g1


def beamform_ref(spec, events, tdoa, abc=None, block=None, k_lo=0, k_hi=None, with_mag=False):
    """-> the list of Y [F, T_e] complex128, one per event; with_mag also the list of A = |g0| |X0| + |g1| |X1| [F, T_e], the
    magnitude the kernel's bound C_BEAM u A is stated in (0 where Y is 0 by definition)."""
    x0, x1 = W.channels(spec)
    bsz, f, t = x0.shape
    k_hi = f if k_hi is None else k_hi
    if abc is None:
        abc, block = L.identity_factors(bsz, f), max(t, 1)
    else:
        block, _ = W.block_of(t, block)
    events = np.asarray(events, np.int64).reshape(-1, 3)
    tdoa = np.asarray(tdoa, np.float64).reshape(-1)
    assert len(tdoa) == len(events)
    ys, mags = [], []
    for (s, first, last), d in zip(events, tdoa):
        n = int(last - first + 1)
        y, mag = np.zeros((f, n), np.complex128), np.zeros((f, n))
        if np.isfinite(d):
            e = steering(f, d)
            for j, t0, t1 in L.segments(int(first), int(last), block):      # the frames of one block share (a, b, c)
                a, b, c = (v[s, :, j] for v in abc)
                ks = np.arange(k_lo, k_hi)
                ks = ks[a[ks] != 0]
                g0, g1 = (g[:, None] for g in coefficients(a[ks], b[ks], c[ks], e[ks]))
                z0, z1 = x0[s, ks, t0:t1 + 1], x1[s, ks, t0:t1 + 1]
                y[ks, t0 - first:t1 - first + 1] = g0 * z0 + g1 * z1
                mag[ks, t0 - first:t1 - first + 1] = np.abs(g0) * np.abs(z0) + np.abs(g1) * np.abs(z1)
        ys.append(y)
        mags.append(mag)
    return (ys, mags) if with_mag else ys


def worst_fraction(got, ref, mag):
    """got [F, T_e, 2] = (Re, Im) against ref [F, T_e] complex: max over real components of |got - ref| / (C_BEAM u A); <= 1
    passes.  Where A == 0 the value must be exactly 0: any difference there counts as infinite."""
    g = np.asarray(got, np.float64)
    err = np.maximum(np.abs(g[..., 0] - ref.real), np.abs(g[..., 1] - ref.imag))
    bound = C_BEAM * U * mag
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(frac.max()) if frac.size else 0.0


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def pack(x0, x1):
    return np.stack([x0.real, x1.real, x0.imag, x1.imag], axis=-1)[None]


def scene_parts(seed, f=257, t=512, interferer_delay=2.5, source_delay=-3.0, source_db=-10.0, noise_db=-20.0, frames=(100, 160)):
    """locate_ref.scene (the same draws in the same order) split into (source, interferer + sensor noise), float64
    [1, F, T, 4] each: their sum is the scene, and each can be passed through the weights of the sum."""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    v, g_n, g_s = cn(f, t), 10.0 ** (noise_db / 20.0), 10.0 ** (source_db / 20.0)
    n0, n1 = v + g_n * cn(f, t), L.delayed(v, interferer_delay) + g_n * cn(f, t)
    s = np.zeros((f, t), np.complex128)
    s[:, frames[0]:frames[1] + 1] = g_s * cn(f, frames[1] - frames[0] + 1)
    return pack(s, L.delayed(s, source_delay)), pack(n0, n1)


def db(x):
    return 10.0 * np.log10(x)


def gains(source, noise, y_source, y_noise, frames, k_lo):
    """(SINR gain in dB, source distortion in dB) over the event's frames and the bins k >= k_lo: the SINR at microphone 0
    before, that of the beamformer's output after (the source and the noise part passed through the SAME weights), and
    sum |Y_source - S0|^2 / sum |S0|^2 - a distortionless beamformer returns the source as microphone 0 hears it."""
    sl = (0, slice(k_lo, None), slice(frames[0], frames[1] + 1))
    s0, n0 = W.channels(source)[0][sl], W.channels(noise)[0][sl]
    ys, yn = y_source[k_lo:], y_noise[k_lo:]
    p = lambda z: float((np.abs(z) ** 2).sum())
    gain = db(p(ys) / p(yn)) - db(p(s0) / p(n0))
    return gain, db(max(p(ys - s0), 1e-300 * p(s0)) / p(s0))
