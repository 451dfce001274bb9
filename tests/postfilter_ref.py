"""The float64 definition of the Wiener post-filter that `transforms.extract_events(postfilter=)`, `FrontendPlan.postfilter` and
the kernel of k_postfilter.h are held to - NumPy, frame by frame, written independently of the host code.

    Y [F, T_e] the beamformer's output over the (widened) event's frames (extract_ref.beamform_ref / track_ref's per-frame
    form), (a, b, c) the factors of noise="quiet" (quiet_ref.factors_ref) made with `loading`, one delay per frame.
    for bin k in [k_lo, k_hi), frame t, block j = t // block, e = steering(delay of t)[k]:
        s1 = b (e - c),  den = a^2 + |s1|^2,  (g0, g1) = extract_ref.coefficients
        S = 1/a^2 + |c|^2/a^2 + 1/b^2,  d = loading S / (2 (1 + loading))
        phi = max(1/den - d (|g0|^2 + |g1|^2), PHI_FLOOR / den)
        gamma = |Y|^2 / phi;  gamma = 0 where a == 0 or the delay is not finite
    along t, p = 1 before the first frame:
        xi = alpha p + (1 - alpha) max(gamma - 1, 0),  G = max(xi / (1 + xi), g_min),  p = G^2 gamma,  Z = G Y
    bins outside [k_lo, k_hi): Z = 0.
"""
import numpy as np

import extract_ref as X
import quiet_ref as Q
import whiten_ref as W

U = 2.0 ** -24
C_POST = 3        # fl32(G), the product, one spare (csrc/k_postfilter.h)
PHI_FLOOR = 1e-3


def noise_power(a, b, c, e, loading):
    """(phi, 1 / den) for arrays of one shape, a != 0: the beamformer's output noise power w^H R w, and the loaded form
    w^H (R + dI) w it is corrected from."""
    g0, g1 = X.coefficients(a, b, c, e)
    den = a ** 2 + np.abs(b * (e - c)) ** 2
    trace = 1 / a ** 2 + np.abs(c) ** 2 / a ** 2 + 1 / b ** 2
    d = loading * trace / (2 * (1 + loading))
    return np.maximum(1 / den - d * (np.abs(g0) ** 2 + np.abs(g1) ** 2), PHI_FLOOR / den), 1 / den


def as_complex(y):
    y = np.asarray(y)
    return y.astype(np.complex128) if np.iscomplexobj(y) else y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


def frame_delays(events, tdoa, per_frame):
    """One float64 array of delays per event, a delay per frame."""
    events = np.asarray(events, np.int64).reshape(-1, 3)
    tdoa = np.asarray(tdoa, np.float64).reshape(-1)
    n = events[:, 2] - events[:, 1] + 1
    if per_frame:
        assert len(tdoa) == n.sum()
        return np.split(tdoa, np.cumsum(n)[:-1])
    assert len(tdoa) == len(events)
    return [np.full(k, d) for k, d in zip(n, tdoa)]


def postfilter_ref(slabs, events, tdoa, abc, block, loading, k_lo, k_hi, alpha, g_min, per_frame=False, n_frames=None):
    """slabs: per event [F, T_e] complex or [F, T_e, 2] -> (the list of Z [F, T_e] complex128, the list of G [F, T_e]).  abc =
    (a, b, c) [B, F, J]; block None: all frames (J == 1).  g_min: one floor per event, or one number."""
    a_all, b_all, c_all = abc
    f, n_blocks = a_all.shape[1], a_all.shape[2]
    k_hi = f if k_hi is None else k_hi
    events = np.asarray(events, np.int64).reshape(-1, 3)
    floors = np.broadcast_to(np.asarray(g_min, np.float64), (len(events),))
    zs, gs = [], []
    for y, (s, first, last), delays, floor in zip(slabs, events, frame_delays(events, tdoa, per_frame), floors):
        y = as_complex(y)
        n = int(last - first + 1)
        assert y.shape == (f, n)
        gamma = np.zeros((f, n))
        ks = np.arange(k_lo, k_hi)
        steer = {}
        for i in range(n):
            d = delays[i]
            j = 0 if block is None else (int(first) + i) // block
            if not np.isfinite(d) or j >= n_blocks:
                continue
            if d not in steer:
                steer[d] = X.steering(f, d)
            a, b, c = a_all[s, ks, j], b_all[s, ks, j], c_all[s, ks, j]
            on = a != 0
            phi, _ = noise_power(a[on], b[on], c[on], steer[d][ks][on], loading)
            gamma[ks[on], i] = (y[ks[on], i].real ** 2 + y[ks[on], i].imag ** 2) / phi
        g = np.zeros((f, n))
        p = np.ones(f)
        for i in range(n):
            xi = alpha * p + (1 - alpha) * np.maximum(gamma[:, i] - 1, 0)
            g[:, i] = np.maximum(xi / (1 + xi), floor)
            p = g[:, i] ** 2 * gamma[:, i]
        z = g * y
        z[:k_lo], z[k_hi:] = 0, 0
        zs.append(z)
        gs.append(g)
    return zs, gs


def worst_fraction(got, z, g, y):
    """got [F, T_e, 2] against z = G Y [F, T_e] complex: max over real components of |got - ref| / (C_POST u |G| |Y|); <= 1
    passes.  Where the bound is 0 the value must be exactly 0: any difference there counts as infinite."""
    got = np.asarray(got, np.float64)
    err = np.maximum(np.abs(got[..., 0] - z.real), np.abs(got[..., 1] - z.imag))
    bound = C_POST * U * np.abs(g) * np.abs(as_complex(y))
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(frac.max()) if frac.size else 0.0


# ---------------------------------------------------------------------------
# the demonstration: a source that is on in a quarter of its cells, under an interferer and sensor noise
# ---------------------------------------------------------------------------
# (F, T, block, event frames, context, k_lo, min_quiet, reach)
SCENES = {"large": (257, 512, None, (100, 355), 16, 8, 32, 1), "small": (33, 128, 32, (48, 79), 8, 2, 16, 1)}
TRUE_DELAY, LOADING, ALPHA, FLOOR_DB = -3.0, 1e-2, 0.98, -20.0
# What `demonstration` measures in float64: per (scene, source dB) = (SINR before, SINR after, total error before, total error
# after, context attenuation), all dB - the middle of the range over seeds 0, 1, 2.  The range itself: at most 0.13 dB on the
# large scene but for the context attenuation (0.95 dB), at most 1.51 dB on the small scene (the context at 0 dB; 1.42 dB the
# error after), so no seed is further than 0.76 dB from its constant and the margin of 1 dB is not widened.
# tests/test_postfilter_host.py asserts every seed within MARGIN_DB of these.
MEASURED = {("large", -10.0): (2.22, 12.24, -2.22, -5.42, -17.36), ("large", 0.0): (12.22, 20.17, -12.22, -11.37, -16.96),
            ("small", -10.0): (2.28, 11.94, -2.28, -5.25, -15.49), ("small", 0.0): (12.28, 20.38, -12.28, -11.54, -14.66)}
MARGIN_DB = 1.0


def phi_identity(which, seed):
    """(median over the bins k >= k_lo of predicted / measured noise power, the same for the loaded form 1 / den).  Predicted:
    phi of the blocks the event touches, averaged over their frames; measured: mean |Y_noise|^2 over the same frames - the
    frames whose covariance phi is a statement about (over the event's own frames alone, all out of sample for a covariance
    of 16 quiet frames a block, the small scene reads 0.89 - 0.91)."""
    f, t, _, frames, _, k_lo = SCENES[which][:6]
    source, noise = sparse_scene(which, seed, -10.0)
    abc, block = quiet_abc(source + noise, which)
    w0, w1 = (frames[0] // block) * block, min((frames[1] // block + 1) * block, t) - 1
    (yn,) = X.beamform_ref(noise, [[0, w0, w1]], [TRUE_DELAY], abc, block, k_lo)
    e, ks = X.steering(f, TRUE_DELAY), np.arange(k_lo, f)
    both = np.stack([noise_power(abc[0][0, ks, j], abc[1][0, ks, j], abc[2][0, ks, j], e[ks], LOADING)
                     for j in np.arange(w0, w1 + 1) // block], -1)          # [2, bins, frames]
    measured = (np.abs(yn[ks]) ** 2).mean(-1)
    return float(np.median(both[0].mean(-1) / measured)), float(np.median(both[1].mean(-1) / measured))


def sparse_scene(which, seed, source_db, on=True):
    """(source, noise) float64 [1, F, T, 4] of extract_ref.scene_parts with the scene's geometry; with `on` the source is kept
    in a random quarter of its (bin, frame) cells at twice the amplitude (the same mean power), the same cells in both
    channels."""
    f, t, _, frames = SCENES[which][:4]
    source, noise = X.scene_parts(seed, f, t, source_delay=TRUE_DELAY, source_db=source_db, frames=frames)
    if on:
        cells = np.random.default_rng(1000 + seed).random((f, t)) < 0.25
        source = source * (2.0 * cells)[None, :, :, None]
    return source, noise


def quiet_abc(spec, which, loading=LOADING):
    """The factors of noise="quiet" (guard 0) for the scene's one event, and its block."""
    _, t, block, frames, _, _, min_quiet, reach = SCENES[which]
    mask = Q.mask_ref([[0, frames[0], frames[1]]], [t], 0)
    ranges, quiet = Q.ranges_ref(mask, [t], block, min_quiet, reach)
    assert (quiet[0, frames[0] // W.block_of(t, block)[0]:frames[1] // W.block_of(t, block)[0] + 1] > 0).all()
    return Q.factors_ref(spec, mask, ranges, loading), W.block_of(t, block)[0]


def power(z):
    return float((np.abs(z) ** 2).sum())


def figures(source, y_source, y_noise, g, frames, wide, k_lo):
    """(SINR before, SINR after, total error before, total error after, context attenuation) in dB.  y_source, y_noise, g:
    [F, T_w] over the widened frames wide = (first, last); the SINRs and the errors over the event's own frames and the bins
    k >= k_lo - the source and the noise part through the SAME gains, the error against the source at microphone 0 - the
    attenuation sum |G Y|^2 / sum |Y|^2 over the context frames."""
    ev = slice(frames[0] - wide[0], frames[1] - wide[0] + 1)
    ctx = np.ones(g.shape[1], bool)
    ctx[ev] = False
    s0 = W.channels(source)[0][0, k_lo:, frames[0]:frames[1] + 1]
    ys, yn, ge = y_source[k_lo:, ev], y_noise[k_lo:, ev], g[k_lo:, ev]
    y = y_source + y_noise
    return (X.db(power(ys) / power(yn)), X.db(power(ge * ys) / power(ge * yn)),
            X.db(power(ys + yn - s0) / power(s0)), X.db(power(ge * (ys + yn) - s0) / power(s0)),
            X.db(power((g * y)[k_lo:, ctx]) / power(y[k_lo:, ctx])))


def demonstration(which, seed, source_db, alpha=ALPHA, floor_db=FLOOR_DB):
    """`figures` of one scene in float64, and the gains G [F, T_w]."""
    f, t, _, frames, context, k_lo = SCENES[which][:6]
    source, noise = sparse_scene(which, seed, source_db)
    abc, block = quiet_abc(source + noise, which)
    wide = (max(frames[0] - context, 0), min(frames[1] + context, t - 1))
    ev, d = [[0, wide[0], wide[1]]], [TRUE_DELAY]
    (ys,), (yn,) = X.beamform_ref(source, ev, d, abc, block, k_lo), X.beamform_ref(noise, ev, d, abc, block, k_lo)
    _, (g,) = postfilter_ref([ys + yn], ev, d, abc, block, LOADING, k_lo, None, alpha, 10.0 ** (floor_db / 20.0))
    return figures(source, ys, yn, g, frames, wide, k_lo), g
