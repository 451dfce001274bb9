"""The float64 definition of delay tracking that `transforms.track_events`, `FrontendPlan.locate_steps` / `track` /
`beamform_frames` and the kernels of k_track.h are held to - NumPy, built on locate_ref / extract_ref.

    frames are grouped into steps of `step` frames counted from frame 0 (block % step == 0: a step lies in one block); an event
    (sample, first, last) is cut into the steps u = first // step .. last // step, the first and last possibly short
    R[u, n] = locate_ref's term sum with "segment" read as "step": the moments over the step's frames, the factors of the step's
    block, the same lags and bins;  n_terms[u] = the step's frames x its contributing bins
    path: D[n] = R[0, n];  D_u[n] = max over n' in [max(0, n - J), min(L - 1, n + J)] of (D_{u-1}[n'] - P[|n - n'|]) + R[u, n],
    P[d] = d pen, the maximiser the smallest such n'; the last step takes the smallest argmax, earlier ones the back-pointers
    per step the parabola through R[u, i - 1 .. i + 1] (locate_peak's rules), tdoa = (i - N + offset) / q, score = R[u, i] / n_terms
    the delay of frame t: the linear interpolation of the finite step delays over the step centres, held constant outside
"""
import numpy as np

import extract_ref as X
import locate_ref as L
import whiten_ref as W


def steps_of(first, last, step):
    """[(u, t0, t1)] with t0 .. t1 inclusive."""
    return [(u, max(first, u * step), min(last, (u + 1) * step - 1)) for u in range(first // step, last // step + 1)]


def step_response(spec, events, abc=None, block=None, step=16, k_lo=0, k_hi=None, n_lag=40, q=8, with_bound=False):
    """-> (R [rows, 2 N + 1] float64, n_terms [rows] int64, offsets [E + 1]); with_bound also the bound [rows, 2 N + 1] of
    |kernel - this|: (2 n_l + 2 n_s + 2 C_TERM) u sum A - the kernels' derived (n_l + n_s + C_TERM) u sum A (one segment per
    row: n_l = ceil(step frames / 64), n_s = ceil((k_hi - k_lo) / 64)) and as much again for this restatement's own roundings,
    as locate_ref does."""
    x0, x1 = W.channels(spec)
    bsz, f, t = x0.shape
    k_hi = f if k_hi is None else k_hi
    if abc is None:
        abc, block = L.identity_factors(bsz, f), max(t, 1)
    else:
        block, _ = W.block_of(t, block)
        assert block % step == 0 or block >= t, (block, step)
    resp, n_terms, bound, offsets = [], [], [], [0]
    for s, first, last in np.asarray(events, np.int64).reshape(-1, 3):
        for _, t0, t1 in steps_of(int(first), int(last), step):
            fac = tuple(v[s, :, t0 // block] for v in abc)
            c, n, mag = L.segment_curve(x0[s, :, t0:t1 + 1], x1[s, :, t0:t1 + 1], fac, k_lo, k_hi, n_lag, q, True)
            n_l, n_s = (t1 - t0 + 1 + 63) // 64, (k_hi - k_lo + 63) // 64
            resp.append(c)
            n_terms.append(n)
            bound.append((2 * n_l + 2 * n_s + 2 * L.C_TERM) * L.U * mag)
        offsets.append(len(resp))
    lags = 2 * n_lag + 1
    out = (np.asarray(resp, np.float64).reshape(-1, lags), np.asarray(n_terms, np.int64), np.asarray(offsets, np.int64))
    return out + (np.asarray(bound, np.float64).reshape(-1, lags),) if with_bound else out


def viterbi(resp, pen, jump):
    """One event's path [n_steps] through resp [n_steps, L]: per candidate one subtraction of a table entry and one comparison,
    per lag one addition - the kernel's operations on the same doubles, so the integers must be equal.  np.argmax takes the
    first maximum: the smallest maximiser."""
    resp = np.asarray(resp, np.float64)
    n_steps, lags = resp.shape
    table = np.arange(lags, dtype=np.float64) * np.float64(pen)
    d, back = resp[0].copy(), np.zeros((n_steps, lags), np.int64)
    for u in range(1, n_steps):
        nxt = np.empty(lags)
        for n in range(lags):
            lo, hi = max(0, n - jump), min(lags - 1, n + jump)
            cand = d[lo:hi + 1] - table[np.abs(np.arange(lo, hi + 1) - n)]
            i = int(np.argmax(cand))
            back[u, n], nxt[n] = lo + i, cand[i] + resp[u, n]
        d = nxt
    path = np.zeros(n_steps, np.int64)
    path[-1] = int(np.argmax(d))
    for u in range(n_steps - 1, 0, -1):
        path[u - 1] = back[u, path[u]]
    return path


def paths(resp, offsets, pen, jump):
    """The paths of all events, concatenated: int64 [rows]."""
    parts = [viterbi(resp[a:z], pen, jump) for a, z in zip(offsets[:-1], offsets[1:])]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def peaks(resp, n_terms, path, q):
    """[rows, 2] = (tdoa, score): the parabola around the path's lag with locate_peak's clipping and edge rules."""
    rows, lags = resp.shape
    out = np.zeros((rows, 2))
    for r in range(rows):
        if n_terms[r] == 0:
            out[r, 0] = np.nan
            continue
        y, i, off = resp[r], int(path[r]), 0.0
        if 0 < i < lags - 1:
            den = 2.0 * (y[i - 1] - 2.0 * y[i] + y[i + 1])
            if den != 0.0:
                off = float(np.clip((y[i - 1] - y[i + 1]) / den, -0.5, 0.5))
        out[r] = ((i - (lags - 1) // 2 + off) / q, y[i] / n_terms[r])
    return out


def delays(steps, tdoa, first, last):
    """The delay of the frames first .. last from steps [(u, t0, t1)] and their delays: interpolated over the finite steps'
    centres, held constant outside; NaN everywhere if none is finite."""
    centres, tdoa = np.asarray([(t0 + t1) / 2.0 for _, t0, t1 in steps]), np.asarray(tdoa, np.float64)
    ok = np.isfinite(tdoa)
    frames = np.arange(first, last + 1, dtype=np.float64)
    return np.interp(frames, centres[ok], tdoa[ok]) if ok.any() else np.full(frames.shape, np.nan)


def beamform_frames_ref(spec, events, tdoa, abc=None, block=None, k_lo=0, k_hi=None):
    """extract_ref.beamform_ref evaluated per frame: tdoa flat, one delay per frame of every event in order -> (Y, A), the lists
    of [F, T_e] complex128 outputs and magnitudes."""
    ev = np.asarray(events, np.int64).reshape(-1, 3)
    single = np.asarray([(s, t, t) for s, first, last in ev for t in range(first, last + 1)], np.int64).reshape(-1, 3)
    ys, mags = X.beamform_ref(spec, single, tdoa, abc, block, k_lo, k_hi, with_mag=True)
    out_y, out_m, at = [], [], 0
    for _, first, last in ev:
        n = int(last - first + 1)
        out_y.append(np.concatenate(ys[at:at + n], axis=1))
        out_m.append(np.concatenate(mags[at:at + n], axis=1))
        at += n
    return out_y, out_m


# ---------------------------------------------------------------------------
# the scene of a moving source
# ---------------------------------------------------------------------------
def moving_scene(seed, f=257, t=512, interferer_delay=2.5, delay_from=-3.0, delay_to=1.0, source_db=-10.0, noise_db=-20.0,
                 frames=(100, 355)):
    """A white interferer at `interferer_delay`, sensor noise `noise_db` under it, and a white source `source_db` under the
    interferer in frames[0] .. frames[1] whose delay moves linearly from delay_from to delay_to.  -> (source, interferer +
    sensor noise), float64 [1, F, T, 4] each (their sum is the scene), and the true delay of every event frame."""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    v, g_n, g_s = cn(f, t), 10.0 ** (noise_db / 20.0), 10.0 ** (source_db / 20.0)
    n0, n1 = v + g_n * cn(f, t), L.delayed(v, interferer_delay) + g_n * cn(f, t)
    n = frames[1] - frames[0] + 1
    truth = np.linspace(delay_from, delay_to, n)
    s0, s1 = np.zeros((f, t), np.complex128), np.zeros((f, t), np.complex128)
    s0[:, frames[0]:frames[1] + 1] = g_s * cn(f, n)
    s1[:, frames[0]:frames[1] + 1] = s0[:, frames[0]:frames[1] + 1] * np.exp(-2j * np.pi * np.arange(f)[:, None] * truth[None, :] / (2 * (f - 1)))
    return X.pack(s0, s1), X.pack(n0, n1), truth
