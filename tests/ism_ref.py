"""The float64 yardstick of the shoebox room simulation (iris_ism_rir, csrc/k_ism.h): the image-source method of Allen &
Berkley (1979) written from the formulas of DESIGN.md (K2s), vectorised over the images, with a pure-Python triple loop over a
tiny lattice as its own cross-check, and the same formulas in float32 NumPy with the kernel's double / float split - the form
the constant C_ISM of the accuracy rule was measured on.

Per voice: room L [3] m, source s [3], microphones r [C, 3], one wall reflection coefficient beta, K taps.  Images n in
[-N_a, N_a]^3, p in {0, 1}^3: x_a = (1 - 2 p_a) s_a + 2 n_a L_a, e = sum_a |n_a - p_a| + |n_a| reflections, distance d to the
microphone, tau = d fs / c samples; tau_min = the smallest direct delay over the channels, d_min its distance;
t = tau - tau_min + W, a = beta^e d_min / d, h[k] = sum a w(k - t), w(x) = sinc(x) 0.5 (1 + cos(pi x / W)) for |x| < W.
N_a = floor(D / (2 L_a)) + 1 with D = c (tau_min + K) / fs; images with t - W >= K - 1 are skipped."""
import numpy as np

C_SOUND = 343.0
W = 16
U = 2.0 ** -24
# The accuracy rule of the kernel: |h - ref| <= C_ISM u A_k + n_k 2^-33 (A_k = sum |a| over the images whose window covers tap
# k, n_k their number).  Measured: the float32 form below against float64 on the shapes of tests/test_shoebox_gpu.py has a
# worst ratio |h32 - ref| / (u A_k) of 1.80 (printed by test_shoebox_host.py); the constant is twice that: the margin covers a
# different sine and a different summation order, both correct fp32.
C_ISM = 3.6


def geometry(room, source, mics, n_taps, fs=16000.0, extra=0):
    """(tau_min, d_min, N [3]) of one voice; `extra` enlarges every N_a (the completeness check)."""
    room, source, mics = np.asarray(room, np.float64), np.asarray(source, np.float64), np.asarray(mics, np.float64).reshape(-1, 3)
    d = np.sqrt(np.sum((mics - source[None, :]) ** 2, axis=1))
    c = int(np.argmin(d * fs / C_SOUND))
    tau_min, d_min = float(d[c] * fs / C_SOUND), float(d[c])
    reach = C_SOUND * (tau_min + n_taps) / fs
    return tau_min, d_min, [int(np.floor(reach / (2.0 * room[a]))) + 1 + int(extra) for a in range(3)]


def _images(room, source, N):
    """Positions [M, 3] and reflection counts [M] of the whole lattice."""
    axes = []
    for a in range(3):
        n = np.arange(-N[a], N[a] + 1, dtype=np.float64)
        pos = np.concatenate([source[a] + 2.0 * n * room[a], -source[a] + 2.0 * n * room[a]])     # p = 0, p = 1
        refl = np.concatenate([np.abs(n) + np.abs(n), np.abs(n - 1.0) + np.abs(n)])
        axes.append((pos, refl))
    px, py, pz = np.meshgrid(axes[0][0], axes[1][0], axes[2][0], indexing="ij")
    ex, ey, ez = np.meshgrid(axes[0][1], axes[1][1], axes[2][1], indexing="ij")
    return np.stack([px.ravel(), py.ravel(), pz.ravel()], axis=1), (ex + ey + ez).ravel()


def _power(beta, e):
    return np.where(e == 0, 1.0, np.power(float(beta), e)) if beta == 0 else np.power(float(beta), e)


def ism_ref(room, source, mics, beta, n_taps, fs=16000.0, extra=0, normalize=False):
    """(h, A, n) each [C, K]: the float64 response, A_k = sum |a| and n_k = the number of the images whose window covers tap k.
    normalize: every channel times the same g = 1 / sqrt(mean_c sum_k h^2) (g = 1 for an all-zero response); A is scaled too."""
    room, source, mics = np.asarray(room, np.float64), np.asarray(source, np.float64), np.asarray(mics, np.float64).reshape(-1, 3)
    K = int(n_taps)
    tau_min, d_min, N = geometry(room, source, mics, K, fs, extra)
    pos, refl = _images(room, source, N)
    h, A, cnt = (np.zeros((mics.shape[0], K)) for _ in range(3))
    m = np.arange(-W, W + 2, dtype=np.float64)[None, :]
    for c, r in enumerate(mics):
        d = np.sqrt(np.sum((pos - r[None, :]) ** 2, axis=1))
        t = d * fs / C_SOUND - tau_min + W
        keep = ~(t - W >= K - 1)
        d, t, e = d[keep], t[keep], refl[keep]
        a = _power(beta, e) * d_min / d
        base = np.floor(t)
        k = base[:, None] + m
        x = k - t[:, None]
        ok = (np.abs(x) < W) & (k >= 0) & (k < K)
        w = np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / W))
        ki = k[ok].astype(np.int64)
        av = np.broadcast_to(a[:, None], x.shape)[ok]
        h[c] = np.bincount(ki, weights=av * w[ok], minlength=K)
        A[c] = np.bincount(ki, weights=np.abs(av), minlength=K)
        cnt[c] = np.bincount(ki, minlength=K)
    if normalize:
        g = gain(h)
        h, A = h * g, A * g
    return h, A, cnt


def gain(h):
    """g = 1 / sqrt(mean_c sum_k h[c, k]^2), the same for every channel; 1 for an all-zero response."""
    energy = float(np.mean(np.sum(np.asarray(h, np.float64) ** 2, axis=1)))
    return 1.0 / np.sqrt(energy) if energy > 0 else 1.0


def ism_loop(room, source, mics, beta, n_taps, fs=16000.0):
    """The same sum as three nested Python loops over the lattice and one over the parities: for tiny lattices only."""
    import math
    room, source = [float(v) for v in room], [float(v) for v in source]
    mics = [[float(v) for v in r] for r in np.asarray(mics, np.float64).reshape(-1, 3)]
    K = int(n_taps)
    direct = [math.sqrt(sum((source[a] - r[a]) ** 2 for a in range(3))) for r in mics]
    d_min = min(direct)
    tau_min = d_min * fs / C_SOUND
    reach = C_SOUND * (tau_min + K) / fs
    N = [int(math.floor(reach / (2.0 * room[a]))) + 1 for a in range(3)]
    h = np.zeros((len(mics), K))
    for c, r in enumerate(mics):
        for nx in range(-N[0], N[0] + 1):
            for ny in range(-N[1], N[1] + 1):
                for nz in range(-N[2], N[2] + 1):
                    n = (nx, ny, nz)
                    for par in range(8):
                        p = (par & 1, (par >> 1) & 1, (par >> 2) & 1)
                        x = [(1 - 2 * p[a]) * source[a] + 2 * n[a] * room[a] for a in range(3)]
                        e = sum(abs(n[a] - p[a]) + abs(n[a]) for a in range(3))
                        d = math.sqrt(sum((x[a] - r[a]) ** 2 for a in range(3)))
                        t = d * fs / C_SOUND - tau_min + W
                        if t - W >= K - 1:
                            continue
                        a_img = (1.0 if e == 0 else beta ** e) * d_min / d
                        for k in range(max(0, int(math.floor(t)) - W - 1), min(K, int(math.floor(t)) + W + 2)):
                            u = k - t
                            if abs(u) < W:
                                s = 1.0 if u == 0 else math.sin(math.pi * u) / (math.pi * u)
                                h[c, k] += a_img * s * 0.5 * (1.0 + math.cos(math.pi * u / W))
    return h


def ism_f32(room, source, mics, beta, n_taps, fs=16000.0):
    """The formulas in float32 NumPy with the kernel's split: positions, d, tau, t, floor(t) and the fraction in double (the
    fraction folded into [-0.5, 0.5] about the nearest tap), the gain formed in double and rounded once; one sine per image
    ((-1)^m sin(-pi f) serves every tap), the window, the products and the sum in float32.  Returns h [C, K] float32."""
    room, source, mics = np.asarray(room, np.float64), np.asarray(source, np.float64), np.asarray(mics, np.float64).reshape(-1, 3)
    K = int(n_taps)
    tau_min, d_min, N = geometry(room, source, mics, K, fs)
    pos, refl = _images(room, source, N)
    h = np.zeros((mics.shape[0], K), np.float32)
    f32, pi32 = np.float32, np.float32(np.pi)
    m = np.arange(-W, W + 1, dtype=np.int64)[None, :]
    for c, r in enumerate(mics):
        d = np.sqrt(np.sum((pos - r[None, :]) ** 2, axis=1))
        t = d * fs / C_SOUND - tau_min + W
        keep = ~(t - W >= K - 1)
        d, t, e = d[keep], t[keep], refl[keep]
        a = (_power(beta, e) * d_min / d).astype(np.float32)
        base = np.floor(t)
        frac = t - base
        up = frac > 0.5
        frac, base = np.where(up, frac - 1.0, frac), np.where(up, base + 1.0, base).astype(np.int64)
        g = frac.astype(np.float32)[:, None]
        s = np.sin(pi32 * g)                                           # sin(pi g), one per image
        x = m.astype(np.float32) - g
        sign = np.where(m % 2 == 0, f32(-1.0), f32(1.0))               # sin(pi (m - g)) = -(-1)^m sin(pi g)
        with np.errstate(divide="ignore", invalid="ignore"):
            sinc = np.where(x == 0, f32(1.0), (sign * s) / (pi32 * x)).astype(np.float32)
        win = f32(0.5) * (f32(1.0) + np.cos(pi32 * x / f32(W)))
        k = base[:, None] + m
        ok = (np.abs(x) < f32(W)) & (k >= 0) & (k < K)
        v = (a[:, None] * (sinc * win)).astype(np.float32)
        np.add.at(h[c], k[ok], v[ok])
    return h


def rule(ref, A, cnt, c_ism=C_ISM):
    """The accuracy rule's right-hand side per tap (normalize = False)."""
    return c_ism * U * A + cnt * 2.0 ** -33


def cases(channels):
    """The ragged table of the accuracy tests, one record per tap count (K = 1, 8 < W, 33, 257, 4096), every voice with its own
    non-cubic room and beta, the source and the array off every symmetry plane; beta = 0 and beta = 0.9 both occur.  In voice 3
    the nearest microphone is 16 samples from the source (343 * 16 / 16000 m along x).  Returns dicts of room, source, mics
    [channels, 3], beta, n_taps."""
    mic3 = np.array([[1.13, 1.71, 1.22], [1.23, 1.74, 1.19], [1.02, 1.69, 1.27]])
    out = [dict(room=[3.1, 4.3, 2.6], source=[2.05, 3.12, 1.57], mics=mic3, beta=0.9, n_taps=4096),
           dict(room=[3.1, 4.3, 2.6], source=[2.05, 3.12, 1.57], mics=mic3, beta=0.0, n_taps=1),
           dict(room=[3.4, 4.0, 2.9], source=[0.71, 2.93, 1.05], mics=mic3 + 0.3, beta=0.5, n_taps=8),
           dict(room=[5.2, 3.3, 2.7], source=[1.13 + 343.0 * 16 / 16000, 1.71, 1.22], mics=mic3, beta=0.9, n_taps=33),
           dict(room=[4.4, 3.7, 3.1], source=[3.3, 0.9, 2.2], mics=mic3 + 0.2, beta=0.0, n_taps=257),
           dict(room=[3.3, 3.9, 2.5], source=[0.8, 3.1, 0.7], mics=mic3, beta=0.7, n_taps=257)]
    return [dict(v, mics=np.ascontiguousarray(v["mics"][:channels])) for v in out]
