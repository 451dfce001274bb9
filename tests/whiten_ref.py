"""The float64 definition of the spatially whitened energy channel that `transforms.mel_whiten`, `FrontendPlan.whiten_factors`,
`FrontendPlan.whiten` and the kernels of k_whiten.h are held to - NumPy, complex arithmetic, written independently of the torch
restatement.

    spec [B, F, T, 4] = (re0, re1, im0, im1),  X0 = re0 + i im0,  X1 = re1 + i im1; blocks of `block` frames from frame 0
    per (sample, bin, block):  r00 = mean |X0|^2, r11 = mean |X1|^2, r10 = mean X1 conj(X0), d = loading (r00 + r11) / 2
        d == 0: a = b = c = 0;  else l00 = sqrt(r00 + d), l10 = r10 / l00, l11 = sqrt(r11 + d - |l10|^2),
        a = 1 / l00, b = 1 / l11, c = l10 / l00
    per frame:  q = |a X0|^2 + |b (X1 - c X0)|^2;   e[m, t] = wnorm[m] sum_k W[k, m] q[k, t],  wnorm = 1 / (2 sum_k W[k, m])
"""
import numpy as np

U = 2.0 ** -24
LOG_EPS = 1e-8
C_APPLY = 16   # the apply kernel's roundings besides the band sum, counted in csrc/k_whiten.h and DESIGN.md


def channels(spec):
    x = np.asarray(spec, np.float64)
    return x[..., 0] + 1j * x[..., 2], x[..., 1] + 1j * x[..., 3]


def block_of(t, block):
    """The block length actually used (None: all t frames) and the block count."""
    block = t if block is None else min(int(block), t)
    block = max(block, 1)
    return block, (t + block - 1) // block


def factors_ref(spec, block=None, loading=1e-2):
    """[B, F, T, 4] -> (a [B, F, J], b [B, F, J], c [B, F, J] complex), float64."""
    x0, x1 = channels(spec)
    bsz, f, t = x0.shape
    block, j = block_of(t, block)
    a, b, c = np.zeros((bsz, f, j)), np.zeros((bsz, f, j)), np.zeros((bsz, f, j), np.complex128)
    for k in range(j):
        s = slice(k * block, min((k + 1) * block, t))
        r00 = (np.abs(x0[..., s]) ** 2).mean(-1)
        r11 = (np.abs(x1[..., s]) ** 2).mean(-1)
        r10 = (x1[..., s] * np.conj(x0[..., s])).mean(-1)
        d = loading * (r00 + r11) / 2
        ok = d != 0
        l00 = np.sqrt(np.where(ok, r00 + d, 1.0))
        l10 = r10 / l00
        l11 = np.sqrt(np.where(ok, r11 + d - np.abs(l10) ** 2, 1.0))
        a[..., k] = np.where(ok, 1 / l00, 0.0)
        b[..., k] = np.where(ok, 1 / l11, 0.0)
        c[..., k] = np.where(ok, l10 / l00, 0.0)
    return a, b, c


def per_frame(v, block, t):
    return np.repeat(v, block, axis=-1)[..., :t]


def q_ref(spec, block=None, loading=1e-2):
    """x^H (R + d I)^-1 x per (sample, bin, frame), and the magnitude A_q = |z0|^2 + ((|X1| + |c| |X0|) b)^2 the fp32 bound
    is stated in: both [B, F, T] float64."""
    x0, x1 = channels(spec)
    t = x0.shape[-1]
    block, _ = block_of(t, block)
    a, b, c = (per_frame(v, block, t) for v in factors_ref(spec, block, loading))
    q = np.abs(a * x0) ** 2 + np.abs(b * (x1 - c * x0)) ** 2
    mag = np.abs(a * x0) ** 2 + ((np.abs(x1) + np.abs(c) * np.abs(x0)) * b) ** 2
    return q, mag


def wnorm_ref(mel_matrix):
    s = np.asarray(mel_matrix, np.float64).sum(axis=0)
    return np.divide(0.5, s, out=np.zeros_like(s), where=s != 0)


def band_mask(bands, b, n):
    """bool [B, n]: inside one of the sample's (offset, size) bands."""
    hit = np.zeros((b, n), bool)
    if bands is not None:
        for i in range(b):
            for off, size in np.asarray(bands)[i]:
                hit[i, int(off):int(off) + int(size)] = True
    return hit


def mel_whiten_ref(spec, mel_matrix, block=None, loading=1e-2, log=True, t_bands=None, f_bands=None, with_bound=False):
    """[B, F, T, 4] -> float64 [B, M, T] (ln(e + 1e-8) with log).  The bands act on the output only.  with_bound: also A[m, t]
    (linear) under the same bands."""
    w = np.asarray(mel_matrix, np.float64)
    q, mag = q_ref(spec, block, loading)
    b, f, t = q.shape
    fm, tm = band_mask(f_bands, b, f), band_mask(t_bands, b, t)
    wn = wnorm_ref(mel_matrix)

    def bands_of(v):
        v = np.where(fm[:, :, None], 0.0, v)
        e = np.einsum('bft,fm->bmt', v, w) * wn[None, :, None]
        return np.where(tm[:, None, :], 0.0, e)
    e = bands_of(q)
    out = np.log(e + LOG_EPS) if log else e
    return (out, bands_of(mag)) if with_bound else out


def band_counts(mel_matrix):
    """n_m: the number of non-zero weights of every band."""
    return (np.asarray(mel_matrix) != 0).sum(axis=0)


def worst_fraction(got, ref, mag, mel_matrix):
    """max over elements of |got - ref| / ((n_m + C) u A): <= 1 passes.  Where A == 0 the value must be exactly the reference's
    (0): any difference there counts as infinite."""
    bound = (band_counts(mel_matrix) + C_APPLY)[None, :, None] * U * mag
    err = np.abs(np.asarray(got, np.float64) - ref)
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(frac.max())


def factor_fraction(got, ref_abc):
    """max over (a, b, |c|) of |got - ref| / (4 u |ref|) for factors [B, F, J, 4] = (a, b, Re c, Im c); c in modulus."""
    a, b, c = ref_abc
    g = np.asarray(got, np.float64)
    gc = g[..., 2] + 1j * g[..., 3]
    worst = 0.0
    for err, ref in ((np.abs(g[..., 0] - a), np.abs(a)), (np.abs(g[..., 1] - b), np.abs(b)), (np.abs(gc - c), np.abs(c))):
        bound = 4 * U * ref
        frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(frac.max()))
    return worst


def interferer_spec(rng, b, f, t, coherence, scale=1.0):
    """A spectrum dominated by one coherent source: X0 = s, X1 = g (rho s + sqrt(1 - rho^2) n) with a fixed complex gain g per
    bin and independent complex normal s, n: inter-channel coherence `coherence`.  float64 [B, F, T, 4]."""
    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    s, n = cn(b, f, t), cn(b, f, t)
    g = (0.5 + rng.uniform(size=(b, f, 1))) * np.exp(2j * np.pi * rng.uniform(size=(b, f, 1)))
    x0 = scale * s
    x1 = scale * g * (coherence * s + np.sqrt(max(1 - coherence ** 2, 0.0)) * n)
    return np.stack([x0.real, x1.real, x0.imag, x1.imag], axis=-1)


def triangular_bands(n_bins, n_bands):
    """A plain triangular filterbank on a linear axis, float32 [F, M] (the issue's 16-band construction)."""
    edges = np.linspace(1, n_bins - 1, n_bands + 2)
    k = np.arange(n_bins)[:, None]
    lo, mid, hi = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    return np.maximum(0, np.minimum((k - lo) / (mid - lo), (hi - k) / (hi - mid))).astype(np.float32)


def mixed_spec(seed, b=3, f=129, t=130, coherence=0.999):
    """Half the bins a coherent interferer, half 0.1 N(0, 1): fp32 [B, F, T, 4]."""
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((b, f, t, 4))
    x[:, ::2] = interferer_spec(rng, b, (f + 1) // 2, t, coherence)
    return x.astype(np.float32)
