"""The float64 definition of the mel-band inter-channel phase difference that `transforms.mel_ipd`, `FrontendPlan.ipd` and the
kernel k_spec_ipd are held to - NumPy, complex arithmetic, written independently of the torch restatement.

    spec [B, F, T, 4] = (re0, re1, im0, im1),  X0 = re0 + i im0,  X1 = re1 + i im1
    out[b, m, t] = sum_k W[k, m] X0 conj(X1) / (sum_k W[k, m] |X0| |X1| + eps)   ->   (real, imag) = (cos, sin)
"""
import numpy as np

EPS = 1e-20
U = 2.0 ** -24


def zero_bands(spec, t_bands=None, f_bands=None):
    """A float64 copy of spec [B, F, T, 4] with the (offset, size) bands zeroed along time / frequency, per sample."""
    x = np.array(spec, dtype=np.float64)
    for b in range(x.shape[0]):
        if t_bands is not None:
            for off, size in np.asarray(t_bands)[b]:
                x[b, :, int(off):int(off) + int(size)] = 0
        if f_bands is not None:
            for off, size in np.asarray(f_bands)[b]:
                x[b, int(off):int(off) + int(size)] = 0
    return x


def mel_ipd_ref(spec, mel_matrix, t_bands=None, f_bands=None, eps=EPS):
    """[B, F, T, 4] -> float64 [B, M, T, 2] = (cos, sin)."""
    x = zero_bands(spec, t_bands, f_bands)
    w = np.asarray(mel_matrix, np.float64)
    x0 = x[..., 0] + 1j * x[..., 2]
    x1 = x[..., 1] + 1j * x[..., 3]
    cross = x0 * np.conj(x1)
    weight = np.abs(x0) * np.abs(x1)
    num = np.einsum('bft,fm->bmt', cross, w.astype(np.complex128))
    den = np.einsum('bft,fm->bmt', weight, w) + eps
    return np.stack([num.real / den, num.imag / den], axis=-1)


def band_counts(mel_matrix):
    """n_m: the number of non-zero weights of every band."""
    return (np.asarray(mel_matrix) != 0).sum(axis=0)


def bound(mel_matrix):
    """The asserted absolute error bound per band, [M]: (2 n_m + 16) u - the derived (2 n_m + 9) u of an fp32 evaluation from
    the same fp32 spectrum plus 7 u of slack for a divide and a square root that are not correctly rounded."""
    return (2.0 * band_counts(mel_matrix) + 16.0) * U


def worst_fraction(got, ref, mel_matrix):
    """max over elements of |got - ref| / bound: <= 1 passes."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float((err / bound(mel_matrix)[None, :, None, None]).max())


def user_matrix(n_bins, n_mel, seed=0):
    """A mel matrix no recipe produces: random positive rectangular bands of 4 bins, then band 1 narrowed to ONE bin, band 2
    all zero (den = 0 -> exactly (0, 0)) and band 3 three times wider than its neighbours (12 bins, overlapping them)."""
    rng = np.random.default_rng(seed)
    w = np.zeros((n_bins, n_mel), np.float32)
    step = max(1, (n_bins - 16) // n_mel)
    for m in range(n_mel):
        lo = 1 + m * step
        w[lo:lo + 4, m] = rng.uniform(0.1, 1.0, 4)
    w[:, 1] = 0
    w[1 + step, 1] = 0.7
    w[:, 2] = 0
    w[:, 3] = 0
    lo = 1 + 3 * step
    w[lo:lo + 12, 3] = rng.uniform(0.1, 1.0, 12)
    return w
