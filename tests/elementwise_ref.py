"""Reference forms, error rules and yardsticks of the three elementwise stages beside the STFT in the unfused chain
(csrc/k_elementwise.h): iris_normalize, iris_minmax_log, iris_complex_to_magphase / iris_magphase_to_complex.  No GPU dependency.

Every reference is float64 on float64 copies of the float32 input, u = 2^-24, and every K comes from a float32 NumPy yardstick by
the repository's recipe (`istft_ref.k_from`: the smallest power of two at or above four times the yardstick's worst ratio);
tests/test_elementwise_host.py derives them over the inputs below and asserts the values recorded here.

normalize         out = x / (10 rms(row)):                      |out - ref| <= K_NORMALIZE u |ref|
                  An all-zero row is 0 / 0: the kernel returns NaN in every element, as oracle.frontend_ref.normalize does.
min-max           v = (x - min) / max(max - min, eps_div):       |v - ref| <= K_MINMAX u; the row's minimum maps to exactly 0, its
                  maximum to within one ulp of 1; a constant row gives 0 (the eps_div path).
log               ln(v + eps_log) through the hardware log2:     |out - ln(v + eps)| <= LOG_ABS = 2.4e-6 for v in [0, 1], the bound
                  csrc/common.h states for `minmax_log_value` (measured 2.364e-6 in profiles/r3/log_accuracy.log).  Behind min-max:
                  an absolute error d of ln is a relative error e^d - 1 <= d (1 + d) of v + eps, so
                  |exp(out) - (ref + eps)| <= K_MINMAX u + LOG_ABS (1 + LOG_ABS) (ref + eps).
                  A NaN in a row: fminf / fmaxf drop it (NumPy's min would not): the row's other elements are what they are
                  without it, bit for bit, and the NaN element stays NaN - in iris_minmax_log and in the fused epilogue alike.
magnitude/phase   |mag - ref| <= K_MAG u ref;  |phase - ref| <= K_PHASE u pi; atan2's signed zeros and +-pi as NumPy gives them.
phasor            out = mag (cos, sin)(ph), ph the exact float32 value, up to 4e5 rad (the vocoder's unreduced phase):
                  |out - ref| <= K_PHASOR u |mag| - the device's argument reduction is held to account.
round trip        |mp2c(c2mp(z)) - z| <= (K_MAG + pi K_PHASE + K_PHASOR) u |z| per component (first order: a relative error of the
                  modulus, a rotation by the phase error, the phasor's own error)."""
import numpy as np

from istft_ref import F32, U, k_from  # noqa: F401

# yardstick's worst ratio -> K (tests/test_elementwise_host.py derives and asserts each pair)
YARD_NORMALIZE, K_NORMALIZE = 2.13, 16
YARD_MINMAX, K_MINMAX = 0.855, 4
YARD_MAG, K_MAG = 1.77, 8
YARD_PHASE, K_PHASE = 1.71, 8
YARD_PHASOR, K_PHASOR = 1.65, 8
LOG_ABS = 2.4e-6
EPS = 1e-8

NORMALIZE_ROW_LENS = (1, 4095, 4096, 4097, 3 * 4096 + 5)
NORMALIZE_LEVELS = (1e-3, 0.7, 30.0)
MINMAX_ROW_LENS = (256 * 4096, 256 * 4096 + 5)      # 256 and 257 partials: the per-wave fold and the block fold
GRID_CAP = 8192 * 256                               # threads of the capped grid of the magnitude / phase kernels
MAX_PHASE = 4e5


# ---- normalize ----
def normalize_rows(row_len, seed=0):
    rng = np.random.default_rng(seed + row_len)
    return (rng.standard_normal((len(NORMALIZE_LEVELS), row_len)) * np.asarray(NORMALIZE_LEVELS)[:, None]).astype(F32)


def normalize_ref(x):
    """rows [R, n] -> float64 x / (10 rms(row))."""
    x = np.asarray(x, np.float64)
    return x / (np.sqrt(np.mean(x * x, axis=1, keepdims=True)) * 10.0)


def normalize_yardstick(x):
    x = np.asarray(x, F32)
    rms = np.sqrt(np.mean(np.square(x), axis=1, keepdims=True, dtype=F32), dtype=F32) * F32(10)
    return (x / rms).astype(F32)


def rel_ratio(out, ref):
    """Worst |out - ref| / (u |ref|); elements with ref == 0 must be exactly 0."""
    out = np.asarray(out, np.float64)
    z = ref == 0
    assert np.all(out[z] == 0)
    return float((np.abs(out - ref)[~z] / (U * np.abs(ref[~z]))).max()) if (~z).any() else 0.0


# ---- min-max / log ----
def minmax_rows(row_len, seed=0, n_rows=2):
    rng = np.random.default_rng(seed + row_len)
    x = rng.standard_normal((n_rows, row_len)) * np.asarray([1.0, 40.0])[:n_rows, None] + np.asarray([0.0, 7.0])[:n_rows, None]
    return np.abs(x).astype(F32)            # >= 0: the log-only form sees them as they are


def minmax_ref(x, eps_div=EPS):
    x = np.asarray(x, np.float64)
    mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    return (x - mn) / np.maximum(mx - mn, eps_div)


def minmax_yardstick(x, eps_div=EPS):
    x = np.asarray(x, F32)
    mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    return ((x - mn) / np.maximum(mx - mn, F32(eps_div))).astype(F32)


def log_ref(v, eps_log=EPS):
    return np.log(np.asarray(v, np.float64) + eps_log)


# ---- magnitude / phase ----
def complex_rows(n_outer, c, seed=0):
    """[n_outer, 2C] float32 (re block | im block), levels 1e-3 ... 1e2 per row."""
    rng = np.random.default_rng(seed + 31 * c)
    z = rng.standard_normal((n_outer, 2 * c)) * 10.0 ** rng.uniform(-3, 2, size=(n_outer, 1))
    return z.astype(F32)


def magphase_ref(z):
    z = np.asarray(z, np.float64)
    c = z.shape[1] // 2
    return np.hypot(z[:, :c], z[:, c:]), np.arctan2(z[:, c:], z[:, :c])


def magphase_yardstick(z):
    z = np.asarray(z, F32)
    c = z.shape[1] // 2
    re, im = z[:, :c], z[:, c:]
    return np.sqrt(re * re + im * im), np.arctan2(im, re)


def magphase_rows(n_outer, c, seed=0):
    """[n_outer, 2C] float32 (magnitude block | phase block): phases uniform in +-4e5 rad."""
    rng = np.random.default_rng(seed + 77 * c)
    mag = np.abs(rng.standard_normal((n_outer, c))) * 10.0 ** rng.uniform(-3, 2, size=(n_outer, 1))
    ph = rng.uniform(-MAX_PHASE, MAX_PHASE, size=(n_outer, c))
    ph[::7] = rng.uniform(-np.pi, np.pi, size=ph[::7].shape)
    return np.concatenate([mag, ph], axis=1).astype(F32)


def phasor_ref(mp):
    mp = np.asarray(mp, np.float64)            # the float32 phase, exactly
    c = mp.shape[1] // 2
    return mp[:, :c] * np.cos(mp[:, c:]), mp[:, :c] * np.sin(mp[:, c:])


def phasor_yardstick(mp):
    mp = np.asarray(mp, F32)
    c = mp.shape[1] // 2
    return mp[:, :c] * np.cos(mp[:, c:]), mp[:, :c] * np.sin(mp[:, c:])


def phase_edges():
    """[n, 2] (re, im) float32: the origin and the axes with signed zeros."""
    z, x = F32(0.0), F32(1.5)
    return np.array([(z, z), (-z, z), (z, -z), (-z, -z), (-x, z), (-x, -z), (x, z), (x, -z), (z, x), (z, -x), (-z, x), (-z, -x)], F32)


def n_outer_above_cap(c):
    return (GRID_CAP + 1000 + c - 1) // c
