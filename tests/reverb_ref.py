"""The float64 definition of the reverberation kernel (iris_fir_batch, csrc/k_fir.h) and its error rule, shared by
tests/test_reverb_host.py and tests/test_reverb_gpu.py."""
import numpy as np

U = 2.0 ** -24   # the unit roundoff of fp32


def fir_ref(x, h):
    """(y, S) for x [C, L] and h [C, K]: y[c] = numpy.convolve(x[c], h[c])[:L] in float64 - the causal convolution cut at the
    input length - and S[c, m] = sum_k |h[c, k]| |x[c, m - k]|, the same on absolute values."""
    x, h = np.asarray(x), np.asarray(h)
    assert x.ndim == 2 and h.ndim == 2 and x.shape[0] == h.shape[0]
    L = x.shape[1]
    y = np.stack([np.convolve(xc.astype(np.float64), hc.astype(np.float64))[:L] for xc, hc in zip(x, h)])
    s = np.stack([np.convolve(np.abs(xc.astype(np.float64)), np.abs(hc.astype(np.float64)))[:L] for xc, hc in zip(x, h)])
    return y, s


def rule_ratio(out, ref, s_abs, n_taps):
    """max |out - ref| / ((K + 2) u S): the forward bound of an fp32 inner product of K terms in any order, with or without
    FMA (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_K <= (K + 2) u for K u << 1, the two
    extra units covering the rounding of the operands' products in the float64 reference's favour).  Where S == 0 the output
    must be 0 exactly (the ratio is then infinite otherwise)."""
    err = np.abs(out.astype(np.float64) - ref)
    bound = (n_taps + 2) * U * s_abs
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0
