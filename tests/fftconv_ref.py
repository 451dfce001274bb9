"""The float64 definition of the partitioned FFT convolution (iris_fft_fir_batch, csrc/k_fft_fir.h), its norm-wise error rule
and the float32 torch.fft engine the rule's constant was measured on; shared by tests/test_fftconv_host.py and
tests/test_fftconv_gpu.py.

An FFT convolution is not bounded tap by tap (an output whose exact value cancels to nothing still carries the rounding of
the whole block), so the rule is norm-wise per output block:
    |y - ref| <= C u R[c, m],   u = 2^-24,   R[c, m] = sum_{p <= j} ||frame_{j - p}||_2 ||part_p||_2,   j = m // B
with the frames x[(j - 1) B, (j + 1) B) (zero outside [0, L)) and the partitions h[p B, (p + 1) B) of the kernel, B = 1024.
C is measured, not chosen: the same partitioned convolution written with torch.fft.rfft / irfft in float32 on the CPU
(`torch_fft_fir`: the engine a user would otherwise reach for) has a worst |y - ref| / (u R) of 1.66 over the table below
(every length crossed with every tap count, the 2049 x 32768 record, scales 1e-4 and 1e3; typically 0.3, the worst in the
degenerate L = 1 records); C = that figure x 4, rounded up to a power of two = 8.  The margin of 4 covers what differs in the
kernel: a Stockham radix 16 x 16 x 4 order instead of pocketfft's, and the extra rounding step of the packed real transform.
"""
import itertools

import numpy as np

U = 2.0 ** -24   # the unit roundoff of fp32
BLOCK = 1024     # B: new samples per frame (frontend.FFT_FIR_BLOCK); the transform has 2 B points
C_RULE = 8.0     # the rule's constant (see above); the torch.fft engine itself stays within C_RULE / 4

LENGTHS = (1, 5, 1023, 1024, 1025, 2049, 5000)
TAPS = (1, 2, 1023, 1024, 1025, 4097, 9000)
LONG = (2049, 32768)            # one more record: the longest response there is
SMALL, LARGE = (2049, 1025), (5000, 9000)   # the records scaled by 1e-4 and by 1e3


def table(seed=2024, chan=2):
    """(cases, waves, taps) of the accuracy table: every length crossed with every tap count and the LONG record; inputs and
    NON-decaying taps ~ N(0, 1), so a dropped partition or a shifted block moves the result by O(1); one record scaled by
    1e-4 and one by 1e3."""
    rng = np.random.default_rng(seed)
    cases = list(itertools.product(LENGTHS, TAPS)) + [LONG]
    waves = [rng.standard_normal((chan, n)).astype(np.float32) for n, _ in cases]
    taps = [rng.standard_normal((chan, k)).astype(np.float32) for _, k in cases]
    waves[cases.index(SMALL)] *= np.float32(1e-4)
    waves[cases.index(LARGE)] *= np.float32(1e3)
    return cases, waves, taps


def frames_and_parts(x, h):
    """The kernel's geometry in float64: frames [C, nblk, 2 B] with frames[c, j] = x[c, (j - 1) B : (j + 1) B] (zeros outside
    [0, L)) and parts [C, P, B] with parts[c, p] = h[c, p B : (p + 1) B] (zeros beyond K)."""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    assert x.ndim == 2 and h.ndim == 2 and x.shape[0] == h.shape[0]
    (chan, n), k = x.shape, h.shape[1]
    nblk, npart = -(-n // BLOCK), -(-k // BLOCK)
    xp = np.zeros((chan, (nblk + 1) * BLOCK))
    xp[:, BLOCK:BLOCK + n] = x
    frames = np.stack([xp[:, j * BLOCK:(j + 2) * BLOCK] for j in range(nblk)], axis=1)
    hp = np.zeros((chan, npart * BLOCK))
    hp[:, :k] = h
    return frames, hp.reshape(chan, npart, BLOCK)


def fft_fir_ref(x, h):
    """(y, R) for x [C, L] and h [C, K]: y[c] = numpy.convolve(x[c], h[c])[:L] in float64 - the causal convolution cut at the
    input length - and the bound term R[c, m] = sum_{p <= j} ||frame_{j - p}||_2 ||part_p||_2, j = m // B, norms in float64."""
    x, h = np.asarray(x), np.asarray(h)
    n = x.shape[1]
    y = np.stack([np.convolve(xc.astype(np.float64), hc.astype(np.float64))[:n] for xc, hc in zip(x, h)])
    frames, parts = frames_and_parts(x, h)
    fn, pn = np.linalg.norm(frames, axis=2), np.linalg.norm(parts, axis=2)      # [C, nblk], [C, P]
    nblk, npart = fn.shape[1], pn.shape[1]
    rb = np.zeros_like(fn)
    for j in range(nblk):
        for p in range(min(npart - 1, j) + 1):
            rb[:, j] += fn[:, j - p] * pn[:, p]
    return y, np.repeat(rb, BLOCK, axis=1)[:, :n]


def partitioned_ref(x, h):
    """The partitioned restatement of the same convolution in float64: per output block j the sum over p <= j of the linear
    convolution of frame_{j - p} with part_p, of which the samples [B, 2 B) are kept.  Equal to numpy.convolve up to float64
    rounding: the frames and partitions are the right ones."""
    frames, parts = frames_and_parts(x, h)
    chan, nblk, npart, n = frames.shape[0], frames.shape[1], parts.shape[1], np.asarray(x).shape[1]
    y = np.zeros((chan, nblk * BLOCK))
    for c in range(chan):
        for j in range(nblk):
            for p in range(min(npart - 1, j) + 1):
                y[c, j * BLOCK:(j + 1) * BLOCK] += np.convolve(frames[c, j - p], parts[c, p])[BLOCK:2 * BLOCK]
    return y[:, :n]


def torch_fft_fir(x, h):
    """The same partitioned overlap-save convolution in float32 on the CPU with torch.fft.rfft / irfft (B = 1024, N = 2048,
    the products summed over the partitions in ascending p): the engine the rule's constant was measured on.  Returns a
    float32 numpy array [C, L]."""
    import torch
    frames, parts = frames_and_parts(x, h)
    n = np.asarray(x).shape[1]
    xf = torch.fft.rfft(torch.from_numpy(frames.astype(np.float32)), n=2 * BLOCK, dim=2)       # [C, nblk, B + 1]
    hf = torch.fft.rfft(torch.from_numpy(parts.astype(np.float32)), n=2 * BLOCK, dim=2)        # [C, P, B + 1]
    nblk, npart = xf.shape[1], hf.shape[1]
    acc = torch.zeros_like(xf)
    for p in range(npart):
        if p < nblk:
            acc[:, p:] += xf[:, :nblk - p] * hf[:, p:p + 1]
    y = torch.fft.irfft(acc, n=2 * BLOCK, dim=2)[:, :, BLOCK:]
    return y.reshape(y.shape[0], -1)[:, :n].contiguous().numpy()


def rule_ratio(out, ref, r_norm):
    """max |out - ref| / (u R): what the rule holds below C.  Where R == 0 the output must be 0 exactly (the ratio is then
    infinite otherwise)."""
    err = np.abs(np.asarray(out, np.float64) - ref)
    bound = U * r_norm
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0
