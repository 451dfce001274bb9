"""Reference forms of the inverse STFT (iris_istft), a helper beside the tests.

Source S [F, T, 2C] in the reference layout (re block j = c, im block j = C + c), N = n_fft, F = N / 2 + 1, h = hop:

    w[i]    = 0.5 - 0.5 cos(2 pi i / N)                formed in float64 and rounded to float32 ONCE
    x_t[i]  = irfft(S[:, t])[i]                         (the imaginary parts of bins 0 and N / 2 are ignored)
    y[c, n] = (sum_t w[p - t h] x_t[p - t h]) / (sum_t w[p - t h]^2),   p = n + N / 2,   0 <= n < len_out <= (T - 1) h

over the frames with 0 <= p - t h < N: torch.istft(n_fft, hop, window = periodic Hann, center = True, length = len_out).

`istft_ref`      : the definition in float64 (numpy.fft.irfft + overlap-add) on a float64 copy of the float32 input; also
                   returns S[c, n] = (sum_t w[p - t h] rms_i(x_t)) / (sum_t w[p - t h]^2), the scale of the error rule
                   |y - y_ref| <= K u S.
`yardstick32`    : torch.istft in float32 on the CPU with that window.  K is derived from ITS error, not from the kernel's.
`yardstick32_w32`: the same with torch.hann_window evaluated in float32 (what a caller writes by default): the cancellation
                   in 0.5 - 0.5 cos costs 1e-3 relative near the window's edge, which the burst inputs expose."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24


def hann(n_fft):
    """The periodic Hann window formed in float64 and rounded to float32 once (returned as float32)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(F32)


def istft_len(n_frames, hop):
    return (int(n_frames) - 1) * int(hop) if n_frames >= 2 else 0


def to_layout(z):
    """complex [C, F, T] -> [F, T, 2C] (re block, im block last), same precision."""
    z = np.asarray(z)
    return np.ascontiguousarray(np.concatenate([z.real, z.imag], axis=0).transpose(1, 2, 0))


def from_layout(spec):
    """[F, T, 2C] -> complex128 [C, F, T]."""
    spec = np.asarray(spec, np.float64)
    c = spec.shape[2] // 2
    return (spec[..., :c] + 1j * spec[..., c:]).transpose(2, 0, 1)


def _overlap_add(frames, hop):
    """frames [..., T, N] -> [..., (T - 1) hop + N]: frame t added at offset t hop."""
    t, n = frames.shape[-2:]
    out = np.zeros(frames.shape[:-2] + ((t - 1) * hop + n,), frames.dtype)
    for i in range(t):
        out[..., i * hop:i * hop + n] += frames[..., i, :]
    return out


def istft_ref(spec, n_fft, hop, length=None):
    """(y [C, L] float64, S [C, L] float64) by the definition, in float64."""
    z = from_layout(spec)                                  # [C, F, T]
    t = z.shape[2]
    full = istft_len(t, hop)
    length = full if length is None else int(length)
    assert z.shape[1] == n_fft // 2 + 1 and t >= 2 and 0 < length <= full and 1 <= hop <= n_fft // 2
    w = hann(n_fft).astype(np.float64)
    x = np.fft.irfft(z.transpose(0, 2, 1), n=n_fft, axis=-1)   # [C, T, N]
    env = _overlap_add(np.broadcast_to(w * w, (t, n_fft)).copy(), hop)
    rms = np.sqrt(np.mean(x * x, axis=-1, keepdims=True))      # [C, T, 1]
    keep = slice(n_fft // 2, n_fft // 2 + length)              # (the envelope is >= 0.5 in here, 0 at the very first sample)
    return _overlap_add(x * w, hop)[:, keep] / env[keep], _overlap_add(rms * w, hop)[:, keep] / env[keep]


def _torch_istft(spec, n_fft, hop, length, window, dtype):
    z = from_layout(spec)
    zt = torch.from_numpy(z).to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    return torch.istft(zt, n_fft, hop_length=hop, win_length=n_fft, window=window.to(dtype), center=True, normalized=False,
                       onesided=True, length=length).numpy()


def torch_istft64(spec, n_fft, hop, length=None):
    return _torch_istft(spec, n_fft, hop, length, torch.from_numpy(hann(n_fft)), torch.float64)


def yardstick32(spec, n_fft, hop, length=None):
    return _torch_istft(spec, n_fft, hop, length, torch.from_numpy(hann(n_fft)), torch.float32)


def yardstick32_w32(spec, n_fft, hop, length=None):
    return _torch_istft(spec, n_fft, hop, length, torch.hann_window(n_fft, periodic=True, dtype=torch.float32), torch.float32)


def rule_ratio(out, ref, s):
    """Worst |out - ref| / (u S) over the elements with S > 0; elements with S == 0 must be exactly 0."""
    out = np.asarray(out)
    err = np.abs(out.astype(np.float64) - ref)
    ok = s > 0
    assert np.all(out[~ok] == 0), "a sample whose covering frames are all zero must be exactly 0"
    return float((err[ok] / (U * s[ok])).max()) if ok.any() else 0.0


def k_from(worst):
    """The repository's recipe: the smallest power of two at or above four times the yardstick's worst ratio."""
    return int(2 ** int(np.ceil(np.log2(4.0 * worst))))


# ---- inputs: all [F, T, 2C] float32 ----
def stft64(wave, n_fft, hop):
    """[C, L] -> complex128 [C, F, 1 + L // hop]: torch.stft in float64 (periodic Hann, center, reflect)."""
    w = torch.from_numpy(hann(n_fft)).to(torch.float64)
    return torch.stft(torch.from_numpy(np.asarray(wave, np.float64)), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True).numpy()


def noise_stft_spec(chan, n_frames, n_fft, hop, level, seed):
    """The first n_frames frames of the STFT of Gaussian noise of rms `level`."""
    rng = np.random.default_rng(seed)
    wave = rng.standard_normal((chan, (n_frames - 1) * hop + n_fft)) * level
    return to_layout(stft64(wave, n_fft, hop)[:, :, :n_frames]).astype(F32)


def random_spec(chan, n_frames, n_fft, seed):
    """Independent Gaussian re / im in every bin: the STFT of no waveform."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_fft // 2 + 1, n_frames, 2 * chan)).astype(F32)


def burst_spec(chan, n_frames, n_fft, seed):
    """Random spectra whose frames span levels 1e-4 ... 1e2, with one frame exactly zero."""
    rng = np.random.default_rng(seed)
    spec = rng.standard_normal((n_fft // 2 + 1, n_frames, 2 * chan))
    spec *= 10.0 ** rng.uniform(-4, 2, size=(1, n_frames, 1))
    spec[:, int(rng.integers(0, n_frames))] = 0
    return spec.astype(F32)


def make_spec(kind, chan, n_frames, n_fft, hop, seed):
    if kind == "noise":
        level = 10.0 ** np.random.default_rng(seed + 7).uniform(-2, 1)
        return noise_stft_spec(chan, n_frames, n_fft, hop, level, seed)
    if kind == "random":
        return random_spec(chan, n_frames, n_fft, seed)
    assert kind == "burst"
    return burst_spec(chan, n_frames, n_fft, seed)


KINDS = ("noise", "random", "burst")
