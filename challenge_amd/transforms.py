"""Drop-in counterpart of the reference's transforms.py on torch tensors.

Same callable names, arguments, defaults and `(x, y=None) -> x | (x, y)` map
convention as the reference (transforms.py:12-195).  The functions on the live
hot path -- `mask`, `complex_to_magphase`, `magphase_to_mel` -- run as HIP kernels
through the C ABI and therefore need tensors on a ROCm device (no CPU fallback).
The remaining signatures (`random_shift`, `log_magphase`, `minmax_norm_magphase`,
`magphase_to_complex`, `phase_vocoder`; only the reference's tests call them) are
device-agnostic torch glue.

Randomness: the reference draws from TensorFlow's global Philox stream, which
cannot be reproduced.  Every random transform here is *draw* (documented
distribution, NumPy Generator, `set_seed`) + deterministic *apply*; the apply
halves are what the parity tests pin (`mask_apply`, `random_shift_apply`)."""
from __future__ import annotations

from math import e, log
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import frontend as _fe
from .dataset import AUTOTUNE  # noqa: F401  (re-exported like transforms.py:6)

EPSILON = 1e-8
LOG_EPSILON = log(EPSILON) / log(e)

_rng = np.random.default_rng()


def set_seed(seed: Optional[int]) -> None:
    """Seed the host RNG used by the random transforms (tf.random.set_seed analogue)."""
    global _rng
    _rng = np.random.default_rng(seed)


def get_rng() -> np.random.Generator:
    return _rng


# ---------------------------------------------------------------------------
# FEATURE INDEPENDENT AUGMENTATIONS
# ---------------------------------------------------------------------------
def mask_draw(total: int, max_mask_size: Optional[int] = None, n_mask: int = 1,
              rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """int32 [n_mask, 2] of (offset, size): size ~ U{0..max_mask_size-1},
    offset ~ U{0..total-size-1} (transforms.py:25-26)."""
    rng = _rng if rng is None else rng
    if max_mask_size is None:
        max_mask_size = total
    if max_mask_size <= 0:
        raise ValueError("mask: max_mask_size must be positive")
    bands = np.zeros((n_mask, 2), np.int32)
    for i in range(n_mask):
        size = int(rng.integers(0, max_mask_size))
        if total - size <= 0:
            raise ValueError("mask: maxval must be > 0 (mask of size %d on an axis of %d)" % (size, total))
        bands[i] = (int(rng.integers(0, total - size)), size)
    return bands


def mask_draw_batch(batch: int, total: int, max_mask_size: Optional[int] = None, n_mask: int = 1,
                    rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """`mask_draw` for a whole batch in two vectorised draws: int32 [batch, n_mask, 2] of (offset, size), every
    (sample, mask) pair independent with the distributions of transforms.py:25-26."""
    rng = _rng if rng is None else rng
    if max_mask_size is None:
        max_mask_size = total
    if max_mask_size <= 0:
        raise ValueError("mask: max_mask_size must be positive")
    size = rng.integers(0, max_mask_size, size=(batch, n_mask))
    if batch * n_mask and int(size.max()) >= total:
        raise ValueError("mask: maxval must be > 0 (mask of size %d on an axis of %d)" % (int(size.max()), total))
    off = rng.integers(0, total - size)  # array `high`: one independent draw per element
    return np.stack([off, size], axis=-1).astype(np.int32)


def mask_apply(specs: torch.Tensor, axis: int, bands) -> torch.Tensor:
    """specs with the bands [offset, offset+size) zeroed along `axis`, in specs.dtype."""
    return _fe.mask_apply(specs, axis, bands)


def mask(specs: torch.Tensor, axis: int, max_mask_size: Optional[int] = None, n_mask: int = 1) -> torch.Tensor:
    """SpecAugment band mask (transforms.py:12-40): multiply by `n_mask` random 0/1 bands."""
    total = specs.shape[axis]
    return mask_apply(specs, axis, mask_draw(total, max_mask_size, n_mask))


def random_shift_apply(specs: torch.Tensor, axis: int, width: int, offset: int) -> torch.Tensor:
    axis = axis % specs.dim()
    pad = [0, 0] * specs.dim()
    pad[2 * (specs.dim() - 1 - axis)] = width
    pad[2 * (specs.dim() - 1 - axis) + 1] = width
    padded = torch.nn.functional.pad(specs, pad)
    return padded.narrow(axis, offset, specs.shape[axis]).contiguous()


def random_shift(specs: torch.Tensor, axis: int = 0, width: int = 16) -> torch.Tensor:
    """Zero-pad `width` both sides of `axis`, crop the original extent at a uniform
    offset in [0, 2*width] (transforms.py:43-47)."""
    return random_shift_apply(specs, axis, width, int(_rng.integers(0, 2 * width + 1)))


# ---------------------------------------------------------------------------
# FilterAugment (Nam, Kim, Park, ICASSP 2022): a random piecewise gain curve over the mel bands of every sample
# ---------------------------------------------------------------------------
FILTAUG_N_BAND = (3, 6)    # band count ~ U{3 .. 6}
FILTAUG_MIN_BW = 6         # mel rows per band, at least
FILTAUG_DB = (-6.0, 6.0)   # dB ~ U[-6, 6)
FILTAUG_KINDS = ("step", "linear")


def filter_augment_gains(bounds, db, n_mel: int, kind: str = "step") -> np.ndarray:
    """The gain curve of one sample, float32 [n_mel], evaluated in float64 - THE definition that the device draw
    (`iris_filter_draw`) and the kernels' `mel_gain` are held to.  `bounds`: n_band + 1 mel-row boundaries 0 = b_0 < b_1 < ...
    < b_n = n_mel.  kind 'step': band j (rows b_j .. b_{j+1} - 1) gets db[j] (n_band values); 'linear': db holds n_band + 1
    values at the boundaries and row m of band j gets db[j] + (db[j+1] - db[j]) (m - b_j) / (b_{j+1} - b_j).  The gain is
    10^(dB / 20): the features are mel MAGNITUDES, not powers."""
    if kind not in FILTAUG_KINDS:
        raise ValueError(f"filter_augment_gains: kind must be one of {FILTAUG_KINDS}, got {kind!r}")
    bounds = np.asarray(bounds, np.int64).reshape(-1)
    db = np.asarray(db, np.float64).reshape(-1)
    n_band = bounds.size - 1
    if n_band < 1 or bounds[0] != 0 or bounds[-1] != int(n_mel) or np.any(np.diff(bounds) <= 0):
        raise ValueError(f"filter_augment_gains: bounds must rise strictly from 0 to n_mel = {n_mel}, got {bounds.tolist()}")
    want = n_band if kind == "step" else n_band + 1
    if db.size != want:
        raise ValueError(f"filter_augment_gains: kind {kind!r} with {n_band} bands takes {want} dB values, got {db.size}")
    m = np.arange(int(n_mel))
    j = np.searchsorted(bounds, m, side="right") - 1          # the band of row m
    if kind == "step":
        curve = db[j]
    else:
        curve = db[j] + (db[j + 1] - db[j]) * (m - bounds[j]) / (bounds[j + 1] - bounds[j])
    return np.power(10.0, curve / 20.0).astype(np.float32)


def filter_augment_bounds(cuts, n_band: int, n_mel: int, min_bw: int = FILTAUG_MIN_BW) -> np.ndarray:
    """Sorted distinct cut points among the n_mel - n_band min_bw + (n_band - 1) free slots -> the n_band + 1 boundaries:
    b_j = j min_bw + cuts[j - 1] - (j - 1) (the minimum widths re-inserted), b_0 = 0, b_n = n_mel."""
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    j = np.arange(1, n_band)
    return np.concatenate([[0], j * min_bw + cuts - (j - 1), [n_mel]]).astype(np.int32)


def filter_augment_draw(rng: Optional[np.random.Generator], batch: int, n_mel: int, kind: str = "step",
                        n_band=FILTAUG_N_BAND, min_bw: int = FILTAUG_MIN_BW, db=FILTAUG_DB):
    """The random half of FilterAugment for a batch, on the host (the counterpart of `mask_draw_batch`; `iris_filter_draw`
    makes the same draws on the device from its own generator): returns (bounds int32 [B, n_band_hi + 1], db float32
    [B, n_band_hi + 1], n_band int32 [B]).  Per sample: n_band ~ U{n_band[0] .. n_band[1]}; the boundaries uniform over every
    placement whose bands are at least `min_bw` rows wide (n_band - 1 distinct cut points among the n_mel - n_band min_bw +
    (n_band - 1) free slots, sorted, minimum widths re-inserted); dB ~ U[db[0], db[1]), n_band values ('step') or n_band + 1
    ('linear').  Unused tail entries: bounds = n_mel, db = 0.  `filter_augment_gains(bounds[b, :n + 1], db[b, :n (+ 1)], ...)`
    is sample b's curve; `filter_augment_gain_batch` evaluates them all."""
    rng = _rng if rng is None else rng
    if kind not in FILTAUG_KINDS:
        raise ValueError(f"filter_augment_draw: kind must be one of {FILTAUG_KINDS}, got {kind!r}")
    lo, hi = int(n_band[0]), int(n_band[1])
    if batch < 0 or lo < 1 or lo > hi or min_bw <= 0 or not db[0] <= db[1]:
        raise ValueError(f"filter_augment_draw: bad arguments (batch {batch}, bands {lo}..{hi}, min_bw {min_bw}, dB {db})")
    if n_mel < hi * min_bw:
        raise ValueError(f"filter_augment_draw: n_mel = {n_mel} < n_band_hi * min_bw = {hi} * {min_bw}")
    bounds = np.full((batch, hi + 1), n_mel, np.int32)
    dbs = np.zeros((batch, hi + 1), np.float32)
    counts = rng.integers(lo, hi + 1, size=batch).astype(np.int32)
    for b in range(batch):
        n = int(counts[b])
        slots = n_mel - n * min_bw + (n - 1)
        cuts = np.sort(rng.choice(slots, size=n - 1, replace=False))
        bounds[b, :n + 1] = filter_augment_bounds(cuts, n, n_mel, min_bw)
        n_db = n if kind == "step" else n + 1
        dbs[b, :n_db] = (db[0] + (db[1] - db[0]) * rng.random(n_db)).astype(np.float32)
    return bounds, dbs, counts


def filter_augment_gain_batch(bounds, db, n_band, n_mel: int, kind: str = "step") -> np.ndarray:
    """`filter_augment_gains` for every sample of a `filter_augment_draw`: float32 [B, n_mel]."""
    out = np.empty((len(n_band), int(n_mel)), np.float32)
    for b, n in enumerate(np.asarray(n_band).tolist()):
        out[b] = filter_augment_gains(bounds[b, :n + 1], db[b, :n if kind == "step" else n + 1], n_mel, kind)
    return out


# ---------------------------------------------------------------------------
# MAGNITUDE-PHASE SPECTROGRAM
# ---------------------------------------------------------------------------
def magphase_to_mel(num_mel_bins: int = 80, num_spectrogram_bins: int = 257, sample_rate: float = 16000,
                    **kwargs):
    """Closure factory (transforms.py:51-77).  The weight matrix is built once here
    (argument errors surface at creation, as in the reference); the closure maps
    [B, F, T, 2C] -> [B, M, T, C] or [F, T, 2C] -> [M, T, C].

    Extension: `mel_matrix=W` ([F, M] float32) replaces the built-in recipe - pass the matrix your TensorFlow build
    returns from tf.signal.linear_to_mel_weight_matrix for bit-exact weights."""
    external = kwargs.pop("mel_matrix", None)
    unknown = set(kwargs) - {"lower_edge_hertz", "upper_edge_hertz"}
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    if external is not None:
        mel_matrix = np.ascontiguousarray(external, np.float32)
        if mel_matrix.shape != (num_spectrogram_bins, num_mel_bins):
            raise ValueError(f"mel_matrix must be [{num_spectrogram_bins}, {num_mel_bins}], got {mel_matrix.shape}")
    else:
        mel_matrix = _fe.mel_weight_matrix(num_mel_bins, num_spectrogram_bins, sample_rate, **kwargs)
    n_fft = 2 * (num_spectrogram_bins - 1)
    fft_ok = n_fft in (256, 512, 1024, 2048)
    plans = {}

    def _plan(device: torch.device, chan: int, batch: int) -> "_fe.FrontendPlan":
        key = (device.index, chan)
        plan = plans.get(key)
        if plan is None or plan.max_batch < batch:
            cap = max(batch, 2 * plan.max_batch if plan else 1)
            if fft_ok:
                plan = _fe.FrontendPlan(n_fft, None, num_mel_bins, sample_rate, chan, cap, n_fft, device,
                                        mel_matrix=mel_matrix)
            else:  # mel-only plan for an arbitrary bin count
                plan = _fe.FrontendPlan.mel_only(num_mel_bins, num_spectrogram_bins, chan, cap, device, mel_matrix)
            plans[key] = plan
        return plan

    def _magphase_to_mel(x, y=None):
        if x.dim() not in (3, 4):
            raise ValueError("len(x.shape) must be 3 or 4")
        xb = x if x.dim() == 4 else x.unsqueeze(0)
        if xb.shape[1] != num_spectrogram_bins:
            raise ValueError(f"expected {num_spectrogram_bins} spectrogram bins on axis -3, got {xb.shape[1]}")
        chan = xb.shape[-1] // 2
        if not xb.is_cuda:
            raise RuntimeError("magphase_to_mel runs as a HIP kernel: x must be on a ROCm device (no CPU fallback)")
        plan = _plan(xb.device, chan, xb.shape[0])
        mel = plan.magmel(xb.float(), is_magphase=True)  # phase half is ignored (transforms.py:64)
        if x.dim() == 3:
            mel = mel[0]
        if y is None:
            return mel
        return mel, y

    _magphase_to_mel.mel_matrix = mel_matrix
    return _magphase_to_mel


IPD_EPS = 1e-20


def mel_ipd(spec: torch.Tensor, mel_matrix, t_bands=None, f_bands=None) -> torch.Tensor:
    """Inter-channel phase difference per mel band.  spec: a STEREO complex spectrum [B, F, T, 4] (or [F, T, 4]) with last
    axis (re0, re1, im0, im1); mel_matrix W [F, M]; t_bands / f_bands ([B, n, 2] (offset, size), optional): zeroed in the
    complex spectrum first, as `complex_to_mel` applies them.  Returns [B, M, T, 2] = (cos, sin):
        re_k = re0 re1 + im0 im1,  im_k = im0 re1 - re0 im1          (X0 conj X1: phase = phi0 - phi1)
        a_k  = sqrt((re0^2 + im0^2)(re1^2 + im1^2))                   (= |X0| |X1|)
        cos_m = sum_k W[k,m] re_k / (sum_k W[k,m] a_k + 1e-20), sin_m likewise with im_k
    a magnitude-weighted band average, so cos^2 + sin^2 <= 1 (the band's coherence), identical channels give (1, 0), swapping
    the channels flips sin, silence gives exactly (0, 0) and a common positive scale cancels.  On a ROCm tensor this is one
    HIP launch (`FrontendPlan.ipd`); on a CPU tensor the torch restatement below, in spec's dtype."""
    w = np.ascontiguousarray(mel_matrix, np.float32)
    x = spec if spec.dim() == 4 else spec.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 4 or w.ndim != 2 or x.shape[1] != w.shape[0]:
        raise ValueError(f"mel_ipd: spec must be [B, F, T, 4] (a stereo complex spectrum) and mel_matrix [F, M]; got "
                         f"{tuple(spec.shape)} and {w.shape}")
    b = int(x.shape[0])
    if x.is_cuda:
        out = _stereo_plan(x, w).ipd(x.float(), t_bands=t_bands, f_bands=f_bands)
    else:
        if not torch.is_floating_point(x):
            x = x.float()
        for bands, n, shape in ((t_bands, x.shape[2], (b, 1, -1, 1)), (f_bands, x.shape[1], (b, -1, 1, 1))):
            if bands is None:
                continue
            hit = _band_hits(bands, b, n, "mel_ipd")
            x = torch.where(hit.reshape(shape), torch.zeros((), dtype=x.dtype), x)
        re0, re1, im0, im1 = x.unbind(-1)
        re = re0 * re1 + im0 * im1
        im = im0 * re1 - re0 * im1
        mag = torch.sqrt((re0 * re0 + im0 * im0) * (re1 * re1 + im1 * im1))
        wt = torch.from_numpy(w).to(x.dtype)
        s_re, s_im, s_a = (torch.einsum('bft,fm->bmt', v, wt) for v in (re, im, mag))
        den = s_a + IPD_EPS
        out = torch.stack((s_re / den, s_im / den), dim=-1)
    return out if spec.dim() == 4 else out[0]


_IPD_PLANS = {}


def _stereo_plan(x: torch.Tensor, w: np.ndarray):
    """The cached stereo `FrontendPlan` of `mel_ipd` / `mel_whiten` for the device of `x`, its batch and the mel matrix `w`."""
    b = int(x.shape[0])
    key = (x.device.index, w.shape, w.tobytes())
    plan = _IPD_PLANS.get(key)
    if plan is None or plan.max_batch < b:
        n_fft = 2 * (w.shape[0] - 1)
        if n_fft in (256, 512, 1024, 2048):
            plan = _fe.FrontendPlan(n_fft, None, w.shape[1], 16000, 2, max(b, 1), n_fft, x.device, mel_matrix=w)
        else:
            plan = _fe.FrontendPlan.mel_only(w.shape[1], w.shape[0], 2, max(b, 1), x.device, w)
        _IPD_PLANS[key] = plan
    return plan


def _band_hits(bands, b: int, n: int, who: str) -> torch.Tensor:
    """bool [B, n]: which of the n indices lie inside one of a sample's (offset, size) bands [B, k, 2]."""
    bd = torch.as_tensor(bands).to(torch.int64).cpu()
    if bd.dim() != 3 or bd.shape[0] != b or bd.shape[2] != 2:
        raise ValueError(f"{who}: bands must have shape [batch={b}, n, 2], got {tuple(bd.shape)}")
    idx = torch.arange(n)[None, None, :]
    return ((idx >= bd[:, :, :1]) & (idx < bd[:, :, :1] + bd[:, :, 1:])).any(dim=1)


WHITEN_LOADING = 1e-2


def mel_whiten(spec: torch.Tensor, mel_matrix, block=None, loading: float = WHITEN_LOADING, log: bool = True,
               t_bands=None, f_bands=None) -> torch.Tensor:
    """Spatially whitened mel-band energy: the two-microphone adaptive-matched-filter statistic x^H (R + d I)^-1 x.  spec: a
    STEREO complex spectrum [B, F, T, 4] (or [F, T, 4]) with last axis (re0, re1, im0, im1); mel_matrix W [F, M].  Frames are
    grouped into consecutive blocks of `block` frames from frame 0 (None: all T; the last block may be shorter).  Per sample,
    bin and block, over the block's n frames (unmasked):
        r00 = mean |X0|^2,  r11 = mean |X1|^2,  r10 = mean X1 conj(X0),  d = loading (r00 + r11) / 2
        d == 0 (a silent block): a = b = c = 0
        else l00 = sqrt(r00 + d),  l10 = r10 / l00,  l11 = sqrt(r11 + d - |l10|^2),  a = 1 / l00,  b = 1 / l11,  c = l10 / l00
    per frame z0 = a X0, z1 = b (X1 - c X0), q = |z0|^2 + |z1|^2, and per band
        e[m, t] = wnorm[m] sum_k W[k, m] q[k, t],   wnorm[m] = 1 / (2 sum_k W[k, m])   (0 for an all-zero band)
    Returns e [B, M, T], or ln(e + 1e-8) with `log` (`log_on_mel`'s form).  A frame that holds only the coherent source which
    dominates R scores about 2 per bin however loud that source is (e about 1); energy from another direction stands out by
    up to 1 / (1 - coherence).  The mean of e over a block lies in (0, 1], zero frames and silent blocks give exactly 0, and
    scaling a bin leaves e unchanged (a power of two: the same bits), so a band gain never reaches this channel.
    t_bands / f_bands ([B, n, 2] (offset, size), optional) act on the OUTPUT only: a frame inside a time band gives e = 0, a
    bin inside a frequency band adds nothing to the sum, and neither the covariance nor wnorm sees the bands - unlike
    `mel_ipd`, which zeroes the spectrum first (here that would change R).  On a ROCm tensor this is two HIP launches
    (`FrontendPlan.whiten`); on a CPU tensor the torch restatement below, in spec's dtype."""
    w = np.ascontiguousarray(mel_matrix, np.float32)
    x = spec if spec.dim() == 4 else spec.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 4 or w.ndim != 2 or x.shape[1] != w.shape[0]:
        raise ValueError(f"mel_whiten: spec must be [B, F, T, 4] (a stereo complex spectrum) and mel_matrix [F, M]; got "
                         f"{tuple(spec.shape)} and {w.shape}")
    b, f, t = (int(v) for v in x.shape[:3])
    blk = t if block is None else int(block)
    if blk < 1:
        raise ValueError(f"mel_whiten: block = {blk} must be at least 1 frame")
    if not (np.isfinite(loading) and loading > 0):
        raise ValueError(f"mel_whiten: loading = {loading} must be finite and positive")
    if x.is_cuda:
        out = _stereo_plan(x, w).whiten(x.float(), blk, loading, log, t_bands, f_bands)
        return out if spec.dim() == 4 else out[0]
    if not torch.is_floating_point(x):
        x = x.float()
    blk = max(min(blk, t), 1)
    j = (t + blk - 1) // blk
    count = torch.full((j,), blk, dtype=x.dtype)
    if j:
        count[-1] = t - (j - 1) * blk

    def block_mean(v):
        return torch.nn.functional.pad(v, (0, j * blk - t)).reshape(b, f, j, blk).sum(-1) / count

    def per_frame(v):
        return v.repeat_interleave(blk, dim=-1)[..., :t]

    re0, re1, im0, im1 = x.unbind(-1)
    r00, r11 = block_mean(re0 * re0 + im0 * im0), block_mean(re1 * re1 + im1 * im1)
    r_re, r_im = block_mean(re1 * re0 + im1 * im0), block_mean(im1 * re0 - re1 * im0)   # X1 conj(X0)
    d = loading * (r00 + r11) / 2
    silent, one, zero = d == 0, torch.ones((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)
    l00 = torch.sqrt(torch.where(silent, one, r00 + d))
    l_re, l_im = r_re / l00, r_im / l00
    l11 = torch.sqrt(torch.where(silent, one, r11 + d - (l_re * l_re + l_im * l_im)))
    fa, fb, c_re, c_im = (per_frame(torch.where(silent, zero, v)) for v in (1 / l00, 1 / l11, l_re / l00, l_im / l00))
    z0_re, z0_im = fa * re0, fa * im0
    z1_re, z1_im = fb * (re1 - (c_re * re0 - c_im * im0)), fb * (im1 - (c_re * im0 + c_im * re0))
    q = z0_re * z0_re + z0_im * z0_im + z1_re * z1_re + z1_im * z1_im
    if f_bands is not None:
        q = torch.where(_band_hits(f_bands, b, f, "mel_whiten")[:, :, None], zero, q)
    wsum = w.astype(np.float64).sum(axis=0)
    wnorm = np.divide(0.5, wsum, out=np.zeros_like(wsum), where=wsum != 0)
    out = torch.einsum('bft,fm->bmt', q, torch.from_numpy(w).to(x.dtype)) * torch.from_numpy(wnorm).to(x.dtype)[None, :, None]
    if t_bands is not None:
        out = torch.where(_band_hits(t_bands, b, t, "mel_whiten")[:, None, :], zero, out)
    if log:
        out = torch.log(out + 1e-8)
    return out if spec.dim() == 4 else out[0]


LOCATE_SOUND = _fe.ISM_SOUND   # 343 m/s, the constant of the room and fly-by simulations


def locate_peak(curve, n_terms, q: int = 8, mic_spacing: float = 0.1, sample_rate: float = 16000.0,
                sound_speed: float = LOCATE_SOUND) -> np.ndarray:
    """The peak of steered-response curves [E, 2 N + 1] (lags -N .. N in steps of 1 / q sample) with their n_terms [E] ->
    float64 [E, 4] = (tdoa, bearing, score, contrast), host arithmetic in float64:
        i = the first argmax; for an interior i the parabola through i - 1, i, i + 1 gives the offset
        (y[i - 1] - y[i + 1]) / (2 (y[i - 1] - 2 y[i] + y[i + 1])), clipped to +-0.5 (a zero denominator, or i at either end
        of the grid: 0);  tdoa = (i - N + offset) / q samples, positive when channel 1 hears the event later
        bearing = degrees(asin(clip(-tdoa sound_speed / (sample_rate mic_spacing), -1, 1))), from broadside towards
        microphone 1 (+x, as `draw_shoebox` places it)
        score = curve[i] / n_terms,  contrast = (curve[i] - median(curve)) / n_terms
    n_terms == 0 (nothing contributed): tdoa and bearing NaN, score and contrast 0.  A pair cannot tell front from back: the
    bearing is that of the cone's trace, mirrored about the microphones' axis."""
    y = np.asarray(curve.cpu() if torch.is_tensor(curve) else curve, np.float64)
    n_t = np.asarray(n_terms.cpu() if torch.is_tensor(n_terms) else n_terms, np.int64).reshape(-1)
    q, mic_spacing, sample_rate, sound_speed = int(q), float(mic_spacing), float(sample_rate), float(sound_speed)
    if y.ndim != 2 or y.shape[1] % 2 != 1 or y.shape[0] != n_t.shape[0]:
        raise ValueError(f"locate_peak: curve must be [E, 2 N + 1] and n_terms [E], got {y.shape} and {n_t.shape}")
    if q < 1 or not (np.isfinite(mic_spacing) and mic_spacing > 0 and np.isfinite(sample_rate) and sample_rate > 0
                     and np.isfinite(sound_speed) and sound_speed > 0):
        raise ValueError(f"locate_peak: q = {q} must be >= 1 and mic_spacing = {mic_spacing}, sample_rate = {sample_rate}, "
                         f"sound_speed = {sound_speed} positive and finite")
    n_ev, lags = y.shape
    n = (lags - 1) // 2
    out = np.zeros((n_ev, 4), np.float64)
    for r in range(n_ev):
        if n_t[r] == 0:
            out[r, :2] = np.nan
            continue
        i = int(np.argmax(y[r]))
        off = 0.0
        if 0 < i < lags - 1:
            den = 2.0 * (y[r, i - 1] - 2.0 * y[r, i] + y[r, i + 1])
            if den != 0.0:
                off = float(np.clip((y[r, i - 1] - y[r, i + 1]) / den, -0.5, 0.5))
        tdoa = (i - n + off) / q
        out[r, 0] = tdoa
        out[r, 1] = np.degrees(np.arcsin(np.clip(-tdoa * sound_speed / (sample_rate * mic_spacing), -1.0, 1.0)))
        out[r, 2] = y[r, i] / n_t[r]
        out[r, 3] = (y[r, i] - np.median(y[r])) / n_t[r]
    return out


_LOCATE_PLANS = {}


def _locate_plan(x: torch.Tensor):
    """The cached stereo `FrontendPlan` of `locate_events` for the device of `x`, its bins and its batch."""
    f, b = int(x.shape[1]), int(x.shape[0])
    key = (x.device.index, f)
    plan = _LOCATE_PLANS.get(key)
    if plan is None or plan.max_batch < b:
        w = np.ones((f, 1), np.float32)   # (the localisation reads no mel matrix)
        plan = _LOCATE_PLANS[key] = _fe.FrontendPlan.mel_only(1, f, 2, max(b, 1), x.device, w)
    return plan


NOISE_KINDS = ("block", "identity", "quiet")


def _count(value, name: str, least: int) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"quiet: {name} = {value!r} must be an integer >= {least}")
    return int(value)


def _sample_lengths(n_frames, batch=None) -> np.ndarray:
    """One frame count per sample, int64 [B]: a sequence as it is, one count repeated `batch` times (None: once)."""
    n = np.asarray(n_frames)
    if n.ndim == 0:
        n = np.repeat(n, 1 if batch is None else int(batch))
    if n.ndim != 1 or n.size == 0 or not np.issubdtype(n.dtype, np.integer) or (n < 1).any() or \
            (batch is not None and n.size != int(batch)):
        raise ValueError(f"quiet: n_frames = {n_frames!r} must be a frame count >= 1, or one per sample")
    return n.astype(np.int64)


def quiet_mask(events, n_frames, guard: int = 0, batch=None) -> np.ndarray:
    """The frames that do NOT count as noise: uint8 [B, T], 1 for every frame inside any event of sample b - events: integers
    [E, 3] = (sample, first frame, last frame), frames inclusive, of any class - widened by `guard` frames a side and clipped
    to the recording.  n_frames: one frame count per sample (B of them; T is the largest) or one count for all of `batch`
    samples (None: one).  Frames past a sample's own end stay 0: no range of `quiet_ranges` holds them.  Host NumPy."""
    lens, guard = _sample_lengths(n_frames, batch), _count(guard, "guard", 0)
    mask = np.zeros((len(lens), int(lens.max())), np.uint8)
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events)
    if ev.size == 0:
        return mask
    if ev.ndim != 2 or ev.shape[1] != 3 or not np.issubdtype(ev.dtype, np.integer):
        raise ValueError(f"quiet: events must be integers [E, 3] = (sample, first frame, last frame), got {ev.dtype} {ev.shape}")
    ev = ev.astype(np.int64)
    inside = (ev[:, 0] >= 0) & (ev[:, 0] < len(lens))
    bad = np.flatnonzero(~inside | (ev[:, 1] < 0) | (ev[:, 1] > ev[:, 2]) | (ev[:, 2] >= lens[np.where(inside, ev[:, 0], 0)]))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"quiet: event {i} = (sample {ev[i, 0]}, frames {ev[i, 1]} .. {ev[i, 2]}) does not fit {len(lens)} sample(s) "
                         f"of {lens.tolist()} frames with first <= last")
    for s, first, last in ev:
        mask[s, max(first - guard, 0):min(last + guard, lens[s] - 1) + 1] = 1
    return mask


def quiet_ranges(mask, n_frames, block=None, min_quiet: int = 32, reach: int = 1):
    """Which frames stand behind the noise covariance of every (sample, block): (ranges int32 [B, J, 3] = (t0, t1, use_mask),
    quiet int64 [B, J]) from mask uint8 [B, T] (`quiet_mask`) and n_frames, one frame count per sample (or one for all).
    Blocks of `block` frames from frame 0 (None, or more than T: all T), J = ceil(T / block).  For block j of a sample of T_b
    frames and r = 0 .. reach, the first r for which [max((j - r) block, 0), min((j + r + 1) block, T_b)) holds at least
    `min_quiet` unmasked frames gives the range, with use_mask = 1 and quiet = that count: the block's own quiet frames, else
    those of the block and r neighbours a side.  If there is none the range is the block's own frames with use_mask = 0 and
    quiet = 0: the block covariance, event included.  A block that starts past the sample's end gets its own (padding) frames
    with use_mask = 0 and quiet = 0: a zero-padded spectrum gives it zero factors.  Host NumPy."""
    m = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)
    if m.ndim != 2 or m.dtype != np.uint8 or m.shape[1] < 1:
        raise ValueError(f"quiet: mask must be uint8 [B, T >= 1], got {m.dtype} {m.shape}")
    bsz, t = m.shape
    lens = _sample_lengths(n_frames, bsz)
    if (lens > t).any():
        raise ValueError(f"quiet: n_frames = {lens.tolist()} exceed the mask's {t} frames")
    min_quiet, reach = _count(min_quiet, "min_quiet", 1), _count(reach, "reach", 0)
    blk = min(t if block is None else _count(block, "block", 1), t)
    n_blocks = (t + blk - 1) // blk
    ahead = np.concatenate([np.zeros((bsz, 1), np.int64), np.cumsum(m == 0, axis=1, dtype=np.int64)], axis=1)   # quiet frames before t
    ranges, quiet = np.zeros((bsz, n_blocks, 3), np.int32), np.zeros((bsz, n_blocks), np.int64)
    for b in range(bsz):
        t_b = int(lens[b])
        for j in range(n_blocks):
            ranges[b, j] = (j * blk, min((j + 1) * blk, t_b if j * blk < t_b else t), 0)
            if j * blk >= t_b:
                continue
            for r in range(reach + 1):
                lo, hi = max((j - r) * blk, 0), min((j + r + 1) * blk, t_b)
                n = int(ahead[b, hi] - ahead[b, lo])
                if n >= min_quiet:
                    ranges[b, j], quiet[b, j] = (lo, hi, 1), n
                    break
                if lo == 0 and hi == t_b:   # the whole recording already: a wider reach finds nothing more
                    break
    return ranges, quiet


def quiet_frames(events, quiet, block) -> np.ndarray:
    """How much noise stands behind each event: int64 [E], the fewest quiet frames (`quiet_ranges`' second result [B, J]) behind
    any block of `block` frames the event (sample, first frame, last frame) touches; 0 when one of them fell back on its own
    frames, event included."""
    ev = np.asarray(events, np.int64).reshape(-1, 3)
    quiet = np.asarray(quiet, np.int64)
    blk = max(int(block), 1)
    return np.asarray([quiet[s, first // blk:last // blk + 1].min() for s, first, last in ev], np.int64).reshape(-1)


def _quiet_factors(plan, x: torch.Tensor, events, block, loading: float, guard: int, min_quiet: int, reach: int, n_frames=None):
    """The factors of noise="quiet" for the spectrum x [B, F, T, 4] and its events: (fac [B, F, J, 4], quiet [B, J])."""
    bsz, t = int(x.shape[0]), int(x.shape[2])
    lens = _sample_lengths(t if n_frames is None else n_frames, bsz)
    mask = quiet_mask(events, lens, guard)
    if mask.shape[1] < t:   # (the longest recording is shorter than the padded spectrum)
        mask = np.pad(mask, ((0, 0), (0, t - mask.shape[1])))
    block = t if block is None else _count(block, "block", 1)
    ranges, quiet = quiet_ranges(mask, lens, block, min_quiet, reach)
    return plan.whiten_factors_ranges(x, mask, ranges, block, loading), quiet


def locate_events(spec: torch.Tensor, events, block=None, loading: float = WHITEN_LOADING, noise: str = "block", k_lo: int = 0,
                  k_hi=None, max_lag: int = 40, q: int = 8, mic_spacing: float = 0.1, sample_rate: float = 16000.0,
                  sound_speed: float = LOCATE_SOUND, guard: int = 0, min_quiet: int = 32, reach: int = 1) -> np.ndarray:
    """Where each event comes from: the noise-whitened steered response of a two-microphone delay vector over the event's
    frames, and its peak.  spec: a STEREO complex spectrum [B, F, T, 4] (or [F, T, 4]) = (re0, re1, im0, im1) on a ROCm device,
    n_fft = 2 (F - 1); events: integers [E, 3] = (sample, first frame, last frame), frames inclusive, 0 <= first <= last < T.
    Definition, in float64 (`tests/locate_ref.py` restates it in NumPy).  Frames are grouped into blocks of `block` frames
    (None: all T) and (a, b, c) are `mel_whiten`'s factors of the block's inter-channel covariance with `loading`
    (noise="block"), or a = b = 1, c = 0 with one block (noise="identity": the plain power-weighted steered response, which
    finds the LOUDEST direction).  An event is cut at block boundaries into segments j = first // block .. last // block.  For
    one segment and one bin k in [k_lo, k_hi) (None: F), with (a, b, c) of (sample, k, j):
        a == 0 (a silent block): the pair contributes nothing; otherwise over the segment's frames
        z0 = a X0,  z1 = b (X1 - c X0),  p00 = sum |z0|^2,  p11 = sum |z1|^2,  p10 = sum z1 conj(z0)
    and for the lag n of the grid -max_lag .. max_lag (steps of 1 / q sample)
        e = exp(-i 2 pi k n / (n_fft q))      (a positive delay: channel 1 hears the event later)
        s0 = a,  s1 = b (e - c)               (the steering vector [1, e], whitened)
        term = (a^2 p00 + |s1|^2 p11 + 2 a Re(conj(s1) p10)) / (a^2 + |s1|^2)        = sum_t |s^H z|^2 / (s^H s)
    curve[E, 2 max_lag + 1] is the sum of the terms over the event's segments and bins, n_terms[E] the sum over the
    contributing (segment, bin) pairs of the segment's frame count: under noise alone curve / n_terms is near 1.  Returns
    `locate_peak` of the curves: float64 [E, 4] = (tdoa in samples, bearing in degrees, score, contrast).
    noise="quiet": the covariance of a block is taken over the frames OUTSIDE the events (`tests/quiet_ref.py` restates it):
    every frame inside any of `events`, widened by `guard` frames a side, is masked (`quiet_mask`); a block uses its own
    unmasked frames if there are at least `min_quiet` of them, else those of itself and up to `reach` neighbours a side, else
    - a fallback - all of its own frames, event included (`quiet_ranges`); the factors are otherwise "block"'s
    (`FrontendPlan.whiten_factors_ranges`, one launch).  guard = 0, min_quiet = 32 and reach = 1 are choices, not measurements.
    The launches are `FrontendPlan.whiten_factors` (noise="block") and `FrontendPlan.locate`; there is no CPU fallback.
    What it cannot do: a pair cannot tell front from back (the bearing is mirrored about the microphones' axis); with
    noise="block", and with noise="quiet" in a fallback block, the block covariance includes the event, so an event that
    dominates its block partly nulls itself; and the estimate is biased towards the interferer when the two delays are within
    about a sample of each other (with two microphones one degree of freedom is left after the null)."""
    if noise not in NOISE_KINDS:
        raise ValueError(f"locate_events: noise = {noise!r} must be 'block', 'identity' or 'quiet'")
    if not isinstance(spec, torch.Tensor):
        raise TypeError(f"spec must be a torch.Tensor, got {type(spec).__name__}")
    x = spec if spec.dim() == 4 else spec.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 4 or x.shape[1] < 2:
        raise ValueError(f"locate_events: spec must be [B, F >= 2, T, 4] (a stereo complex spectrum), got {tuple(spec.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"locate_events: spec is on {x.device}: the localisation runs only as HIP kernels on a ROCm device "
                           "(there is no CPU fallback); move the tensor to 'cuda'")
    x = x.float().contiguous()
    plan = _locate_plan(x)
    if noise == "quiet":
        fac, _ = _quiet_factors(plan, x, events, block, loading, guard, min_quiet, reach)
    else:
        fac = plan.whiten_factors(x, block, loading) if noise == "block" else None
    curve, n_terms = plan.locate(x, events, fac, block, k_lo, k_hi, max_lag, q)
    return locate_peak(curve, n_terms, q, mic_spacing, sample_rate, sound_speed)


def track_peak(resp, n_terms, path, q: int = 8) -> np.ndarray:
    """The delay of every step on its path: step responses R [rows, 2 N + 1] (lags -N .. N in steps of 1 / q sample), their
    n_terms [rows] and the path's lag index i per row -> float64 [rows, 2] = (tdoa, score), host arithmetic in float64 in
    `locate_peak`'s style: for an interior i the parabola through R[row, i - 1 .. i + 1] gives the offset (y[i - 1] - y[i + 1]) /
    (2 (y[i - 1] - 2 y[i] + y[i + 1])), clipped to +-0.5 (a zero denominator, or i at either end of the grid: 0);
    tdoa = (i - N + offset) / q;  score = R[row, i] / n_terms[row].  n_terms == 0: tdoa NaN, score 0.  (On a path, unlike at
    the argmax, i need not be a local maximum: the clip then holds the delay within half a lag step of the path.)"""
    y = np.asarray(resp.cpu() if torch.is_tensor(resp) else resp, np.float64)
    n_t = np.asarray(n_terms.cpu() if torch.is_tensor(n_terms) else n_terms, np.int64).reshape(-1)
    idx = np.asarray(path.cpu() if torch.is_tensor(path) else path, np.int64).reshape(-1)
    q = int(q)
    if y.ndim != 2 or y.shape[1] % 2 != 1 or y.shape[0] != n_t.shape[0] or y.shape[0] != idx.shape[0]:
        raise ValueError(f"track_peak: R must be [rows, 2 N + 1], n_terms and path [rows], got {y.shape}, {n_t.shape}, {idx.shape}")
    if q < 1 or (idx.size and (idx.min() < 0 or idx.max() >= y.shape[1])):
        raise ValueError(f"track_peak: q = {q} must be >= 1 and every path index inside [0, {y.shape[1]})")
    rows, lags = y.shape
    n = (lags - 1) // 2
    out = np.zeros((rows, 2), np.float64)
    for r in range(rows):
        if n_t[r] == 0:
            out[r, 0] = np.nan
            continue
        i, off = int(idx[r]), 0.0
        if 0 < i < lags - 1:
            den = 2.0 * (y[r, i - 1] - 2.0 * y[r, i] + y[r, i + 1])
            if den != 0.0:
                off = float(np.clip((y[r, i - 1] - y[r, i + 1]) / den, -0.5, 0.5))
        out[r] = ((i - n + off) / q, y[r, i] / n_t[r])
    return out


def track_rows(events, row_offsets, step: int, peaks) -> List[np.ndarray]:
    """Per event the float64 [n_steps, 4] = (first frame of step, last frame, tdoa, score) of `track_events` from the call's
    events [E, 3], `FrontendPlan.locate_steps`' row_offsets [E + 1] and `track_peak`'s [rows, 2]."""
    ev, off = np.asarray(events, np.int64).reshape(-1, 3), np.asarray(row_offsets, np.int64).reshape(-1)
    peaks, step, out = np.asarray(peaks, np.float64).reshape(-1, 2), int(step), []
    for (_, first, last), r0, r1 in zip(ev, off[:-1], off[1:]):
        u = np.arange(first // step, last // step + 1, dtype=np.int64)
        rows = np.empty((len(u), 4), np.float64)
        rows[:, 0], rows[:, 1] = np.maximum(u * step, first), np.minimum((u + 1) * step - 1, last)
        rows[:, 2:] = peaks[r0:r1]
        out.append(rows)
    return out


def track_delays(track, first: int, last: int) -> np.ndarray:
    """The delay of every frame first .. last (inclusive) from one event's track [n_steps, 4] = (first frame of step, last
    frame, tdoa, score): float64 [last - first + 1], the linear interpolation of the FINITE step delays over the step centres
    (t0 + t1) / 2, held constant before the first and after the last centre - so frames outside the event (`extract`'s context)
    take the nearest end value - and NaN for every frame if no step is finite."""
    tr = np.asarray(track, np.float64).reshape(-1, 4)
    first, last = int(first), int(last)
    if last < first:
        raise ValueError(f"track_delays: frames {first} .. {last}")
    frames = np.arange(first, last + 1, dtype=np.float64)
    ok = np.isfinite(tr[:, 2])
    if not ok.any():
        return np.full(frames.shape, np.nan)
    return np.interp(frames, (tr[ok, 0] + tr[ok, 1]) / 2.0, tr[ok, 2])


def track_events(spec: torch.Tensor, events, block=None, loading: float = WHITEN_LOADING, noise: str = "block", k_lo: int = 0,
                 k_hi=None, max_lag: int = 40, q: int = 8, step: int = 16, pen: float = 0.0, max_jump: int = 40, guard: int = 0,
                 min_quiet: int = 32, reach: int = 1) -> List[np.ndarray]:
    """The delay of each event as it MOVES: `locate_events`' response per step of frames, and the best path through its lags.
    spec, events, block, loading, noise, bins, lags, guard, min_quiet and reach are `locate_events`'.  Returns per event a
    float64 [n_steps, 4] = (first frame of step, last frame, tdoa in samples, score); `track_delays` turns it into a delay per
    frame.  Definition, in float64 (`tests/track_ref.py` restates it in NumPy):
      1. Steps.  Frames are grouped into steps of `step` frames counted from frame 0; block % step == 0 is required (ValueError),
         so a step lies in one block.  An event (sample, first, last) is cut into the steps u = first // step .. last // step;
         the first and the last may be short.
      2. Step response.  R[u, n] is `locate_events`' term sum with "segment" read as "step": the moments p00, p11, p10 over the
         step's frames, (a, b, c) those of the step's block, the lags n = -max_lag .. max_lag in steps of 1 / q sample and the bins
         [k_lo, k_hi) unchanged; n_terms[u] = the step's frame count x its contributing bins.  A short step sums over fewer
         frames and so weighs less by itself.
      3. Path.  With pen >= 0 (response units per lag step), the jump limit J = max_jump >= 0 (lag steps per step), L = 2 max_lag
         + 1 and P[d] = d pen (formed once, in float64): D[n] = R[first step, n]; every later step
             D_u[n] = max over n' in [max(0, n - J), min(L - 1, n + J)] of (D_{u-1}[n'] - P[|n - n'|]) + R[u, n]
         where the maximiser is the smallest such n'; the last step takes the smallest argmax of D, earlier steps follow the
         back-pointers.  The recurrence holds only subtractions, additions and comparisons of doubles - nothing that could be
         contracted into an fma - so a NumPy loop with the same two operations per candidate gives the same path exactly.
      4. Refinement (`track_peak`, host float64): per step the parabola through R[u, i - 1 .. i + 1] around the path's i with
         `locate_peak`'s clipping and edge rules, tdoa_u = (i - max_lag + offset) / q, score_u = R[u, i] / n_terms[u]; a step with
         n_terms == 0 gets tdoa NaN and score 0.
    The launches are the factors' (as in `locate_events`), `FrontendPlan.locate_steps` (two) and `FrontendPlan.track` (one), and
    one copy back; there is no CPU fallback.  At most 2049 lags (max_lag <= 1024).  noise="identity" is allowed here - the path
    does not care what the response's unit is - but `pen` is in that unit: `detect.TrackSettings` presumes whitening.
    What it cannot do: follow a delay that moves by more than max_jump lag steps per step, or resolve motion inside one step."""
    if noise not in NOISE_KINDS:
        raise ValueError(f"track_events: noise = {noise!r} must be 'block', 'identity' or 'quiet'")
    if not isinstance(spec, torch.Tensor):
        raise TypeError(f"spec must be a torch.Tensor, got {type(spec).__name__}")
    x = spec if spec.dim() == 4 else spec.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 4 or x.shape[1] < 2:
        raise ValueError(f"track_events: spec must be [B, F >= 2, T, 4] (a stereo complex spectrum), got {tuple(spec.shape)}")
    lags = 2 * int(max_lag) + 1
    _fe.track_step(step, None if noise == "identity" or block is None else block)
    _fe.track_penalties(pen, max_jump, lags)   # (refuses pen, max_jump and more than 2049 lags before any device work)
    if not x.is_cuda:
        raise RuntimeError(f"track_events: spec is on {x.device}: the tracking runs only as HIP kernels on a ROCm device "
                           "(there is no CPU fallback); move the tensor to 'cuda'")
    x = x.float().contiguous()
    plan = _locate_plan(x)
    if noise == "quiet":
        fac, _ = _quiet_factors(plan, x, events, block, loading, guard, min_quiet, reach)
    else:
        fac = plan.whiten_factors(x, block, loading) if noise == "block" else None
    return _track(plan, x, events, fac, block, step, k_lo, k_hi, max_lag, q, pen, max_jump)


def _track(plan, x: torch.Tensor, events, fac, block, step: int, k_lo: int, k_hi, max_lag: int, q: int, pen: float,
           max_jump: int) -> List[np.ndarray]:
    """`track_events` behind the factors: three launches and ONE copy back (R, n_terms and the path share a buffer)."""
    table = _fe.locate_table(events, int(step), int(x.shape[2]), int(x.shape[0]))
    if len(table) == 0:
        return []
    lags = 2 * int(max_lag) + 1
    rows = int(table[-1, 3]) + int(table[-1, 2]) // int(step) - int(table[-1, 1]) // int(step) + 1
    flat, resp, n_terms, path = _fe.track_buffers(rows, lags, x.device)
    _, _, offsets = plan.locate_steps(x, table[:, :3], fac, block, step, k_lo, k_hi, max_lag, q, out=(resp, n_terms))
    plan.track(resp, offsets, pen, max_jump, out=path)
    host = _fe.track_unpack(flat, rows, lags)   # the one copy back
    return track_rows(table[:, :3], offsets, step, track_peak(*host, q))


def widen_events(events, context: int, n_frames) -> np.ndarray:
    """Events [E, 3] = (sample, first frame, last frame) widened by `context` frames a side and clipped to [0, n_frames) -
    n_frames one count or one per event.  int64 [E, 3]."""
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events)
    if ev.size == 0:
        return np.zeros((0, 3), np.int64)
    if ev.ndim != 2 or ev.shape[1] != 3 or not np.issubdtype(ev.dtype, np.integer):
        raise ValueError(f"extract: events must be integers [E, 3] = (sample, first frame, last frame), got {ev.dtype} {ev.shape}")
    if isinstance(context, bool) or not isinstance(context, (int, np.integer)) or context < 0:
        raise ValueError(f"extract: context = {context!r} must be a number of frames >= 0")
    ev = ev.astype(np.int64)
    limit = np.broadcast_to(np.asarray(n_frames, np.int64), (len(ev),))
    bad = np.flatnonzero((ev[:, 1] < 0) | (ev[:, 1] > ev[:, 2]) | (ev[:, 2] >= limit))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"extract: event {i} spans frames {ev[i, 1]} .. {ev[i, 2]} of {limit[i]}")
    ev[:, 1] = np.maximum(ev[:, 1] - int(context), 0)
    ev[:, 2] = np.minimum(ev[:, 2] + int(context), limit - 1)
    return ev


def frame_delays(tdoa, wide) -> Tuple[np.ndarray, bool]:
    """`extract_events`' tdoa as (flat float64 delays, per_frame): one delay per event - a flat sequence of E numbers - passes
    through with per_frame False; a sequence of E arrays, the e-th with one delay per frame of the (widened) event wide[e] =
    (sample, first, last) (`track_delays(track, first, last)`), is concatenated with per_frame True.  ValueError: a length that
    fits neither."""
    wide = np.asarray(wide, np.int64).reshape(-1, 3)
    if torch.is_tensor(tdoa):
        tdoa = tdoa.cpu().numpy()
    if isinstance(tdoa, np.ndarray) and tdoa.ndim <= 1 or not len(tdoa) or all(np.ndim(d) == 0 for d in tdoa):
        return np.asarray(tdoa, np.float64).reshape(-1), False
    parts = [np.asarray(d.cpu() if torch.is_tensor(d) else d, np.float64).reshape(-1) for d in tdoa]
    want = (wide[:, 2] - wide[:, 1] + 1).tolist()
    if [len(p) for p in parts] != want:
        raise ValueError(f"extract: per-frame delays of {[len(p) for p in parts][:8]} frames for events of {want[:8]} (widened) frames")
    return np.concatenate(parts), True


def clips_from_slabs(slabs, hop=None):
    """The waveforms of beamformed slabs (`FrontendPlan.beamform`: [F, T_e, 2] float32 each, on one ROCm device): ONE
    `iris_istft` launch per 65535 slabs on a cached one-channel plan of n_fft = 2 (F - 1) and `hop` (None: n_fft // 2,
    load_wav's).  Returns (clips, flat): clips[e] a 1-D float32 view of (T_e - 1) hop samples of the flat device buffer `flat`
    (a slab of one frame gives an empty clip).  Bit for bit `frontend.istft_batch` of the slabs."""
    slabs = list(slabs)
    if not slabs:
        return [], None
    f, dev = int(slabs[0].shape[0]), slabs[0].device
    n_fft = 2 * (f - 1)
    plan = _fe.get_plan(dev, n_fft, hop, 64, 16000, 1, 1, n_fft)
    lens = [_fe.istft_len(int(s.shape[1]), plan.hop) for s in slabs]
    if sum(lens) > 2 ** 31 - 1 or max(lens) > 2 ** 31 - 1:
        raise ValueError("extract: more than 2^31 - 1 samples")
    flat = torch.empty((sum(lens),), dtype=torch.float32, device=dev)
    table, at = np.zeros(len(slabs), _fe.ISTFT_SRC), 0
    clips = []
    for i, (s, n) in enumerate(zip(slabs, lens)):
        if tuple(s.shape) != (f, int(s.shape[1]), 2) or s.dtype != torch.float32 or not s.is_contiguous() or s.device != dev:
            raise ValueError(f"extract: slab {i} must be a contiguous float32 [{f}, T, 2] on {dev}, got {s.dtype} {tuple(s.shape)}")
        clips.append(flat[at:at + n])
        table[i] = (s.data_ptr(), flat.data_ptr() + 4 * at, int(s.shape[1]), n)
        at += n
    table = table[table["len_out"] > 0]          # (a one-frame slab has no samples: no record)
    for i in range(0, len(table), 65535):         # (the launch's grid holds 65535 records)
        _fe.istft_launch(table[i:i + 65535], plan, int(table["n_frames"][i:i + 65535].max()))
    for s in slabs:                               # (they must outlive the kernel on this stream)
        s.record_stream(torch.cuda.current_stream(dev))
    return clips, flat


def postfilter_floors(postfilter, behind) -> Tuple[float, np.ndarray]:
    """`extract_events`' postfilter = (alpha, floor_db) and the quiet frames behind each event (`quiet_frames`) as (alpha,
    g_min float64 [E]): g_min = 10^(floor_db / 20), and 1 - the bypass - for an event with 0 quiet frames behind it (a fallback
    block: its covariance contains the event, so the filter would take the event for noise).  ValueError: anything but a pair
    of numbers with alpha in [0, 1) and a finite floor_db <= 0."""
    try:
        alpha, floor_db = postfilter
        bad = any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) for v in (alpha, floor_db))
    except (TypeError, ValueError):
        bad = True
    if bad or not 0.0 <= float(alpha) < 1.0 or not (np.isfinite(floor_db) and float(floor_db) <= 0.0):
        raise ValueError(f"extract: postfilter = {postfilter!r} must be None or (alpha in [0, 1), floor_db: finite, <= 0)")
    floor = 10.0 ** (float(floor_db) / 20.0)
    if not floor > 0.0:
        raise ValueError(f"extract: postfilter floor_db = {floor_db!r} underflows to a gain of 0")
    behind = np.asarray(behind, np.int64).reshape(-1)
    return float(alpha), np.where(behind > 0, floor, 1.0)


def extract_events(spec: torch.Tensor, events, tdoa, block=None, loading: float = WHITEN_LOADING, noise: str = "block",
                   k_lo: int = 0, k_hi=None, context: int = 0, hop=None, guard: int = 0, min_quiet: int = 32, reach: int = 1,
                   postfilter=None):
    """The sound of each event with the interferer nulled: the MVDR (minimum-variance distortionless-response) beamformer
    w = R^-1 d / (d^H R^-1 d) of a two-microphone delay vector, applied over the event's frames, and the inverse STFT of the
    result.  spec: a STEREO complex spectrum [B, F, T, 4] (or [F, T, 4]) = (re0, re1, im0, im1) on a ROCm device, n_fft =
    2 (F - 1); events: integers [E, 3] = (sample, first frame, last frame), frames inclusive; tdoa [E]: each event's delay in
    samples, positive when channel 1 hears it later (`locate_peak`'s sign).  Every event is first widened by `context` frames a
    side, clipped to [0, T).
    Definition, in float64 (`tests/extract_ref.py` restates it in NumPy).  (a, b, c) are `mel_whiten`'s factors of the
    inter-channel covariance of blocks of `block` frames (None: all T) with `loading` (noise="block"), or a = b = 1, c = 0
    (noise="identity": delay-and-sum).  For frame t of an event, block j = t // block, bin k, (a, b, c) of (sample, k, j):
        k outside [k_lo, k_hi) (None: F), a == 0 (a silent block) or tdoa not finite:  Y = 0 exactly
        r = k tdoa / n_fft,  r -= rint(r),  e = cos(2 pi r) - i sin(2 pi r)
        s1 = b (e - c),  den = a^2 + |s1|^2,  g1 = b conj(s1) / den,  g0 = a^2 / den - g1 c
        Y = g0 X0 + g1 X1     ( = s^H z / (s^H s) with z = (a X0, b (X1 - c X0)), s = (a, s1): the MVDR output for d = [1, e] )
    A signal with X1 = e X0 comes through unchanged (distortionless); without factors Y = (X0 + conj(e) X1) / 2.
    Returns (clips, spans): clips[e] a 1-D float32 device tensor of (T_e - 1) hop samples (T_e the widened event's frames; one
    frame gives an empty clip), the inverse STFT (`hop` None: n_fft // 2, load_wav's) of the event's [F, T_e] frames; spans
    int64 [E, 2] = (first hop, last hop), the sample range of the recording the clip stands for.
    The launches are `FrontendPlan.whiten_factors` (noise="block"), `FrontendPlan.beamform` and one `iris_istft` per 65535
    events; there is no CPU fallback.
    noise="quiet" with `guard`, `min_quiet` and `reach`: the covariance from the frames outside the events, as
    `locate_events` describes it; the mask is that of `events` as given, before the context widens them.
    What it cannot do: with noise="block", and with noise="quiet" in a fallback block (`quiet_ranges`), the block covariance
    contains the event, so a steering error on an event that dominates its block makes the beamformer null the event itself
    (1/8 sample on a source 10 dB above the interferer costs 3.5 dB, 10 dB when the event fills 400 of the block's 512 frames;
    at 10 dB under the interferer the loss is under 0.1 dB).
    postfilter = (alpha, floor_db), only with noise="quiet" (ValueError otherwise: a block covariance contains the event, so the
    filter would take the event for noise and remove it, and "identity" has no covariance at all): a decision-directed Wiener
    gain on Y before the inverse STFT - one more launch, `FrontendPlan.postfilter` (`tests/postfilter_ref.py` restates it).
    The beamformer spends its one degree of freedom on the coherent interferer; what it leaves is sensor and diffuse noise,
    whose power at its output is known from the quiet covariance R in closed form.  In float64, with den, g0, g1 as above
    (before any rounding) for bin k in [k_lo, k_hi), frame t, block j:
        S = 1/a^2 + |c|^2/a^2 + 1/b^2                   (the trace of the loaded covariance R + dI)
        d = loading S / (2 (1 + loading))               (the loading itself)
        phi = max(1/den - d (|g0|^2 + |g1|^2), 1e-3 / den)         ( = w^H R w; the floor guards a perfectly coherent R )
        gamma = |Y|^2 / phi;   gamma = 0 where Y is 0 by the definition above
    and along the widened event's frames, p = 1 before the first (Ephraim & Malah's decision-directed a-priori SNR with the
    Wiener gain):
        xi = alpha p + (1 - alpha) max(gamma - 1, 0),   G = max(xi / (1 + xi), g_min),   p = G^2 gamma,   Z = fl32(G) Y
    g_min = 10^(floor_db / 20); an event with no quiet frames behind one of its blocks (`quiet_frames` of the event as given is
    0: a fallback block) gets g_min = 1 and comes out bit for bit as without the filter.  Per real component |Z - exact| <=
    3 x 2^-24 |G| |Y|.  What it costs: the gain floor distorts a source that is already clear of the noise (at 0 dB under the
    interferer the total error against the source rises by about 1 dB while the SINR still gains 8), and it leans on the
    noise being stationary between the quiet frames and the event."""
    if noise not in NOISE_KINDS:
        raise ValueError(f"extract_events: noise = {noise!r} must be 'block', 'identity' or 'quiet'")
    if postfilter is not None:
        if noise != "quiet":
            raise ValueError(f"extract_events: postfilter needs noise='quiet' (a covariance free of the event), not {noise!r}")
        postfilter_floors(postfilter, [])   # (refuses the pair before any device work)
    if not isinstance(spec, torch.Tensor):
        raise TypeError(f"spec must be a torch.Tensor, got {type(spec).__name__}")
    x = spec if spec.dim() == 4 else spec.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 4 or x.shape[1] < 2:
        raise ValueError(f"extract_events: spec must be [B, F >= 2, T, 4] (a stereo complex spectrum), got {tuple(spec.shape)}")
    wide = widen_events(events, context, int(x.shape[2]))
    delays, per_frame = frame_delays(tdoa, wide)
    if not x.is_cuda:
        raise RuntimeError(f"extract_events: spec is on {x.device}: the extraction runs only as HIP kernels on a ROCm device "
                           "(there is no CPU fallback); move the tensor to 'cuda'")
    x = x.float().contiguous()
    plan = _locate_plan(x)
    n_fft = 2 * (int(x.shape[1]) - 1)
    hop = n_fft // 2 if hop is None else int(hop)
    if noise == "quiet":   # (the mask is that of the events as given, not widened by the context)
        fac, quiet = _quiet_factors(plan, x, events, block, loading, guard, min_quiet, reach)
    else:
        fac = plan.whiten_factors(x, block, loading) if noise == "block" else None
    slabs = (plan.beamform_frames if per_frame else plan.beamform)(x, wide, delays, fac, block, k_lo, k_hi)
    if postfilter is not None and len(wide):
        blk = int(x.shape[2]) if block is None else max(min(int(block), int(x.shape[2])), 1)
        alpha, floors = postfilter_floors(postfilter, quiet_frames(events.cpu() if torch.is_tensor(events) else events, quiet, blk))
        slabs = plan.postfilter(slabs, wide, delays, fac, blk, loading, k_lo, k_hi, alpha, floors, per_frame)
    clips, _ = clips_from_slabs(slabs, hop)
    return clips, wide[:, 1:] * hop


def log_magphase(specs: torch.Tensor, labels=None, n_chan: int = 2):
    """ln(x + EPSILON) on the first n_chan trailing channels, the rest passes through
    (transforms.py:80-86)."""
    if not torch.is_floating_point(specs):
        specs = specs.to(torch.float32)
    specs = torch.cat([torch.log(specs[..., :n_chan] + EPSILON), specs[..., n_chan:]], dim=-1)
    if labels is not None:
        return specs, labels
    return specs


def minmax_norm_magphase(specs: torch.Tensor, labels=None):
    """(x - min) / (max - min + EPSILON) per sample, separately for the magnitude and
    the phase halves (transforms.py:89-107)."""
    n_chan = specs.shape[-1] // 2
    axis = tuple(range(1, specs.dim()))
    out = []
    for part in (specs[..., :n_chan], specs[..., n_chan:]):
        mx = torch.amax(part, dim=axis, keepdim=True)
        mn = torch.amin(part, dim=axis, keepdim=True)
        out.append((part - mn) / (mx - mn + EPSILON))
    specs = torch.cat(out, dim=-1)
    if labels is not None:
        return specs, labels
    return specs


# ---------------------------------------------------------------------------
# COMPLEX-SPECTROGRAMS
# ---------------------------------------------------------------------------
def complex_to_magphase(complex_tensor: torch.Tensor, y=None):
    """[..., 2C] (re block, im block) -> (|z|, atan2(im, re)) (transforms.py:111-123)."""
    magphase = _fe.complex_to_magphase(complex_tensor)
    if y is None:
        return magphase
    return magphase, y


def magphase_to_complex(magphase: torch.Tensor) -> torch.Tensor:
    """Inverse of complex_to_magphase (transforms.py:126-134)."""
    if magphase.is_cuda:
        return _fe.magphase_to_complex(magphase)
    n_chan = magphase.shape[-1] // 2
    mag, phase = magphase[..., :n_chan], magphase[..., n_chan:]
    return torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], dim=-1)


def phase_vocoder(complex_spec: torch.Tensor, rate: float = 1.0) -> torch.Tensor:
    """Time-stretch a [freq, time, chan*2] spectrogram by `rate` (transforms.py:137-195):
    hop_length = freq - 1, phase advance linspace(0, pi*hop, freq), wrapped phase
    differences accumulated with the first frame's phase prepended, magnitudes linearly
    interpolated.  Output time length ceil(time / rate).
    (Torch glue on any device and dtype; `time_stretch` is the batched HIP form, with the phase kept in [-pi, pi].)"""
    if rate == 1:
        return complex_spec
    spec = complex_spec
    freq = spec.shape[0]
    hop_length = freq - 1
    n_chan = spec.shape[-1] // 2
    dt = spec.dtype

    def angle(s):
        return torch.atan2(s[..., n_chan:], s[..., :n_chan])

    phase_advance = torch.linspace(0.0, float(np.pi * hop_length), freq, dtype=dt, device=spec.device).reshape(-1, 1, 1)
    time_steps = torch.arange(0, spec.shape[1], rate, dtype=dt, device=spec.device)
    padded = torch.nn.functional.pad(spec, (0, 0, 0, 2))
    i0 = time_steps.to(torch.int64)
    i1 = (time_steps + 1).to(torch.int64)
    spec_0, spec_1 = padded[:, i0], padded[:, i1]
    angle_0, angle_1 = angle(spec_0), angle(spec_1)
    norm_0 = torch.sqrt(spec_0[..., :n_chan] ** 2 + spec_0[..., n_chan:] ** 2)
    norm_1 = torch.sqrt(spec_1[..., :n_chan] ** 2 + spec_1[..., n_chan:] ** 2)
    phase_0 = angle(padded[:, :1])
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * np.pi * torch.round(phase / (2 * np.pi))  # round half to even, as tf.math.round
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[:, :-1]], dim=1)
    phase_acc = torch.cumsum(phase, dim=1)
    alphas = (time_steps % 1.0).reshape(1, -1, 1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return torch.cat([mag * torch.cos(phase_acc), mag * torch.sin(phase_acc)], dim=-1)


def time_stretch(complex_spec: torch.Tensor, rate: float = 1.0) -> torch.Tensor:
    """`phase_vocoder` of one [freq, time, chan*2] float32 spectrogram on a ROCm device as ONE HIP launch
    (`frontend.phase_vocoder_batch`, iris_phase_vocoder): the same frame pairs and formulas with the time grid in double
    and the running phase reduced to [-pi, pi], three orders of magnitude closer to a float64 evaluation than the fp32
    torch form above.  Returns a new tensor (a copy at rate 1).  CPU tensors raise: there is no CPU fallback."""
    return _fe.phase_vocoder_batch([complex_spec], [rate])[0]


def speed_perturb(wav: torch.Tensor, rate: float = 1.0) -> torch.Tensor:
    """Speed perturbation of one [chan, samples] (or [samples]) float32 waveform on a ROCm device as ONE HIP launch
    (`frontend.speed_perturb_batch`, iris_speed_perturb): resampled by `rate` with torchaudio's Hann-windowed sinc and played
    back at the old sample rate, so tempo and pitch move together (rate > 1 = faster, shorter, higher); ceil(samples / rate)
    samples.  Returns a new tensor (a copy at rate 1).  CPU tensors raise: there is no CPU fallback."""
    if isinstance(wav, torch.Tensor) and wav.dim() == 1:
        return _fe.speed_perturb_batch([wav.unsqueeze(0)], [rate])[0][0]
    return _fe.speed_perturb_batch([wav], [rate])[0]


def reverb(wav: torch.Tensor, rir) -> torch.Tensor:
    """Reverberation of one [chan, samples] (or [samples]) float32 waveform on a ROCm device as ONE HIP launch
    (`frontend.fir_batch`, iris_fir_batch): every channel convolved with its row of the room impulse response `rir`
    [chan, taps <= 4096] (a tensor on the same device, or an array such as `synth_rir` returns), causal and cut at the input
    length - the direct sound at tap 0, the ringing past the end dropped.  Returns a new tensor of the input's shape.  CPU
    waveforms raise: there is no CPU fallback."""
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        raise ValueError("reverb: the waveform must be a float32 tensor on a ROCm device (there is no CPU fallback)")
    if not isinstance(rir, torch.Tensor):
        rir = torch.as_tensor(np.ascontiguousarray(np.asarray(rir, np.float32))).to(wav.device)
    if wav.dim() == 1:
        return _fe.fir_batch([wav.unsqueeze(0)], [rir.reshape(1, -1)])[0][0]
    return _fe.fir_batch([wav], [rir])[0]


def reverb_fft(wav: torch.Tensor, rir) -> torch.Tensor:
    """`reverb` for long responses: the same causal convolution cut at the input length, run as a partitioned overlap-save
    convolution on the FFT core (`frontend.fft_fir_batch`, iris_fft_fir_batch: two launches), `rir` [chan, taps <= 32768]
    (2 s at 16 kHz).  Accurate norm-wise per block of 1024 outputs, not tap by tap: an identity response
    copies the waveform within that rule, not bit for bit.  Returns a new tensor of the input's shape.  CPU waveforms raise:
    there is no CPU fallback."""
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        raise ValueError("reverb_fft: the waveform must be a float32 tensor on a ROCm device (there is no CPU fallback)")
    if not isinstance(rir, torch.Tensor):
        rir = torch.as_tensor(np.ascontiguousarray(np.asarray(rir, np.float32))).to(wav.device)
    if wav.dim() == 1:
        return _fe.fft_fir_batch([wav.unsqueeze(0)], [rir.reshape(1, -1)])[0][0]
    return _fe.fft_fir_batch([wav], [rir])[0]


def load_rirs(rir_dir: str, channels: int, sample_rate: int = 16000, max_taps: int = 16384) -> list:
    """Measured room impulse responses for `WaveMixer.enable_reverb(rirs=)`: sorted(glob(rir_dir/*.wav)) read by
    `data_utils.read_wav_file` as a list of float32 [channels, K_i <= max_taps] arrays.  A file at another rate is brought to
    `sample_rate` by `frontend.resample` (that needs a ROCm device; files at `sample_rate` never touch one).  Per file: the
    samples before max(0, i0 - 16) are dropped, i0 = the earliest channel's peak index (the direct sound then sits within
    the first millisecond and the delay between the channels is kept); the response is cut at `max_taps`; all channels are
    scaled by ONE factor so that the loudest channel has unit L2 norm (the level difference between the channels is kept; no
    rms scaling as for recordings).  A mono file is copied to every channel.  A file with another channel count, a
    directory without *.wav, or a response that is all zeros is a ValueError."""
    import os
    from glob import glob

    from .data_utils import read_wav_file
    channels, max_taps = int(channels), int(max_taps)
    if channels < 1 or max_taps < 1:
        raise ValueError(f"load_rirs: channels = {channels} and max_taps = {max_taps} must be positive")
    paths = sorted(glob(os.path.join(rir_dir, "*.wav")))
    if not paths:
        raise ValueError(f"load_rirs: no *.wav in {rir_dir!r}")
    rirs = []
    for path in paths:
        data, sr = read_wav_file(path)
        if data.shape[0] not in (1, channels):
            raise ValueError(f"load_rirs: {path!r} has {data.shape[0]} channels; expected 1 or {channels}")
        if data.shape[1] < 1:
            raise ValueError(f"load_rirs: {path!r} is empty")
        if int(sr) != int(sample_rate):
            if not torch.cuda.is_available():
                raise RuntimeError(f"load_rirs: {path!r} is at {sr} Hz; resampling to {sample_rate} Hz needs a ROCm device")
            data = _fe.resample(torch.from_numpy(np.ascontiguousarray(data, np.float32)).to("cuda"), int(sr), int(sample_rate)).cpu().numpy()
        h = np.asarray(data, np.float64)
        if h.shape[0] == 1:
            h = np.repeat(h, channels, axis=0)
        if not np.any(h):
            raise ValueError(f"load_rirs: {path!r} is all zeros")
        i0 = int(np.abs(h).argmax(axis=1).min())
        h = h[:, max(0, i0 - 16):][:, :max_taps]
        norm = float(np.sqrt((h * h).sum(axis=1)).max())
        if not norm > 0:
            raise ValueError(f"load_rirs: {path!r} is all zeros within its first {max_taps} taps")
        rirs.append(np.ascontiguousarray((h / norm).astype(np.float32)))
    return rirs


def synth_rir(rng: np.random.Generator, channels: int, rt60: float, drr_db: float = 0.0, sample_rate: int = 16000,
              floor_db: float = -40.0, max_taps: int = 4096) -> np.ndarray:
    """A synthetic room impulse response [channels, K] float32, built on the host in float64: the exponentially decaying
    Gaussian-noise model.  K = min(max_taps, max(1, ceil(rt60 * sample_rate * (-floor_db) / 60))) - the decay followed down to
    `floor_db`; h[c, 0] = 1 (the direct sound) and h[c, k] = g_c n[c, k] 10^(-3 k / (rt60 sample_rate)) for k >= 1 (60 dB of
    decay per `rt60` seconds) with n ~ N(0, 1) drawn from `rng` independently per channel, g_c such that the tail's energy is
    10^(-drr_db / 10) times the direct tap's (`drr_db`: the direct-to-reverberant ratio); each channel is finally scaled to
    unit L2 norm, so a white input keeps its power.  rt60 <= 0 is the identity [[1.0]] * channels."""
    channels, max_taps = int(channels), int(max_taps)
    rt60, drr_db, sample_rate, floor_db = float(rt60), float(drr_db), float(sample_rate), float(floor_db)
    if channels < 1 or max_taps < 1:
        raise ValueError(f"synth_rir: channels = {channels} and max_taps = {max_taps} must be positive")
    if not (np.isfinite(rt60) and np.isfinite(drr_db)):
        raise ValueError(f"synth_rir: rt60 = {rt60} and drr_db = {drr_db} must be finite")
    if not (np.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"synth_rir: sample_rate = {sample_rate} must be positive and finite")
    if not (np.isfinite(floor_db) and floor_db < 0):
        raise ValueError(f"synth_rir: floor_db = {floor_db} must be negative and finite (how far down the decay is followed)")
    if rt60 <= 0:
        return np.ones((channels, 1), np.float32)
    n_taps = min(max_taps, max(1, int(np.ceil(rt60 * sample_rate * (-floor_db) / 60.0))))
    h = np.zeros((channels, n_taps), np.float64)
    h[:, 0] = 1.0
    if n_taps > 1:
        k = np.arange(1, n_taps, dtype=np.float64)
        tail = rng.standard_normal((channels, n_taps - 1)) * np.power(10.0, -3.0 * k / (rt60 * sample_rate))[None, :]
        energy = np.sum(tail * tail, axis=1, keepdims=True)
        if np.any(energy <= 0):
            raise ValueError("synth_rir: the drawn tail has no energy")
        h[:, 1:] = tail * np.sqrt(np.power(10.0, -drr_db / 10.0) / energy)
    h /= np.sqrt(np.sum(h * h, axis=1, keepdims=True))
    return h.astype(np.float32)


def shoebox_beta(room, rt60: float) -> float:
    """The wall reflection coefficient (one for the six walls) of a shoebox `room` (L_x, L_y, L_z in metres) whose reverberation
    time is `rt60` seconds, by Eyring's formula: beta = exp(-12 ln(10) V / (c S rt60)) with V the volume, S the surface and
    c = 343 m/s (rt60 = 24 ln(10) V / (-c S ln(beta^2))).  rt60 <= 0 gives 0: the anechoic response."""
    room, rt60 = np.asarray(room, np.float64).reshape(-1), float(rt60)
    if room.shape != (3,) or not (np.all(np.isfinite(room)) and np.all(room > 0)):
        raise ValueError(f"shoebox_beta: room = {room} must be three positive finite sizes")
    if not np.isfinite(rt60):
        raise ValueError(f"shoebox_beta: rt60 = {rt60} must be finite")
    if rt60 <= 0:
        return 0.0
    volume = float(np.prod(room))
    surface = 2.0 * float(room[0] * room[1] + room[1] * room[2] + room[0] * room[2])
    return float(np.exp(-12.0 * np.log(10.0) * volume / (_fe.ISM_SOUND * surface * rt60)))


def shoebox_taps(rt60: float, sample_rate: int = 16000, floor_db: float = -40.0, max_taps: int = 4096) -> int:
    """Taps of a shoebox response that follows the decay down to `floor_db`: `synth_rir`'s rule
    min(max_taps, max(1, ceil(rt60 sample_rate (-floor_db) / 60))) plus the 2 W = 32 taps of the fractional-delay filter (the
    direct sound sits at tap W, not 0), capped at `max_taps`."""
    rt60, sample_rate, floor_db, max_taps = float(rt60), float(sample_rate), float(floor_db), int(max_taps)
    if not np.isfinite(rt60) or max_taps < 1:
        raise ValueError(f"shoebox_taps: rt60 = {rt60} must be finite and max_taps = {max_taps} positive")
    if not (np.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"shoebox_taps: sample_rate = {sample_rate} must be positive and finite")
    if not (np.isfinite(floor_db) and floor_db < 0):
        raise ValueError(f"shoebox_taps: floor_db = {floor_db} must be negative and finite")
    decay = min(max_taps, max(1, int(np.ceil(max(rt60, 0.0) * sample_rate * (-floor_db) / 60.0))))
    return min(max_taps, decay + 2 * _fe.ISM_HALF_WIDTH)


def draw_shoebox(rng: np.random.Generator, channels: int, rt60: float, mic_spacing: float = 0.1, margin: float = 0.5,
                 sample_rate: int = 16000, max_taps: int = 4096, tries: int = 100) -> dict:
    """One random shoebox geometry on the host: a dict of room [3], source [3], mics [channels, 3] (float64, metres), beta
    (`shoebox_beta(room, rt60)`) and n_taps (`shoebox_taps(rt60)`).  The room is U[3, 8) x U[3, 8) x U[2.5, 4) m; the array
    centre is uniform in the room at least `margin` from every wall, the microphones sit on a line along x, `mic_spacing`
    apart, centred there; the source is uniform at least `margin` from every wall and at least `margin` from the array centre,
    redrawn until that holds (`tries` times at most, then a ValueError).  These ranges are defaults of the augmentation - a
    living-room-sized box and a small array - not measurements of any corpus."""
    channels, rt60, mic_spacing, margin = int(channels), float(rt60), float(mic_spacing), float(margin)
    if not 1 <= channels <= _fe.ISM_MAX_CHAN:
        raise ValueError(f"draw_shoebox: channels = {channels}; 1 .. {_fe.ISM_MAX_CHAN} microphones are supported")
    if not (np.isfinite(rt60) and np.isfinite(mic_spacing) and np.isfinite(margin) and mic_spacing >= 0 and margin > 0):
        raise ValueError(f"draw_shoebox: rt60 = {rt60}, mic_spacing = {mic_spacing} >= 0 and margin = {margin} > 0 must be finite")
    half = 0.5 * mic_spacing * (channels - 1)
    if 2.0 * margin >= 2.5 or 2.0 * (margin + half) >= 3.0:
        raise ValueError(f"draw_shoebox: margin = {margin} and an array {2 * half} m long do not fit the smallest room (3 x 3 x 2.5 m)")
    room = np.array([rng.uniform(3.0, 8.0), rng.uniform(3.0, 8.0), rng.uniform(2.5, 4.0)])
    lo = np.array([margin + half, margin, margin])
    centre = lo + rng.uniform(0.0, 1.0, 3) * (room - 2.0 * lo)
    mics = np.repeat(centre[None, :], channels, axis=0)
    mics[:, 0] += mic_spacing * (np.arange(channels) - 0.5 * (channels - 1))
    for _ in range(int(tries)):
        source = margin + rng.uniform(0.0, 1.0, 3) * (room - 2.0 * margin)
        if np.sqrt(np.sum((source - centre) ** 2)) >= margin:
            return {"room": room, "source": source, "mics": mics, "beta": shoebox_beta(room, rt60),
                    "n_taps": shoebox_taps(rt60, sample_rate, max_taps=max_taps)}
    raise ValueError(f"draw_shoebox: no source at least {margin} m from the array in {tries} tries")


def _flyby_range(name: str, rng_, lo_min: float, lo_open: bool = False):
    """(lo, hi) of a `draw_flyby` range: finite, lo_min <= lo <= hi (lo_min < lo with lo_open)."""
    try:
        lo, hi = (float(x) for x in rng_)
    except (TypeError, ValueError):
        raise ValueError(f"draw_flyby: {name} = {rng_!r} must be a (lo, hi) pair") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi and (lo > lo_min if lo_open else lo >= lo_min)):
        raise ValueError(f"draw_flyby: {name} = ({lo}, {hi}) must be finite with {lo_min} {'<' if lo_open else '<='} lo <= hi")
    return lo, hi


def draw_flyby(rng: np.random.Generator, channels: int, seconds: float, mic_spacing: float = 0.1, altitude=(5.0, 30.0),
               speed=(0.0, 15.0), miss=(0.0, 20.0), z_s: float = 1.5, beta=(0.0, 0.6)) -> dict:
    """One random fly-by on the host: a dict of p0 [3] (the array centre at t = 0), v [3] (float64, metres and metres per
    second), z_s, beta and mics [channels, 3] (offsets from the centre) - what `frontend.flyby_records` packs.  The source stands
    at (0, 0, z_s) on the ground plane z = 0.  Level flight at an altitude ~ U[altitude) with speed ~ U[speed) on a heading ~
    U[0, 2 pi) that passes the source at a horizontal distance ~ U[miss) at a time ~ U[0, seconds); ground reflection coefficient
    ~ U[beta) (drawn in this order).  The microphones sit on a line along x, `mic_spacing` apart and centred, as `draw_shoebox`
    places them; the array does not rotate.  With hi == lo a range is that value.  These ranges are defaults of the augmentation
    - a small drone over a standing person - not measurements of any corpus.  ValueError: channels outside 1 .. 8, seconds,
    mic_spacing or z_s negative or not finite, a range that is not a finite (lo <= hi) pair, an altitude that does not stay above
    z_s, a speed range outside [0, 343), a miss distance below 0, beta outside [0, 1)."""
    channels, seconds, mic_spacing, z_s = int(channels), float(seconds), float(mic_spacing), float(z_s)
    if not 1 <= channels <= _fe.FLYBY_MAX_CHAN:
        raise ValueError(f"draw_flyby: channels = {channels}; 1 .. {_fe.FLYBY_MAX_CHAN} microphones are supported")
    if not (np.isfinite(seconds) and np.isfinite(mic_spacing) and np.isfinite(z_s) and seconds >= 0 and mic_spacing >= 0 and z_s >= 0):
        raise ValueError(f"draw_flyby: seconds = {seconds}, mic_spacing = {mic_spacing} and z_s = {z_s} must be finite and >= 0")
    altitude, speed = _flyby_range("altitude", altitude, z_s, lo_open=True), _flyby_range("speed", speed, 0.0)
    miss, beta = _flyby_range("miss", miss, 0.0), _flyby_range("beta", beta, 0.0)
    if not speed[1] < _fe.ISM_SOUND:
        raise ValueError(f"draw_flyby: speed = {speed} must stay below the sound speed {_fe.ISM_SOUND} m/s")
    if beta[0] >= 1.0 or beta[1] > 1.0:
        raise ValueError(f"draw_flyby: beta = {beta} must stay inside [0, 1)")
    h, s, heading = rng.uniform(*altitude), rng.uniform(*speed), rng.uniform(0.0, 2.0 * np.pi)
    b, t_c, refl = rng.uniform(*miss), rng.uniform(0.0, seconds), rng.uniform(*beta)
    v = np.array([s * np.cos(heading), s * np.sin(heading), 0.0])
    closest = np.array([-b * np.sin(heading), b * np.cos(heading), h])   # the centre at t_c: abeam of the source
    mics = np.zeros((channels, 3))
    mics[:, 0] = mic_spacing * (np.arange(channels) - 0.5 * (channels - 1))
    return {"p0": closest - v * t_c, "v": v, "z_s": z_s, "beta": float(refl), "mics": mics}


def flyby(wav: torch.Tensor, geometry: dict) -> torch.Tensor:
    """The fly-by of one [chan, samples] (or [samples]) float32 voice at 16 kHz on a ROCm device as ONE HIP launch
    (`frontend.flyby_batch`, iris_flyby): every channel under the time-varying delay and spreading gain of its microphone of
    `geometry` (a `draw_flyby` dict), plus the ground reflection.  Returns a new tensor of the input's shape.  CPU tensors
    raise: there is no CPU fallback."""
    if isinstance(wav, torch.Tensor) and wav.dim() == 1:
        return _fe.flyby_batch([wav.unsqueeze(0)], [geometry])[0][0]
    return _fe.flyby_batch([wav], [geometry])[0]


def shoebox_rir(room, source, mics, rt60: float, device, n_taps=None, normalize: bool = True, sample_rate: int = 16000) -> torch.Tensor:
    """One shoebox room impulse response [chan, K] float32 on a ROCm `device` as ONE HIP launch (`frontend.shoebox_rir_batch`,
    iris_ism_rir): the image-source method for the room (L_x, L_y, L_z), the `source` and the microphones `mics` [chan, 3], the
    wall reflection coefficient from `rt60` by Eyring's formula (`shoebox_beta`), K = `n_taps` or `shoebox_taps(rt60)`.  The
    nearest microphone's direct sound is a unit tap (before `normalize`) at k = 16.  There is no CPU fallback."""
    k = shoebox_taps(rt60, sample_rate) if n_taps is None else int(n_taps)
    mics = np.asarray(mics, np.float64)
    mics = mics.reshape(1, 3) if mics.ndim == 1 else mics
    return _fe.shoebox_rir_batch([room], [source], [mics], [shoebox_beta(room, rt60)], [k], normalize=normalize,
                                 sample_rate=sample_rate, device=device)[0]
