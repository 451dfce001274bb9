"""Torch-facing wrapper of the HIP frontend (C ABI: include/iris_frontend.h).

PyTorch is plumbing here: it owns device memory and streams; every numeric op on
the hot path is a hand-written HIP kernel in csrc/iris_frontend.hip.  Tensors
must be float32, contiguous and on a ROCm device -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import weakref
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native as N

EPSILON = 1e-8


def _require_device_f32(x: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(
            f"{name} is on {x.device}: the feature frontend runs only as HIP kernels on a "
            "ROCm device (there is no CPU fallback); move the tensor to 'cuda'")
    if x.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {x.dtype}")
    return x.contiguous()


def _stream_ptr(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _bands_arg(bands, batch: int, device: torch.device, name: str):
    """bands: None or int tensor/array [B, n, 2] of (offset, size)."""
    if bands is None:
        return None, C.c_void_p(0), 0
    t = torch.as_tensor(bands)
    if t.dim() != 3 or t.shape[0] != batch or t.shape[2] != 2:
        raise ValueError(f"{name} must have shape [batch={batch}, n, 2], got {tuple(t.shape)}")
    t = t.to(device=device, dtype=torch.int32).contiguous()
    if t.shape[1] == 0:
        return None, C.c_void_p(0), 0
    return t, C.c_void_p(t.data_ptr()), int(t.shape[1])


def _gain_arg(mel_gain, batch: int, n_mel: int, device: torch.device):
    """mel_gain: None or float32 [B, n_mel] (FilterAugment: one gain per sample and mel band, shared by the channels)."""
    if mel_gain is None:
        return None
    g = torch.as_tensor(mel_gain)
    if tuple(g.shape) != (batch, n_mel):
        raise ValueError(f"mel_gain must have shape [batch={batch}, n_mel={n_mel}], got {tuple(g.shape)}")
    return g.to(device=device, dtype=torch.float32).contiguous()


def mel_weight_matrix(num_mel_bins: int = 20, num_spectrogram_bins: int = 129,
                      sample_rate: float = 8000, lower_edge_hertz: float = 125.0,
                      upper_edge_hertz: float = 3800.0) -> np.ndarray:
    """W[F, M] as the reference's closure builds it (transforms.py:55-56), via
    the library's host routine (fp32 recipe).  Raises ValueError on bad edges."""
    out = np.empty((num_spectrogram_bins, num_mel_bins), np.float32)
    rc = N.lib().iris_mel_weight_matrix(int(num_mel_bins), int(num_spectrogram_bins),
                                        float(sample_rate), float(lower_edge_hertz),
                                        float(upper_edge_hertz),
                                        out.ctypes.data_as(C.POINTER(C.c_float)))
    N.check(rc, "iris_mel_weight_matrix")
    return out


_LIVE_PLANS: "weakref.WeakSet[FrontendPlan]" = weakref.WeakSet()


def check_plans(device=None) -> None:
    """Raise EpilogueTimeout if any live plan (on `device`, or anywhere) reports a failed fused-epilogue wait.
    Synchronises; meant for the places that synchronise anyway (`sj_train.fit` calls it once per epoch)."""
    dev = None if device is None else torch.device(device)
    for plan in list(_LIVE_PLANS):
        if plan._handle is None or plan.n_fft == 0:
            continue
        if dev is not None and dev.type == "cuda" and dev.index is not None and plan.device != dev:
            continue
        plan.raise_on_failure()


class FrontendPlan:
    """State of `Spectrogram(n_fft, power=None)` (data_utils.py:17) plus the
    `magphase_to_mel(...)` closure (transforms.py:51-56) on one device."""

    def __init__(self, n_fft: int = 512, hop: Optional[int] = None, n_mel: int = 80,
                 sample_rate: float = 16000, channels: int = 1, max_batch: int = 64,
                 max_len: int = 160000, device=None, lower_edge_hertz: float = 125.0,
                 upper_edge_hertz: float = 3800.0, mel_matrix: Optional[np.ndarray] = None):
        self._handle = None
        lib = N.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("FrontendPlan needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback for the feature frontend")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"FrontendPlan device must be a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_fft, self.hop = int(n_fft), int(n_fft // 2 if hop is None else hop)
        self.n_mel, self.n_bins = int(n_mel), int(n_fft) // 2 + 1
        self.sample_rate, self.channels = float(sample_rate), int(channels)
        self.max_batch, self.max_len = int(max_batch), int(max_len)
        mel_ptr = None
        if mel_matrix is not None:
            mel_matrix = np.ascontiguousarray(mel_matrix, np.float32)
            if mel_matrix.shape != (self.n_bins, self.n_mel):
                raise ValueError(f"mel_matrix must be [{self.n_bins}, {self.n_mel}]")
            mel_ptr = mel_matrix.ctypes.data_as(C.POINTER(C.c_float))
        handle = C.c_void_p()
        rc = lib.iris_plan_create(C.byref(handle), self.device.index, self.n_fft, self.hop,
                                  self.n_mel, self.n_bins, self.sample_rate,
                                  float(lower_edge_hertz), float(upper_edge_hertz), self.channels,
                                  self.max_batch, self.max_len, mel_ptr)
        N.check(rc, "iris_plan_create")
        self._handle = handle
        self._lock = threading.Lock()
        self.mel_precision = "fp32"
        masked = "ROC_GLOBAL_CU_MASK" in os.environ or "HSA_CU_MASK" in os.environ  # the library starts such plans on two kernels
        env = os.environ.get("IRIS_EPILOGUE")
        self.epilogue = "two_kernels" if (env == "1" or (masked and env is None)) else ("in_place" if env == "2" else "fused")
        _LIVE_PLANS.add(self)

    @classmethod
    def mel_only(cls, n_mel: int, n_bins: int, channels: int, max_batch: int, device,
                 mel_matrix: np.ndarray) -> "FrontendPlan":
        """Plan for magphase_to_mel on spectra of an arbitrary bin count (no FFT ops)."""
        self = cls.__new__(cls)
        self._handle = None
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_fft, self.hop, self.n_mel, self.n_bins = 0, 1, int(n_mel), int(n_bins)
        self.sample_rate, self.channels = 0.0, int(channels)
        self.max_batch, self.max_len = int(max_batch), 1
        mel_matrix = np.ascontiguousarray(mel_matrix, np.float32)
        if mel_matrix.shape != (self.n_bins, self.n_mel):
            raise ValueError(f"mel_matrix must be [{self.n_bins}, {self.n_mel}]")
        handle = C.c_void_p()
        rc = N.lib().iris_plan_create(C.byref(handle), self.device.index, 0, 1, self.n_mel, self.n_bins, 1.0, 0.0,
                                      0.5, self.channels, self.max_batch, 1,
                                      mel_matrix.ctypes.data_as(C.POINTER(C.c_float)))
        N.check(rc, "iris_plan_create")
        self._handle = handle
        self._lock = threading.Lock()
        return self

    def set_mel_precision(self, precision: str = "fp32") -> None:
        """'fp32' (default): banded fp32 mel reduction, 1e-5.  'fp16_mfma': |X| and W in fp16 on the matrix cores
        (v_mfma_f32_16x16x32_f16, fp32 accumulate; BASELINE configs[4]), 2e-3; raises ValueError when the plan's
        shape / filterbank cannot use it.  Calls that carry SpecAugment bands always run fp32."""
        code = {"fp32": N.IRIS_MEL_F32, "fp16_mfma": N.IRIS_MEL_F16_MFMA}[precision]
        N.check(N.lib().iris_plan_set_mel_precision(self._handle, code), "iris_plan_set_mel_precision")
        self.mel_precision = precision

    def set_epilogue(self, mode: str = "fused") -> None:
        """'fused' (default): min-max / log inside the fused kernel, one launch per call.  'two_kernels': raw mel +
        per-wave partials, then the min-max / log kernel - for several plans running CONCURRENTLY on one device
        (see iris_plan_set_epilogue in include/iris_frontend.h); calls under hipGraph capture take it by themselves."""
        code = {"fused": N.IRIS_EPILOGUE_FUSED, "two_kernels": N.IRIS_EPILOGUE_TWO_KERNELS, "in_place": N.IRIS_EPILOGUE_IN_PLACE}[mode]
        N.check(N.lib().iris_plan_set_epilogue(self._handle, code), "iris_plan_set_epilogue")
        self.epilogue = mode

    def last_epilogue(self) -> Optional[str]:
        """Form the last `wav_to_logmel` call took: 'fused' (min-max / log from the chunk's LDS tile), 'in_place' (one launch,
        the workgroup finishes its rows of `out` in place: chunks too large for the tile), 'two_kernels'; None before the
        first call or when neither min-max nor log was applied."""
        form = C.c_int(-1)
        N.check(N.lib().iris_plan_last_epilogue(self._handle, C.byref(form)), "iris_plan_last_epilogue")
        return {N.IRIS_EPILOGUE_FUSED: "fused", N.IRIS_EPILOGUE_TWO_KERNELS: "two_kernels", N.IRIS_EPILOGUE_IN_PLACE: "in_place"}.get(form.value)

    def status(self) -> int:
        """0 = every bounded in-kernel wait of the fused epilogue completed so far; 1 = one gave up (clips written as
        NaN).  Synchronises with the device and resets the word; after a 1 the plan stays on the two-kernel form."""
        st = C.c_int(0)
        N.check(N.lib().iris_plan_status(self._handle, C.byref(st)), "iris_plan_status")
        if st.value:
            self.epilogue = "two_kernels"
        return st.value

    def raise_on_failure(self) -> None:
        """`status()` as an exception: EpilogueTimeout naming the plan.  Call where a synchronisation happens anyway
        (end of an epoch, after reading a loss); the hot path itself reports a failed EARLIER launch without any
        synchronisation - the next `wav_to_logmel` on the plan raises the same exception."""
        if self._handle is not None and self.status():
            raise N.EpilogueTimeout(
                f"FrontendPlan(n_fft={self.n_fft}, hop={self.hop}, n_mel={self.n_mel}, channels={self.channels}, "
                f"max_batch={self.max_batch}, device={self.device}): a fused min-max / log epilogue gave up waiting for "
                "its clip's other workgroups (not co-resident: concurrent kernels, a CU mask or another process on the "
                "device) and wrote NaN features; the plan now uses the two-kernel form")

    def set_epilogue_timeout(self, microseconds: int) -> None:
        """Bound of the fused epilogue's in-kernel waits (default 2 s).  0 gives up after the first sweep: the test hook
        that makes the failure path reachable on a healthy device."""
        N.check(N.lib().iris_plan_set_epilogue_timeout(self._handle, int(microseconds)), "iris_plan_set_epilogue_timeout")

    def close(self) -> None:
        if self._handle is not None:
            N.lib().iris_plan_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- introspection ---------------------------------------------------
    def num_frames(self, length: int) -> int:
        return 1 + int(length) // self.hop

    @property
    def mel_matrix(self) -> np.ndarray:
        out = np.empty((self.n_bins, self.n_mel), np.float32)
        N.check(N.lib().iris_plan_get_mel(self._handle, out.ctypes.data_as(C.POINTER(C.c_float))),
                "iris_plan_get_mel")
        return out

    def _check_wav(self, wav: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
        wav = _require_device_f32(wav, "wav")
        if wav.device != self.device:
            raise RuntimeError(f"wav is on {wav.device}, plan is on {self.device}")
        if wav.dim() != 3 or wav.shape[1] != self.channels:
            raise ValueError(f"wav must be [B, C={self.channels}, L], got {tuple(wav.shape)}")
        return wav, int(wav.shape[0]), int(wav.shape[2])

    # ---- ops ---------------------------------------------------------------
    def stft(self, wav: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """wav [B,C,L] -> spec [B,F,T,2C] (load_wav, data_utils.py:17-27).  `normalize`: the wav / (10 rms) of
        data_utils.py:22-23 folded in (per clip, all channels jointly; the spectrum is scaled as it is written)."""
        wav, b, length = self._check_wav(wav)
        t = self.num_frames(length)
        spec = torch.empty((b, self.n_bins, t, 2 * self.channels), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_stft(self._handle, wav.data_ptr(), spec.data_ptr(), b, length,
                                   N.IRIS_F_NORMALIZE if normalize else 0, _stream_ptr(self.device))
        N.check(rc, "iris_stft")
        return spec

    def istft(self, spec: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
        """spec [B,F,T,2C] -> wav [B,C,L]: the inverse of `stft` (torch.istft with the periodic Hann window, center=True),
        L = `length` or (T - 1) hop, at most (T - 1) hop.  Each clip is one record of one `iris_istft` launch."""
        spec = _require_device_f32(spec, "spec")
        if spec.device != self.device:
            raise RuntimeError(f"spec is on {spec.device}, plan is on {self.device}")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 2 * self.channels or self.n_fft == 0:
            raise ValueError(f"spec must be [B, F={self.n_bins}, T, 2C={2 * self.channels}] on a plan with an FFT, got {tuple(spec.shape)}")
        b, t = int(spec.shape[0]), int(spec.shape[2])
        full = istft_len(t, self.hop)
        length = full if length is None else int(length)
        if t < 2 or not 0 < length <= full:
            raise ValueError(f"istft: {t} frames at hop {self.hop} give at most {full} samples, asked for {length}")
        wav = torch.empty((b, self.channels, length), dtype=torch.float32, device=self.device)
        if b == 0:
            return wav
        table = np.zeros(b, ISTFT_SRC)
        table["src"] = spec.data_ptr() + np.arange(b, dtype=np.uint64) * np.uint64(spec.stride(0) * 4)
        table["dst"] = wav.data_ptr() + np.arange(b, dtype=np.uint64) * np.uint64(wav.stride(0) * 4)
        table["n_frames"], table["len_out"] = t, length
        istft_launch(table, self, t)
        spec.record_stream(torch.cuda.current_stream(self.device))
        return wav

    def magmel(self, spec: torch.Tensor, is_magphase: bool = False, t_bands=None, f_bands=None, mel_gain=None) -> torch.Tensor:
        """spec [B,F,T,2C] -> mel [B,M,T,C] (complex_to_magphase + magphase_to_mel).  mel_gain ([B, M] float32, optional:
        FilterAugment): every mel value times its sample's band gain inside the kernel (`iris_magmel_gain`)."""
        spec = _require_device_f32(spec, "spec")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 2 * self.channels:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, {2 * self.channels}], got {tuple(spec.shape)}")
        b, t = int(spec.shape[0]), int(spec.shape[2])
        mel = torch.empty((b, self.n_mel, t, self.channels), dtype=torch.float32, device=spec.device)
        tb, tbp, ntb = _bands_arg(t_bands, b, spec.device, "t_bands")
        fb, fbp, nfb = _bands_arg(f_bands, b, spec.device, "f_bands")
        gain = _gain_arg(mel_gain, b, self.n_mel, spec.device)
        if b == 0 or t == 0:
            return mel
        with self._lock, torch.cuda.device(self.device):
            if gain is None:
                rc = N.lib().iris_magmel(self._handle, spec.data_ptr(), mel.data_ptr(), b, t,
                                         1 if is_magphase else 0, tbp, ntb, fbp, nfb, _stream_ptr(self.device))
            else:
                rc = N.lib().iris_magmel_gain(self._handle, spec.data_ptr(), mel.data_ptr(), b, t, 1 if is_magphase else 0,
                                              tbp, ntb, fbp, nfb, gain.data_ptr(), _stream_ptr(self.device))
                gain.record_stream(torch.cuda.current_stream(self.device))
        N.check(rc, "iris_magmel" if gain is None else "iris_magmel_gain")
        return mel

    def ipd(self, spec: torch.Tensor, t_bands=None, f_bands=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stereo complex spec [B,F,T,4] = (re0, re1, im0, im1) -> [B,M,T,2] = (cos, sin) of the inter-channel phase difference
        per mel band: the magnitude-weighted band average of X0 conj(X1) over |X0||X1| (`iris_spec_ipd`, its own kernel;
        `transforms.mel_ipd` states the definition).  t_bands / f_bands as for `magmel`.  `out`: a contiguous float32
        [B,M,T,2] device tensor to write into (8-byte aligned)."""
        spec = _require_device_f32(spec, "spec")
        if self.channels != 2:
            raise ValueError(f"ipd: the plan has {self.channels} channel(s); the phase difference is that of a stereo pair")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 4:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, 4], got {tuple(spec.shape)}")
        if spec.data_ptr() % 16:
            spec = spec.clone()   # (a view at an odd offset: the kernel loads 16 bytes per bin)
        b, t = int(spec.shape[0]), int(spec.shape[2])
        if out is None:
            out = torch.empty((b, self.n_mel, t, 2), dtype=torch.float32, device=spec.device)
        else:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                    and tuple(out.shape) == (b, self.n_mel, t, 2) and out.device == spec.device and out.data_ptr() % 8 == 0):
                raise ValueError(f"out must be a contiguous, 8-byte aligned float32 tensor {(b, self.n_mel, t, 2)} on {spec.device}")
        tb, tbp, ntb = _bands_arg(t_bands, b, spec.device, "t_bands")
        fb, fbp, nfb = _bands_arg(f_bands, b, spec.device, "f_bands")
        if b == 0 or t == 0:
            return out
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_spec_ipd(self._handle, spec.data_ptr(), out.data_ptr(), b, t, 0, tbp, ntb, fbp, nfb,
                                       _stream_ptr(self.device))
        N.check(rc, "iris_spec_ipd")
        return out

    def _whiten_args(self, spec, block, what):
        """The checked spectrum and block length of `whiten_factors` / `whiten`: (spec, B, T, block, J)."""
        spec = _require_device_f32(spec, "spec")
        if self.channels != 2:
            raise ValueError(f"{what}: the plan has {self.channels} channel(s); the covariance is that of a stereo pair")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 4:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, 4], got {tuple(spec.shape)}")
        if spec.data_ptr() % 16:
            spec = spec.clone()   # (a view at an odd offset: the kernels load 16 bytes per bin)
        b, t = int(spec.shape[0]), int(spec.shape[2])
        block = t if block is None else int(block)
        if block < 1:
            raise ValueError(f"{what}: block = {block} must be at least 1 frame")
        block = max(min(block, t), 1)
        return spec, b, t, block, (t + block - 1) // block

    def whiten_factors(self, spec: torch.Tensor, block: Optional[int] = None, loading: float = 1e-2) -> torch.Tensor:
        """Stereo complex spec [B,F,T,4] = (re0, re1, im0, im1) -> the whitening factors [B,F,J,4] = (a, b, Re c, Im c) of every
        (sample, bin, block of `block` frames; None: all T frames, J = ceil(T / block)): the inverted Cholesky factor of the
        block's 2x2 inter-channel covariance R + d I, d = loading (r00 + r11) / 2 (`iris_spec_whiten_factors`: accumulated and
        factorised in double; `transforms.mel_whiten` states the definition).  No bands: the covariance never sees them."""
        spec, b, t, block, j = self._whiten_args(spec, block, "whiten_factors")
        loading = float(loading)
        if not (math.isfinite(loading) and loading > 0):
            raise ValueError(f"whiten_factors: loading = {loading} must be finite and positive")
        fac = torch.empty((b, self.n_bins, j, 4), dtype=torch.float32, device=spec.device)
        if b == 0 or t == 0:
            return fac
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_spec_whiten_factors(self._handle, spec.data_ptr(), fac.data_ptr(), b, t, 0, block, loading,
                                                  _stream_ptr(self.device))
        N.check(rc, "iris_spec_whiten_factors")
        return fac

    def whiten_factors_ranges(self, spec: torch.Tensor, mask, ranges, block: Optional[int] = None,
                              loading: float = 1e-2) -> torch.Tensor:
        """`whiten_factors` with the covariance of every (sample, block) taken over the frames a table names - the noise
        covariance from the frames outside detected events (`iris_spec_whiten_factors_ranges`, one launch;
        `transforms.quiet_mask` and `transforms.quiet_ranges` build the two inputs, `tests/quiet_ref.py` states the
        definition).  mask: uint8 [B,T], non-zero where a frame is inside an event - a tensor on spec's device, or a host array
        that is uploaded here; ranges: int32 [B,J,3] = (t0, t1, use_mask) per (sample, block), J = ceil(T / min(block, T)), on
        the host (an array or a CPU tensor; checked and uploaded here): the means run over the frames of [t0, t1), without the
        masked ones when use_mask is 1.  use_mask = 1 without an unmasked frame gives zero factors.  G, the lanes that share a
        range, follows from `block` as given (None: T), not cut to T.  Returns the factors [B,F,J,4]."""
        what = "whiten_factors_ranges"
        given = None if block is None else int(block)
        spec, b, t, _, j = self._whiten_args(spec, block, what)
        given = max(t, 1) if given is None else given
        loading = float(loading)
        if not (math.isfinite(loading) and loading > 0):
            raise ValueError(f"{what}: loading = {loading} must be finite and positive")
        if isinstance(mask, torch.Tensor):
            if mask.dtype != torch.uint8 or tuple(mask.shape) != (b, t) or mask.device != spec.device:
                raise ValueError(f"{what}: mask must be uint8 [{b}, {t}] on {spec.device}, got {mask.dtype} {tuple(mask.shape)} on "
                                 f"{mask.device}")
            mask = mask.contiguous()
        else:
            m = np.asarray(mask)
            if m.dtype != np.uint8 or m.shape != (b, t):
                raise ValueError(f"{what}: mask must be uint8 [{b}, {t}], got {m.dtype} {m.shape}")
            mask = torch.from_numpy(np.ascontiguousarray(m)).to(spec.device, non_blocking=True)
        if isinstance(ranges, torch.Tensor):
            if ranges.is_cuda:
                raise ValueError(f"{what}: ranges must be on the host (it is checked there and uploaded here), got {ranges.device}")
            ranges = ranges.numpy()
        table = np.asarray(ranges)
        if table.dtype != np.int32 or table.shape != (b, j, 3):
            raise ValueError(f"{what}: ranges must be int32 [{b}, {j}, 3] = (t0, t1, use_mask) for blocks of {min(given, max(t, 1))} "
                             f"frames, got {table.dtype} {table.shape}")
        table = np.ascontiguousarray(table)
        bad = np.argwhere((table[..., 0] < 0) | (table[..., 0] >= table[..., 1]) | (table[..., 1] > t)
                          | (table[..., 2] < 0) | (table[..., 2] > 1))
        if bad.size:
            i, k = (int(v) for v in bad[0])
            raise ValueError(f"{what}: sample {i}, block {k}: (t0, t1, use_mask) = {tuple(int(v) for v in table[i, k])} must hold "
                             f"0 <= t0 < t1 <= {t} and use_mask 0 or 1")
        fac = torch.empty((b, self.n_bins, j, 4), dtype=torch.float32, device=spec.device)
        if b == 0 or t == 0:
            return fac
        table_dev = torch.from_numpy(table).to(spec.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_spec_whiten_factors_ranges(self._handle, spec.data_ptr(), mask.data_ptr(), table_dev.data_ptr(),
                                                         table.ctypes.data, fac.data_ptr(), b, t, given, loading,
                                                         _stream_ptr(self.device))
        N.check(rc, "iris_spec_whiten_factors_ranges")
        for x in (table_dev, mask):   # (they must outlive the kernel on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return fac

    def whiten(self, spec: torch.Tensor, block: Optional[int] = None, loading: float = 1e-2, log: bool = True,
               t_bands=None, f_bands=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stereo complex spec [B,F,T,4] -> the spatially whitened mel-band energy [B,M,T]: x^H (R + d I)^-1 x per bin, with R
        the covariance of the frame's block (`whiten_factors`), averaged over the mel bands with weights W[k,m] / (2 sum_k
        W[k,m]); `log`: ln(e + 1e-8), `log_on_mel`'s form (two launches: `iris_spec_whiten_factors`, `iris_spec_whiten`;
        `transforms.mel_whiten` states the definition).  t_bands / f_bands act on the OUTPUT only - a masked frame gives e = 0,
        a masked bin adds nothing to its bands' sums - and neither the covariance nor the normalisation sees them: unlike
        `ipd` and `magmel`, whose bands zero the spectrum first (that would change R).  `out`: a contiguous float32 [B,M,T]
        device tensor to write into."""
        spec, b, t, block, _ = self._whiten_args(spec, block, "whiten")
        if out is None:
            out = torch.empty((b, self.n_mel, t), dtype=torch.float32, device=spec.device)
        else:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                    and tuple(out.shape) == (b, self.n_mel, t) and out.device == spec.device and out.data_ptr() % 4 == 0):
                raise ValueError(f"out must be a contiguous, 4-byte aligned float32 tensor {(b, self.n_mel, t)} on {spec.device}")
        tb, tbp, ntb = _bands_arg(t_bands, b, spec.device, "t_bands")
        fb, fbp, nfb = _bands_arg(f_bands, b, spec.device, "f_bands")
        fac = self.whiten_factors(spec, block, loading)
        if b == 0 or t == 0:
            return out
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_spec_whiten(self._handle, spec.data_ptr(), fac.data_ptr(), out.data_ptr(), b, t, 0, block,
                                          1 if log else 0, tbp, ntb, fbp, nfb, _stream_ptr(self.device))
        N.check(rc, "iris_spec_whiten")
        return out

    def locate(self, spec: torch.Tensor, events, fac: Optional[torch.Tensor] = None, block: Optional[int] = None, k_lo: int = 0,
               k_hi: Optional[int] = None, max_lag: int = 40, q: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
        """Stereo complex spec [B,F,T,4] and events int32 [E,3] = (sample, first frame, last frame; frames inclusive) -> the
        noise-whitened steered response curve [E, 2 max_lag + 1] float64 over the lags -max_lag .. max_lag in steps of 1 / q
        sample and bins [k_lo, k_hi) (None: F), and n_terms [E] int64, both on the device (`iris_locate_events`, two launches;
        `transforms.locate_events` states the definition).  fac: the factors [B,F,J,4] `whiten_factors` returns for `block`
        (None: all T frames); fac=None: a = b = 1, c = 0 and one block, the plain power-weighted steered response (`block` is
        then not used).  Every check happens before a launch: ValueError."""
        spec = _require_device_f32(spec, "spec")
        if self.channels != 2:
            raise ValueError(f"locate: the plan has {self.channels} channel(s); the delay is that of a stereo pair")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 4:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, 4], got {tuple(spec.shape)}")
        if spec.data_ptr() % 16:
            spec = spec.clone()   # (a view at an odd offset: the kernels load 16 bytes per bin)
        b, t = int(spec.shape[0]), int(spec.shape[2])
        k_hi = self.n_bins if k_hi is None else int(k_hi)
        k_lo, max_lag, q = int(k_lo), int(max_lag), int(q)
        if not 0 <= k_lo < k_hi <= self.n_bins:
            raise ValueError(f"locate: bins [{k_lo}, {k_hi}) must be a non-empty range inside [0, {self.n_bins}]")
        if q < 1 or max_lag < 0 or 2 * max_lag + 1 > LOCATE_MAX_LAGS:
            raise ValueError(f"locate: q = {q} must be >= 1 and max_lag = {max_lag} in 0 .. {(LOCATE_MAX_LAGS - 1) // 2}")
        if fac is None:
            block, j = max(t, 1), 1
        else:
            fac = _require_device_f32(fac, "fac")
            block = t if block is None else int(block)
            if block < 1:
                raise ValueError(f"locate: block = {block} must be at least 1 frame")
            block = max(min(block, t), 1)
            j = (t + block - 1) // block
            if tuple(fac.shape) != (b, self.n_bins, j, 4) or fac.device != spec.device:
                raise ValueError(f"locate: fac must be [{b}, {self.n_bins}, {j}, 4] on {spec.device} for blocks of {block} frames, "
                                 f"got {tuple(fac.shape)} on {fac.device}")
            if fac.data_ptr() % 16:
                fac = fac.clone()
        table = locate_table(events, block, t, b)
        e, lags = int(table.shape[0]), 2 * max_lag + 1
        curve = torch.empty((e, lags), dtype=torch.float64, device=spec.device)
        n_terms = torch.empty((e,), dtype=torch.int64, device=spec.device)
        if e == 0:
            return curve, n_terms
        n_seg = int(table[-1, 3]) + int(table[-1, 2]) // block - int(table[-1, 1]) // block + 1
        work = torch.empty((n_seg, k_hi - k_lo, 4), dtype=torch.float64, device=spec.device)
        table_dev = torch.from_numpy(table).to(spec.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_locate_events(self._handle, spec.data_ptr(), None if fac is None else fac.data_ptr(), j,
                                            table_dev.data_ptr(), table.ctypes.data, e, b, t, block, k_lo, k_hi, max_lag, q,
                                            work.data_ptr(), work.numel() * 8, curve.data_ptr(), n_terms.data_ptr(),
                                            _stream_ptr(self.device))
        N.check(rc, "iris_locate_events")
        for x in (table_dev, work):   # (allocated here: they must outlive the kernels on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return curve, n_terms

    def locate_steps(self, spec: torch.Tensor, events, fac: Optional[torch.Tensor] = None, block: Optional[int] = None,
                     step: int = 16, k_lo: int = 0, k_hi: Optional[int] = None, max_lag: int = 40, q: int = 8, out=None):
        """`locate` per STEP of `step` frames (counted from frame 0) instead of per event, for events whose delay moves: -> (R
        [rows, 2 max_lag + 1] float64, n_terms [rows] int64, both on the device, row_offsets int32 [E + 1] on the host): event e
        owns the rows row_offsets[e] .. row_offsets[e + 1] - 1, one per step first // step .. last // step, and R[row] is
        `locate`'s term sum over the step's frames with the factors of the step's block (`iris_locate_steps`, two launches;
        `transforms.track_events` states the definition).  With factors `block % step == 0` is required, so a step lies in one
        block.  out: (R, n_terms) preallocated (`track_buffers`).  Every check happens before a launch: ValueError."""
        spec = _require_device_f32(spec, "spec")
        if self.channels != 2:
            raise ValueError(f"locate_steps: the plan has {self.channels} channel(s); the delay is that of a stereo pair")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 4:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, 4], got {tuple(spec.shape)}")
        if spec.data_ptr() % 16:
            spec = spec.clone()   # (a view at an odd offset: the kernels load 16 bytes per bin)
        b, t = int(spec.shape[0]), int(spec.shape[2])
        k_hi = self.n_bins if k_hi is None else int(k_hi)
        k_lo, max_lag, q = int(k_lo), int(max_lag), int(q)
        if not 0 <= k_lo < k_hi <= self.n_bins:
            raise ValueError(f"locate_steps: bins [{k_lo}, {k_hi}) must be a non-empty range inside [0, {self.n_bins}]")
        if q < 1 or max_lag < 0 or 2 * max_lag + 1 > LOCATE_MAX_LAGS:
            raise ValueError(f"locate_steps: q = {q} must be >= 1 and max_lag = {max_lag} in 0 .. {(LOCATE_MAX_LAGS - 1) // 2}")
        if fac is not None and block is not None and int(block) < 1:
            raise ValueError(f"locate_steps: block = {block} must be at least 1 frame")
        step = track_step(step, None if fac is None or block is None else int(block))   # (None: one block holds every step)
        if fac is None:
            block, j = max(t, 1), 1
        else:
            fac = _require_device_f32(fac, "fac")
            block = max(min(t if block is None else int(block), t), 1)
            j = (t + block - 1) // block
            if tuple(fac.shape) != (b, self.n_bins, j, 4) or fac.device != spec.device:
                raise ValueError(f"locate_steps: fac must be [{b}, {self.n_bins}, {j}, 4] on {spec.device} for blocks of {block} "
                                 f"frames, got {tuple(fac.shape)} on {fac.device}")
            if fac.data_ptr() % 16:
                fac = fac.clone()
        table = locate_table(events, step, t, b)   # (the same table with steps for blocks: column 3 counts rows)
        e, lags = int(table.shape[0]), 2 * max_lag + 1
        offsets = np.zeros(e + 1, np.int32)
        if e:
            offsets[:-1] = table[:, 3]
            offsets[-1] = int(table[-1, 3]) + int(table[-1, 2]) // step - int(table[-1, 1]) // step + 1
        rows = int(offsets[-1])
        if out is None:
            out = track_buffers(rows, lags, spec.device)[1:3]
        resp, n_terms = out
        if not (torch.is_tensor(resp) and resp.dtype == torch.float64 and tuple(resp.shape) == (rows, lags) and resp.is_contiguous()
                and torch.is_tensor(n_terms) and n_terms.dtype == torch.int64 and tuple(n_terms.shape) == (rows,)
                and n_terms.is_contiguous() and resp.device == spec.device == n_terms.device):
            raise ValueError(f"locate_steps: out must be (float64 [{rows}, {lags}], int64 [{rows}]) on {spec.device}")
        if e == 0:
            return resp, n_terms, offsets
        work = torch.empty((rows, k_hi - k_lo, 4), dtype=torch.float64, device=spec.device)
        table_dev = torch.from_numpy(table).to(spec.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_locate_steps(self._handle, spec.data_ptr(), None if fac is None else fac.data_ptr(), j,
                                           table_dev.data_ptr(), table.ctypes.data, e, b, t, block, step, k_lo, k_hi, max_lag, q,
                                           work.data_ptr(), work.numel() * 8, resp.data_ptr(), n_terms.data_ptr(),
                                           _stream_ptr(self.device))
        N.check(rc, "iris_locate_steps")
        for x in (table_dev, work):   # (allocated here: they must outlive the kernels on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return resp, n_terms, offsets

    def track(self, resp: torch.Tensor, row_offsets, pen: float, max_jump: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The best path through the lags of every event's step responses: resp [rows, L] float64 on the device and row_offsets
        [E + 1] (`locate_steps`) -> path int32 [rows] on the device, the lag index of every step (`iris_track_lags`, one launch,
        one workgroup per event; `transforms.track_events` states the recurrence).  pen >= 0: response units per lag step
        between neighbouring steps; max_jump >= 0: the most lag steps a path may move per step.  At most 2049 lags.  Every
        check happens before the launch: ValueError."""
        resp = torch.as_tensor(resp)
        if not (resp.is_cuda and resp.dtype == torch.float64 and resp.dim() == 2 and resp.is_contiguous()):
            raise ValueError(f"track: R must be a contiguous float64 [rows, L] on a ROCm device, got {resp.dtype} {tuple(resp.shape)} "
                             f"on {resp.device}")
        rows, lags = int(resp.shape[0]), int(resp.shape[1])
        offsets, table = track_offsets(row_offsets, rows), track_penalties(pen, max_jump, lags)
        if out is None:
            out = torch.empty((rows,), dtype=torch.int32, device=resp.device)
        if not (torch.is_tensor(out) and out.dtype == torch.int32 and tuple(out.shape) == (rows,) and out.is_contiguous()
                and out.device == resp.device):
            raise ValueError(f"track: out must be int32 [{rows}] on {resp.device}")
        e = len(offsets) - 1
        if e == 0:
            return out
        back = torch.empty((rows, lags), dtype=torch.int32, device=resp.device)
        off_dev = torch.from_numpy(offsets).to(resp.device, non_blocking=True)
        pen_dev = torch.from_numpy(table).to(resp.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_track_lags(self._handle, resp.data_ptr(), off_dev.data_ptr(), offsets.ctypes.data, e, rows,
                                         (lags - 1) // 2, pen_dev.data_ptr(), int(table.shape[0]), min(int(max_jump), 2 ** 31 - 1),
                                         back.data_ptr(), back.numel() * 4, out.data_ptr(), _stream_ptr(self.device))
        N.check(rc, "iris_track_lags")
        for x in (off_dev, pen_dev, back, resp):   # (they must outlive the kernel on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return out

    def beamform_frames(self, spec: torch.Tensor, events, tdoa, fac: Optional[torch.Tensor] = None, block: Optional[int] = None,
                        k_lo: int = 0, k_hi: Optional[int] = None) -> List[torch.Tensor]:
        """`beamform` steered per FRAME: tdoa is flat, one delay per output frame - the frames of event 0, then those of event 1,
        ... (`transforms.track_delays`) - and a frame whose delay is not finite is exactly 0 (`iris_beamform_frames`, one launch).
        A delay that is constant over each event gives `beamform`'s bits."""
        return self.beamform(spec, events, tdoa, fac, block, k_lo, k_hi, _frames=True)

    def beamform(self, spec: torch.Tensor, events, tdoa, fac: Optional[torch.Tensor] = None, block: Optional[int] = None,
                 k_lo: int = 0, k_hi: Optional[int] = None, _frames: bool = False) -> List[torch.Tensor]:
        """Stereo complex spec [B,F,T,4], events int [E,3] = (sample, first frame, last frame; frames inclusive) and their
        delays tdoa [E] (samples, float64; positive: channel 1 hears the event later - `locate_peak`'s sign) -> the list of the
        events' MVDR-beamformed spectra, [F, T_e, 2] = (Re Y, Im Y) float32 each (T_e = last - first + 1; `iris_istft`'s record
        layout for one channel), views of ONE flat device buffer (`iris_beamform_events`, one launch; `transforms.extract_events`
        states the definition).  fac: the factors [B,F,J,4] `whiten_factors` returns for `block` (None: all T frames);
        fac=None: a = b = 1, c = 0 and one block, the delay-and-sum beamformer (`block` is then not used).  Bins outside
        [k_lo, k_hi) (None: F), silent blocks and events whose delay is not finite are exactly 0.  Every check happens before a
        launch: ValueError."""
        spec = _require_device_f32(spec, "spec")
        if self.channels != 2:
            raise ValueError(f"beamform: the plan has {self.channels} channel(s); the delay is that of a stereo pair")
        if spec.dim() != 4 or spec.shape[1] != self.n_bins or spec.shape[3] != 4:
            raise ValueError(f"spec must be [B, {self.n_bins}, T, 4], got {tuple(spec.shape)}")
        if spec.data_ptr() % 16:
            spec = spec.clone()   # (a view at an odd offset: the kernel loads 16 bytes per bin)
        b, t = int(spec.shape[0]), int(spec.shape[2])
        k_hi = self.n_bins if k_hi is None else int(k_hi)
        k_lo = int(k_lo)
        if not 0 <= k_lo < k_hi <= self.n_bins:
            raise ValueError(f"beamform: bins [{k_lo}, {k_hi}) must be a non-empty range inside [0, {self.n_bins}]")
        if fac is None:
            block, j = max(t, 1), 1
        else:
            fac = _require_device_f32(fac, "fac")
            block = t if block is None else int(block)
            if block < 1:
                raise ValueError(f"beamform: block = {block} must be at least 1 frame")
            block = max(min(block, t), 1)
            j = (t + block - 1) // block
            if tuple(fac.shape) != (b, self.n_bins, j, 4) or fac.device != spec.device:
                raise ValueError(f"beamform: fac must be [{b}, {self.n_bins}, {j}, 4] on {spec.device} for blocks of {block} frames, "
                                 f"got {tuple(fac.shape)} on {fac.device}")
            if fac.data_ptr() % 16:
                fac = fac.clone()
        table = beamform_table(events, t, b)
        e = int(table.shape[0])
        delays = np.ascontiguousarray(np.asarray(tdoa.cpu() if torch.is_tensor(tdoa) else tdoa, np.float64).reshape(-1))
        frames = (table[:, 2] - table[:, 1] + 1).astype(np.int64)
        if _frames and delays.shape[0] != int(frames.sum()):
            raise ValueError(f"beamform_frames: {delays.shape[0]} delay(s) for {int(frames.sum())} output frame(s)")
        if not _frames and delays.shape[0] != e:
            raise ValueError(f"beamform: {delays.shape[0]} delay(s) for {e} event(s)")
        if e == 0:
            return []
        per = 2 * self.n_bins
        flat = torch.empty((per * int(frames.sum()),), dtype=torch.float32, device=spec.device)
        table_dev = torch.from_numpy(table).to(spec.device, non_blocking=True)
        tdoa_dev = torch.from_numpy(delays).to(spec.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            if _frames:
                rc = N.lib().iris_beamform_frames(self._handle, spec.data_ptr(), None if fac is None else fac.data_ptr(), j,
                                                  table_dev.data_ptr(), table.ctypes.data, tdoa_dev.data_ptr(), delays.shape[0], e, b,
                                                  t, block, k_lo, k_hi, flat.data_ptr(), flat.numel(), _stream_ptr(self.device))
            else:
                rc = N.lib().iris_beamform_events(self._handle, spec.data_ptr(), None if fac is None else fac.data_ptr(), j,
                                                  table_dev.data_ptr(), table.ctypes.data, tdoa_dev.data_ptr(), e, b, t, block, k_lo,
                                                  k_hi, flat.data_ptr(), flat.numel(), _stream_ptr(self.device))
        N.check(rc, "iris_beamform_frames" if _frames else "iris_beamform_events")
        for x in (table_dev, tdoa_dev, spec) + (() if fac is None else (fac,)):   # (they must outlive the kernel on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return [flat[per * int(o):per * int(o + n)].view(self.n_bins, int(n), 2) for o, n in zip(table[:, 3], frames)]

    def postfilter(self, slabs, events, tdoa, fac: torch.Tensor, block: Optional[int], loading: float, k_lo: int, k_hi: Optional[int],
                   alpha: float, g_min, per_frame: bool = False) -> List[torch.Tensor]:
        """The decision-directed Wiener post-filter over the slabs `beamform` (or, per_frame=True, `beamform_frames`) returned
        for the SAME events, tdoa, fac, block and bins: new slabs [F, T_e, 2] float32, views of ONE flat device buffer
        (`iris_postfilter_events`, one launch; `transforms.extract_events` states the definition).  fac must be the factors of
        a covariance that does not contain the events (`whiten_factors_ranges`: noise="quiet") made with `loading`; fac=None
        is refused - there is no noise model.  alpha in [0, 1): the smoothing of the a-priori SNR; g_min: one gain floor in
        (0, 1] per event (a number: the same for all); g_min = 1 returns that event's slab bit for bit.  Bins outside
        [k_lo, k_hi) (None: F) are exactly 0.  Every check happens before a launch: ValueError."""
        if self.channels != 2:
            raise ValueError(f"postfilter: the plan has {self.channels} channel(s); the delay is that of a stereo pair")
        if fac is None:
            raise ValueError("postfilter: fac=None - there is no noise model without the factors of noise='quiet'")
        fac = _require_device_f32(fac, "fac")
        if fac.dim() != 4 or fac.shape[1] != self.n_bins or fac.shape[3] != 4:
            raise ValueError(f"postfilter: fac must be [B, {self.n_bins}, J, 4], got {tuple(fac.shape)}")
        b, j = int(fac.shape[0]), int(fac.shape[2])
        if block is None and j == 1:
            block = 1 << 30                               # one block over all frames, however many there were
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block < 1:
            raise ValueError(f"postfilter: block = {block!r} must be the frames per block of fac {tuple(fac.shape)}, at least 1 "
                             "(None: fac holds one block)")
        block = min(int(block), 1 << 30) if j == 1 else int(block)   # (the entry point takes at most 2^30 frames)
        if j < 1 or j * block > 1 << 30:
            raise ValueError(f"postfilter: fac {tuple(fac.shape)} in blocks of {block} frames: between 1 and 2^30 frames in all")
        for name, v, ok in (("alpha", alpha, lambda v: 0.0 <= v < 1.0), ("loading", loading, lambda v: v > 0.0 and np.isfinite(v))):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or not ok(float(v)):
                raise ValueError(f"postfilter: {name} = {v!r} must be " + ("in [0, 1)" if name == "alpha" else "positive and finite"))
        k_hi = self.n_bins if k_hi is None else int(k_hi)
        k_lo = int(k_lo)
        if not 0 <= k_lo < k_hi <= self.n_bins:
            raise ValueError(f"postfilter: bins [{k_lo}, {k_hi}) must be a non-empty range inside [0, {self.n_bins}]")
        # (the spectrum is not an argument: any frame count whose blocks make J fits; the records are checked against the largest)
        t = j * block
        table = beamform_table(events, t, b)
        e = int(table.shape[0])
        frames = (table[:, 2] - table[:, 1] + 1).astype(np.int64)
        delays = np.ascontiguousarray(np.asarray(tdoa.cpu() if torch.is_tensor(tdoa) else tdoa, np.float64).reshape(-1))
        if delays.shape[0] != (int(frames.sum()) if per_frame else e):
            raise ValueError(f"postfilter: {delays.shape[0]} delay(s) for {e} event(s) of {int(frames.sum())} output frame(s), "
                             f"per_frame={bool(per_frame)}")
        floors = np.asarray(g_min.cpu() if torch.is_tensor(g_min) else g_min, np.float64)
        floors = np.full((e,), floors) if floors.ndim == 0 else np.ascontiguousarray(floors.reshape(-1))
        if floors.shape[0] != e or not np.all((floors > 0.0) & (floors <= 1.0)):
            raise ValueError(f"postfilter: g_min must be one gain floor in (0, 1] per event ({e}), got {floors[:8].tolist()}")
        slabs = list(slabs)
        if len(slabs) != e:
            raise ValueError(f"postfilter: {len(slabs)} slab(s) for {e} event(s)")
        for i, (s, n) in enumerate(zip(slabs, frames)):
            if not torch.is_tensor(s) or not s.is_cuda:
                raise RuntimeError(f"postfilter: slab {i} is not on a ROCm device: the post-filter runs only as a HIP kernel "
                                   "(there is no CPU fallback)")
            if tuple(s.shape) != (self.n_bins, int(n), 2) or s.dtype != torch.float32 or not s.is_contiguous() or s.device != fac.device:
                raise ValueError(f"postfilter: slab {i} must be a contiguous float32 [{self.n_bins}, {int(n)}, 2] on {fac.device}, "
                                 f"got {s.dtype} {tuple(s.shape)} on {s.device}")
        if e == 0:
            return []
        per = 2 * self.n_bins
        base = slabs[0].data_ptr()
        if base % 8 == 0 and all(s.data_ptr() == base + 4 * per * int(o) for s, o in zip(slabs, table[:, 3])) and \
                all(s.untyped_storage().data_ptr() == slabs[0].untyped_storage().data_ptr() for s in slabs):
            src, keep = base, slabs                      # `beamform`'s own flat buffer, in place
        else:
            keep = [torch.cat([s.reshape(-1) for s in slabs])]
            src = keep[0].data_ptr()
        if fac.data_ptr() % 16:
            fac = fac.clone()
        flat = torch.empty((per * int(frames.sum()),), dtype=torch.float32, device=fac.device)
        table_dev = torch.from_numpy(table).to(fac.device, non_blocking=True)
        tdoa_dev = torch.from_numpy(delays).to(fac.device, non_blocking=True)
        floors_dev = torch.from_numpy(floors).to(fac.device, non_blocking=True)
        with self._lock, torch.cuda.device(self.device):
            rc = N.lib().iris_postfilter_events(self._handle, src, fac.data_ptr(), j, table_dev.data_ptr(), table.ctypes.data,
                                                tdoa_dev.data_ptr(), delays.shape[0], int(bool(per_frame)), floors_dev.data_ptr(),
                                                floors.ctypes.data, e, b, t, block, float(loading), float(alpha), k_lo, k_hi,
                                                flat.data_ptr(), flat.numel(), _stream_ptr(self.device))
        N.check(rc, "iris_postfilter_events")
        for x in [table_dev, tdoa_dev, floors_dev, fac] + list(keep):   # (they must outlive the kernel on this stream)
            x.record_stream(torch.cuda.current_stream(self.device))
        return [flat[per * int(o):per * int(o + n)].view(self.n_bins, int(n), 2) for o, n in zip(table[:, 3], frames)]

    def wav_to_logmel(self, wav: torch.Tensor, minmax: bool = True, log: bool = True,
                      normalize: bool = False, t_bands=None, f_bands=None,
                      out: Optional[torch.Tensor] = None, mel_gain=None) -> torch.Tensor:
        """The fused hot path: wav [B,C,L] -> log-mel [B,M,T,C].  mel_gain ([B, M] float32, optional: FilterAugment): every
        mel magnitude times its sample's band gain inside the kernel, before min-max / log (`iris_wav_to_logmel_gain`);
        None takes the ungained entry, untouched."""
        wav, b, length = self._check_wav(wav)
        t = self.num_frames(length)
        if out is None:
            out = torch.empty((b, self.n_mel, t, self.channels), dtype=torch.float32, device=self.device)
        else:
            out = _require_device_f32(out, "out")
            if tuple(out.shape) != (b, self.n_mel, t, self.channels):
                raise ValueError(f"out must be {(b, self.n_mel, t, self.channels)}, got {tuple(out.shape)}")
        tb, tbp, ntb = _bands_arg(t_bands, b, self.device, "t_bands")
        fb, fbp, nfb = _bands_arg(f_bands, b, self.device, "f_bands")
        flags = (N.IRIS_F_MINMAX if minmax else 0) | (N.IRIS_F_LOG if log else 0) | \
            (N.IRIS_F_NORMALIZE if normalize else 0)
        gain = _gain_arg(mel_gain, b, self.n_mel, self.device)
        with self._lock, torch.cuda.device(self.device):
            if gain is None:
                rc = N.lib().iris_wav_to_logmel(self._handle, wav.data_ptr(), out.data_ptr(), b, length, flags,
                                                tbp, ntb, fbp, nfb, _stream_ptr(self.device))
            else:
                rc = N.lib().iris_wav_to_logmel_gain(self._handle, wav.data_ptr(), out.data_ptr(), b, length, flags,
                                                     tbp, ntb, fbp, nfb, gain.data_ptr(), _stream_ptr(self.device))
                gain.record_stream(torch.cuda.current_stream(self.device))
        if rc == N.IRIS_E_EPILOGUE_TIMEOUT:
            self.epilogue = "two_kernels"  # the library has switched the plan for good
        N.check(rc, "iris_wav_to_logmel")
        return out

    # ---- prepared launches ------------------------------------------------------
    def prepare(self, wav: torch.Tensor, out: Optional[torch.Tensor] = None, minmax: bool = True, log: bool = True,
                normalize: bool = False, t_bands=None, f_bands=None, mel_gain=None) -> "PreparedCall":
        """Validate once, launch many times: returns an object whose `.launch()` is nothing but the C-ABI call of
        `wav_to_logmel(wav, out=out, ...)` with pre-converted arguments (about 3 us of host time instead of ~12 us for the
        checked path) - for steady-state loops over long-lived buffers (serving, benchmarks).  Tensors are bound BY
        ADDRESS (refill them in place); launches go to the stream that is current NOW; not thread-safe.  mel_gain: a float32
        [B, M] DEVICE tensor bound by address like the others (FilterAugment: refill it, e.g. by `filter_draw(out=...)`)."""
        return PreparedCall(self, wav, out, minmax, log, normalize, t_bands, f_bands, mel_gain)

    # ---- hipGraph ------------------------------------------------------------
    def capture(self, wav: torch.Tensor, out: Optional[torch.Tensor] = None, **kwargs) -> "CapturedStep":
        """Capture `wav_to_logmel(wav, out=out, **kwargs)` into a hipGraph (torch.cuda.CUDAGraph) once and return an
        object whose `.replay()` re-runs it on the current stream with no per-launch host work; `.out` is the output
        tensor.  The entry points never allocate or synchronise and keep no per-call host state, so a replay is
        the same device work.  `wav`, `out` and any bands tensors are captured BY ADDRESS: refill them in place."""
        return CapturedStep(self, wav, out, kwargs)

    # ---- bench hooks ---------------------------------------------------------
    def fused_kernel_name(self, with_bands: bool = False) -> str:
        buf = C.create_string_buffer(128)
        N.check(N.lib().iris_plan_kernel_name(self._handle, 1 if with_bands else 0, buf, 128), "iris_plan_kernel_name")
        return buf.value.decode()

    def timing_enable(self, enable=True) -> None:
        """True / 1: every launch of the main kernel carries an event pair; n > 1: every n-th; False / 0: off."""
        N.check(N.lib().iris_timing_enable(self._handle, int(enable)), "iris_timing_enable")

    def timing_read(self) -> Tuple[int, float]:
        n, ms = C.c_int(0), C.c_float(0)
        N.check(N.lib().iris_timing_read(self._handle, C.byref(n), C.byref(ms)), "iris_timing_read")
        return n.value, ms.value

    def timing_samples(self, kernel: int = 0) -> np.ndarray:
        """Durations (ms) of the sampled launches of kernel 0 (fused) / 1 (min-max + log) since timing_enable."""
        cap = 4096
        buf = np.zeros(cap, np.float32)
        n = C.c_int(0)
        N.check(N.lib().iris_timing_samples(self._handle, int(kernel), buf.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                            C.byref(n)), "iris_timing_samples")
        return buf[:min(n.value, cap)].copy()


class PreparedCall:
    """One fused frontend call with its arguments converted once (see FrontendPlan.prepare)."""
    __slots__ = ("out", "_fn", "_args", "_keep")

    def __init__(self, plan: FrontendPlan, wav, out, minmax, log, normalize, t_bands, f_bands, mel_gain=None):
        wav, b, length = plan._check_wav(wav)
        t = plan.num_frames(length)
        if out is None:
            out = torch.empty((b, plan.n_mel, t, plan.channels), dtype=torch.float32, device=plan.device)
        else:
            out = _require_device_f32(out, "out")
            if tuple(out.shape) != (b, plan.n_mel, t, plan.channels):
                raise ValueError(f"out must be {(b, plan.n_mel, t, plan.channels)}, got {tuple(out.shape)}")
        tb, tbp, ntb = _bands_arg(t_bands, b, plan.device, "t_bands")
        fb, fbp, nfb = _bands_arg(f_bands, b, plan.device, "f_bands")
        flags = (N.IRIS_F_MINMAX if minmax else 0) | (N.IRIS_F_LOG if log else 0) | (N.IRIS_F_NORMALIZE if normalize else 0)
        if mel_gain is not None:
            if not (isinstance(mel_gain, torch.Tensor) and mel_gain.is_cuda and mel_gain.dtype == torch.float32 and
                    mel_gain.is_contiguous() and tuple(mel_gain.shape) == (b, plan.n_mel)):
                raise ValueError(f"mel_gain must be a contiguous float32 device tensor [batch={b}, n_mel={plan.n_mel}] (bound by address)")
        self.out, self._keep = out, (plan, wav, tb, fb, mel_gain)     # keep everything the raw pointers refer to alive
        self._args = (plan._handle, C.c_void_p(wav.data_ptr()), C.c_void_p(out.data_ptr()), b, length, flags, tbp, ntb, fbp, nfb)
        if mel_gain is None:
            self._fn = N.lib().iris_wav_to_logmel
        else:
            self._fn = N.lib().iris_wav_to_logmel_gain
            self._args += (C.c_void_p(mel_gain.data_ptr()),)
        self._args += (_stream_ptr(plan.device),)

    def launch(self) -> torch.Tensor:
        rc = self._fn(*self._args)
        if rc:
            N.check(rc, "iris_wav_to_logmel")
        return self.out


class CapturedStep:
    """One fused frontend call as a replayable hipGraph (see FrontendPlan.capture)."""

    def __init__(self, plan: FrontendPlan, wav: torch.Tensor, out: Optional[torch.Tensor], kwargs: dict):
        self.plan, self.wav = plan, wav
        dev = plan.device
        # bands must be device tensors that outlive the graph (they are read at replay time)
        for k in ("t_bands", "f_bands"):
            if kwargs.get(k) is not None:
                kwargs[k] = torch.as_tensor(kwargs[k]).to(device=dev, dtype=torch.int32).contiguous()
        if kwargs.get("mel_gain") is not None:   # likewise read at replay time (FilterAugment: refill it in place)
            kwargs["mel_gain"] = torch.as_tensor(kwargs["mel_gain"]).to(device=dev, dtype=torch.float32).contiguous()
        self.kwargs = kwargs
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up outside the capture: geometry cache, lazy module load
            self.out = plan.wav_to_logmel(wav, out=out, **kwargs)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            plan.wav_to_logmel(wav, out=self.out, **kwargs)

    def replay(self) -> torch.Tensor:
        self.graph.replay()
        return self.out


# ---------------------------------------------------------------------------
# plan-free ops (run on the tensor's device / current stream)
# ---------------------------------------------------------------------------
def filter_draw(batch: int, n_mel: int, kind: str = "step", n_band=(3, 6), min_bw: int = 6, db=(-6.0, 6.0), seed: int = 0,
                state: Optional[torch.Tensor] = None, device=None, out=None):
    """The FilterAugment draws of a batch ON THE DEVICE, one `iris_filter_draw` launch: (bounds int32 [B, n_band_hi + 1],
    db float32 [B, n_band_hi + 1], gain float32 [B, n_mel]); `gain` is the `mel_gain` of `FrontendPlan.wav_to_logmel` /
    `.magmel`.  Per sample a band count ~ U{n_band[0] .. n_band[1]}, boundaries uniform over every placement with bands of at
    least `min_bw` mel rows, dB ~ U[db[0], db[1]) per band ('step') or per boundary ('linear': interpolated across the band),
    gain = 10^(dB / 20) (`transforms.filter_augment_gains` is the definition).  Philox keyed by `seed`; `state`: an int64 [1]
    device tensor of this draw's own, zero-initialised once, advanced by every call on the device (None: a fresh zero state,
    i.e. the first draw of `seed`).  `out`: the (bounds, db, gain) tensors of an earlier call, overwritten in place (for
    prepared / captured calls that bound `gain` by address).  Capturable."""
    if kind not in ("step", "linear"):
        raise ValueError(f"filter_draw: kind must be 'step' or 'linear', got {kind!r}")
    if state is not None:
        device = state.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("filter_draw draws on a ROCm device (transforms.filter_augment_draw is the host draw)")
    batch, n_mel, hi = int(batch), int(n_mel), int(n_band[1])
    if state is None:
        state = torch.zeros(1, dtype=torch.int64, device=device)
    elif state.dtype != torch.int64 or state.numel() != 1 or not state.is_cuda:
        raise ValueError("filter_draw: state must be an int64 device tensor of one element")
    if batch < 0 or n_mel <= 0 or hi < 1:
        raise ValueError(f"filter_draw: bad sizes (batch {batch}, n_mel {n_mel}, n_band {tuple(n_band)})")
    if out is None:
        bounds = torch.empty((batch, hi + 1), dtype=torch.int32, device=device)
        dbs = torch.empty((batch, hi + 1), dtype=torch.float32, device=device)
        gain = torch.empty((batch, n_mel), dtype=torch.float32, device=device)
    else:
        bounds, dbs, gain = out
        if (tuple(bounds.shape), tuple(dbs.shape), tuple(gain.shape)) != ((batch, hi + 1), (batch, hi + 1), (batch, n_mel)) or \
                bounds.dtype != torch.int32 or dbs.dtype != torch.float32 or gain.dtype != torch.float32 or \
                not (bounds.is_contiguous() and dbs.is_contiguous() and gain.is_contiguous()) or gain.device != device:
            raise ValueError("filter_draw: out must be the (bounds, db, gain) of a call with the same batch, n_mel and n_band")
    with torch.cuda.device(device):
        rc = N.lib().iris_filter_draw(batch, n_mel, N.IRIS_FILTER_LINEAR if kind == "linear" else N.IRIS_FILTER_STEP,
                                      int(n_band[0]), hi, int(min_bw), float(db[0]), float(db[1]),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, state.data_ptr(), bounds.data_ptr(), dbs.data_ptr(),
                                      gain.data_ptr(), _stream_ptr(device))
    N.check(rc, "iris_filter_draw")
    return bounds, dbs, gain


# mirrors iris_crop_rec (include/iris_frontend.h)
CROP_REC = np.dtype([("base", "<u8"), ("row_stride", "<i8"), ("len", "<i4"), ("ev_first", "<i4"), ("ev_count", "<i4"),
                     ("reserved", "<i4")])
assert CROP_REC.itemsize == 32


def _require_device_int(t, dtype, name: str, what: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: {name} must be a tensor on a ROCm device (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{what}: {name} must be a contiguous {dtype} tensor")
    return t


def crop_windows(recs: torch.Tensor, events: torch.Tensor, draws: torch.Tensor, channels: int, hop: int, n_frame: int,
                 n_classes: int = 3, out=None):
    """A batch of windows of labelled recordings and their frame labels, ONE `iris_crop_windows` launch:
    (wav float32 [B, channels, (n_frame - 1) * hop], y float32 [B, n_frame, n_classes]).  recs: the CROP_REC table of the
    recordings as a uint8 device tensor (device addresses, row strides, lengths, event rows); events: int32 [rows, 3] of
    (class, start frame, end frame) on the device; draws: int32 [B, 2] of (recording, first frame) on the device
    (`crop_draw`).  Samples at or beyond a recording's length are exactly 0 and are never read; y counts the events that
    cover a frame.  `out`: the (wav, y) of an earlier call of the same shape, overwritten in place.  Capturable."""
    what = "crop_windows"
    recs = _require_device_int(recs, torch.uint8, "recs", what)
    events = _require_device_int(events, torch.int32, "events", what)
    draws = _require_device_int(draws, torch.int32, "draws", what)
    if recs.numel() == 0 or recs.numel() % CROP_REC.itemsize:
        raise ValueError(f"{what}: recs must hold a whole, positive number of {CROP_REC.itemsize}-byte records")
    if draws.dim() != 2 or draws.shape[1] != 2:
        raise ValueError(f"{what}: draws must be [batch, 2], got {tuple(draws.shape)}")
    if events.dim() != 2 or events.shape[1] != 3 or events.shape[0] < 1:
        raise ValueError(f"{what}: events must be [rows >= 1, 3], got {tuple(events.shape)}")
    device, batch = draws.device, int(draws.shape[0])
    channels, hop, n_frame, n_classes = int(channels), int(hop), int(n_frame), int(n_classes)
    shapes = (batch, channels, max(n_frame - 1, 0) * max(hop, 0)), (batch, max(n_frame, 0), max(n_classes, 0))
    if out is None:
        wav = torch.empty(shapes[0], dtype=torch.float32, device=device)
        y = torch.empty(shapes[1], dtype=torch.float32, device=device)
    else:
        wav, y = out
        if (tuple(wav.shape), tuple(y.shape)) != shapes or wav.dtype != torch.float32 or y.dtype != torch.float32 or \
                not (wav.is_contiguous() and y.is_contiguous()) or wav.device != device or y.device != device:
            raise ValueError(f"{what}: out must be the (wav, y) of a call with the same batch and sizes")
    with torch.cuda.device(device):
        rc = N.lib().iris_crop_windows(recs.data_ptr(), recs.numel() // CROP_REC.itemsize, events.data_ptr(), draws.data_ptr(),
                                       batch, channels, hop, n_frame, n_classes, wav.data_ptr(), y.data_ptr(), _stream_ptr(device))
    N.check(rc, "iris_crop_windows")
    return wav, y


def crop_draw(prefix: torch.Tensor, batch: int, seed: int = 0, state: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
    """The window draws of a batch ON THE DEVICE, one `iris_crop_draw` launch: int32 [B, 2] of (recording, first frame), every
    window of the corpus equally likely.  prefix: int64 [n + 1] device tensor, the prefix sums of the recordings' position
    counts max((len - L) // hop, 0) + 1.  Philox keyed by `seed`; `state`: an int64 [1] device tensor of this draw's own,
    zero-initialised once, advanced by every call on the device (None: a fresh zero state, i.e. the first draw of `seed`).
    `out`: the draws of an earlier call of the same batch, overwritten in place.  Capturable."""
    what = "crop_draw"
    prefix = _require_device_int(prefix, torch.int64, "prefix", what)
    if prefix.dim() != 1 or prefix.numel() < 2:
        raise ValueError(f"{what}: prefix must be [n + 1] with n >= 1, got {tuple(prefix.shape)}")
    device, batch = prefix.device, int(batch)
    if state is None:
        state = torch.zeros(1, dtype=torch.int64, device=device)
    elif not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or state.numel() != 1 or state.device != device:
        raise ValueError(f"{what}: state must be an int64 tensor of one element on the device of prefix")
    if out is None:
        out = torch.empty((max(batch, 0), 2), dtype=torch.int32, device=device)
    elif tuple(out.shape) != (batch, 2) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: out must be the int32 [batch, 2] draws of an earlier call")
    with torch.cuda.device(device):
        rc = N.lib().iris_crop_draw(prefix.data_ptr(), int(prefix.numel()) - 1, batch, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    state.data_ptr(), out.data_ptr(), _stream_ptr(device))
    N.check(rc, "iris_crop_draw")
    return out


def bias_relu_(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """In place max(x + bias[c], 0) on a channels-last activation: x is [B, C, H, W] with channels_last strides (or any
    dense tensor whose innermost axis is the channel axis).  One HIP launch (iris_bias_relu)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError("bias_relu_: x must be a float32 tensor on a ROCm device (no CPU fallback)")
    nhwc = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
    if not nhwc and not (x.is_contiguous() and x.shape[-1] == bias.shape[0]):
        raise ValueError("bias_relu_: x must be channels_last [B, C, H, W], or contiguous with the channel axis innermost")
    if (nhwc and x.shape[1] != bias.shape[0]) or bias.dtype != torch.float32 or not bias.is_contiguous():
        raise ValueError("bias_relu_: bias must be a contiguous float32 vector with one entry per channel")
    c = int(bias.shape[0])
    with torch.cuda.device(x.device):
        rc = N.lib().iris_bias_relu(x.data_ptr(), bias.data_ptr(), x.numel() // c, c, _stream_ptr(x.device))
    N.check(rc, "iris_bias_relu")
    return x


def bias_relu_nchw_(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """In place max(x + bias[c], 0) on a CONTIGUOUS [B, C, H, W] activation (iris_bias_relu_nchw)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bias_relu_nchw_: x must be a contiguous float32 [B, C, H, W] tensor on a ROCm device")
    b, c, h, w = (int(v) for v in x.shape)
    with torch.cuda.device(x.device):
        rc = N.lib().iris_bias_relu_nchw(x.data_ptr(), bias.data_ptr(), b, c, h * w, _stream_ptr(x.device))
    N.check(rc, "iris_bias_relu_nchw")
    return x


def bias_relu_maxpool_nchw(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """maxpool2x2('same')(relu(x + bias)) reading a CONTIGUOUS [B, C, H, W] activation and returning the pooled tensor in
    channels_last memory format (iris_bias_relu_maxpool_nchw): the hand-over from an NCHW block to the NHWC rest."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bias_relu_maxpool_nchw: x must be a contiguous float32 [B, C, H, W] tensor on a ROCm device")
    b, c, h, w = (int(v) for v in x.shape)
    y = torch.empty((b, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = N.lib().iris_bias_relu_maxpool_nchw(x.data_ptr(), bias.data_ptr(), y.data_ptr(), b, h, w, c, _stream_ptr(x.device))
    N.check(rc, "iris_bias_relu_maxpool_nchw")
    return y


def bias_relu_maxpool(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """maxpool2x2('same')(relu(x + bias)) for a channels_last [B, C, H, W] activation in ONE pass (iris_bias_relu_maxpool):
    reads x once, writes a quarter of it.  Returns a channels_last [B, C, ceil(H/2), ceil(W/2)] tensor."""
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("bias_relu_maxpool: x must be a float32 channels_last [B, C, H, W] device tensor")
    b, c, h, w = (int(v) for v in x.shape)
    y = torch.empty((b, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device,
                    memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = N.lib().iris_bias_relu_maxpool(x.data_ptr(), bias.data_ptr(), y.data_ptr(), b, h, w, c, _stream_ptr(x.device))
    N.check(rc, "iris_bias_relu_maxpool")
    return y


def conv3x3_small_bias_relu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    """relu(conv2d(x, weight, padding=1) + bias) for a contiguous [B, 1 or 2, H, W] input in ONE pass: the CRNN's first layer,
    which writes 16-32x what it reads.  Output contiguous (iris_conv3x3_small_bias_relu_nchw; W a multiple of 4) or
    channels_last (iris_conv3x3_small_bias_relu_nhwc; W <= 2048, output channels 4 .. 256 dividing 1024).
    A NaN in x is a NaN in every output (all channels) whose 3x3 window holds it, as with torch's conv2d + relu - the ReLU does not
    turn it into 0 - and no other output changes; an infinity leaves those outputs non-finite wherever conv2d + relu does."""
    if (x.dim() != 4 or not x.is_contiguous() or not x.is_cuda or x.dtype != torch.float32 or x.shape[1] not in (1, 2)
            or tuple(weight.shape[1:]) != (x.shape[1], 3, 3) or not weight.is_contiguous()):
        raise ValueError("conv3x3_small_bias_relu: x must be a contiguous float32 device tensor [B, 1|2, H, W], "
                         "weight [Cout, Cin, 3, 3] contiguous")
    b, cin, h, w = (int(v) for v in x.shape)
    cout = int(weight.shape[0])
    if channels_last:
        if cout % 4 or cout > 256 or 1024 % cout or w > 2048:
            raise ValueError("conv3x3_small_bias_relu(channels_last): output channels 4 .. 256 dividing 1024, W <= 2048")
        y = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        fn, name = N.lib().iris_conv3x3_small_bias_relu_nhwc, "iris_conv3x3_small_bias_relu_nhwc"
    else:
        if w % 4:
            raise ValueError("conv3x3_small_bias_relu: W must be a multiple of 4 for the contiguous output")
        y = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device)
        fn, name = N.lib().iris_conv3x3_small_bias_relu_nchw, "iris_conv3x3_small_bias_relu_nchw"
    with torch.cuda.device(x.device):
        rc = fn(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), b, cin, cout, h, w, _stream_ptr(x.device))
    N.check(rc, name)
    return y


def conv3x3_small_bias_relu_nchw(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return conv3x3_small_bias_relu(x, weight, bias, channels_last=False)


def conv3x3_c32_bias_relu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, pool: bool = False,
                          out_chunked: bool = False) -> torch.Tensor:
    """relu(conv2d(x, weight, padding=1) + bias), with `pool` max-pooled 2x2 'same' behind it, for a channels_last
    [B, 32, H, W] input and a [32, 32, 3, 3] weight, on the fp32 matrix cores (iris_conv3x3_c32_bias_relu).  Returns a
    channels_last tensor, or with `out_chunked` the channel-chunked [B, 4, Ho, Wo, 8] activation of the Winograd layers."""
    if (x.dim() != 4 or x.shape[1] != 32 or not x.is_contiguous(memory_format=torch.channels_last) or not x.is_cuda
            or x.dtype != torch.float32 or tuple(weight.shape) != (32, 32, 3, 3) or not weight.is_contiguous()):
        raise ValueError("conv3x3_c32_bias_relu: x must be a float32 channels_last device tensor [B, 32, H, W], weight a contiguous "
                         "[32, 32, 3, 3]")
    b, _, h, w = (int(v) for v in x.shape)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if pool else (h, w)
    if out_chunked:  # [B, 4, Ho, Wo, 8]: what the Winograd layers behind it read (no conversion pass)
        y = torch.empty((b, 4, oh, ow, 8), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((b, 32, oh, ow), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = N.lib().iris_conv3x3_c32_bias_relu(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), b, h, w,
                                                1 if pool else 0, 1 if out_chunked else 0, _stream_ptr(x.device))
    N.check(rc, "iris_conv3x3_c32_bias_relu")
    return y


def conv3x3_c32(x: torch.Tensor, weight: torch.Tensor, transposed: bool = False, bn_sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bare conv2d(x, weight, padding=1) of a 32 -> 32 layer on the fp32 matrix cores (iris_conv3x3_c32: the inference
    kernel without bias / ReLU) for a channels_last [B, 32, H, W] input and a [32, 32, 3, 3] weight in any dense layout;
    `transposed`: the backward-data pass, conv2d(x, weight.flip(2, 3).transpose(0, 1), padding=1) with x = dz.
    A NaN in x (or in a weight) is a NaN in every output that sums it and in no other; with `bn_sums` the sums of a channel whose z
    holds a NaN are NaN (the BatchNorm behind it then gives NaN over that channel, as torch's does).  conv3x3_c32_bias_relu: its
    ReLU and its max-pool keep a NaN too (a pooled window with a NaN among its in-image elements is NaN)."""
    if (x.dim() != 4 or x.shape[1] != 32 or not x.is_contiguous(memory_format=torch.channels_last) or not x.is_cuda
            or x.dtype != torch.float32 or tuple(weight.shape) != (32, 32, 3, 3) or weight.dtype != torch.float32):
        raise ValueError("conv3x3_c32: x must be a float32 channels_last device tensor [B, 32, H, W], weight a float32 [32, 32, 3, 3]")
    b, _, h, w = (int(v) for v in x.shape)
    y = torch.empty((b, 32, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    so, si, sh, sw = (int(v) for v in weight.stride())
    with torch.cuda.device(x.device):
        if bn_sums is not None:   # + the statistics of the BatchNorm behind it into the zeroed [iris_bn_sums_len(32)] doubles
            if transposed or bn_sums.dtype != torch.float64 or bn_sums.numel() < int(N.lib().iris_bn_sums_len(32)):
                raise ValueError("conv3x3_c32: bn_sums must be float64 [iris_bn_sums_len(32)] (forward pass only)")
            rc = N.lib().iris_conv3x3_c32_bn(x.data_ptr(), weight.data_ptr(), so, si, sh, sw, y.data_ptr(), b, h, w, bn_sums.data_ptr(),
                                             _stream_ptr(x.device))
        else:
            rc = N.lib().iris_conv3x3_c32(x.data_ptr(), weight.data_ptr(), so, si, sh, sw, 1 if transposed else 0, y.data_ptr(), b, h, w,
                                          _stream_ptr(x.device))
    N.check(rc, "iris_conv3x3_c32")
    return y


def wino_pack_weights(weight: torch.Tensor) -> torch.Tensor:
    """U = G g G^T of a [Cout, Cin, 3, 3] convolution weight in the Winograd kernel's LDS order (iris_wino_pack_weights, on the
    host, once per layer); returns a device tensor of 16 Cin Cout floats on the weight's device."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("wino_pack_weights: a [Cout, Cin, 3, 3] weight is expected")
    host = np.ascontiguousarray(weight.detach().to(torch.float32).cpu().contiguous().numpy())
    out = np.empty(int(N.lib().iris_wino_packed_len(cin, cout)), np.float32)
    N.check(N.lib().iris_wino_pack_weights(host.ctypes.data, cin, cout, out.ctypes.data), "iris_wino_pack_weights")
    return torch.from_numpy(out).to(weight.device)


def to_chunked(x: torch.Tensor) -> torch.Tensor:
    """channels_last [B, C, H, W] (or any layout) -> the channel-chunked activation [B, C / 8, H, W, 8] of the Winograd layers."""
    b, c, h, w = (int(v) for v in x.shape)
    return x.permute(0, 2, 3, 1).reshape(b, h, w, c // 8, 8).permute(0, 3, 1, 2, 4).contiguous()


# The library functions of the two Winograd kernel families, by `split_bf16`: the exact-fp32 kernel and the one on the BF16 matrix
# cores at fp32 accuracy.  Their packings differ in format and size: a packing goes only to the kernel of its own family.
_WINO_FNS = {
    False: {"packed_len": "iris_wino_packed_len", "pack": "iris_wino_pack_weights_device",
            "conv": "iris_conv3x3_wino", "conv_bn": "iris_conv3x3_wino_bn"},
    True: {"packed_len": "iris_wino_b3_packed_len", "pack": "iris_wino_b3_pack_weights_device",
           "conv": "iris_conv3x3_wino_b3", "conv_bn": "iris_conv3x3_wino_b3_bn"},
}


def wino_pack_weights_device(weight: torch.Tensor, transposed: bool = False, out: Optional[torch.Tensor] = None,
                             split_bf16: bool = False) -> torch.Tensor:
    """The same packing on the device, on the current stream, from the weight as it lies in memory (any strides: a
    channels_last parameter needs no copy) - what a training step does every step.  `transposed`: the weights of the
    backward-data pass (dx = conv(dz, W'), W'[ci][co][i][j] = W[co][ci][2 - i][2 - j]).  `split_bf16`: U split into three bf16
    terms in the operand order of iris_conv3x3_wino_b3 (the convolution on the BF16 matrix cores at fp32 accuracy).
    `out`: a float32 tensor of at least wino_packed_len floats on the weight's device."""
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
        raise ValueError("wino_pack_weights_device: a float32 device weight [Cout, Cin, 3, 3] is expected (no CPU fallback)")
    co, ci = int(weight.shape[0]), int(weight.shape[1])
    cin, cout = (co, ci) if transposed else (ci, co)
    n = wino_packed_len(cin, cout, split_bf16)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=weight.device)
    elif not (out.dtype == torch.float32 and out.device == weight.device and out.numel() >= n):
        raise ValueError(f"wino_pack_weights_device: out must be a float32 tensor of at least {n} elements on {weight.device}")
    so, si, sh, sw = (int(v) for v in weight.stride())
    name = _WINO_FNS[bool(split_bf16)]["pack"]
    with torch.cuda.device(weight.device):
        rc = getattr(N.lib(), name)(weight.data_ptr(), so, si, sh, sw, cin, cout, 1 if transposed else 0, out.data_ptr(),
                                    _stream_ptr(weight.device))
    N.check(rc, name)
    return out


def wino_packed_len(cin: int, cout: int, split_bf16: bool = False) -> int:
    """floats of the packed weights of a cin -> cout layer (iris_wino_packed_len / iris_wino_b3_packed_len)."""
    return int(getattr(N.lib(), _WINO_FNS[bool(split_bf16)]["packed_len"])(int(cin), int(cout)))


def wino_pack_weights_device_multi(jobs, split_bf16: bool = False) -> None:
    """`jobs`: [(weight [Cout, Cin, 3, 3] float32 device tensor, transposed, out float32 device tensor of wino_packed_len floats)]:
    every packing in ONE launch on the current stream (iris_wino_pack_weights_device_multi), same results as
    `wino_pack_weights_device` per job."""
    if not jobs:
        return
    arr = (N.PackJob * len(jobs))()
    dev = jobs[0][0].device
    for k, (weight, transposed, out) in enumerate(jobs):
        if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)
                and out.is_cuda and out.dtype == torch.float32 and weight.device == dev and out.device == dev):
            raise ValueError("wino_pack_weights_device_multi: float32 device tensors on one device are expected (no CPU fallback)")
        co, ci = int(weight.shape[0]), int(weight.shape[1])
        cin, cout = (co, ci) if transposed else (ci, co)
        if out.numel() < wino_packed_len(cin, cout, split_bf16):
            raise ValueError("wino_pack_weights_device_multi: output buffer too small")
        so, si, sh, sw = (int(v) for v in weight.stride())
        arr[k] = N.PackJob(weight.data_ptr(), out.data_ptr(), so, si, sh, sw, cin, cout, 1 if transposed else 0, 0)
    with torch.cuda.device(dev):
        rc = N.lib().iris_wino_pack_weights_device_multi(C.cast(arr, C.c_void_p), len(jobs), 1 if split_bf16 else 0, _stream_ptr(dev))
    N.check(rc, "iris_wino_pack_weights_device_multi")


def conv3x3_wino(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, pool: bool = False,
                 out_nhwc: bool = False, relu: bool = True, split_bf16: bool = False, bn_sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2d(x, weight, padding=1) (+ bias, + ReLU, + MaxPool 2x2 'same') as Winograd F(2x2, 3x3) on the fp32 matrix cores
    (iris_conv3x3_wino).  x: channel-chunked [B, Cin / 8, H, W, 8], or a channels_last [B, Cin, H, W] tensor (read where it
    lies: IRIS_WINO_IN_NHWC); packed: `wino_pack_weights[_device]` with the same `split_bf16`, on x's device (a shorter packing is
    refused; a split-bf16 packing given to the fp32 kernel is long enough and cannot be told apart); returns the chunked
    [B, cout / 8, Ho, Wo, 8] or, with `out_nhwc`, a channels_last [B, cout, Ho, Wo] tensor.
    NaN: a NaN in x is a NaN in every output, in all channels, whose 3x3 window holds it - through bias + ReLU, through the max-pool (a
    window with a NaN among its in-image elements is NaN) and in the bare form (relu=False, which hands z on as it is, no -inf in its
    place) - and, with `bn_sums`, in the channel's sums.  The other outputs of the 2x2 tiles whose 4x4 input patch holds it may be
    NaN as well (the Winograd transform mixes the patch); every other tile has the bits of the run without it.  An infinity leaves
    the same places non-finite."""
    if not (x.is_cuda and x.dtype == torch.float32):
        raise ValueError("conv3x3_wino: x must be a float32 device tensor (no CPU fallback)")
    if x.dim() == 5 and x.shape[4] == 8 and x.is_contiguous():
        b, cbk, h, w, _ = (int(v) for v in x.shape)
        cin, in_nhwc = 8 * cbk, False
    elif x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        b, cin, h, w = (int(v) for v in x.shape)
        in_nhwc = True
    else:
        raise ValueError("conv3x3_wino: x must be contiguous [B, Cin / 8, H, W, 8] or channels_last [B, Cin, H, W]")
    need = wino_packed_len(cin, int(cout), split_bf16)   # what the kernel reads
    if not (packed.dtype == torch.float32 and packed.device == x.device and packed.is_contiguous() and packed.numel() >= need):
        raise ValueError(f"conv3x3_wino: packed must be a contiguous float32 tensor of at least {need} elements on {x.device} "
                         f"(wino_pack_weights_device(..., split_bf16={bool(split_bf16)}))")
    ho, wo = ((h + 1) // 2, (w + 1) // 2) if pool else (h, w)
    if out_nhwc:
        y = torch.empty((b, cout, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    else:
        y = torch.empty((b, cout // 8, ho, wo, 8), dtype=torch.float32, device=x.device)
    flags = (N.IRIS_WINO_POOL if pool else 0) | (N.IRIS_WINO_OUT_NHWC if out_nhwc else 0) | \
        (N.IRIS_WINO_IN_NHWC if in_nhwc else 0) | (N.IRIS_WINO_RELU if relu else 0)
    lib, fns = N.lib(), _WINO_FNS[bool(split_bf16)]
    with torch.cuda.device(x.device):
        if bn_sums is not None:   # the bare convolution + the statistics of the BatchNorm behind it (zeroed float64 [iris_bn_sums_len(cout)])
            if bias is not None or bn_sums.dtype != torch.float64 or bn_sums.numel() < int(lib.iris_bn_sums_len(int(cout))):
                raise ValueError("conv3x3_wino: bn_sums goes with the bare convolution (no bias) and must be float64 [iris_bn_sums_len(cout)]")
            rc = getattr(lib, fns["conv_bn"])(x.data_ptr(), packed.data_ptr(), y.data_ptr(), b, h, w, cin, int(cout), flags, bn_sums.data_ptr(),
                                              _stream_ptr(x.device))
        else:
            rc = getattr(lib, fns["conv"])(x.data_ptr(), packed.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                           b, h, w, cin, int(cout), flags, _stream_ptr(x.device))
    N.check(rc, fns["conv"])
    return y


# (device index, stream) -> scratch tensors of conv3x3_wino_wrw.  Grow-only: a captured hipGraph keeps its pointers.  One set per
# STREAM: the partial sums of two backward passes running on different streams of a device (a graph replay beside an eager
# step, two models on side streams) must not share a buffer; calls on one stream are ordered by the stream.
_WRW_WORKSPACES = {}


def _wrw_workspace(device: torch.device, floats: int) -> torch.Tensor:
    held = _WRW_WORKSPACES.setdefault((device.index, int(torch.cuda.current_stream(device).cuda_stream)), [])
    if not held or held[-1].numel() < floats:
        held.append(torch.empty(max(floats, 1 << 24), dtype=torch.float32, device=device))
    return held[-1]


def conv3x3_wino_wrw(x: torch.Tensor, dy: torch.Tensor, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The weight gradient of z = conv2d(x, weight, padding=1) given dy = dL/dz, as Winograd F(2x2, 3x3) on the fp32 matrix
    cores (iris_conv3x3_wino_wrw).  x [B, Cin, H, W] and dy [B, Cout, H, W]: channels_last float32 device tensors, Cin and
    Cout multiples of 32.  Returns dW [Cout, Cin, 3, 3] with the strides of `like` (the weight) or channels_last.
    The partial sums go through one scratch buffer per (device, stream): calls on one stream are ordered by it, calls on
    different streams do not share a buffer."""
    if not (x.is_cuda and x.dtype == torch.float32 and dy.dtype == torch.float32 and dy.device == x.device):
        raise ValueError("conv3x3_wino_wrw: x and dy must be float32 tensors on one device (no CPU fallback)")
    if not (x.dim() == 4 and dy.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and dy.is_contiguous(memory_format=torch.channels_last) and x.shape[0] == dy.shape[0] and x.shape[2:] == dy.shape[2:]):
        raise ValueError("conv3x3_wino_wrw: x [B, Cin, H, W] and dy [B, Cout, H, W] must be channels_last and of one geometry")
    b, cin, h, w = (int(v) for v in x.shape)
    cout = int(dy.shape[1])
    if like is not None and tuple(like.shape) == (cout, cin, 3, 3) and like.dtype == torch.float32:
        dw = torch.empty_like(like)   # preserves the parameter's strides: AccumulateGrad takes it without a copy
    else:
        dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last)
    lib = N.lib()
    with torch.cuda.device(x.device):
        ws = _wrw_workspace(x.device, int(lib.iris_wino_wrw_workspace_len(b, h, w, cin, cout)))
        so, si, sh, sw = (int(v) for v in dw.stride())
        rc = lib.iris_conv3x3_wino_wrw(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), so, si, sh, sw, b, h, w, cin, cout, 0,
                                       ws.data_ptr(), ws.numel(), _stream_ptr(x.device))
    N.check(rc, "iris_conv3x3_wino_wrw")
    return dw


def conv3x3_wino_bias_relu(x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, cout: int, pool: bool = False,
                           out_nhwc: bool = False, split_bf16: bool = False) -> torch.Tensor:
    """The inference form: relu(conv2d(x, weight, padding=1) + bias), with `pool` max-pooled, on the chunked layout."""
    if not (x.dim() == 5 and x.shape[-1] == 8):
        raise ValueError("conv3x3_wino_bias_relu: x must be the channel-chunked activation [B, Cin / 8, H, W, 8]")
    return conv3x3_wino(x, packed, bias, cout, pool=pool, out_nhwc=out_nhwc, relu=True, split_bf16=split_bf16)


def _check_bilstm(gx, w_hh, who):
    if (gx.dim() != 4 or tuple(gx.shape[2:]) != (2, 512) or tuple(w_hh.shape) != (2, 512, 128) or not gx.is_cuda
            or gx.dtype != torch.float32 or w_hh.dtype != torch.float32 or w_hh.device != gx.device):
        raise ValueError(f"{who}: gx must be a float32 device tensor [B, T, 2, 512], w_hh [2, 512, 128] beside it")


def bilstm128_forward(gx: torch.Tensor, w_hh: torch.Tensor, save: bool = False):
    """Recurrent half of Bidirectional(LSTM(128, return_sequences=True)) in ONE launch (iris_bilstm128_forward).
    gx [B, T, 2, 512]: input pre-activations x_t W_ih^T + b_ih + b_hh per direction, gate rows i, f, g, o;
    w_hh [2, 512, 128]: recurrent matrices.  Returns [B, T, 256] = (h forward, h backward) per step, h_0 = c_0 = 0;
    with `save` also the activations [B, T, 2, 5, 128] = (i, f, g, o, c) that `bilstm128_backward` needs."""
    _check_bilstm(gx, w_hh, "bilstm128_forward")
    gx, w_hh = gx.contiguous(), w_hh.contiguous()
    b, t = int(gx.shape[0]), int(gx.shape[1])
    out = torch.empty((b, t, 256), dtype=torch.float32, device=gx.device)
    act = torch.empty((b, t, 2, 5, 128), dtype=torch.float32, device=gx.device) if save else None
    with torch.cuda.device(gx.device):
        rc = N.lib().iris_bilstm128_forward(gx.data_ptr(), w_hh.data_ptr(), out.data_ptr(),
                                            act.data_ptr() if save else None, b, t, _stream_ptr(gx.device))
    N.check(rc, "iris_bilstm128_forward")
    return (out, act) if save else out


def bilstm128_backward(dout: torch.Tensor, act: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """Back-propagation through time of `bilstm128_forward` in ONE launch: dout [B, T, 256] and the saved activations ->
    the gradient of the input pre-activations, dgx [B, T, 2, 512]."""
    # refused before .contiguous() and before any launch: a host tensor here would hand the kernel a host pointer
    if (dout.dim() != 3 or dout.shape[2] != 256 or tuple(act.shape) != (dout.shape[0], dout.shape[1], 2, 5, 128)
            or tuple(w_hh.shape) != (2, 512, 128) or not (dout.is_cuda and act.is_cuda and w_hh.is_cuda)
            or act.device != dout.device or w_hh.device != dout.device
            or dout.dtype != torch.float32 or act.dtype != torch.float32 or w_hh.dtype != torch.float32):
        raise ValueError("bilstm128_backward: dout [B, T, 256], act [B, T, 2, 5, 128], w_hh [2, 512, 128], all float32 on one device")
    b, t = int(dout.shape[0]), int(dout.shape[1])
    dout, act, w_hh = dout.contiguous(), act.contiguous(), w_hh.contiguous()
    dgx = torch.empty((b, t, 2, 512), dtype=torch.float32, device=dout.device)
    with torch.cuda.device(dout.device):
        rc = N.lib().iris_bilstm128_backward(dout.data_ptr(), act.data_ptr(), w_hh.data_ptr(), dgx.data_ptr(), b, t,
                                             _stream_ptr(dout.device))
    N.check(rc, "iris_bilstm128_backward")
    return dgx


class PipelinedFrontend:
    """Independent batches through the fused path on `n_streams` HIP streams, one `FrontendPlan` each (a plan's
    workspace belongs to one stream, include/iris_frontend.h), in the two-kernel form of the step: one stream's
    min-max/log kernel and launch gaps run in the shadow of another's fused kernel.

        pipe = PipelinedFrontend(2, n_fft=1024, hop=256, n_mel=64, channels=1, max_batch=32, max_len=160000, device=dev)
        for wav, out in batches:                 # device tensors; `out` is written asynchronously
            pipe.submit(wav, out=out)
        pipe.synchronize()                       # ... or order consumers after pipe.streams[i] with events

    The caller's current stream at `submit` time is waited for (inputs produced on it are ready), and every submit's
    stream is joined back by `synchronize()` / `join()` so that later work on the current stream sees the outputs."""

    def __init__(self, n_streams: int = 2, **plan_kwargs):
        if n_streams < 1:
            raise ValueError("n_streams must be >= 1")
        self.plans = [FrontendPlan(**plan_kwargs) for _ in range(n_streams)]
        if n_streams > 1:  # concurrent launches on one device: no in-kernel waits between workgroups
            for p in self.plans:
                p.set_epilogue("two_kernels")
        self.device = self.plans[0].device
        self.streams = [torch.cuda.Stream(self.device) for _ in range(n_streams)]
        self._next = 0

    def submit(self, wav: torch.Tensor, wait_current: bool = True, **kwargs) -> torch.Tensor:
        """wait_current=False skips the event wait on the current stream and the allocator bookkeeping (about 7 us
        of host time per call, enough to make a 23 us step host-bound): for inputs and `out` buffers that are
        long-lived and already complete, as in a steady-state loop over preallocated batches."""
        i, self._next = self._next, (self._next + 1) % len(self.plans)
        stream = self.streams[i]
        if wait_current:
            stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream):
            out = self.plans[i].wav_to_logmel(wav, **kwargs)
        if wait_current:
            wav.record_stream(stream)
            out.record_stream(stream)
        return out

    def join(self) -> None:
        """Order the current stream after everything submitted so far (no host wait)."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    def synchronize(self) -> None:
        for s in self.streams:
            s.synchronize()


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """torchaudio.compliance.kaldi.resample_waveform(wav, orig_freq, new_freq) (data_utils.py:20-21) for a device waveform
    [chan, samples] (or [samples]): the Hann-windowed-sinc polyphase filter of torchaudio.functional.resample
    (lowpass_filter_width 6, rolloff 0.99) as one HIP launch (iris_resample); returns [chan, ceil(new_freq samples / orig_freq)]."""
    wav = _require_device_f32(wav, "wav")
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
        raise ValueError("resample: the sample rates must be positive integers")   # (torchaudio raises for non-integer rates too)
    flat = wav.dim() == 1
    if wav.dim() not in (1, 2) or wav.numel() == 0:
        raise ValueError("resample: wav must be a non-empty [chan, samples] or [samples] tensor")
    w2 = (wav.unsqueeze(0) if flat else wav).contiguous()
    chan, n = int(w2.shape[0]), int(w2.shape[1])
    lib = N.lib()
    n_out = int(lib.iris_resample_len(n, int(orig_freq), int(new_freq)))
    out = torch.empty((chan, n_out), dtype=torch.float32, device=wav.device)
    with torch.cuda.device(wav.device):
        rc = lib.iris_resample(w2.data_ptr(), chan, n, int(orig_freq), int(new_freq), out.data_ptr(), _stream_ptr(wav.device))
    N.check(rc, "iris_resample")
    return out[0] if flat else out


def normalize(wav: torch.Tensor) -> torch.Tensor:
    """wav / (10 rms) with the rms over the whole tensor for [C,L] input
    (data_utils.py:32-34) or per leading item for [B,C,L]."""
    wav = _require_device_f32(wav, "wav")
    if wav.dim() not in (2, 3):
        raise ValueError("wav must be [C, L] or [B, C, L]")
    n_rows = 1 if wav.dim() == 2 else int(wav.shape[0])
    row_len = wav.numel() // max(n_rows, 1)
    out = torch.empty_like(wav)
    lib = N.lib()
    ws = torch.empty(max(int(lib.iris_normalize_workspace(n_rows, row_len)), 1), dtype=torch.float32,
                     device=wav.device)
    with torch.cuda.device(wav.device):
        rc = lib.iris_normalize(wav.data_ptr(), out.data_ptr(), n_rows, row_len, ws.data_ptr(), ws.numel(),
                                _stream_ptr(wav.device))
    N.check(rc, "iris_normalize")
    return out


def minmax_log(x: torch.Tensor, do_minmax: bool = True, do_log: bool = True, eps_div: float = EPSILON,
               eps_log: float = EPSILON) -> torch.Tensor:
    """Out-of-place min-max over every axis except 0, then ln(x + eps)."""
    x = _require_device_f32(x, "x").clone()
    if x.dim() < 1 or x.numel() == 0:
        return x
    n_rows = int(x.shape[0])
    row_len = x.numel() // n_rows
    lib = N.lib()
    ws = torch.empty(max(int(lib.iris_minmax_log_workspace(n_rows, row_len)), 1), dtype=torch.float32,
                     device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.iris_minmax_log(x.data_ptr(), n_rows, row_len, 1 if do_minmax else 0, 1 if do_log else 0,
                                 float(eps_div), float(eps_log), ws.data_ptr(), ws.numel(),
                                 _stream_ptr(x.device))
    N.check(rc, "iris_minmax_log")
    return x


# PCEN defaults (librosa.pcen's): time constant 0.4 s, gain a, bias d, power r, eps
PCEN_TIME_CONSTANT, PCEN_GAIN, PCEN_BIAS, PCEN_POWER, PCEN_EPS = 0.4, 0.98, 2.0, 0.5, 1e-6


def pcen_smooth(time_constant_s: float = PCEN_TIME_CONSTANT, sr: int = 16000, hop: int = 256) -> float:
    """The smoother coefficient s of a time constant, as librosa.pcen derives it: T = time_constant_s * sr / hop frames,
    s = (sqrt(1 + 4 T^2) - 1) / (2 T^2)."""
    t = float(time_constant_s) * float(sr) / float(hop)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"pcen_smooth: the time constant must give a positive number of frames, got {t}")
    return float((np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t))


def _pcen_view(x: torch.Tensor, time_axis: int, out: Optional[torch.Tensor], who: str):
    x = _require_device_f32(x, "x")
    if x.dim() < 1:
        raise ValueError(f"{who}: x must have a time axis")
    ax = time_axis % x.dim() if -x.dim() <= time_axis < x.dim() else None
    if ax is None:
        raise ValueError(f"{who}: time_axis {time_axis} is out of range for a {x.dim()}-d tensor")
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == tuple(x.shape) and out.device == x.device):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of shape {tuple(x.shape)} on {x.device}")
    shape = tuple(int(v) for v in x.shape)
    n_rows = int(np.prod(shape[:ax], dtype=np.int64))
    n_inner = int(np.prod(shape[ax + 1:], dtype=np.int64))
    return x, out, n_rows, shape[ax], n_inner


def pcen(x: torch.Tensor, smooth: Optional[float] = None, gain: float = PCEN_GAIN, bias: float = PCEN_BIAS,
         power: float = PCEN_POWER, eps: float = PCEN_EPS, time_axis: int = -2,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-channel energy normalisation of mel magnitudes x >= 0 along `time_axis` (iris_pcen, one HIP launch): every
    sequence along time, i.e. every (clip, mel, channel) of a batched [B, M, T, C] or (mel, channel) of an unbatched
    [M, T, C] tensor, runs
        M[0] = E[0],  M[t] = (1 - s) M[t-1] + s E[t],  out = (E / (eps + M)^gain + bias)^power - bias^power
    (evaluated as bias^power expm1(power log1p(...))).  smooth = s, default `pcen_smooth()` (0.4 s at 16 kHz, hop 256);
    the other defaults are librosa's.  Zeros stay exactly 0; a NaN propagates forward in time.  Returns a new tensor, or
    writes into `out` (which may be `x` itself: in place).  Out-of-range parameters raise ValueError."""
    x, out, n_rows, n_time, n_inner = _pcen_view(x, time_axis, out, "pcen")
    s = pcen_smooth() if smooth is None else float(smooth)
    if x.numel():
        with torch.cuda.device(x.device):
            rc = N.lib().iris_pcen(x.data_ptr(), out.data_ptr(), n_rows, n_time, n_inner, s, float(gain), float(bias),
                                   float(power), float(eps), _stream_ptr(x.device))
        N.check(rc, "iris_pcen")
    return out


def pcen_smoother(x: torch.Tensor, smooth: Optional[float] = None, time_axis: int = -2,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The smoother M of `pcen` itself (iris_pcen_smoother): M[0] = E[0], M[t] = (1 - s) M[t-1] + s E[t] along time_axis."""
    x, out, n_rows, n_time, n_inner = _pcen_view(x, time_axis, out, "pcen_smoother")
    s = pcen_smooth() if smooth is None else float(smooth)
    if x.numel():
        with torch.cuda.device(x.device):
            rc = N.lib().iris_pcen_smoother(x.data_ptr(), out.data_ptr(), n_rows, n_time, n_inner, s, _stream_ptr(x.device))
        N.check(rc, "iris_pcen_smoother")
    return out


def _pcen_banded_view(x: torch.Tensor, params: torch.Tensor, time_axis: int, out: Optional[torch.Tensor], who: str):
    """`_pcen_view` plus the band axis: the axis in front of `time_axis` holds the bands, params is [4, n_bands]."""
    x, out, n_rows, n_time, n_inner = _pcen_view(x, time_axis, out, who)
    ax = time_axis % x.dim()
    if ax < 1:
        raise ValueError(f"{who}: x needs a band axis in front of the time axis (got time_axis {time_axis} of a {x.dim()}-d tensor)")
    n_bands = int(x.shape[ax - 1])
    if not (isinstance(params, torch.Tensor) and params.is_cuda and params.device == x.device and params.dtype == torch.float32
            and params.is_contiguous() and tuple(params.shape) == (4, n_bands)):
        raise ValueError(f"{who}: params must be a contiguous float32 tensor of shape (4, {n_bands}) on {x.device} "
                         "(rows: smooth s, gain a, bias d, power r)")
    return x, out, n_rows, n_time, n_inner, n_bands


def pcen_banded(x: torch.Tensor, params: torch.Tensor, eps: float = PCEN_EPS, time_axis: int = -2,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`pcen` with its own parameters for every band (iris_pcen_banded, one HIP launch): the axis in front of `time_axis`
    is the band axis (M of a batched [B, M, T, C] or an unbatched [M, T, C] tensor) and `params` [4, n_bands] holds the
    effective s (0 < s <= 1), a (>= 0), d (> 0), r (0 < r <= 1) of each band on the device.  Their ranges are the caller's
    to keep (`model.PCEN` does by construction): they cannot be checked without a host synchronisation.  Zero / NaN
    semantics, `out` and in place as `pcen`."""
    x, out, n_rows, n_time, n_inner, n_bands = _pcen_banded_view(x, params, time_axis, out, "pcen_banded")
    if x.numel():
        with torch.cuda.device(x.device):
            rc = N.lib().iris_pcen_banded(x.data_ptr(), out.data_ptr(), n_rows, n_time, n_inner, params.data_ptr(), n_bands,
                                          float(eps), _stream_ptr(x.device))
        N.check(rc, "iris_pcen_banded")
    return out


def pcen_banded_grad(x: torch.Tensor, dout: torch.Tensor, params: torch.Tensor, eps: float = PCEN_EPS,
                     time_axis: int = -2) -> torch.Tensor:
    """Gradient [4, n_bands] of a scalar loss with respect to `pcen_banded`'s effective parameters, given the loss's
    gradient `dout` with respect to its output (iris_pcen_banded_grad: two HIP launches, no atomics, bitwise reproducible).
    The smoother is recomputed from x; x is data, so no gradient with respect to it exists."""
    x = _require_device_f32(x, "x")
    x, _, n_rows, n_time, n_inner, n_bands = _pcen_banded_view(x, params, time_axis, x, "pcen_banded_grad")  # (no output tensor)
    if not (isinstance(dout, torch.Tensor) and dout.is_cuda and dout.device == x.device and dout.dtype == torch.float32
            and tuple(dout.shape) == tuple(x.shape)):
        raise ValueError(f"pcen_banded_grad: dout must be a float32 tensor of shape {tuple(x.shape)} on {x.device}")
    dout = dout.contiguous()
    dparams = (torch.empty if x.numel() else torch.zeros)((4, n_bands), dtype=torch.float32, device=x.device)
    if x.numel():
        lib = N.lib()
        ws = torch.empty(max(int(lib.iris_pcen_banded_grad_workspace(n_rows, n_time, n_inner)), 1), dtype=torch.float32,
                         device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.iris_pcen_banded_grad(x.data_ptr(), dout.data_ptr(), n_rows, n_time, n_inner, params.data_ptr(), n_bands,
                                           float(eps), dparams.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(x.device))
        N.check(rc, "iris_pcen_banded_grad")
    return dparams


# mirrors iris_voc_src (include/iris_frontend.h)
VOC_SRC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("n_in", "<i4"), ("n_out", "<i4"), ("rate", "<f8")])
assert VOC_SRC.itemsize == 32


def _scaled_len(n: int, rate: float, word: str) -> int:
    """ceil(n / rate) in double, the length of numpy.arange(0, n, rate): the one length law of `stretched_frames` and
    `speed_len` (`word` names the caller's rate in the error)."""
    rate = float(rate)
    if not (np.isfinite(rate) and rate > 0):
        raise ValueError(f"{word} rate must be a positive finite number, got {rate}")
    return int(np.ceil(float(n) / rate))


def stretched_frames(n_frames: int, rate: float) -> int:
    """Frames of a spectrogram of `n_frames` frames stretched by `rate`: ceil(n_frames / rate) in double, the length of
    numpy.arange(0, n_frames, rate)."""
    return _scaled_len(n_frames, rate, "stretch")


def _launch_records(table: np.ndarray, device: torch.device, table_dev: Optional[torch.Tensor], name: str, call) -> torch.Tensor:
    """Upload a table of records (into `table_dev`, a long-lived uint8 device buffer, when given) and run
    `call(device table pointer, record count, stream)` - the C entry point `name` - on the current stream of `device`.
    Returns the device table (tied to the stream when it was allocated here)."""
    raw = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(-1))
    if table_dev is None:
        dev_table = raw.to(device, non_blocking=True)
    else:
        dev_table = table_dev[:raw.numel()]
        dev_table.copy_(raw)
    with torch.cuda.device(device):
        rc = call(dev_table.data_ptr(), int(table.shape[0]), _stream_ptr(device))
    N.check(rc, name)
    if table_dev is None and dev_table.numel():
        dev_table.record_stream(torch.cuda.current_stream(device))
    return dev_table


LOCATE_MAX_LAGS = 4097    # the lag limit of iris_locate_events (include/iris_frontend.h): max_lag <= 2048


def locate_table(events, block: int, n_frames: int, batch: int) -> np.ndarray:
    """The int32 [E, 4] event table of iris_locate_events from events [E, 3] = (sample, first frame, last frame; inclusive):
    column 3 is the event's first segment, the running count of the segments of the events before it - an event is cut at the
    boundaries of blocks of `block` frames into last // block - first // block + 1 segments.  ValueError: a shape other than
    [E, 3], values that are not integers, a sample outside [0, batch), frames outside [0, n_frames) or first > last."""
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events)
    if ev.size == 0:
        return np.zeros((0, 4), np.int32)
    if ev.ndim != 2 or ev.shape[1] != 3 or not np.issubdtype(ev.dtype, np.integer):
        raise ValueError(f"locate: events must be integers [E, 3] = (sample, first frame, last frame), got {ev.dtype} {ev.shape}")
    ev, block = ev.astype(np.int64), int(block)
    if block < 1:
        raise ValueError(f"locate: block = {block} must be at least 1 frame")
    bad = np.flatnonzero((ev[:, 0] < 0) | (ev[:, 0] >= batch) | (ev[:, 1] < 0) | (ev[:, 1] > ev[:, 2]) | (ev[:, 2] >= n_frames))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"locate: event {i} = (sample {ev[i, 0]}, frames {ev[i, 1]} .. {ev[i, 2]}) does not fit {batch} sample(s) of "
                         f"{n_frames} frames with first <= last")
    n_seg = ev[:, 2] // block - ev[:, 1] // block + 1
    if int(n_seg.sum()) > 2 ** 31 - 1:
        raise ValueError("locate: more than 2^31 - 1 segments")
    table = np.empty((len(ev), 4), np.int32)
    table[:, :3] = ev
    table[:, 3] = np.concatenate([[0], np.cumsum(n_seg)[:-1]])
    return table


TRACK_MAX_LAGS = 2049     # the lag limit of iris_track_lags (include/iris_frontend.h): max_lag <= 1024


def track_step(step, block=None) -> int:
    """`step` as a frame count >= 1; with `block` (the frames per block of the factors) block % step == 0, so that a step lies
    in one block.  ValueError otherwise."""
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 1:
        raise ValueError(f"track: step = {step!r} must be a number of frames >= 1")
    if block is not None and int(block) % int(step):
        raise ValueError(f"track: block = {block} is not a multiple of step = {step}: a step must lie in one block")
    return int(step)


def track_offsets(row_offsets, rows: int) -> np.ndarray:
    """row_offsets as a contiguous int32 [E + 1] that starts at 0, strictly ascends (every event has a step) and ends at `rows`;
    E = 0: [0] with rows == 0.  ValueError otherwise."""
    off = np.asarray(row_offsets.cpu() if torch.is_tensor(row_offsets) else row_offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"track: row_offsets must be integers [E + 1], got {off.dtype} {off.shape}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != rows or (np.diff(off) < 1).any() or rows > 2 ** 31 - 1:
        raise ValueError(f"track: row_offsets must start at 0, ascend strictly and end at the {rows} rows of R, got {off.tolist()[:8]}"
                         f"{' ...' if off.size > 8 else ''}")
    return np.ascontiguousarray(off, np.int32)


def track_penalties(pen, max_jump, lags: int) -> np.ndarray:
    """The table P[d] = d x pen of iris_track_lags, float64 [min(max_jump, lags - 1) + 1], formed once here.  ValueError: pen not
    a finite number >= 0, max_jump not an integer >= 0, lags even, < 1 or above TRACK_MAX_LAGS."""
    if isinstance(pen, bool) or not isinstance(pen, (int, float, np.integer, np.floating)) or not (np.isfinite(pen) and pen >= 0):
        raise ValueError(f"track: pen = {pen!r} must be a finite number >= 0")
    if isinstance(max_jump, bool) or not isinstance(max_jump, (int, np.integer)) or max_jump < 0:
        raise ValueError(f"track: max_jump = {max_jump!r} must be an integer >= 0")
    if lags < 1 or lags % 2 != 1 or lags > TRACK_MAX_LAGS:
        raise ValueError(f"track: {lags} lags; an odd count 2 N + 1 of at most {TRACK_MAX_LAGS} is tracked")
    return np.arange(min(int(max_jump), lags - 1) + 1, dtype=np.float64) * np.float64(pen)


def track_buffers(rows: int, lags: int, device):
    """(flat, R [rows, lags] float64, n_terms [rows] int64, path [rows] int32): the outputs of `locate_steps` and `track` as views
    of ONE flat int64 device buffer, so that one copy brings all three back."""
    flat = torch.empty((rows * lags + rows + (rows + 1) // 2,), dtype=torch.int64, device=device)
    resp = flat[:rows * lags].view(torch.float64).view(rows, lags)
    return flat, resp, flat[rows * lags:rows * lags + rows], flat[rows * lags + rows:].view(torch.int32)[:rows]


def track_unpack(flat, rows: int, lags: int):
    """(R, n_terms, path) as NumPy arrays from a host copy of `track_buffers`' flat buffer."""
    a = np.ascontiguousarray(flat.cpu().numpy() if torch.is_tensor(flat) else flat)
    return (a[:rows * lags].view(np.float64).reshape(rows, lags), a[rows * lags:rows * lags + rows],
            a[rows * lags + rows:].view(np.int32)[:rows])


def beamform_table(events, n_frames: int, batch: int) -> np.ndarray:
    """The int32 [E, 4] event table of iris_beamform_events from events [E, 3] = (sample, first frame, last frame; inclusive):
    column 3 is the event's first output frame, the running count of the frames of the events before it (slab e starts at
    float 2 F x column 3).  ValueError: a shape other than [E, 3], values that are not integers, a sample outside [0, batch),
    frames outside [0, n_frames), first > last, or more than 2^31 - 1 output frames."""
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events)
    if ev.size == 0:
        return np.zeros((0, 4), np.int32)
    if ev.ndim != 2 or ev.shape[1] != 3 or not np.issubdtype(ev.dtype, np.integer):
        raise ValueError(f"beamform: events must be integers [E, 3] = (sample, first frame, last frame), got {ev.dtype} {ev.shape}")
    ev = ev.astype(np.int64)
    bad = np.flatnonzero((ev[:, 0] < 0) | (ev[:, 0] >= batch) | (ev[:, 1] < 0) | (ev[:, 1] > ev[:, 2]) | (ev[:, 2] >= n_frames))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"beamform: event {i} = (sample {ev[i, 0]}, frames {ev[i, 1]} .. {ev[i, 2]}) does not fit {batch} sample(s) of "
                         f"{n_frames} frames with first <= last")
    frames = ev[:, 2] - ev[:, 1] + 1
    if int(frames.sum()) > 2 ** 31 - 1:
        raise ValueError("beamform: more than 2^31 - 1 output frames")
    table = np.empty((len(ev), 4), np.int32)
    table[:, :3] = ev
    table[:, 3] = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return table


def phase_vocoder_launch(table: np.ndarray, n_bins: int, chan2: int, max_out_frames: int, device: torch.device,
                         table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload a VOC_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_phase_vocoder over
    it on the current stream: one launch.  Returns the device table (tied to the stream when it was allocated here)."""
    return _launch_records(table, device, table_dev, "iris_phase_vocoder", lambda ptr, n, stream: N.lib().iris_phase_vocoder(
        ptr, n, int(n_bins), int(chan2), int(max_out_frames), stream))


def phase_vocoder_batch(specs, rates, out=None):
    """Time-stretch a ragged batch of complex spectrograms in ONE launch (iris_phase_vocoder): specs is a list of
    [F, T_i, 2C] float32 tensors on one ROCm device (re block, im block last, equal F and 2C), rates as many positive
    numbers.  Returns a list of [F, ceil(T_i / rate_i), 2C] tensors: the reference's `phase_vocoder` with the time grid in
    double and the running phase kept in [-pi, pi] (|out - fp64| <= mag (1e-5 + 16 u pi (t + 1)), where the reference's own
    fp32 form is 1e-2 of the peak off); a rate of 1 copies its source.  out: optional list of preallocated contiguous
    float32 buffers on the same device, out[i] holding at least F * n_i * 2C floats; the result i is a view of the start of
    out[i] and the floats beyond it are left alone.  CPU tensors raise: there is no CPU fallback."""
    specs, rates = list(specs), [float(r) for r in rates]
    if len(specs) != len(rates):
        raise ValueError(f"phase_vocoder_batch: {len(specs)} spectrograms but {len(rates)} rates")
    if out is not None and len(out) != len(specs):
        raise ValueError(f"phase_vocoder_batch: {len(specs)} spectrograms but {len(out)} output buffers")
    if not specs:
        return []
    specs = [_require_device_f32(s, f"specs[{i}]") for i, s in enumerate(specs)]
    dev = specs[0].device
    if specs[0].dim() != 3:
        raise ValueError("phase_vocoder_batch: every spectrogram must be [freq, time, chan * 2]")
    n_bins, chan2 = int(specs[0].shape[0]), int(specs[0].shape[2])
    if n_bins < 2 or chan2 < 2 or chan2 % 2:
        raise ValueError(f"phase_vocoder_batch: [freq = {n_bins}, time, chan2 = {chan2}] needs freq >= 2 and an even chan2")
    table = np.zeros(len(specs), VOC_SRC)
    results = []
    for i, (s, r) in enumerate(zip(specs, rates)):
        if s.dim() != 3 or int(s.shape[0]) != n_bins or int(s.shape[2]) != chan2 or s.device != dev or int(s.shape[1]) < 1:
            raise ValueError(f"phase_vocoder_batch: specs[{i}] has shape {tuple(s.shape)} on {s.device}; expected "
                             f"[{n_bins}, T >= 1, {chan2}] on {dev}")
        n = stretched_frames(int(s.shape[1]), r)
        if out is None:
            o = torch.empty((n_bins, n, chan2), dtype=torch.float32, device=dev)
        else:
            buf = out[i]
            if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.device == dev and buf.dtype == torch.float32
                    and buf.is_contiguous()):
                raise ValueError(f"phase_vocoder_batch: out[{i}] must be a contiguous float32 tensor on {dev}")
            if buf.numel() < n_bins * n * chan2:
                raise ValueError(f"phase_vocoder_batch: out[{i}] holds {buf.numel()} floats, fewer than the {n_bins} x {n} x "
                                 f"{chan2} of {int(s.shape[1])} frames at rate {r}")
            if buf.data_ptr() == s.data_ptr():
                raise ValueError(f"phase_vocoder_batch: out[{i}] is specs[{i}] itself (the stretch is not in place)")
            o = buf.view(-1)[:n_bins * n * chan2].view(n_bins, n, chan2)
        table[i] = (s.data_ptr(), o.data_ptr(), int(s.shape[1]), n, r)
        results.append(o)
    phase_vocoder_launch(table, n_bins, chan2, int(table["n_out"].max()), dev)
    for s in specs:   # (a contiguous copy made above must outlive the kernel)
        s.record_stream(torch.cuda.current_stream(dev))
    return results


# mirrors iris_speed_src (include/iris_frontend.h)
SPEED_SRC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len_in", "<i4"), ("len_out", "<i4"), ("rate", "<f8")])
assert SPEED_SRC.itemsize == 32


def speed_len(length: int, rate: float) -> int:
    """Samples of a waveform of `length` samples played `rate` times faster: ceil(length / rate) in double, the length of
    numpy.arange(0, length, rate) (the law of `stretched_frames`)."""
    return _scaled_len(length, rate, "speed")


def speed_perturb_launch(table: np.ndarray, channels: int, max_out_len: int, device: torch.device,
                         table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload a SPEED_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_speed_perturb over
    it on the current stream: one launch.  Returns the device table (tied to the stream when it was allocated here)."""
    return _launch_records(table, device, table_dev, "iris_speed_perturb", lambda ptr, n, stream: N.lib().iris_speed_perturb(
        ptr, n, int(channels), int(max_out_len), stream))


def speed_perturb_batch(waves, rates):
    """Speed-perturb a ragged batch of waveforms in ONE launch (iris_speed_perturb): waves is a list of [C, L_i] float32
    tensors on one ROCm device (equal C), rates as many positive numbers (rate > 1 = faster and shorter: tempo and pitch move
    together).  Returns a list of new [C, ceil(L_i / rate_i)] tensors: the Hann-windowed sinc of torchaudio's `resample`
    (width 6, rolloff 0.99) evaluated at the real-valued positions m * rate_i, |out - fp64| <= 8 u cut sum |x| over the
    support; a rate of 1 copies its source.  CPU tensors raise: there is no CPU fallback."""
    waves, rates = list(waves), [float(r) for r in rates]
    if len(waves) != len(rates):
        raise ValueError(f"speed_perturb_batch: {len(waves)} waveforms but {len(rates)} rates")
    if not waves:
        return []
    waves = [_require_device_f32(w, f"waves[{i}]") for i, w in enumerate(waves)]
    dev = waves[0].device
    if waves[0].dim() != 2:
        raise ValueError("speed_perturb_batch: every waveform must be [chan, samples]")
    chan = int(waves[0].shape[0])
    table = np.zeros(len(waves), SPEED_SRC)
    results = []
    for i, (w, r) in enumerate(zip(waves, rates)):
        if w.dim() != 2 or int(w.shape[0]) != chan or w.device != dev or int(w.shape[1]) < 1 or chan < 1:
            raise ValueError(f"speed_perturb_batch: waves[{i}] has shape {tuple(w.shape)} on {w.device}; expected "
                             f"[{chan} >= 1, L >= 1] on {dev}")
        n = speed_len(int(w.shape[1]), r)
        if n > 2 ** 31 - 1:
            raise ValueError(f"speed_perturb_batch: waves[{i}] at rate {r} would have {n} samples (> 2^31 - 1)")
        o = torch.empty((chan, n), dtype=torch.float32, device=dev)
        table[i] = (w.data_ptr(), o.data_ptr(), int(w.shape[1]), n, r)
        results.append(o)
    speed_perturb_launch(table, chan, int(table["len_out"].max()), dev)
    for w in waves:   # (a contiguous copy made above must outlive the kernel)
        w.record_stream(torch.cuda.current_stream(dev))
    return results


# mirrors iris_gate_rec (include/iris_frontend.h)
GATE_REC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("mask", "<u8"), ("energy", "<u8"), ("len", "<i4"), ("reserved", "<i4")])
assert GATE_REC.itemsize == 40
GATE_MAX_FRAMES = 131072   # IRIS_GATE_MAX_FRAMES: frames per record (35 minutes at hop 256 and 16 kHz)
_LAUNCH_RECORDS = 65535    # records per launch (a grid dimension)


def gate_ratio(range_db: float) -> float:
    """10^(-range_db / 10) in double, for range_db in (0, 200]: the share of a clip's peak frame energy below which a frame is
    silent."""
    range_db = float(range_db)
    if not 0.0 < range_db <= 200.0:
        raise ValueError(f"activity gate: range_db = {range_db} is outside (0, 200]")
    return 10.0 ** (-range_db / 10.0)


def check_gate_settings(hop, range_db, floor, min_gap, min_event, hang) -> None:
    """ValueError for gate settings outside their ranges (host only: nothing touches the device)."""
    gate_ratio(range_db)
    for name, value, low in (("hop", hop, 1), ("min_gap", min_gap, 0), ("min_event", min_event, 1), ("hang", hang, 0)):
        if int(value) != value or not low <= int(value) <= 2 ** 31 - 1:
            raise ValueError(f"activity gate: {name} = {value!r} must be an integer >= {low}")
    if not float(floor) >= 0.0:
        raise ValueError(f"activity gate: floor = {floor!r} must be >= 0")


def activity_gate_launch(table: np.ndarray, channels: int, hop: int, min_gap: int, min_event: int, hang: int, ratio: float,
                         floor: float, max_len: int, device: torch.device, table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload a GATE_REC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_activity_gate over
    it on the current stream: three launches.  Returns the device table (tied to the stream when it was allocated here)."""
    return _launch_records(table, device, table_dev, "iris_activity_gate", lambda ptr, n, stream: N.lib().iris_activity_gate(
        ptr, n, int(channels), int(hop), int(min_gap), int(min_event), int(hang), float(ratio), float(floor), int(max_len), stream))


def activity_gate_batch(waves, hop: int = 256, range_db: float = 40.0, floor: float = 0.0, min_gap: int = 12, min_event: int = 6,
                        hang: int = 1, out=None):
    """Gate a ragged batch of waveforms (iris_activity_gate, three launches per 65535 records): waves is a list of [C, L_i]
    float32 tensors on one ROCm device (equal C).  Per waveform, with T = 1 + L // hop frames and frame t owning the samples s
    with min((s + hop // 2) // hop, T - 1) == t: the frame energies E (sum of squares over channels and samples, in double);
    m0 = E >= max(max(E) * 10^(-range_db / 10), floor) and E > 0; runs of zeros of at most `min_gap` frames between ones are
    closed, runs of ones shorter than `min_event` dropped, and what is left widened by `hang` frames a side.  Returns (gated,
    masks, energies): lists of [C, L_i] float32 (the samples of active frames bit for bit, +0.0 elsewhere), uint8 [T_i] and
    float64 [T_i] tensors (views of one buffer per kind).  out: a list of contiguous [C, L_i] float32 tensors on the device
    that receive the gated waveforms; out=waves gates in place (every energy is read before anything is written).  The
    defaults (40 dB under the clip's loudest frame, 12 / 6 / 1 frames of 16 ms) are choices, not measurements.  At most 131072
    frames per waveform.  CPU tensors raise: there is no CPU fallback."""
    waves = list(waves)
    check_gate_settings(hop, range_db, floor, min_gap, min_event, hang)
    ratio, hop = gate_ratio(range_db), int(hop)
    if out is not None and len(out) != len(waves):
        raise ValueError(f"activity_gate_batch: {len(waves)} waveforms but {len(out)} outputs")
    if not waves:
        return [], [], []
    if out is not None:   # (an output must be the caller's own memory: no contiguous copy is made of it)
        for i, (o, w) in enumerate(zip(out, waves)):
            if not (isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float32 and o.is_contiguous()
                    and isinstance(w, torch.Tensor) and o.shape == w.shape and o.device == w.device):
                raise ValueError(f"activity_gate_batch: out[{i}] must be a contiguous float32 tensor of waves[{i}]'s shape on its device")
    waves = [_require_device_f32(w, f"waves[{i}]") for i, w in enumerate(waves)]
    dev = waves[0].device
    if waves[0].dim() != 2:
        raise ValueError("activity_gate_batch: every waveform must be [chan, samples]")
    chan = int(waves[0].shape[0])
    for i, w in enumerate(waves):
        if w.dim() != 2 or int(w.shape[0]) != chan or w.device != dev or int(w.shape[1]) < 1 or chan < 1:
            raise ValueError(f"activity_gate_batch: waves[{i}] has shape {tuple(w.shape)} on {w.device}; expected "
                             f"[{chan} >= 1, L >= 1] on {dev}")
        if int(w.shape[1]) > 2 ** 31 - 1 or 1 + int(w.shape[1]) // hop > GATE_MAX_FRAMES:
            raise ValueError(f"activity_gate_batch: waves[{i}] has {int(w.shape[1])} samples: {1 + int(w.shape[1]) // hop} frames at "
                             f"hop {hop} (> {GATE_MAX_FRAMES})")
    lens = np.array([int(w.shape[1]) for w in waves], np.int64)
    frames = 1 + lens // hop
    masks = list(torch.empty(int(frames.sum()), dtype=torch.uint8, device=dev).split(frames.tolist()))
    energies = list(torch.empty(int(frames.sum()), dtype=torch.float64, device=dev).split(frames.tolist()))
    if out is None:
        flat = torch.empty(int(lens.sum()) * chan, dtype=torch.float32, device=dev)
        gated = [g.view(chan, -1) for g in flat.split((lens * chan).tolist())]
    else:
        gated = list(out)
    table = np.zeros(len(waves), GATE_REC)
    table["src"], table["dst"] = [w.data_ptr() for w in waves], [g.data_ptr() for g in gated]
    table["mask"], table["energy"] = [m.data_ptr() for m in masks], [e.data_ptr() for e in energies]
    table["len"] = lens
    for first in range(0, len(waves), _LAUNCH_RECORDS):
        part = table[first:first + _LAUNCH_RECORDS]
        activity_gate_launch(part, chan, hop, min_gap, min_event, hang, ratio, floor, int(part["len"].max()), dev)
    for w in waves:   # (a contiguous copy made above must outlive the kernels)
        w.record_stream(torch.cuda.current_stream(dev))
    return gated, masks, energies


# mirrors iris_fir_src (include/iris_frontend.h)
FIR_SRC =np.dtype([("src", "<u8"), ("dst", "<u8"), ("taps", "<u8"), ("len", "<i4"), ("n_taps", "<i4")])
assert FIR_SRC.itemsize == 32
FIR_MAX_TAPS = 4096   # the longest impulse response `fir_batch` and the mixers take (a quarter of a second at 16 kHz)


def fir_launch(table: np.ndarray, channels: int, max_len: int, max_taps: int, device: torch.device,
               table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload a FIR_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_fir_batch over it
    on the current stream: one launch.  Returns the device table (tied to the stream when it was allocated here)."""
    return _launch_records(table, device, table_dev, "iris_fir_batch", lambda ptr, n, stream: N.lib().iris_fir_batch(
        ptr, n, int(channels), int(max_len), int(max_taps), stream))


def fir_batch(waves, taps):
    """Convolve a ragged batch of waveforms with their own impulse responses in ONE launch (iris_fir_batch): waves is a list of
    [C, L_i] float32 tensors on one ROCm device (equal C), taps as many [C, K_i] float32 tensors on it, 1 <= K_i <= 4096.
    Returns a list of new [C, L_i] tensors, y[c, m] = sum_k taps[c, k] x[c, m - k]: the causal convolution cut at the input
    length (the direct sound at tap 0, the ringing past the end dropped), |out - fp64| <= (K_i + 2) u sum_k |taps| |x|; taps
    [[1.0]] copy their source.  A mismatch, an empty tap vector, K_i > 4096 or a CPU tensor is a ValueError: there is no CPU
    fallback."""
    waves, taps = list(waves), list(taps)
    if len(waves) != len(taps):
        raise ValueError(f"fir_batch: {len(waves)} waveforms but {len(taps)} tap arrays")
    if not waves:
        return []
    for name, group in (("waves", waves), ("taps", taps)):
        for i, t in enumerate(group):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
                what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"fir_batch: {name}[{i}] must be a 2-D float32 tensor on a ROCm device (there is no CPU "
                                 f"fallback), got {what}")
    dev, chan = waves[0].device, int(waves[0].shape[0])
    table = np.zeros(len(waves), FIR_SRC)
    results, keep = [], []
    for i, (w, h) in enumerate(zip(waves, taps)):
        if int(w.shape[0]) != chan or w.device != dev or int(w.shape[1]) < 1 or chan < 1:
            raise ValueError(f"fir_batch: waves[{i}] has shape {tuple(w.shape)} on {w.device}; expected [{chan} >= 1, L >= 1] "
                             f"on {dev}")
        if int(h.shape[0]) != chan or h.device != dev:
            raise ValueError(f"fir_batch: taps[{i}] has shape {tuple(h.shape)} on {h.device} for a waveform of {chan} "
                             f"channel(s) on {dev}: one row of taps per channel")
        if int(h.shape[1]) < 1:
            raise ValueError(f"fir_batch: taps[{i}] is empty (an impulse response has at least its direct tap)")
        if int(h.shape[1]) > FIR_MAX_TAPS:
            raise ValueError(f"fir_batch: taps[{i}] has {int(h.shape[1])} taps per channel (> {FIR_MAX_TAPS})")
        if int(w.shape[1]) > 2 ** 31 - 1:
            raise ValueError(f"fir_batch: waves[{i}] has {int(w.shape[1])} samples (> 2^31 - 1)")
        w, h = w.contiguous(), h.contiguous()
        o = torch.empty_like(w)
        table[i] = (w.data_ptr(), o.data_ptr(), h.data_ptr(), int(w.shape[1]), int(h.shape[1]))
        results.append(o)
        keep += [w, h]
    fir_launch(table, chan, int(table["len"].max()), int(table["n_taps"].max()), dev)
    for t in keep:   # (a contiguous copy made above must outlive the kernel)
        t.record_stream(torch.cuda.current_stream(dev))
    return results


def fir_pitch_launch(table: np.ndarray, channels: int, max_len: int, max_taps: int, tap_pitch: int, device: torch.device,
                     table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`fir_launch` with the rows of every record's taps `tap_pitch` floats apart (iris_fir_batch_pitch): the layout
    `shoebox_rir_launch` writes.  One launch."""
    return _launch_records(table, device, table_dev, "iris_fir_batch_pitch", lambda ptr, n, stream: N.lib().iris_fir_batch_pitch(
        ptr, n, int(channels), int(max_len), int(max_taps), int(tap_pitch), stream))


# mirrors iris_fft_fir_src (include/iris_frontend.h)
FFT_FIR_SRC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("taps", "<u8"), ("len", "<i4"), ("n_taps", "<i4"), ("ws_off", "<i8")])
assert FFT_FIR_SRC.itemsize == 40
FFT_FIR_MAX_TAPS = 32768   # the longest impulse response `fft_fir_batch` and a long-path mixer take (2 s at 16 kHz)
FFT_FIR_BLOCK = 1024       # new samples per frame of the partitioned convolution; its transform has 2048 points


def fft_fir_workspace(channels: int, length: int, n_taps: int) -> int:
    """Bytes of workspace one record of `fft_fir_launch` needs (iris_fft_fir_workspace): channels * (ceil(length / 1024) +
    ceil(n_taps / 1024)) spectra of 8256 bytes, a multiple of 16; 0 for a malformed record (a count <= 0, n_taps > 32768)."""
    return int(N.lib().iris_fft_fir_workspace(int(channels), int(length), int(n_taps)))


def fft_fir_groups(table: np.ndarray, channels: int, workspace_budget: int):
    """Split the records of an FFT_FIR_SRC table (len and n_taps filled) into consecutive groups whose workspace stays within
    `workspace_budget` bytes - a single record may exceed it and is then a group of its own - and fill `ws_off` per group.
    Returns (list of (first, last + 1) index pairs, the bytes of the largest group)."""
    need = [fft_fir_workspace(channels, int(r["len"]), int(r["n_taps"])) for r in table]
    groups, first, used, largest = [], 0, 0, 0
    for i, n in enumerate(need):
        if i > first and used + n > workspace_budget:
            groups.append((first, i))
            first, used = i, 0
        table["ws_off"][i] = used
        used += n
        largest = max(largest, used)
    if len(need):
        groups.append((first, len(need)))
    return groups, largest


def fft_fir_launch(table: np.ndarray, channels: int, max_len: int, max_taps: int, tap_pitch: int, workspace: torch.Tensor,
                   device: torch.device, table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload an FFT_FIR_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run
    iris_fft_fir_batch over it on the current stream: two launches.  `workspace` is a uint8 device tensor that holds every
    record's slice (`ws_off`); `tap_pitch` = 0 for dense tap rows.  Returns the device table (tied to the stream when it was
    allocated here)."""
    if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("fft_fir_launch: workspace must be a contiguous uint8 tensor on a ROCm device")
    return _launch_records(table, device, table_dev, "iris_fft_fir_batch", lambda ptr, n, stream: N.lib().iris_fft_fir_batch(
        ptr, n, int(channels), int(max_len), int(max_taps), int(tap_pitch), workspace.data_ptr(), int(workspace.numel()), stream))


def fft_fir_batch(waves, taps, workspace_budget: int = 256 << 20):
    """`fir_batch` for long impulse responses (iris_fft_fir_batch: a partitioned overlap-save convolution on the FFT core):
    waves is a list of [C, L_i] float32 tensors on one ROCm device (equal C), taps as many [C, K_i] float32 tensors on it,
    1 <= K_i <= 32768.  Returns a list of new [C, L_i] tensors, the causal convolution cut at the input length, norm-wise
    accurate per block of 1024 outputs: |out - fp64| <= 8 u sum_p ||frame_{j-p}|| ||partition_p||, not tap
    by tap as `fir_batch`; taps [[1.0]] give a copy within that rule, not bit for bit.  The records are run in consecutive
    groups whose spectra fit `workspace_budget` bytes (a single larger record is a group of its own), one launch pair per
    group: the results do not depend on the grouping.  A mismatch, an empty tap vector, K_i > 32768 or a CPU tensor is a
    ValueError: there is no CPU fallback."""
    waves, taps = list(waves), list(taps)
    if len(waves) != len(taps):
        raise ValueError(f"fft_fir_batch: {len(waves)} waveforms but {len(taps)} tap arrays")
    if not waves:
        return []
    for name, group in (("waves", waves), ("taps", taps)):
        for i, t in enumerate(group):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
                what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"fft_fir_batch: {name}[{i}] must be a 2-D float32 tensor on a ROCm device (there is no CPU "
                                 f"fallback), got {what}")
    dev, chan = waves[0].device, int(waves[0].shape[0])
    table = np.zeros(len(waves), FFT_FIR_SRC)
    results, keep = [], []
    for i, (w, h) in enumerate(zip(waves, taps)):
        if int(w.shape[0]) != chan or w.device != dev or int(w.shape[1]) < 1 or chan < 1:
            raise ValueError(f"fft_fir_batch: waves[{i}] has shape {tuple(w.shape)} on {w.device}; expected [{chan} >= 1, "
                             f"L >= 1] on {dev}")
        if int(h.shape[0]) != chan or h.device != dev:
            raise ValueError(f"fft_fir_batch: taps[{i}] has shape {tuple(h.shape)} on {h.device} for a waveform of {chan} "
                             f"channel(s) on {dev}: one row of taps per channel")
        if int(h.shape[1]) < 1:
            raise ValueError(f"fft_fir_batch: taps[{i}] is empty (an impulse response has at least its direct tap)")
        if int(h.shape[1]) > FFT_FIR_MAX_TAPS:
            raise ValueError(f"fft_fir_batch: taps[{i}] has {int(h.shape[1])} taps per channel (> {FFT_FIR_MAX_TAPS})")
        if int(w.shape[1]) > 2 ** 31 - 1 - 2 * FFT_FIR_BLOCK:
            raise ValueError(f"fft_fir_batch: waves[{i}] has {int(w.shape[1])} samples (> 2^31 - 1 - 2048)")
        w, h = w.contiguous(), h.contiguous()
        o = torch.empty_like(w)
        table[i] = (w.data_ptr(), o.data_ptr(), h.data_ptr(), int(w.shape[1]), int(h.shape[1]), 0)
        results.append(o)
        keep += [w, h]
    groups, largest = fft_fir_groups(table, chan, int(workspace_budget))
    workspace = torch.empty(largest, dtype=torch.uint8, device=dev)
    for a, b in groups:
        part = table[a:b]
        fft_fir_launch(part, chan, int(part["len"].max()), int(part["n_taps"].max()), 0, workspace, dev)
    for t in keep + [workspace]:   # (a contiguous copy made above, and the spectra, must outlive the kernels)
        t.record_stream(torch.cuda.current_stream(dev))
    return results


# mirrors iris_ism_src (include/iris_frontend.h)
ISM_MAX_CHAN = 8      # microphones per record (IRIS_ISM_MAX_CHAN)
ISM_SRC = np.dtype([("dst", "<u8"), ("room", "<f8", (3,)), ("src", "<f8", (3,)), ("beta", "<f8"), ("n_taps", "<i4"),
                    ("reserved", "<i4"), ("mic", "<f8", (ISM_MAX_CHAN, 3))])
assert ISM_SRC.itemsize == 72 + 24 * ISM_MAX_CHAN
ISM_HALF_WIDTH = 16   # W: half width of the fractional-delay filter; the nearest microphone's direct sound peaks at tap W
ISM_SOUND = 343.0     # speed of sound, m / s


def shoebox_rir_launch(table: np.ndarray, chan: int, max_taps: int, device: torch.device,
                       table_dev: Optional[torch.Tensor] = None, sample_rate: float = 16000.0, normalize: bool = True) -> torch.Tensor:
    """Upload an ISM_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_ism_rir over it on
    the current stream: one launch.  The C entry point checks the host copy of the records before it launches (a ValueError
    names the record).  Returns the device table (tied to the stream when it was allocated here)."""
    table = np.ascontiguousarray(table)
    return _launch_records(table, device, table_dev, "iris_ism_rir", lambda ptr, n, stream: N.lib().iris_ism_rir(
        table.ctypes.data, ptr, n, int(chan), int(max_taps), float(sample_rate), int(bool(normalize)), stream))


def shoebox_records(rooms, sources, mics, betas, n_taps, max_taps: int = FIR_MAX_TAPS, sample_rate: float = 16000.0) -> np.ndarray:
    """The ISM_SRC table (dst left 0) of rooms [n, 3], sources [n, 3], mics [n, C, 3], betas [n], n_taps [n], after the checks
    iris_ism_rir makes in C, here as ValueErrors: shapes, 1 <= C <= 8, n_taps in 1 .. min(max_taps, 4096), positive finite room
    sizes, the source and every microphone inside the room, the source off its nearest microphone, beta in [0, 1), a lattice of
    at most 2^31 - 1 images."""
    rooms, sources = np.asarray(rooms, np.float64), np.asarray(sources, np.float64)
    mics, betas, n_taps = np.asarray(mics, np.float64), np.asarray(betas, np.float64).reshape(-1), np.asarray(n_taps).reshape(-1)
    n = rooms.shape[0] if rooms.ndim == 2 else -1
    if rooms.shape != (n, 3) or sources.shape != (n, 3) or mics.ndim != 3 or mics.shape[0] != n or mics.shape[2] != 3 \
            or betas.shape != (n,) or n_taps.shape != (n,):
        raise ValueError(f"shoebox_rir_batch: expected rooms [n, 3], sources [n, 3], mics [n, C, 3], betas [n], n_taps [n]; got "
                         f"{rooms.shape}, {sources.shape}, {mics.shape}, {betas.shape}, {n_taps.shape}")
    chan = int(mics.shape[1])
    if not 1 <= chan <= ISM_MAX_CHAN:
        raise ValueError(f"shoebox_rir_batch: {chan} microphones per voice; 1 .. {ISM_MAX_CHAN} are supported")
    if not 1 <= int(max_taps) <= FIR_MAX_TAPS:
        raise ValueError(f"shoebox_rir_batch: max_taps = {max_taps} is outside 1 .. {FIR_MAX_TAPS}")
    if not (np.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"shoebox_rir_batch: sample_rate = {sample_rate} must be positive and finite")
    if n and not np.all(n_taps == np.floor(n_taps)):
        raise ValueError("shoebox_rir_batch: n_taps must be whole numbers")
    for i in range(n):
        k = int(n_taps[i])
        if not 1 <= k <= int(max_taps):
            raise ValueError(f"shoebox_rir_batch: n_taps[{i}] = {k} is outside 1 .. {int(max_taps)}")
        if not (np.all(np.isfinite(rooms[i])) and np.all(rooms[i] > 0)):
            raise ValueError(f"shoebox_rir_batch: rooms[{i}] = {rooms[i]} must be positive and finite")
        if not np.all((sources[i] >= 0) & (sources[i] <= rooms[i])):
            raise ValueError(f"shoebox_rir_batch: sources[{i}] = {sources[i]} is outside the room {rooms[i]}")
        if not np.all((mics[i] >= 0) & (mics[i] <= rooms[i][None, :])):
            raise ValueError(f"shoebox_rir_batch: a microphone of mics[{i}] is outside the room {rooms[i]}")
        if not 0 <= betas[i] < 1:
            raise ValueError(f"shoebox_rir_batch: betas[{i}] = {betas[i]} is outside [0, 1)")
        d_min = float(np.sqrt(np.sum((mics[i] - sources[i][None, :]) ** 2, axis=1)).min())
        if not d_min > 0:
            raise ValueError(f"shoebox_rir_batch: sources[{i}] sits on its nearest microphone")
        reach = ISM_SOUND * (d_min * sample_rate / ISM_SOUND + k) / sample_rate
        images = 8.0 * np.prod(2.0 * (np.floor(reach / (2.0 * rooms[i])) + 1.0) + 1.0)
        if not images <= 2 ** 31 - 1:
            raise ValueError(f"shoebox_rir_batch: voice {i} has a lattice of {images:.0f} images (> 2^31 - 1)")
    table = np.zeros(n, ISM_SRC)
    table["room"], table["src"], table["beta"], table["n_taps"] = rooms, sources, betas, n_taps.astype(np.int32)
    table["mic"][:, :chan, :] = mics
    return table


def shoebox_rir_batch(rooms, sources, mics, betas, n_taps, normalize: bool = True, out=None, sample_rate: float = 16000.0,
                      device=None):
    """Shoebox room impulse responses of a ragged batch of voices in ONE launch (iris_ism_rir; Allen & Berkley 1979): rooms
    [n, 3] m, sources [n, 3], mics [n, C <= 8, 3], betas [n] in [0, 1) and n_taps [n] in 1 .. 4096 are arrays.  Returns a list of
    [C, K_i] float32 device tensors (views of one new buffer with rows max K_i apart), or views out[i][:, :K_i] of the given
    contiguous float32 [C, max_taps <= 4096] device buffers, whose floats beyond K_i are left alone.  The nearest microphone's
    direct sound is a unit tap at k = 16 and the delay between the channels is kept; normalize: every channel of a voice
    times the same 1 / sqrt(mean_c sum_k h^2).  |h - fp64| <= 3.6 u A_k + n_k 2^-33 (include/iris_frontend.h), bitwise
    reproducible.  device: where to compute when `out` is not given (default cuda:0).  CPU `out` tensors raise: there is no
    CPU fallback."""
    n_taps = np.asarray(n_taps).reshape(-1)
    if out is not None:
        out = list(out)
        if len(out) != n_taps.shape[0]:
            raise ValueError(f"shoebox_rir_batch: {n_taps.shape[0]} voices but {len(out)} output buffers")
        chan = int(np.asarray(mics).shape[1]) if np.asarray(mics).ndim == 3 else -1
        for i, buf in enumerate(out):
            if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()
                    and buf.dim() == 2 and int(buf.shape[0]) == chan and buf.shape == out[0].shape and buf.device == out[0].device):
                raise ValueError(f"shoebox_rir_batch: out[{i}] must be a contiguous float32 [{chan}, max_taps] tensor on one ROCm "
                                 f"device (there is no CPU fallback)")
        max_taps = int(out[0].shape[1]) if out else FIR_MAX_TAPS
        dev = out[0].device if out else None
    else:
        max_taps = int(n_taps.max()) if n_taps.size else 1
        dev = torch.device("cuda", 0) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("shoebox_rir_batch: the device must be a ROCm device (there is no CPU fallback)")
    table = shoebox_records(rooms, sources, mics, betas, n_taps, max_taps, sample_rate)
    if not len(table):
        return []
    chan = int(np.asarray(mics).shape[1])
    if out is None:
        whole = torch.zeros((len(table), chan, max_taps), dtype=torch.float32, device=dev)
        out = list(whole.unbind(0))
    table["dst"] = [b.data_ptr() for b in out]
    shoebox_rir_launch(table, chan, max_taps, dev, None, sample_rate, normalize)
    for b in out:
        b.record_stream(torch.cuda.current_stream(dev))
    return [b[:, :int(k)] for b, k in zip(out, table["n_taps"])]


# mirrors iris_flyby_src (include/iris_frontend.h)
FLYBY_MAX_CHAN = ISM_MAX_CHAN   # microphones per record (IRIS_FLYBY_MAX_CHAN)
FLYBY_SRC = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<i4"), ("n_paths", "<i4"), ("p0", "<f8", (3,)), ("v", "<f8", (3,)),
                      ("z_s", "<f8"), ("beta", "<f8"), ("r_ref", "<f8"), ("mic", "<f8", (FLYBY_MAX_CHAN, 3))])
assert FLYBY_SRC.itemsize == 96 + 24 * FLYBY_MAX_CHAN
FLYBY_FS = 16000.0              # the sample rate iris_flyby is written for


def flyby_r_ref(p0, v, z_s: float, mics, length: int) -> float:
    """The reference distance of a flight: the smallest distance between the source (0, 0, z_s) and any microphone
    p0 + v t + mics[c] over t in [0, (length - 1) / 16000], in closed form - per microphone the squared distance is a
    quadratic in t, whose vertex is clamped to the interval.  Delays and gains of `iris_flyby` are measured against it."""
    p0, v, mics = np.asarray(p0, np.float64), np.asarray(v, np.float64), np.asarray(mics, np.float64).reshape(-1, 3)
    t_end = (int(length) - 1) / FLYBY_FS
    vv = float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    best = np.inf
    for m in mics:
        q = p0 + m
        q[2] -= float(z_s)
        t = 0.0 if vv == 0.0 else min(max(-float(q[0] * v[0] + q[1] * v[1] + q[2] * v[2]) / vv, 0.0), t_end)
        dx, dy, dz = q[0] + v[0] * t, q[1] + v[1] * t, q[2] + v[2] * t
        best = min(best, float(np.sqrt(dx * dx + dy * dy + dz * dz)))
    return best


def flyby_records(geometry, lengths, channels: int) -> np.ndarray:
    """The FLYBY_SRC table (src / dst left 0) of one flight per voice: geometry[i] is a dict of p0 [3], v [3] (metres, metres per
    second), z_s, beta and mics [channels, 3] (offsets from the array centre) - what `transforms.draw_flyby` returns - or None
    for the identity record (n_paths 0: a copy); lengths[i] the voice's samples per channel.  beta == 0 packs one path, exactly;
    r_ref is `flyby_r_ref` of the flight.  ValueError: a length below 1, 1 <= channels <= 8 violated, a shape that does not fit,
    a value that is not finite, z_s < 0, beta outside [0, 1), |v| >= 343 m/s, a flight that touches the source (r_ref = 0)."""
    geometry, lengths, channels = list(geometry), [int(n) for n in lengths], int(channels)
    if len(geometry) != len(lengths):
        raise ValueError(f"flyby_records: {len(geometry)} geometries but {len(lengths)} lengths")
    if not 1 <= channels <= FLYBY_MAX_CHAN:
        raise ValueError(f"flyby_records: {channels} microphones per voice; 1 .. {FLYBY_MAX_CHAN} are supported")
    table = np.zeros(len(geometry), FLYBY_SRC)
    for i, (g, n) in enumerate(zip(geometry, lengths)):
        if not 1 <= n <= 2 ** 31 - 1:
            raise ValueError(f"flyby_records: lengths[{i}] = {n} is outside 1 .. 2^31 - 1")
        table["len"][i] = n
        if g is None:
            continue
        p0, v = np.asarray(g["p0"], np.float64), np.asarray(g["v"], np.float64)
        mics, z_s, beta = np.asarray(g["mics"], np.float64), float(g["z_s"]), float(g["beta"])
        if p0.shape != (3,) or v.shape != (3,) or mics.shape != (channels, 3):
            raise ValueError(f"flyby_records: geometry[{i}] has p0 {p0.shape}, v {v.shape}, mics {mics.shape}; expected [3], [3], "
                             f"[{channels}, 3]")
        if not (np.all(np.isfinite(p0)) and np.all(np.isfinite(v)) and np.all(np.isfinite(mics)) and np.isfinite(z_s)
                and np.isfinite(beta)):
            raise ValueError(f"flyby_records: geometry[{i}] holds a value that is not finite")
        if z_s < 0 or not 0 <= beta < 1:
            raise ValueError(f"flyby_records: geometry[{i}] has z_s = {z_s} (must be >= 0) and beta = {beta} (must be in [0, 1))")
        if not float(np.sqrt(np.sum(v * v))) < ISM_SOUND:
            raise ValueError(f"flyby_records: geometry[{i}] moves at {float(np.sqrt(np.sum(v * v)))} m/s, not below the sound speed")
        r_ref = flyby_r_ref(p0, v, z_s, mics, n)
        if not r_ref > 0:
            raise ValueError(f"flyby_records: the flight of geometry[{i}] touches the source (reference distance {r_ref})")
        table["n_paths"][i] = 1 if beta == 0.0 else 2
        table["p0"][i], table["v"][i], table["z_s"][i], table["beta"][i], table["r_ref"][i] = p0, v, z_s, beta, r_ref
        table["mic"][i, :channels] = mics
    return table


def flyby_launch(table: np.ndarray, chan: int, max_len: int, device: torch.device,
                 table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload a FLYBY_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_flyby over it on
    the current stream: one launch.  Returns the device table (tied to the stream when it was allocated here)."""
    return _launch_records(table, device, table_dev, "iris_flyby", lambda ptr, n, stream: N.lib().iris_flyby(
        ptr, n, int(chan), int(max_len), stream))


def flyby_batch(waves, geometry):
    """Fly a moving microphone array past a ragged batch of voices in ONE launch (iris_flyby): waves is a list of [C, L_i]
    float32 tensors on one ROCm device (equal C <= 8, sampled at 16 kHz), geometry as many flights (`flyby_records`; None: a
    copy).  Returns a list of new [C, L_i] tensors: channel c is row c of the source under the time-varying delay and
    spherical-spreading gain of microphone c, plus the ground reflection at beta > 0 - the Doppler shift, the moving
    inter-channel delay and the level swell of a pass; what arrives later than the buffer is cut.  |out - fp64| <= 4 u cut
    sum_p |g_p| sum |x| over the support.  CPU tensors raise: there is no CPU fallback."""
    waves, geometry = list(waves), list(geometry)
    if len(waves) != len(geometry):
        raise ValueError(f"flyby_batch: {len(waves)} waveforms but {len(geometry)} geometries")
    if not waves:
        return []
    waves = [_require_device_f32(w, f"waves[{i}]") for i, w in enumerate(waves)]
    dev = waves[0].device
    if waves[0].dim() != 2:
        raise ValueError("flyby_batch: every waveform must be [chan, samples]")
    chan = int(waves[0].shape[0])
    for i, w in enumerate(waves):
        if w.dim() != 2 or int(w.shape[0]) != chan or w.device != dev or int(w.shape[1]) < 1 or chan < 1:
            raise ValueError(f"flyby_batch: waves[{i}] has shape {tuple(w.shape)} on {w.device}; expected [{chan} >= 1, L >= 1] on "
                             f"{dev}")
    table = flyby_records(geometry, [int(w.shape[1]) for w in waves], chan)
    results = [torch.empty_like(w) for w in waves]
    table["src"], table["dst"] = [w.data_ptr() for w in waves], [o.data_ptr() for o in results]
    flyby_launch(table, chan, int(table["len"].max()), dev)
    for w in waves:   # (a contiguous copy made above must outlive the kernel)
        w.record_stream(torch.cuda.current_stream(dev))
    return results


# mirrors iris_istft_src (include/iris_frontend.h)
ISTFT_SRC =np.dtype([("src", "<u8"), ("dst", "<u8"), ("n_frames", "<i4"), ("len_out", "<i4")])
assert ISTFT_SRC.itemsize == 24


def istft_len(n_frames: int, hop: int) -> int:
    """Samples the inverse STFT of `n_frames` frames returns by default: (n_frames - 1) * hop (iris_istft_len); 0 below two
    frames."""
    n_frames, hop = int(n_frames), int(hop)
    if hop <= 0:
        raise ValueError(f"hop must be positive, got {hop}")
    return (n_frames - 1) * hop if n_frames >= 2 else 0


def istft_launch(table: np.ndarray, plan: "FrontendPlan", max_frames: int, table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload an ISTFT_SRC table (into `table_dev`, a long-lived uint8 device buffer, when given) and run iris_istft over it on
    the current stream of the plan's device: one launch.  Returns the device table (tied to the stream when it was allocated
    here)."""
    def call(ptr, n, stream):
        with plan._lock:
            return N.lib().iris_istft(plan._handle, ptr, n, int(max_frames), stream)
    return _launch_records(table, plan.device, table_dev, "iris_istft", call)


def istft_batch(plan: "FrontendPlan", specs):
    """Invert a ragged batch of complex spectrograms in ONE launch (iris_istft): specs is a list of [F, T_i >= 2, 2C] float32
    tensors on the plan's device (re block, im block last; F = n_fft / 2 + 1 and C of the plan).  Returns a list of new
    [C, (T_i - 1) hop] waveforms: torch.istft with the periodic Hann window and center=True, |out - fp64| <= 128 u S (see
    include/iris_frontend.h).  CPU tensors raise: there is no CPU fallback."""
    specs = list(specs)
    if not specs:
        return []
    specs = [_require_device_f32(s, f"specs[{i}]") for i, s in enumerate(specs)]
    table = np.zeros(len(specs), ISTFT_SRC)
    results = []
    for i, s in enumerate(specs):
        if s.dim() != 3 or int(s.shape[0]) != plan.n_bins or int(s.shape[2]) != 2 * plan.channels or s.device != plan.device \
                or int(s.shape[1]) < 2:
            raise ValueError(f"istft_batch: specs[{i}] has shape {tuple(s.shape)} on {s.device}; expected "
                             f"[{plan.n_bins}, T >= 2, {2 * plan.channels}] on {plan.device}")
        n = istft_len(int(s.shape[1]), plan.hop)
        if n > 2 ** 31 - 1:
            raise ValueError(f"istft_batch: specs[{i}] would have {n} samples (> 2^31 - 1)")
        o = torch.empty((plan.channels, n), dtype=torch.float32, device=plan.device)
        table[i] = (s.data_ptr(), o.data_ptr(), int(s.shape[1]), n)
        results.append(o)
    istft_launch(table, plan, int(table["n_frames"].max()))
    for s in specs:   # (a contiguous copy made above must outlive the kernel)
        s.record_stream(torch.cuda.current_stream(plan.device))
    return results


def complex_to_magphase(x: torch.Tensor) -> torch.Tensor:
    x = _require_device_f32(x, "complex_tensor")
    c2 = int(x.shape[-1])
    if c2 % 2:
        raise ValueError("last axis must hold [re block, im block] (even length)")
    out = torch.empty_like(x)
    if x.numel():
        with torch.cuda.device(x.device):
            rc = N.lib().iris_complex_to_magphase(x.data_ptr(), out.data_ptr(), x.numel() // c2, c2 // 2,
                                                  _stream_ptr(x.device))
        N.check(rc, "iris_complex_to_magphase")
    return out


def magphase_to_complex(x: torch.Tensor) -> torch.Tensor:
    x = _require_device_f32(x, "magphase")
    c2 = int(x.shape[-1])
    if c2 % 2:
        raise ValueError("last axis must hold [mag block, phase block] (even length)")
    out = torch.empty_like(x)
    if x.numel():
        with torch.cuda.device(x.device):
            rc = N.lib().iris_magphase_to_complex(x.data_ptr(), out.data_ptr(), x.numel() // c2, c2 // 2,
                                                  _stream_ptr(x.device))
        N.check(rc, "iris_magphase_to_complex")
    return out


def mask_apply(x: torch.Tensor, axis: int, bands, outer_per_group: Optional[int] = None) -> torch.Tensor:
    """Zero the bands [offset, offset+size) along `axis` (out of place).

    bands: int [n, 2] (one group for the whole tensor) or [G, n, 2] with
    `outer_per_group` leading-index rows per group."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("mask_apply runs as a HIP kernel: x must be a tensor on a ROCm device")
    if x.element_size() not in (4, 8):
        raise TypeError(f"mask_apply supports 4- and 8-byte dtypes, got {x.dtype}")
    x = x.contiguous().clone()
    axis = axis % x.dim()
    n_outer = int(np.prod(x.shape[:axis], dtype=np.int64)) if axis > 0 else 1
    n_inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64)) if axis + 1 < x.dim() else 1
    b = torch.as_tensor(bands).to(device=x.device, dtype=torch.int32)
    if b.dim() == 2:
        b = b[None]
    if b.dim() != 3 or b.shape[-1] != 2:
        raise ValueError("bands must be [n, 2] or [G, n, 2]")
    b = b.contiguous()
    groups = int(b.shape[0])
    if outer_per_group is None:
        outer_per_group = max(n_outer // groups, 1) if groups > 1 else max(n_outer, 1)
    if groups * outer_per_group < n_outer:
        raise ValueError("bands groups do not cover the outer extent")
    if x.numel() and b.shape[1]:
        with torch.cuda.device(x.device):
            rc = N.lib().iris_mask_apply(x.data_ptr(), n_outer, int(x.shape[axis]), n_inner, x.element_size(),
                                         b.data_ptr(), int(b.shape[1]), int(outer_per_group),
                                         _stream_ptr(x.device))
        N.check(rc, "iris_mask_apply")
    return x


# ---------------------------------------------------------------------------
# plan cache for the closure-style API of transforms.py
# ---------------------------------------------------------------------------
_plans = {}
_plans_lock = threading.Lock()


def get_plan(device, n_fft: int, hop: Optional[int], n_mel: int, sample_rate: float, channels: int,
             batch: int, length: int, **mel_kw) -> FrontendPlan:
    """Cached plan with capacity >= (batch, length); grown geometrically."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    hop = n_fft // 2 if hop is None else hop
    key = (device.index, n_fft, hop, n_mel, float(sample_rate), channels, tuple(sorted(mel_kw.items())))
    with _plans_lock:
        plan = _plans.get(key)
        if plan is None or plan.max_batch < batch or plan.max_len < length:
            cap_b = max(batch, plan.max_batch if plan else 0)
            cap_l = max(length, plan.max_len if plan else 0, n_fft)
            if plan is not None:  # grow with headroom
                cap_b, cap_l = max(cap_b, 2 * plan.max_batch), max(cap_l, plan.max_len)
            plan = FrontendPlan(n_fft, hop, n_mel, sample_rate, channels, cap_b, cap_l, device, **mel_kw)
            _plans[key] = plan
        return plan
