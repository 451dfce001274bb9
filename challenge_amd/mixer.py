"""GPU-resident sample synthesis: make_pipeline + merge_complex_specs for whole batches.

The reference builds every training sample on the host, one at a time: a tf.data graph
picks a background, up to N voices and noises and mixes them in the complex-STFT domain
(pipeline.py:6-175).  On an MI355X every source spectrogram of the corpus fits in HBM, so
this module keeps them resident and synthesises a whole batch with two kernel launches
(`iris_mix_specs`, include/iris_frontend.h): the host only draws the random decisions
(`pipeline.merge_draw`, same distributions as the reference) and uploads a table of a few
dozen bytes per source.

No CPU fallback: `DeviceMixer` needs a ROCm device and the HIP library.  The per-sample
drop-in (`pipeline.make_pipeline`) stays available for code that wants the tf.data shape.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import frontend as _fe
from . import pipeline as _pl
from . import transforms as _tr

# mirrors iris_mix_src (include/iris_frontend.h)
MIX_SRC = np.dtype([("src", "<u8"), ("active", "<u8"), ("T", "<i4"), ("pad", "<i4"), ("off", "<i4"),
                    ("gain", "<f4"), ("kind", "<i4"), ("slot", "<i4"), ("label_row", "<i4"), ("reserved", "<i4")])
assert MIX_SRC.itemsize == 48

KIND_BACKGROUND, KIND_VOICE, KIND_NOISE, KIND_UNUSED = 0, 1, 2, -1


class _Corpus(C.Structure):
    """iris_mix_corpus (include/iris_frontend.h): device arrays describing one corpus."""
    _fields_ = [("src", C.c_void_p), ("active", C.c_void_p), ("T", C.c_void_p), ("len", C.c_void_p), ("n", C.c_int32)]


class _Stream:
    """`Dataset.from_generator(data).repeat().shuffle(len(data))` as an index stream: a fresh
    random permutation per epoch (pipeline.py:147-160)."""

    def __init__(self, n: int, rng: np.random.Generator):
        self.n, self.rng = n, rng
        self._perm = np.empty(0, np.int64)
        self._pos = 0

    def take(self, k: int) -> np.ndarray:
        out = np.empty(k, np.int64)
        got = 0
        while got < k:
            if self._pos >= len(self._perm):
                self._perm, self._pos = self.rng.permutation(self.n), 0
            m = min(k - got, len(self._perm) - self._pos)
            out[got:got + m] = self._perm[self._pos:self._pos + m]
            got, self._pos = got + m, self._pos + m
        return out


def _check_rate_range(word: str, lo: float, hi: float) -> None:
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"{word} rates must satisfy 0 < lo <= hi (finite), got lo = {lo}, hi = {hi}")


def check_stretch_range(lo: float, hi: float) -> None:
    """The rate range of `DeviceMixer.enable_stretch`: finite, 0 < lo <= hi."""
    _check_rate_range("stretch", lo, hi)


def check_speed_range(lo: float, hi: float) -> None:
    """The rate range of `WaveMixer.enable_speed`: finite, 0 < lo <= hi."""
    _check_rate_range("speed", lo, hi)


def stretch_rates(rng: np.random.Generator, n: int, lo: float = 0.8, hi: float = 1.2) -> np.ndarray:
    """The random half of `DeviceMixer.restretch`: n rates ~ U[lo, hi) (float64) from `rng`."""
    check_stretch_range(lo, hi)
    return rng.uniform(float(lo), float(hi), size=int(n))


@dataclass
class _VoiceAug:
    """The voice corpus under `enable_stretch` / `enable_speed`: the originals, their never-moving copies and the launch table.
    Lengths (`orig_n`, `cap`) are frames for the spectrum mixer and samples per channel for the waveform mixer."""
    lo: float
    hi: float
    orig: list                      # the voices as given (device tensors)
    orig_n: np.ndarray              # their lengths
    cap: np.ndarray                 # ceil(orig_n / lo): what each buffer holds
    bufs: list                      # one flat float32 buffer per voice
    acts: list                      # its frame-activity vector
    table: np.ndarray               # VOC_SRC / SPEED_SRC records, src / dst / input length filled once
    table_dev: torch.Tensor         # long-lived device copy of `table`
    act_ptr_dev: Optional[torch.Tensor] = None   # device array of the `acts` addresses (waveform mixer: one batched launch)
    rates: Optional[np.ndarray] = None           # the rates of the latest re-augmentation


def _enable_voice_aug(mixer, word: str, lo: float, hi: float) -> None:
    """`enable_stretch` / `enable_speed` (word = 'stretch' / 'speed'): allocate the copies, switch the pointer tables to them
    and fill them at rate 1.  The range is checked before `mixer` is touched."""
    _check_rate_range(word, lo, hi)
    if mixer._aug is not None:
        raise RuntimeError(f"enable_{word} was already called on this mixer" if isinstance(mixer._aug, _VoiceAug) else
                           f"{_aug_name(mixer._aug)} was already called on this mixer (a mixer holds one voice augmentation)")
    dev = mixer.device
    dtype, f_in, _ = mixer._aug_record
    orig = list(mixer.voices)
    orig_n = (mixer._v_T if mixer._v_L is None else mixer._v_L).copy()
    cap = np.array([_fe._scaled_len(int(n), lo, word) for n in orig_n], np.int64)
    buf_floats, act_len = mixer._aug_sizes(cap, lo)
    bufs = [torch.zeros(int(n), device=dev, dtype=torch.float32) for n in buf_floats]
    acts = [torch.zeros(int(n), device=dev, dtype=torch.float32) for n in act_len]
    table = np.zeros(len(orig), dtype)
    table["src"], table["dst"] = [t.data_ptr() for t in orig], [b.data_ptr() for b in bufs]
    table[f_in] = orig_n
    mixer._aug = aug = _VoiceAug(float(lo), float(hi), orig, orig_n, cap, bufs, acts, table,
                                 torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=dev))
    mixer.voice_active = acts
    mixer._v_ptr = np.array([b.data_ptr() for b in bufs], np.uint64)
    mixer._v_act = np.array([a.data_ptr() for a in acts], np.uint64)
    if mixer._v_L is not None:
        aug.act_ptr_dev = torch.from_numpy(mixer._v_act.astype(np.int64)).to(dev)
    if mixer._dd is not None:
        mixer._dd["voice_arrays"]["src"].copy_(torch.from_numpy(mixer._v_ptr.astype(np.int64)))
        mixer._dd["voice_arrays"]["act"].copy_(torch.from_numpy(mixer._v_act.astype(np.int64)))
    _reaugment(mixer, word, np.ones(len(orig)))


def _reaugment(mixer, word: str, rates) -> np.ndarray:
    """`restretch` / `respeed`: draw the rates (unless given), check that every result fits its buffer, run the class's launch
    and activity pass, then move the voices' lengths on the host and in the device corpus of `enable_device_draw`."""
    aug = mixer._aug if isinstance(mixer, DeviceMixer) else None   # (called unbound on something that is no mixer: not enabled)
    if not isinstance(aug, _VoiceAug):   # (nothing enabled, or the slot holds `enable_reverb`'s state)
        raise RuntimeError(f"re{word} needs enable_{word}() first")
    n_voice = len(aug.orig)
    if rates is None:
        rates = stretch_rates(mixer.rng, n_voice, aug.lo, aug.hi)
    rates = np.asarray(rates, np.float64).reshape(-1)
    if rates.shape[0] != n_voice:
        raise ValueError(f"re{word}: {rates.shape[0]} rates for {n_voice} voices")
    n_out = np.array([_fe._scaled_len(int(n), r, word) for n, r in zip(aug.orig_n, rates)], np.int64)
    if np.any(n_out > aug.cap):
        i = int(np.argmax(n_out > aug.cap))
        raise ValueError(f"re{word}: voice {i} at rate {rates[i]} needs {n_out[i]} {mixer._aug_unit} but its buffer holds "
                         f"{aug.cap[i]} (rates below lo = {aug.lo} do not fit)")
    aug.table[mixer._aug_record[2]], aug.table["rate"] = n_out, rates
    mixer._aug_launch(aug, n_out)
    mixer._aug_adopt(aug, n_out)
    if mixer._dd is not None:
        mixer._dd["voice_arrays"]["T"].copy_(torch.from_numpy(mixer._v_T.astype(np.int32)))
        if mixer._v_L is not None:
            mixer._dd["voice_arrays"]["len"].copy_(torch.from_numpy(mixer._v_L.astype(np.int32)))
    aug.rates = rates.copy()
    return aug.rates


@dataclass
class _ReverbAug:
    """The voice corpus under `WaveMixer.enable_reverb` (it takes the mixer's one `_aug` slot): the originals, their
    never-moving reverberated copies, the resident tap buffers and the launch table."""
    rt60: Tuple[float, float]
    drr: Tuple[float, float]
    orig: list                      # the voices as given (device tensors [C, L_i])
    bufs: list                      # one [C, L_i] buffer per voice: what the mixer reads
    taps: list                      # one [C, FIR_MAX_TAPS] tap buffer per voice (the first C * K_i floats hold [C, K_i])
    table: np.ndarray               # FIR_SRC records, src / dst / taps / len filled once
    table_dev: torch.Tensor         # long-lived device copy of `table`
    rirs: Optional[list] = None     # the impulse responses of the latest `rereverb`
    model: str = "noise"            # "noise" (`transforms.synth_rir`) or "shoebox" (`iris_ism_rir`)
    geometry: Optional[list] = None            # shoebox: the `transforms.draw_shoebox` dicts (+ rt60) of the latest draw
    ism_table: Optional[np.ndarray] = None     # shoebox: ISM_SRC records, dst (the tap buffers) filled once
    ism_table_dev: Optional[torch.Tensor] = None   # shoebox: long-lived device copy of `ism_table`
    max_taps: int = _fe.FIR_MAX_TAPS           # the tap buffers' row pitch; above FIR_MAX_TAPS the mixer is on the long path
    pool: Optional[list] = None                # measured responses (`transforms.load_rirs`) a plain `rereverb()` draws from
    groups: Optional[list] = None              # long path: (first, last + 1) voice ranges, one `iris_fft_fir_batch` each
    workspace: Optional[torch.Tensor] = None   # long path: the spectra of the largest group, allocated once


@dataclass
class _FlybyAug:
    """The voice corpus under `WaveMixer.enable_flyby` (it takes the mixer's one `_aug` slot): the originals, their never-moving
    copies and activity vectors, the launch table and the resident table of the activity pass."""
    ranges: dict                    # `transforms.draw_flyby`'s keyword arguments of a plain `reflyby()`
    orig: list                      # the voices as given (device tensors [C, L_i])
    bufs: list                      # one [C, L_i] buffer per voice: what the mixer reads
    acts: list                      # its frame-activity vector, recomputed from the buffer by every `reflyby`
    table: np.ndarray               # FLYBY_SRC records, src / dst / len filled once
    table_dev: torch.Tensor         # long-lived device copy of `table`, uploaded by every `reflyby`
    act_table_dev: torch.Tensor     # SPEED_SRC records of `iris_mix_wave_frame_active_batch` (dst / len_out), uploaded once
    act_ptr_dev: torch.Tensor       # device array of the `acts` addresses
    geometry: Optional[list] = None   # the flights of the latest `reflyby` (None per voice: the identity)


def _aug_name(aug) -> str:
    """The enable call whose state sits in a mixer's `_aug` slot."""
    return "enable_flyby" if isinstance(aug, _FlybyAug) else "enable_reverb" if isinstance(aug, _ReverbAug) else "enable_speed"


def _check_reverb_range(rt60_lo: float, rt60_hi: float, drr_lo: float, drr_hi: float) -> None:
    vals = [float(v) for v in (rt60_lo, rt60_hi, drr_lo, drr_hi)]
    if not (all(np.isfinite(v) for v in vals) and 0 <= vals[0] <= vals[1] and vals[2] <= vals[3]):
        raise ValueError(f"reverb ranges must satisfy 0 <= rt60_lo <= rt60_hi and drr_lo <= drr_hi (finite), got rt60 "
                         f"[{vals[0]}, {vals[1]}), drr [{vals[2]}, {vals[3]})")


class BatchDraw:
    """The random decisions of one batch as arrays (B samples, V = max_voices, N = max_noises):
    bg [B], bg_offset [B], voices [B, V], v_len [B], n_voices [B], v_gain [B, V] f32, v_offset [B, V],
    noises [B, N] | None, n_len [B], n_noises [B], n_gain [B, N] f32, n_offset [B, N]."""
    __slots__ = ("bg", "bg_offset", "voices", "v_len", "n_voices", "v_gain", "v_offset", "noises", "n_len", "n_noises",
                 "n_gain", "n_offset")

    def __len__(self):
        return int(self.bg.shape[0])

    def as_dicts(self) -> List[dict]:
        """Per-sample dicts in the layout of `pipeline.merge_draw` (what the oracle's apply takes)."""
        out = []
        for i in range(len(self)):
            nv, nn = int(self.n_voices[i]), int(self.n_noises[i])
            out.append({"bg": int(self.bg[i]), "bg_offset": int(self.bg_offset[i]), "voices": [int(v) for v in self.voices[i]],
                        "v_len": int(self.v_len[i]), "n_voices": nv, "v_gain": [float(g) for g in self.v_gain[i, :nv]],
                        "v_offset": [int(o) for o in self.v_offset[i, :nv]],
                        "noises": None if self.noises is None else [int(n) for n in self.noises[i]],
                        "n_len": int(self.n_len[i]), "n_noises": nn, "n_gain": [float(g) for g in self.n_gain[i, :nn]],
                        "n_offset": [int(o) for o in self.n_offset[i, :nn]]})
        return out

    @classmethod
    def from_dicts(cls, draws: List[dict], max_voices: int, max_noises: int) -> "BatchDraw":
        b = len(draws)
        d = cls()
        d.bg = np.array([x["bg"] for x in draws], np.int64)
        d.bg_offset = np.array([x["bg_offset"] for x in draws], np.int64)
        d.voices = np.array([x["voices"] for x in draws], np.int64).reshape(b, max_voices)
        d.v_len = np.array([x["v_len"] for x in draws], np.int64)
        d.n_voices = np.array([x["n_voices"] for x in draws], np.int64)
        d.v_gain, d.v_offset = np.zeros((b, max_voices), np.float32), np.zeros((b, max_voices), np.int64)
        has_noise = b > 0 and draws[0]["noises"] is not None
        d.noises = np.array([x["noises"] for x in draws], np.int64).reshape(b, max_noises) if has_noise else None
        d.n_len = np.array([x["n_len"] for x in draws], np.int64)
        d.n_noises = np.array([x["n_noises"] for x in draws], np.int64)
        nn = max_noises if has_noise else 0
        d.n_gain, d.n_offset = np.zeros((b, nn), np.float32), np.zeros((b, nn), np.int64)
        for i, x in enumerate(draws):
            d.v_gain[i, :x["n_voices"]], d.v_offset[i, :x["n_voices"]] = x["v_gain"], x["v_offset"]
            if has_noise:
                d.n_gain[i, :x["n_noises"]], d.n_offset[i, :x["n_noises"]] = x["n_gain"], x["n_offset"]
        return d


class DeviceMixer:
    """Batched, device-resident counterpart of `make_pipeline(...)` (pipeline.py:113-175):

        mixer = DeviceMixer(backgrounds, voices, labels, noises, n_frame=512, ...)
        spec, label = mixer.mix(batch)     # [B, F, n_frame, 2C], [B, max_voices, n_frame, n_classes]

    backgrounds / voices / noises: sequences of [F, T_i, 2C] arrays (ragged in T); labels:
    [n_voices, n_classes] rows (one-hot in the reference).  Source picking follows the
    reference's dataset graph: one background, the next `max_voices` voices and the next
    `max_noises` noises of shuffled, repeated streams; each group is zero-padded to its longest
    member (`padded_batch`), of which `merge_complex_specs` uses the first n_voices / n_noises.
    The host side of a batch is a handful of vectorised NumPy draws and one structured-array fill
    (no per-sample Python loop): ~0.1 ms for a batch of 64.
    """

    # what the constructor asks the class (`WaveMixer` differs in these): the values below and the methods `_source_ok`,
    # `_set_dims`, `_frames` and `_frame_active`
    _no_device = "DeviceMixer needs a ROCm device (no CPU fallback); use pipeline.make_pipeline"
    _rank, _rank_error = 3, 'each spec must be a 3D-tensor'
    _takes_tensors = False          # sources that already are torch tensors are taken as they are
    _in_samples = False             # a source's second axis counts samples (not frames): keep the `_L` tables
    _shape_errors = ("sources must be [freq, time, chan2] with equal freq and chan2",
                     "voices / noises must share the backgrounds' freq and chan2 sizes")

    def __init__(self, backgrounds: Sequence, voices: Sequence, labels, noises: Optional[Sequence] = None,
                 n_frame: int = 300, max_voices: int = 10, max_noises: int = 10, n_classes: int = 3, device=None,
                 min_ratio: float = 2 / 3, min_noise_ratio: float = 1 / 2, snr: float = -20, seed=None):
        labels = np.asarray(labels, np.float32)
        as_tensor = lambda x: self._takes_tensors and isinstance(x, torch.Tensor)  # noqa: E731
        first = backgrounds[0]
        assert len(first.shape if as_tensor(first) else np.asarray(first).shape) == self._rank, self._rank_error
        assert len(voices) == len(labels)
        assert labels.ndim == 2 and labels.shape[1] == n_classes, \
            'labels must be in the form of [n_samples, n_classes]'
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError(self._no_device)
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(self._no_device)
        N.lib()  # fail loudly when the HIP library is missing
        self.n_frame, self.max_voices, self.max_noises, self.n_classes = n_frame, max_voices, max_noises, n_classes
        self.min_ratio, self.min_noise_ratio, self.snr = min_ratio, min_noise_ratio, snr
        self.rng = np.random.default_rng(seed)
        self._dd = None    # the device-side corpus and draw state of `enable_device_draw`
        self._aug = None   # the `_VoiceAug` of `enable_stretch` / `enable_speed`, or the `_ReverbAug` of `enable_reverb`

        def upload(items):
            # (a float32 tensor - e.g. a waveform `sj_train.waves_from_specs` left on the device - is taken as it is)
            out = [x.detach().to(self.device, torch.float32).contiguous() if as_tensor(x)
                   else torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32))).to(self.device) for x in items]
            for t in out:
                if not self._source_ok(t, out[0]):
                    raise ValueError(self._shape_errors[0])
            return out

        self.backgrounds, self.voices = upload(backgrounds), upload(voices)
        self.noises = upload(noises) if noises is not None else None
        self._set_dims(self.backgrounds[0])
        for group in (self.voices, self.noises or []):
            for t in group:
                if not self._source_ok(t, self.backgrounds[0]):
                    raise ValueError(self._shape_errors[1])
        self.label_vecs = torch.from_numpy(labels).to(self.device)
        # which frames of a voice are active (max over freq, chan2 > 0; pipeline.py:57) is a property of
        # the source: one pass over the corpus now instead of one per use
        self.voice_active = []
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for v in self.voices:
                act = torch.empty(int(self._frames(int(v.shape[1]))), device=self.device, dtype=torch.float32)
                self._frame_active(v, int(v.shape[1]), act, stream)
                self.voice_active.append(act)
        # pointer / length / frame-count lookup tables of every source, indexed per batch when its table is built
        ptrs = lambda ts: np.array([t.data_ptr() for t in ts], np.uint64)  # noqa: E731
        lens = lambda ts: np.array([int(t.shape[1]) for t in ts], np.int64)  # noqa: E731
        self._bg_ptr, self._v_ptr, self._v_act = ptrs(self.backgrounds), ptrs(self.voices), ptrs(self.voice_active)
        self._n_ptr = ptrs(self.noises) if self.noises is not None else None
        bg_len, v_len = lens(self.backgrounds), lens(self.voices)
        n_len = lens(self.noises) if self.noises is not None else None
        self._bg_T, self._v_T = self._frames(bg_len), self._frames(v_len)
        self._n_T = self._frames(n_len) if n_len is not None else None
        self._bg_L = self._v_L = self._n_L = None   # samples per channel: waveform sources only
        if self._in_samples:
            self._bg_L, self._v_L, self._n_L = bg_len, v_len, n_len
        self._b = _Stream(len(self.backgrounds), self.rng)
        self._v = _Stream(len(self.voices), self.rng)
        self._n = _Stream(len(self.noises), self.rng) if self.noises is not None else None

    def _source_ok(self, t: torch.Tensor, ref: torch.Tensor) -> bool:
        """The shape rule: `t` is [freq, time, chan2] with the freq and chan2 of `ref`."""
        return t.dim() == 3 and t.shape[0] == ref.shape[0] and t.shape[2] == ref.shape[2]

    def _set_dims(self, ref: torch.Tensor) -> None:
        self.n_bins, self.chan2 = int(ref.shape[0]), int(ref.shape[2])

    def _frames(self, n):
        """Frames of a source whose second axis has `n` entries (an int or an array of them)."""
        return n

    def _frame_active(self, src: torch.Tensor, n: int, act: torch.Tensor, stream) -> None:
        """Launch the frame-activity pass of a source of `n` frames (`WaveMixer`: samples) into `act`."""
        N.check(N.lib().iris_mix_frame_active(src.data_ptr(), self.n_bins, n, self.chan2, act.data_ptr(), stream),
                "iris_mix_frame_active")

    # -- random half ------------------------------------------------------------------
    @staticmethod
    def _padded_len(frames: np.ndarray, ratio: float, n_frame: int) -> Tuple[np.ndarray, np.ndarray]:
        """(pad, padded length) of a source of `frames` frames: pad = n_frame - int(ratio * frames) on both sides
        when positive (pipeline.py:59-66, :95-101; the product is an fp32 one, truncated)."""
        pad = n_frame - (np.float32(ratio) * frames.astype(np.float32)).astype(np.int64)
        return pad, np.where(pad > 0, frames + 2 * pad, frames)

    def draw_arrays(self, batch: int) -> BatchDraw:
        """Which sources (dataset graph, pipeline.py:147-174) and the draws of merge_complex_specs
        (`pipeline.merge_draw`, pipeline.py:29-106) for a whole batch, vectorised: the same distributions,
        every sample independent.  Draws beyond a sample's n_voices / n_noises are made and ignored."""
        rng, nf, V, Nn = self.rng, self.n_frame, self.max_voices, self.max_noises
        d = BatchDraw()
        d.bg = self._b.take(batch)
        d.voices = self._v.take(batch * V).reshape(batch, V)
        d.noises = self._n.take(batch * Nn).reshape(batch, Nn) if self._n is not None else None
        d.v_len = self._v_T[d.voices].max(axis=1) if V else np.zeros(batch, np.int64)   # padded_batch: longest of the group
        d.n_len = self._n_T[d.noises].max(axis=1) if (d.noises is not None and Nn) else np.zeros(batch, np.int64)
        bg_T = self._bg_T[d.bg]
        reps = (nf + bg_T - 1) // bg_T
        d.bg_offset = rng.integers(0, reps * bg_T - nf + 1)                               # tf.image.random_crop, :35
        d.n_voices = rng.integers(1, V, size=batch) if V > 1 else np.ones(batch, np.int64)  # :42-46
        d.v_gain = np.power(np.float32(10.0), (-rng.uniform(0, -self.snr / 10, size=(batch, V))).astype(np.float32))  # :50
        _, length = self._padded_len(d.v_len, self.min_ratio, nf)
        maxval = (length - nf)[:, None]                                                   # :68-69
        d.v_offset = np.where(maxval > 0, rng.integers(0, np.maximum(maxval, 1), size=(batch, V)), 0)
        if d.noises is not None:
            d.n_noises = rng.integers(0, Nn, size=batch) if Nn > 0 else np.zeros(batch, np.int64)  # :87-88
            d.n_gain = np.power(np.float32(10.0), (-rng.uniform(0, 2, size=(batch, Nn))).astype(np.float32))  # :94
            _, length = self._padded_len(d.n_len, self.min_noise_ratio, nf)
            d.n_offset = rng.integers(0, (np.maximum(length - nf, 0) + 1)[:, None], size=(batch, Nn))  # :103
        else:
            d.n_noises = np.zeros(batch, np.int64)
            d.n_gain, d.n_offset = np.zeros((batch, 0), np.float32), np.zeros((batch, 0), np.int64)
        return d

    def draw(self, batch: int) -> List[dict]:
        """`draw_arrays` as per-sample dicts (the layout of `pipeline.merge_draw`)."""
        return self.draw_arrays(batch).as_dicts()

    # -- deterministic half ----------------------------------------------------------
    def table(self, draws) -> Tuple[np.ndarray, np.ndarray]:
        """Source table (iris_mix_src records, sample-major: background, voices, noises) and the per-sample
        ranges for a BatchDraw (or a list of per-sample dicts)."""
        d = draws if isinstance(draws, BatchDraw) else BatchDraw.from_dicts(draws, self.max_voices, self.max_noises)
        b, V = len(d), self.max_voices
        Nn = self.max_noises if d.noises is not None else 0
        cols = 1 + V + Nn
        use = np.zeros((b, cols), bool)
        use[:, 0] = True
        use[:, 1:1 + V] = np.arange(V)[None, :] < d.n_voices[:, None]
        if Nn:
            use[:, 1 + V:] = np.arange(Nn)[None, :] < d.n_noises[:, None]
        full = np.zeros((b, cols), MIX_SRC)
        full["src"][:, 0], full["T"][:, 0], full["off"][:, 0] = self._bg_ptr[d.bg], self._bg_T[d.bg], d.bg_offset
        full["gain"][:, 0], full["kind"][:, 0] = 1.0, KIND_BACKGROUND
        pad_v, _ = self._padded_len(d.v_len, self.min_ratio, self.n_frame)
        v = full[:, 1:1 + V]
        v["src"], v["active"], v["T"] = self._v_ptr[d.voices], self._v_act[d.voices], self._v_T[d.voices]
        v["pad"], v["off"], v["gain"] = np.maximum(pad_v, 0)[:, None], d.v_offset, d.v_gain
        v["kind"], v["slot"], v["label_row"] = KIND_VOICE, np.arange(V)[None, :], d.voices
        if Nn:
            pad_n, _ = self._padded_len(d.n_len, self.min_noise_ratio, self.n_frame)
            n = full[:, 1 + V:]
            n["src"], n["T"] = self._n_ptr[d.noises], self._n_T[d.noises]
            n["pad"], n["off"], n["gain"], n["kind"] = np.maximum(pad_n, 0)[:, None], d.n_offset, d.n_gain, KIND_NOISE
        if self._bg_L is not None:  # waveform sources (WaveMixer): samples per channel
            full["reserved"][:, 0] = self._bg_L[d.bg]
            full["reserved"][:, 1:1 + V] = self._v_L[d.voices]
            if Nn:
                full["reserved"][:, 1 + V:] = self._n_L[d.noises]
        first = np.concatenate([[0], np.cumsum(use.sum(axis=1))]).astype(np.int32)
        return np.ascontiguousarray(full[use]), first

    def _batch_table(self, batch: int, draws):
        """(table_d, first_d, n_srcs, batch, keep) of one batch: drawn and written on the device after `enable_device_draw`
        (unless `draws` are given), else drawn on the host and uploaded.  keep: what must be tied to the stream."""
        if draws is None and self._dd is not None:
            return (*self._draw_on_device(batch), batch, ())
        draws = self.draw_arrays(batch) if draws is None else draws
        table, first = self.table(draws)
        table_d = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(self.device, non_blocking=True)
        first_d = torch.from_numpy(first).to(self.device, non_blocking=True)
        return table_d, first_d, int(table.shape[0]), len(draws), (table_d, first_d)

    def _launch_mix(self, name: str, n_srcs: int, keep, call) -> None:
        """Allocate the workspace, run `call(workspace pointer, its floats, stream)` - the C entry point `name` - and tie the
        workspace and `keep` to the stream: they must outlive the kernels."""
        dev = self.device
        ws_floats = int(N.lib().iris_mix_workspace(n_srcs, self.n_frame))
        ws = torch.empty(max(ws_floats, 1), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = call(ws.data_ptr(), ws_floats, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        N.check(rc, name)
        for t in (*keep, ws):
            t.record_stream(torch.cuda.current_stream(dev))

    def mix(self, batch: int, draws=None):
        """One batch of (complex spectrogram [B, F, n_frame, 2C], labels [B, max_voices, n_frame,
        n_classes]) - `merge_complex_specs` (pipeline.py:6-110) for every sample, two launches.
        draws: a BatchDraw or a list of per-sample dicts (default: a fresh `draw_arrays(batch)`)."""
        table_d, first_d, n_srcs, batch, keep = self._batch_table(batch, draws)
        spec = torch.empty((batch, self.n_bins, self.n_frame, self.chan2), device=self.device, dtype=torch.float32)
        label = torch.empty((batch, self.max_voices, self.n_frame, self.n_classes), device=self.device, dtype=torch.float32)
        self._launch_mix("iris_mix_specs", n_srcs, keep, lambda ws, ws_floats, stream: N.lib().iris_mix_specs(
            table_d.data_ptr(), n_srcs, first_d.data_ptr(), self.label_vecs.data_ptr(), spec.data_ptr(), label.data_ptr(), batch,
            self.n_bins, self.n_frame, self.chan2, self.max_voices, self.n_classes, ws, ws_floats, stream))
        return spec, label

    # -- random half on the device ----------------------------------------------------
    def enable_device_draw(self, seed: int = 0) -> None:
        """Draw every later `mix(batch)` ON THE DEVICE (`iris_mix_draw`): no NumPy draws, no table upload - the source
        table is written by one small kernel from a Philox generator keyed by `seed`, whose call counter and stream
        positions live in device memory (so a captured batch replays with fresh draws).  Same distributions as
        `draw_arrays`; `last_table()` returns the records of the latest batch for replay through the oracle."""
        dev = self.device
        i64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)  # noqa: E731
        i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)  # noqa: E731
        self._dd = {"seed": int(seed) & 0xFFFFFFFFFFFFFFFF, "state": torch.zeros(4, dtype=torch.int64, device=dev),
                    "keep": [], "bufs": {}}

        def corpus(ptr, act, T, L):
            t = {"src": i64(ptr.astype(np.int64)), "act": None if act is None else i64(act.astype(np.int64)), "T": i32(T),
                 "len": None if L is None else i32(L)}
            self._dd["keep"].append(t)
            return _Corpus(t["src"].data_ptr(), 0 if t["act"] is None else t["act"].data_ptr(), t["T"].data_ptr(),
                           0 if t["len"] is None else t["len"].data_ptr(), int(len(ptr)))
        self._dd["bg"] = corpus(self._bg_ptr, None, self._bg_T, self._bg_L)
        self._dd["voice"] = corpus(self._v_ptr, self._v_act, self._v_T, self._v_L)
        self._dd["noise"] = corpus(self._n_ptr, None, self._n_T, self._n_L) if self.noises is not None else None
        self._dd["voice_arrays"] = self._dd["keep"][1]   # `_reaugment` rewrites the voices' T / len (and, once, src / act) in place

    # -- time-stretch augmentation of the voice corpus ----------------------------------
    def enable_stretch(self, lo: float = 0.8, hi: float = 1.2) -> None:
        """Keep a time-stretched copy of every voice beside the original and mix from the copies: `restretch()` then
        re-stretches the whole voice corpus by fresh rates ~ U[lo, hi) in one launch (`iris_phase_vocoder`, the
        reference's `transforms.phase_vocoder` with the running phase kept in [-pi, pi]).  The defaults are the two rates of
        the reference's own test.  One buffer per voice with room for ceil(T_i / lo) frames and its frame-activity vector
        of the same capacity are allocated here and never move: the pointer tables (and the device-side corpus of
        `enable_device_draw`, in either call order) are switched to them once, so a captured `mix` replayed after a
        `restretch` reads the new contents through unchanged addresses.  Until the first `restretch` the copies hold the
        voices at rate 1 (bit-identical).  Backgrounds and noises are not stretched: they carry no labels, and the
        reference's function was written for voices.  No accuracy claim is made for the augmentation."""
        _enable_voice_aug(self, "stretch", lo, hi)

    def restretch(self, rates=None) -> np.ndarray:
        """Stretch every ORIGINAL voice anew into its buffer: rate_i ~ U[lo, hi) from the mixer's own NumPy generator
        (or the given `rates`, one per voice, each >= lo so that the result fits its buffer), ONE `iris_phase_vocoder`
        launch over the whole voice corpus, then every voice's frame activity recomputed from the stretched voice
        (`iris_mix_frame_active`: the labels follow from `max(voice) > 0`, as in the reference).  The voices' frame counts
        change to ceil(T_i / rate_i), on the host (`_v_T`) and in place in the device corpus of `enable_device_draw`.  Call
        it outside any graph capture.  Backgrounds and noises are not stretched.  Returns the rates used."""
        return _reaugment(self, "stretch", rates)

    # what differs between `restretch` and `WaveMixer.respeed` (`_enable_voice_aug`, `_reaugment`)
    _aug_record = (_fe.VOC_SRC, "n_in", "n_out")   # the launch table's dtype and its input / output length fields
    _aug_unit = "frames"

    def _aug_sizes(self, cap: np.ndarray, lo: float):
        """(floats of each voice's buffer, length of its activity vector) for capacities `cap`."""
        return cap * (self.n_bins * self.chan2), cap

    def _aug_launch(self, aug: _VoiceAug, n_out: np.ndarray) -> None:
        _fe.phase_vocoder_launch(aug.table, self.n_bins, self.chan2, int(aug.cap.max()), self.device, aug.table_dev)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for buf, act, n in zip(aug.bufs, aug.acts, n_out):
                self._frame_active(buf, int(n), act, stream)

    def _aug_adopt(self, aug: _VoiceAug, n_out: np.ndarray) -> None:
        self._v_T = n_out
        self.voices = [b[:self.n_bins * int(n) * self.chan2].view(self.n_bins, int(n), self.chan2)
                       for b, n in zip(aug.bufs, n_out)]

    def enable_speed(self, lo: float = 0.9, hi: float = 1.1) -> None:
        raise NotImplementedError("DeviceMixer.enable_speed: a spectrum corpus cannot be resampled in time (speed perturbation "
                                  "works on waveforms: use WaveMixer; this corpus has enable_stretch)")

    def enable_reverb(self, rt60_lo: float = 0.1, rt60_hi: float = 0.4, drr_lo: float = -3.0, drr_hi: float = 12.0) -> None:
        raise NotImplementedError("DeviceMixer.enable_reverb: a spectrum corpus has no waveform to convolve (reverberation "
                                  "works on waveforms: use WaveMixer; this corpus has enable_stretch)")

    def enable_flyby(self, **ranges) -> None:
        raise NotImplementedError("DeviceMixer.enable_flyby: a spectrum corpus has no waveform to delay (the fly-by works on "
                                  "waveforms: use WaveMixer; this corpus has enable_stretch)")

    def _draw_on_device(self, batch: int):
        """(table_d [batch * stride, 48 B], first_d [batch + 1], n_srcs) written by iris_mix_draw on the current stream."""
        dd, dev = self._dd, self.device
        nn = self.max_noises if self.noises is not None else 0
        stride = 1 + self.max_voices + nn
        key = (batch, stride)
        if key not in dd["bufs"]:  # long-lived: a captured graph keeps their addresses
            dd["bufs"][key] = (torch.empty(batch * stride * MIX_SRC.itemsize, dtype=torch.uint8, device=dev),
                               torch.empty(batch + 1, dtype=torch.int32, device=dev))
        table_d, first_d = dd["bufs"][key]
        with torch.cuda.device(dev):
            rc = N.lib().iris_mix_draw(C.byref(dd["bg"]), C.byref(dd["voice"]),
                                       C.byref(dd["noise"]) if dd["noise"] is not None else None, batch, self.n_frame,
                                       self.max_voices, nn, float(self.min_ratio), float(self.min_noise_ratio), float(self.snr),
                                       dd["seed"], dd["state"].data_ptr(), table_d.data_ptr(), first_d.data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        N.check(rc, "iris_mix_draw")
        return table_d, first_d, batch * stride

    def last_table(self, batch: int) -> np.ndarray:
        """The device-drawn records of the latest `mix(batch)` as a host structured array [batch, stride] (synchronises)."""
        nn = self.max_noises if self.noises is not None else 0
        stride = 1 + self.max_voices + nn
        raw = self._dd["bufs"][(batch, stride)][0].cpu().numpy()
        return raw.view(MIX_SRC).reshape(batch, stride)

    def table_to_draws(self, table: np.ndarray) -> List[dict]:
        """Per-sample draw dicts (layout of `pipeline.merge_draw`) recovered from device-drawn records: what the oracle's
        apply takes.  Sources are identified by their device address."""
        V = self.max_voices
        nn = table.shape[1] - 1 - V
        bg_of = {int(p): i for i, p in enumerate(self._bg_ptr)}
        v_of = {int(p): i for i, p in enumerate(self._v_ptr)}
        n_of = {int(p): i for i, p in enumerate(self._n_ptr)} if self._n_ptr is not None else {}
        out = []
        for row in table:
            voices, noises = row[1:1 + V], row[1 + V:]
            nv, n_n = int((voices["kind"] == KIND_VOICE).sum()), int((noises["kind"] == KIND_NOISE).sum())
            assert np.all(voices["kind"][:nv] == KIND_VOICE) and np.all(voices["kind"][nv:] == KIND_UNUSED)
            assert np.all(noises["kind"][:n_n] == KIND_NOISE) and np.all(noises["kind"][n_n:] == KIND_UNUSED)
            v_idx = [v_of[int(p)] for p in voices["src"]]
            n_idx = [n_of[int(p)] for p in noises["src"]]
            out.append({"bg": bg_of[int(row[0]["src"])], "bg_offset": int(row[0]["off"]), "voices": v_idx,
                        "v_len": int(max(self._v_T[v_idx])), "n_voices": nv,
                        "v_gain": [float(g) for g in voices["gain"][:nv]], "v_offset": [int(o) for o in voices["off"][:nv]],
                        "noises": n_idx if nn else None, "n_len": int(max(self._n_T[n_idx])) if nn else 0, "n_noises": n_n,
                        "n_gain": [float(g) for g in noises["gain"][:n_n]], "n_offset": [int(o) for o in noises["off"][:n_n]]})
        return out

    def __iter__(self):
        raise TypeError("DeviceMixer yields whole batches: call mix(batch)")


class WaveMixer(DeviceMixer):
    """`DeviceMixer` in the waveform domain (second half): the corpus stays
    resident as waveforms [C, L_i] - a quarter of the bytes of its spectrograms at n_fft 1024 / hop 256 - and a
    batch is mixed before the STFT, which is linear:

        mixer = WaveMixer(backgrounds, voices, labels, noises, n_frame=512, n_fft=1024, hop=256, ...)
        wav, label = mixer.mix(batch)      # [B, C, (n_frame - 1) * hop], [B, max_voices, n_frame, n_classes]
        logmel = WaveFrontend(...)(wav)    # fused kernel: no spectrum is ever materialised

    Same draws (in frames: a source of L samples has 1 + L // hop of them), same label rule and the same table as
    the spectrum-domain mixer; every frame quantity is multiplied by `hop`.  STFT(wav) equals `DeviceMixer`'s output
    for the sources' STFTs on every frame whose window crosses no crop / pad / tiling boundary
    (`iris_mix_waves`, include/iris_frontend.h; oracle: `mix_waves_apply`)."""

    _no_device = "WaveMixer needs a ROCm device (no CPU fallback)"
    _rank, _rank_error = 2, 'each waveform must be [chan, samples]'
    _takes_tensors = True
    _in_samples = True
    _shape_errors = ("sources must be [chan, samples] with equal chan",
                     "voices / noises must have the backgrounds' channel count")

    def __init__(self, backgrounds: Sequence, voices: Sequence, labels, noises: Optional[Sequence] = None,
                 n_frame: int = 300, n_fft: int = 1024, hop: int = 256, max_voices: int = 10, max_noises: int = 10,
                 n_classes: int = 3, device=None, min_ratio: float = 2 / 3, min_noise_ratio: float = 1 / 2,
                 snr: float = -20, seed=None):
        self.n_fft, self.hop = n_fft, hop
        super().__init__(backgrounds, voices, labels, noises, n_frame=n_frame, max_voices=max_voices, max_noises=max_noises,
                         n_classes=n_classes, device=device, min_ratio=min_ratio, min_noise_ratio=min_noise_ratio, snr=snr,
                         seed=seed)

    def _source_ok(self, t: torch.Tensor, ref: torch.Tensor) -> bool:
        """The shape rule: `t` is [chan, samples >= 1] with the channel count of `ref`."""
        return t.dim() == 2 and t.shape[0] == ref.shape[0] and t.shape[1] >= 1

    def _set_dims(self, ref: torch.Tensor) -> None:
        self.channels = int(ref.shape[0])

    def _frames(self, n):
        return 1 + n // self.hop

    def _frame_active(self, src: torch.Tensor, n: int, act: torch.Tensor, stream) -> None:
        N.check(N.lib().iris_mix_wave_frame_active(src.data_ptr(), self.channels, n, self.n_fft, self.hop, act.data_ptr(), stream),
                "iris_mix_wave_frame_active")

    def enable_stretch(self, lo: float = 0.8, hi: float = 1.2) -> None:
        raise NotImplementedError("WaveMixer.enable_stretch: a waveform corpus has no spectra to stretch (the phase vocoder "
                                  "works on complex spectrograms: use DeviceMixer)")

    # -- speed perturbation of the voice corpus ------------------------------------------
    def enable_speed(self, lo: float = 0.9, hi: float = 1.1) -> None:
        """Keep a speed-perturbed copy of every voice beside the original and mix from the copies: `respeed()` then resamples
        the whole voice corpus by fresh rates ~ U[lo, hi) in one launch (`iris_speed_perturb`: tempo and pitch move together,
        the standard 0.9 .. 1.1 of speech and sound-event training).  One buffer per voice with room for ceil(L_i / lo) samples
        per channel and its frame-activity vector of 1 + capacity // hop frames are allocated here and never move: the pointer
        tables (and the device-side corpus of `enable_device_draw`, in either call order) are switched to them once, so a
        captured `mix` replayed after a `respeed` reads the new contents through unchanged addresses.  Until the first
        `respeed` the copies hold the voices at rate 1 (bit-identical).  Backgrounds and noises are not perturbed: they carry
        no labels.  No accuracy claim is made for the augmentation."""
        _enable_voice_aug(self, "speed", lo, hi)

    def respeed(self, rates=None) -> np.ndarray:
        """Resample every ORIGINAL voice anew into its buffer: rate_i ~ U[lo, hi) from the mixer's own NumPy generator (or the
        given `rates`, one per voice, each >= lo so that the result fits its buffer), ONE `iris_speed_perturb` launch over the
        whole voice corpus and ONE `iris_mix_wave_frame_active_batch` launch for the frame activity of the results (the labels
        follow the perturbed voice; a silent tail stays exactly zero).  The voices' lengths change to L' = ceil(L_i / rate_i)
        and their frame counts to 1 + L' // hop, on the host (`_v_L`, `_v_T`, `voices`) and in place in the device corpus of
        `enable_device_draw`.  Call it outside any graph capture.  Backgrounds and noises are not perturbed.  Returns the rates
        used."""
        return _reaugment(self, "speed", rates)

    _aug_record = (_fe.SPEED_SRC, "len_in", "len_out")
    _aug_unit = "samples"

    def _aug_sizes(self, cap: np.ndarray, lo: float):
        if cap.max() > 2 ** 31 - 1:
            raise ValueError(f"enable_speed: a voice at rate {lo} would have {cap.max()} samples (> 2^31 - 1)")
        return cap * self.channels, 1 + cap // self.hop

    def _aug_launch(self, aug: _VoiceAug, n_out: np.ndarray) -> None:
        max_len = int(aug.cap.max())
        table_dev = _fe.speed_perturb_launch(aug.table, self.channels, max_len, self.device, aug.table_dev)
        with torch.cuda.device(self.device):
            rc = N.lib().iris_mix_wave_frame_active_batch(table_dev.data_ptr(), len(aug.orig), self.channels, self.n_fft, self.hop,
                                                          aug.act_ptr_dev.data_ptr(), 1 + max_len // self.hop,
                                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        N.check(rc, "iris_mix_wave_frame_active_batch")

    def _aug_adopt(self, aug: _VoiceAug, n_out: np.ndarray) -> None:
        self._v_L, self._v_T = n_out, 1 + n_out // self.hop
        self.voices = [b[:self.channels * int(n)].view(self.channels, int(n)) for b, n in zip(aug.bufs, n_out)]

    # -- reverberation of the voice corpus ------------------------------------------------
    def enable_reverb(self, rt60_lo: float = 0.1, rt60_hi: float = 0.4, drr_lo: float = -3.0, drr_hi: float = 12.0,
                      model: str = "noise", max_taps: int = _fe.FIR_MAX_TAPS, rirs=None,
                      workspace_budget: int = 256 << 20) -> None:
        """Keep a reverberated copy of every voice beside the original and mix from the copies: `rereverb()` then convolves the
        whole voice corpus with fresh synthetic room impulse responses (`transforms.synth_rir`: rt60 ~ U[rt60_lo, rt60_hi)
        seconds, direct-to-reverberant ratio ~ U[drr_lo, drr_hi) dB per voice) in one launch (`iris_fir_batch`; Ko et al. 2017,
        Kaldi's reverberate_data_dir).  One [C, L_i] buffer and one [C, 4096] tap buffer per voice are allocated here and never
        move: the pointer tables (and the device-side corpus of `enable_device_draw`, in either call order) are switched to
        them once, so a captured `mix` replayed after a `rereverb` reads the new contents through unchanged addresses.  Until
        the first `rereverb` the copies hold the voices under the identity response (bit-identical).
        The labels follow the DRY voice: the convolution is cut at the voice's length, so lengths and frame counts do not
        move, and the frame-activity vectors stay the ones computed from the originals at construction - an exactly silent
        gap inside a voice stays labelled silent although the tail now rings into it.  Backgrounds and noises are not
        reverberated: they carry no labels.  A mixer holds one voice augmentation: this after `enable_speed` (or the other way
        round) raises; combining the two is out of scope.  No accuracy claim is made for the augmentation.
        model = "shoebox": `rereverb()` draws one random shoebox room per voice (`transforms.draw_shoebox`, rt60 ~ U[rt60_lo,
        rt60_hi)) and computes its image-source response for all channels on the device (`iris_ism_rir`, straight into the
        resident tap buffers): both channels hear the same room, so the inter-channel delay and level of a voice are those of
        its geometry, where the "noise" model draws unrelated responses per channel.  The `drr_*` bounds are unused in this
        model: the direct-to-reverberant ratio follows from the geometry.  The direct sound of the nearest microphone sits at
        tap 16 (1 ms, far below one hop), so the dry labels stay valid.  At most 8 channels.
        max_taps (default 4096: everything above, bit for bit) in 4097 .. 32768 selects the LONG path: the tap buffers are
        [C, max_taps], `synth_rir` follows the decay up to max_taps, and `rereverb` runs the partitioned FFT convolution
        (`iris_fft_fir_batch`) over EVERY voice, short responses included - a mixer uses one engine, so its results do not
        depend on which voices drew short rooms.  The voices are split once, here, into consecutive groups whose spectra fit
        `workspace_budget` bytes at max_taps (one launch pair per group) and the workspace of the largest group is allocated
        once.  On this path the copies under the identity response equal the originals within the convolution's norm-wise
        rule, not bit for bit.  The shoebox model stops at 4096 taps and is refused on the long path.  With
        tails of a second, the policy above - a silent gap stays labelled silent although the room rings into it - matters
        more than it did at a quarter of a second.
        rirs: a list of measured responses [C, K <= max_taps] (`transforms.load_rirs`); a `rereverb()` without arguments then
        draws one of them per voice, uniformly, from the mixer's generator instead of synthesising."""
        _check_reverb_range(rt60_lo, rt60_hi, drr_lo, drr_hi)
        if model not in ("noise", "shoebox"):
            raise ValueError(f"enable_reverb: model = {model!r}; 'noise' (synth_rir) or 'shoebox' (image-source rooms)")
        max_taps = int(max_taps)
        if not _fe.FIR_MAX_TAPS <= max_taps <= _fe.FFT_FIR_MAX_TAPS:
            raise ValueError(f"enable_reverb: max_taps = {max_taps} is outside {_fe.FIR_MAX_TAPS} (the direct form) .. "
                             f"{_fe.FFT_FIR_MAX_TAPS} (the partitioned FFT convolution)")
        long_path = max_taps > _fe.FIR_MAX_TAPS
        if long_path and model == "shoebox":
            raise ValueError(f"enable_reverb: the shoebox model computes at most {_fe.FIR_MAX_TAPS} taps; max_taps = {max_taps} "
                             "needs model = 'noise' or measured responses")
        if rirs is not None:
            if model == "shoebox":
                raise ValueError("enable_reverb: measured responses (rirs=) replace the room model; drop model = 'shoebox'")
            rirs = [np.ascontiguousarray(np.asarray(h, np.float32)) for h in rirs]
            if not rirs:
                raise ValueError("enable_reverb: rirs is empty")
            for i, h in enumerate(rirs):
                if h.ndim != 2 or h.shape[0] != self.channels or not 1 <= h.shape[1] <= max_taps:
                    raise ValueError(f"enable_reverb: rirs[{i}] has shape {h.shape}; expected [{self.channels}, 1 <= K <= {max_taps}]")
        if self._aug is not None:
            raise RuntimeError("enable_reverb was already called on this mixer" if isinstance(self._aug, _ReverbAug) else
                               f"{_aug_name(self._aug)} was already called on this mixer (a mixer holds one voice augmentation)")
        dev, orig = self.device, list(self.voices)
        bufs = [torch.zeros_like(v) for v in orig]
        taps = [torch.zeros((self.channels, max_taps), device=dev, dtype=torch.float32) for _ in orig]
        table = np.zeros(len(orig), _fe.FFT_FIR_SRC if long_path else _fe.FIR_SRC)
        table["src"], table["dst"] = [v.data_ptr() for v in orig], [b.data_ptr() for b in bufs]
        table["taps"], table["len"] = [t.data_ptr() for t in taps], self._v_L
        self._aug = _ReverbAug((float(rt60_lo), float(rt60_hi)), (float(drr_lo), float(drr_hi)), orig, bufs, taps, table,
                               torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=dev), model=model,
                               max_taps=max_taps, pool=rirs)
        if long_path:
            # the groups and every voice's slice are laid out for max_taps: whatever response a voice draws later fits
            table["n_taps"] = max_taps
            self._aug.groups, largest = _fe.fft_fir_groups(table, self.channels, int(workspace_budget))
            self._aug.workspace = torch.empty(max(largest, 16), dtype=torch.uint8, device=dev)
        if model == "shoebox":
            if self.channels > _fe.ISM_MAX_CHAN:
                self._aug = None
                raise ValueError(f"enable_reverb: the shoebox model takes at most {_fe.ISM_MAX_CHAN} channels, not {self.channels}")
            self._aug.ism_table = np.zeros(len(orig), _fe.ISM_SRC)
            self._aug.ism_table["dst"] = [t.data_ptr() for t in taps]
            self._aug.ism_table_dev = torch.empty(max(self._aug.ism_table.nbytes, 1), dtype=torch.uint8, device=dev)
        self.voices = bufs
        self._v_ptr = np.array([b.data_ptr() for b in bufs], np.uint64)
        if self._dd is not None:
            self._dd["voice_arrays"]["src"].copy_(torch.from_numpy(self._v_ptr.astype(np.int64)))
        self.rereverb([np.ones((self.channels, 1), np.float32)] * len(orig))

    def rereverb(self, rirs=None) -> list:
        """Reverberate every ORIGINAL voice anew into its buffer: per voice rt60 ~ U[rt60_lo, rt60_hi) and drr_db ~
        U[drr_lo, drr_hi) from the mixer's own NumPy generator and a `transforms.synth_rir` of them (or the given `rirs`, one
        [C, K_i <= 4096] array per voice), uploaded into the resident tap buffers, then ONE `iris_fir_batch` launch over the
        whole voice corpus (on the long path of `enable_reverb(max_taps > 4096)`: K_i <= max_taps and one `iris_fft_fir_batch`
        launch pair per group of voices; with `enable_reverb(rirs=)` the responses are drawn from that list).  Lengths, frame counts and the frame-activity vectors (the labels) do not change: see
        `enable_reverb`.  Call it outside any graph capture.  Backgrounds and noises are not reverberated.  Returns the list
        of impulse responses used.
        Shoebox model with rirs = None: rt60 ~ U[rt60_lo, rt60_hi) and a `transforms.draw_shoebox` per voice from the mixer's
        generator (kept in `_aug.geometry`), then ONE `iris_ism_rir` launch into the resident tap buffers (rows 4096 apart) and
        ONE `iris_fir_batch_pitch` launch: two launches, no tap upload.  Returns the list of [C, K_i] device views of the tap
        buffers.  Given `rirs` work as in the noise model."""
        aug = self._aug
        if not isinstance(aug, _ReverbAug):
            raise RuntimeError("rereverb needs enable_reverb() first")
        n_voice, chan = len(aug.orig), self.channels
        if rirs is None and aug.model == "shoebox":
            geometry = []
            for _ in range(n_voice):
                rt60 = self.rng.uniform(*aug.rt60)
                geometry.append(dict(_tr.draw_shoebox(self.rng, chan, rt60, max_taps=_fe.FIR_MAX_TAPS), rt60=rt60))
            if n_voice:
                rec = _fe.shoebox_records([g["room"] for g in geometry], [g["source"] for g in geometry],
                                          [g["mics"] for g in geometry], [g["beta"] for g in geometry],
                                          [g["n_taps"] for g in geometry], _fe.FIR_MAX_TAPS)
                for f in ("room", "src", "beta", "n_taps", "mic"):
                    aug.ism_table[f] = rec[f]
                _fe.shoebox_rir_launch(aug.ism_table, chan, _fe.FIR_MAX_TAPS, self.device, aug.ism_table_dev)
                aug.table["n_taps"] = aug.ism_table["n_taps"]
                _fe.fir_pitch_launch(aug.table, chan, int(self._v_L.max()), int(aug.table["n_taps"].max()), _fe.FIR_MAX_TAPS,
                                     self.device, aug.table_dev)
            aug.geometry = geometry
            aug.rirs = [t[:, :int(k)] for t, k in zip(aug.taps, aug.ism_table["n_taps"])]
            return aug.rirs
        if rirs is None and aug.pool is not None:
            rirs = [aug.pool[int(i)] for i in self.rng.integers(0, len(aug.pool), n_voice)]
        if rirs is None:
            rirs = []
            for _ in range(n_voice):
                rt60, drr_db = self.rng.uniform(*aug.rt60), self.rng.uniform(*aug.drr)
                rirs.append(_tr.synth_rir(self.rng, chan, rt60, drr_db, max_taps=aug.max_taps))
        rirs = [np.ascontiguousarray(np.asarray(h, np.float32)) for h in rirs]
        if len(rirs) != n_voice:
            raise ValueError(f"rereverb: {len(rirs)} impulse responses for {n_voice} voices")
        for i, h in enumerate(rirs):
            if h.ndim != 2 or h.shape[0] != chan or not 1 <= h.shape[1] <= aug.max_taps:
                raise ValueError(f"rereverb: rirs[{i}] has shape {h.shape}; expected [{chan}, 1 <= K <= {aug.max_taps}]")
        for h, buf in zip(rirs, aug.taps):
            buf.view(-1)[:h.size].copy_(torch.from_numpy(h.reshape(-1)), non_blocking=True)
        aug.table["n_taps"] = [h.shape[1] for h in rirs]
        if aug.groups is not None:
            # the long path: every voice, short responses included, through the partitioned FFT convolution, group by group
            # (the groups' tables sit one after the other in the resident device table)
            for a, b in aug.groups:
                part = aug.table[a:b]
                _fe.fft_fir_launch(part, chan, int(part["len"].max()), int(part["n_taps"].max()), 0, aug.workspace, self.device,
                                   aug.table_dev[a * part.itemsize:b * part.itemsize])
        elif n_voice:
            _fe.fir_launch(aug.table, chan, int(self._v_L.max()), int(aug.table["n_taps"].max()), self.device, aug.table_dev)
        aug.rirs = rirs
        return rirs

    # -- fly-by of the voice corpus ---------------------------------------------------------
    def enable_flyby(self, **ranges) -> None:
        """Keep a copy of every voice as a moving microphone array hears it beside the original and mix from the copies:
        `reflyby()` then flies the array past every voice anew - one random level pass per voice (`transforms.draw_flyby`, whose
        keyword arguments `ranges` are: mic_spacing, altitude, speed, miss, z_s, beta) - in one launch (`iris_flyby`): per
        channel the time-varying delay of its microphone (Doppler shift, a moving inter-channel delay), the level that swells
        and fades with the distance, and one ground reflection.  The voices are taken to be sampled at 16 kHz.  One [C, L_i]
        buffer and one frame-activity vector per voice are allocated here and never move: the pointer tables (and the
        device-side corpus of `enable_device_draw`, in either call order) are switched to them once, so a captured `mix`
        replayed after a `reflyby` reads the new contents through unchanged addresses.  The copies are filled here through
        identity records: until the first `reflyby` the mixer mixes bit-identically to one on which this was never called.
        Lengths and frame counts do not move - what arrives later than a voice's buffer is cut, as the reverberation's tail
        is.  Backgrounds and noises are left alone: they carry no labels.  A mixer holds one voice augmentation: this after
        `enable_speed` / `enable_reverb` (or the other way round) raises.  At most 8 channels.  The ranges are choices, not
        measurements of any corpus; no accuracy claim is made for the augmentation."""
        _tr.draw_flyby(np.random.default_rng(0), self.channels, 1.0, **ranges)   # (the ranges are checked before the mixer is touched)
        if self._aug is not None:
            raise RuntimeError("enable_flyby was already called on this mixer" if isinstance(self._aug, _FlybyAug) else
                               f"{_aug_name(self._aug)} was already called on this mixer (a mixer holds one voice augmentation)")
        dev, orig = self.device, list(self.voices)
        bufs = [torch.zeros_like(v) for v in orig]
        acts = [torch.zeros_like(a) for a in self.voice_active]
        table = _fe.flyby_records([None] * len(orig), self._v_L, self.channels)
        table["src"], table["dst"] = [v.data_ptr() for v in orig], [b.data_ptr() for b in bufs]
        act_table = np.zeros(len(orig), _fe.SPEED_SRC)   # only dst / len_out are read by the activity pass
        act_table["dst"], act_table["len_out"] = table["dst"], self._v_L
        i64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)  # noqa: E731
        v_act = np.array([a.data_ptr() for a in acts], np.uint64)
        self._aug = _FlybyAug(dict(ranges), orig, bufs, acts, table, torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=dev),
                              torch.from_numpy(act_table.view(np.uint8).reshape(-1).copy()).to(dev), i64(v_act))
        self.voices, self.voice_active = bufs, acts
        self._v_ptr, self._v_act = np.array([b.data_ptr() for b in bufs], np.uint64), v_act
        if self._dd is not None:
            self._dd["voice_arrays"]["src"].copy_(torch.from_numpy(self._v_ptr.astype(np.int64)))
            self._dd["voice_arrays"]["act"].copy_(torch.from_numpy(self._v_act.astype(np.int64)))
        self.reflyby([None] * len(orig))

    def reflyby(self, geometry=None) -> list:
        """Fly the array past every ORIGINAL voice anew, into its buffer: one `transforms.draw_flyby` per voice from the mixer's
        own NumPy generator, over the voice's own duration (or the given `geometry`, one dict per voice; None: the identity),
        packed by `frontend.flyby_records` and uploaded into the resident table, then ONE `iris_flyby` launch over the whole
        voice corpus and ONE `iris_mix_wave_frame_active_batch` launch for the frame activity of the results: the labels follow
        the delayed voice, and a silent tail stays exactly zero.  Lengths, frame counts and addresses do not change.  Call it
        outside any graph capture.  Backgrounds and noises are left alone.  Returns the list of flights used."""
        aug = getattr(self, "_aug", None)
        if not isinstance(aug, _FlybyAug):
            raise RuntimeError("reflyby needs enable_flyby() first")
        n_voice, chan = len(aug.orig), self.channels
        if geometry is None:
            geometry = [_tr.draw_flyby(self.rng, chan, int(n) / _fe.FLYBY_FS, **aug.ranges) for n in self._v_L]
        geometry = list(geometry)
        if len(geometry) != n_voice:
            raise ValueError(f"reflyby: {len(geometry)} flights for {n_voice} voices")
        records = _fe.flyby_records(geometry, self._v_L, chan)
        for f in ("n_paths", "p0", "v", "z_s", "beta", "r_ref", "mic"):
            aug.table[f] = records[f]
        if n_voice:
            max_len = int(self._v_L.max())
            _fe.flyby_launch(aug.table, chan, max_len, self.device, aug.table_dev)
            with torch.cuda.device(self.device):
                rc = N.lib().iris_mix_wave_frame_active_batch(aug.act_table_dev.data_ptr(), n_voice, chan, self.n_fft, self.hop,
                                                              aug.act_ptr_dev.data_ptr(), 1 + max_len // self.hop,
                                                              C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            N.check(rc, "iris_mix_wave_frame_active_batch")
        aug.geometry = geometry
        return geometry

    def mix(self, batch: int, draws=None):
        """One batch of (waveforms [B, C, (n_frame - 1) * hop], labels [B, max_voices, n_frame, n_classes])."""
        table_d, first_d, n_srcs, batch, keep = self._batch_table(batch, draws)
        wav = torch.empty((batch, self.channels, (self.n_frame - 1) * self.hop), device=self.device, dtype=torch.float32)
        label = torch.empty((batch, self.max_voices, self.n_frame, self.n_classes), device=self.device, dtype=torch.float32)
        self._launch_mix("iris_mix_waves", n_srcs, keep, lambda ws, ws_floats, stream: N.lib().iris_mix_waves(
            table_d.data_ptr(), n_srcs, first_d.data_ptr(), self.label_vecs.data_ptr(), wav.data_ptr(), label.data_ptr(), batch,
            self.channels, self.hop, self.n_frame, self.max_voices, self.n_classes, ws, ws_floats, stream))
        return wav, label
