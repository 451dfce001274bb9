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
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import pipeline as _pl

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


def check_stretch_range(lo: float, hi: float) -> None:
    """The rate range of `DeviceMixer.enable_stretch`: finite, 0 < lo <= hi."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"stretch rates must satisfy 0 < lo <= hi (finite), got lo = {lo}, hi = {hi}")


def stretch_rates(rng: np.random.Generator, n: int, lo: float = 0.8, hi: float = 1.2) -> np.ndarray:
    """The random half of `DeviceMixer.restretch`: n rates ~ U[lo, hi) (float64) from `rng`."""
    check_stretch_range(lo, hi)
    return rng.uniform(float(lo), float(hi), size=int(n))


def check_speed_range(lo: float, hi: float) -> None:
    """The rate range of `WaveMixer.enable_speed`: finite, 0 < lo <= hi."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"speed rates must satisfy 0 < lo <= hi (finite), got lo = {lo}, hi = {hi}")


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

    def __init__(self, backgrounds: Sequence, voices: Sequence, labels, noises: Optional[Sequence] = None,
                 n_frame: int = 300, max_voices: int = 10, max_noises: int = 10, n_classes: int = 3, device=None,
                 min_ratio: float = 2 / 3, min_noise_ratio: float = 1 / 2, snr: float = -20, seed=None):
        labels = np.asarray(labels, np.float32)
        assert len(np.asarray(backgrounds[0]).shape) == 3, 'each spec must be a 3D-tensor'
        assert len(voices) == len(labels)
        assert labels.ndim == 2 and labels.shape[1] == n_classes, \
            'labels must be in the form of [n_samples, n_classes]'
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("DeviceMixer needs a ROCm device (no CPU fallback); use pipeline.make_pipeline")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceMixer needs a ROCm device (no CPU fallback); use pipeline.make_pipeline")
        N.lib()  # fail loudly when the HIP library is missing
        self.n_frame, self.max_voices, self.max_noises, self.n_classes = n_frame, max_voices, max_noises, n_classes
        self.min_ratio, self.min_noise_ratio, self.snr = min_ratio, min_noise_ratio, snr
        self.rng = np.random.default_rng(seed)

        def upload(items):
            out = [torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32))).to(self.device) for x in items]
            for t in out:
                if t.dim() != 3 or t.shape[0] != out[0].shape[0] or t.shape[2] != out[0].shape[2]:
                    raise ValueError("sources must be [freq, time, chan2] with equal freq and chan2")
            return out

        self.backgrounds, self.voices = upload(backgrounds), upload(voices)
        self.noises = upload(noises) if noises is not None else None
        self.n_bins, self.chan2 = int(self.backgrounds[0].shape[0]), int(self.backgrounds[0].shape[2])
        for group in (self.voices, self.noises or []):
            for t in group:
                if t.shape[0] != self.n_bins or t.shape[2] != self.chan2:
                    raise ValueError("voices / noises must share the backgrounds' freq and chan2 sizes")
        self.label_vecs = torch.from_numpy(labels).to(self.device)
        # which frames of a voice are active (max over freq, chan2 > 0; pipeline.py:57) is a property of
        # the source: one pass over the corpus now instead of one per use
        self.voice_active = []
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for v in self.voices:
                act = torch.empty(int(v.shape[1]), device=self.device, dtype=torch.float32)
                N.check(N.lib().iris_mix_frame_active(v.data_ptr(), self.n_bins, int(v.shape[1]), self.chan2,
                                                      act.data_ptr(), stream), "iris_mix_frame_active")
                self.voice_active.append(act)
        # pointer / frame-count lookup tables of every source, indexed per batch when its table is built
        self._bg_ptr = np.array([t.data_ptr() for t in self.backgrounds], np.uint64)
        self._bg_T = np.array([int(t.shape[1]) for t in self.backgrounds], np.int64)
        self._v_ptr = np.array([t.data_ptr() for t in self.voices], np.uint64)
        self._v_act = np.array([a.data_ptr() for a in self.voice_active], np.uint64)
        self._v_T = np.array([int(t.shape[1]) for t in self.voices], np.int64)
        self._n_ptr = np.array([t.data_ptr() for t in self.noises], np.uint64) if self.noises is not None else None
        self._n_T = np.array([int(t.shape[1]) for t in self.noises], np.int64) if self.noises is not None else None
        self._b = _Stream(len(self.backgrounds), self.rng)
        self._v = _Stream(len(self.voices), self.rng)
        self._n = _Stream(len(self.noises), self.rng) if self.noises is not None else None

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
        if getattr(self, "_bg_L", None) is not None:  # waveform sources (WaveMixer): samples per channel
            full["reserved"][:, 0] = self._bg_L[d.bg]
            full["reserved"][:, 1:1 + V] = self._v_L[d.voices]
            if Nn:
                full["reserved"][:, 1 + V:] = self._n_L[d.noises]
        first = np.concatenate([[0], np.cumsum(use.sum(axis=1))]).astype(np.int32)
        return np.ascontiguousarray(full[use]), first

    def mix(self, batch: int, draws=None):
        """One batch of (complex spectrogram [B, F, n_frame, 2C], labels [B, max_voices, n_frame,
        n_classes]) - `merge_complex_specs` (pipeline.py:6-110) for every sample, two launches.
        draws: a BatchDraw or a list of per-sample dicts (default: a fresh `draw_arrays(batch)`)."""
        dev = self.device
        on_device = draws is None and getattr(self, "_dd", None) is not None
        if on_device:
            table_d, first_d, n_srcs = self._draw_on_device(batch)
        else:
            draws = self.draw_arrays(batch) if draws is None else draws
            batch = len(draws)
            table, first = self.table(draws)
            n_srcs = int(table.shape[0])
            table_d = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev, non_blocking=True)
            first_d = torch.from_numpy(first).to(dev, non_blocking=True)
        spec = torch.empty((batch, self.n_bins, self.n_frame, self.chan2), device=dev, dtype=torch.float32)
        label = torch.empty((batch, self.max_voices, self.n_frame, self.n_classes), device=dev, dtype=torch.float32)
        ws_floats = int(N.lib().iris_mix_workspace(n_srcs, self.n_frame))
        ws = torch.empty(max(ws_floats, 1), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = N.lib().iris_mix_specs(table_d.data_ptr(), n_srcs, first_d.data_ptr(), self.label_vecs.data_ptr(),
                                        spec.data_ptr(), label.data_ptr(), batch, self.n_bins, self.n_frame,
                                        self.chan2, self.max_voices, self.n_classes, ws.data_ptr(), ws_floats,
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        N.check(rc, "iris_mix_specs")
        # the table, ranges and workspace must outlive the kernels: tie them to the stream
        for t in ((ws,) if on_device else (table_d, first_d, ws)):
            t.record_stream(torch.cuda.current_stream(dev))
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
        wave = getattr(self, "_bg_L", None) is not None
        self._dd["bg"] = corpus(self._bg_ptr, None, self._bg_T, self._bg_L if wave else None)
        self._dd["voice"] = corpus(self._v_ptr, self._v_act, self._v_T, self._v_L if wave else None)
        self._dd["noise"] = corpus(self._n_ptr, None, self._n_T, self._n_L if wave else None) if self.noises is not None else None
        self._dd["voice_arrays"] = self._dd["keep"][1]   # `restretch` rewrites the voices' T (and, once, src / act) in place

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
        check_stretch_range(lo, hi)
        if getattr(self, "_st", None) is not None:
            raise RuntimeError("enable_stretch was already called on this mixer")
        from . import frontend as _fe
        orig, orig_T = list(self.voices), self._v_T.copy()
        cap = np.array([_fe.stretched_frames(int(t), lo) for t in orig_T], np.int64)
        row = self.n_bins * self.chan2
        bufs = [torch.zeros(int(c) * row, device=self.device, dtype=torch.float32) for c in cap]
        acts = [torch.zeros(int(c), device=self.device, dtype=torch.float32) for c in cap]
        table = np.zeros(len(orig), _fe.VOC_SRC)
        table["src"], table["dst"] = [t.data_ptr() for t in orig], [b.data_ptr() for b in bufs]
        table["n_in"] = orig_T
        self._st = {"lo": float(lo), "hi": float(hi), "orig": orig, "orig_T": orig_T, "cap": cap, "bufs": bufs, "acts": acts,
                    "table": table, "rates": None,
                    "table_dev": torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=self.device)}
        self.voice_active = acts
        self._v_ptr = np.array([b.data_ptr() for b in bufs], np.uint64)
        self._v_act = np.array([a.data_ptr() for a in acts], np.uint64)
        dd = getattr(self, "_dd", None)
        if dd is not None:
            dd["voice_arrays"]["src"].copy_(torch.from_numpy(self._v_ptr.astype(np.int64)))
            dd["voice_arrays"]["act"].copy_(torch.from_numpy(self._v_act.astype(np.int64)))
        self.restretch(np.ones(len(orig)))

    def restretch(self, rates=None) -> np.ndarray:
        """Stretch every ORIGINAL voice anew into its buffer: rate_i ~ U[lo, hi) from the mixer's own NumPy generator
        (or the given `rates`, one per voice, each >= lo so that the result fits its buffer), ONE `iris_phase_vocoder`
        launch over the whole voice corpus, then every voice's frame activity recomputed from the stretched voice
        (`iris_mix_frame_active`: the labels follow from `max(voice) > 0`, as in the reference).  The voices' frame counts
        change to ceil(T_i / rate_i), on the host (`_v_T`) and in place in the device corpus of `enable_device_draw`.  Call
        it outside any graph capture.  Backgrounds and noises are not stretched.  Returns the rates used."""
        st = getattr(self, "_st", None)
        if st is None:
            raise RuntimeError("restretch needs enable_stretch() first")
        from . import frontend as _fe
        n_voice = len(st["orig"])
        if rates is None:
            rates = stretch_rates(self.rng, n_voice, st["lo"], st["hi"])
        rates = np.asarray(rates, np.float64).reshape(-1)
        if rates.shape[0] != n_voice:
            raise ValueError(f"restretch: {rates.shape[0]} rates for {n_voice} voices")
        n_out = np.array([_fe.stretched_frames(int(t), r) for t, r in zip(st["orig_T"], rates)], np.int64)
        if np.any(n_out > st["cap"]):
            i = int(np.argmax(n_out > st["cap"]))
            raise ValueError(f"restretch: voice {i} at rate {rates[i]} needs {n_out[i]} frames but its buffer holds "
                             f"{st['cap'][i]} (rates below lo = {st['lo']} do not fit)")
        table = st["table"]
        table["n_out"], table["rate"] = n_out, rates
        _fe.phase_vocoder_launch(table, self.n_bins, self.chan2, int(st["cap"].max()), self.device, st["table_dev"])
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for buf, act, n in zip(st["bufs"], st["acts"], n_out):
                N.check(N.lib().iris_mix_frame_active(buf.data_ptr(), self.n_bins, int(n), self.chan2, act.data_ptr(), stream),
                        "iris_mix_frame_active")
        self._v_T = n_out
        self.voices = [b[:self.n_bins * int(n) * self.chan2].view(self.n_bins, int(n), self.chan2)
                       for b, n in zip(st["bufs"], n_out)]
        dd = getattr(self, "_dd", None)
        if dd is not None:
            dd["voice_arrays"]["T"].copy_(torch.from_numpy(n_out.astype(np.int32)))
        st["rates"] = rates.copy()
        return st["rates"]

    def enable_speed(self, lo: float = 0.9, hi: float = 1.1) -> None:
        raise NotImplementedError("DeviceMixer.enable_speed: a spectrum corpus cannot be resampled in time (speed perturbation "
                                  "works on waveforms: use WaveMixer; this corpus has enable_stretch)")

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

    def __init__(self, backgrounds: Sequence, voices: Sequence, labels, noises: Optional[Sequence] = None,
                 n_frame: int = 300, n_fft: int = 1024, hop: int = 256, max_voices: int = 10, max_noises: int = 10,
                 n_classes: int = 3, device=None, min_ratio: float = 2 / 3, min_noise_ratio: float = 1 / 2,
                 snr: float = -20, seed=None):
        labels = np.asarray(labels, np.float32)
        assert len(backgrounds[0].shape if isinstance(backgrounds[0], torch.Tensor) else np.asarray(backgrounds[0]).shape) == 2, 'each waveform must be [chan, samples]'
        assert len(voices) == len(labels)
        assert labels.ndim == 2 and labels.shape[1] == n_classes, \
            'labels must be in the form of [n_samples, n_classes]'
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("WaveMixer needs a ROCm device (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("WaveMixer needs a ROCm device (no CPU fallback)")
        N.lib()
        self.n_frame, self.max_voices, self.max_noises, self.n_classes = n_frame, max_voices, max_noises, n_classes
        self.n_fft, self.hop = n_fft, hop
        self.min_ratio, self.min_noise_ratio, self.snr = min_ratio, min_noise_ratio, snr
        self.rng = np.random.default_rng(seed)

        def upload(items):
            # (a float32 tensor - e.g. a waveform `sj_train.waves_from_specs` left on the device - is taken as it is)
            out = [x.detach().to(self.device, torch.float32).contiguous() if isinstance(x, torch.Tensor)
                   else torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32))).to(self.device) for x in items]
            for t in out:
                if t.dim() != 2 or t.shape[0] != out[0].shape[0] or t.shape[1] < 1:
                    raise ValueError("sources must be [chan, samples] with equal chan")
            return out

        self.backgrounds, self.voices = upload(backgrounds), upload(voices)
        self.noises = upload(noises) if noises is not None else None
        self.channels = int(self.backgrounds[0].shape[0])
        for group in (self.voices, self.noises or []):
            for t in group:
                if t.shape[0] != self.channels:
                    raise ValueError("voices / noises must have the backgrounds' channel count")
        self.label_vecs = torch.from_numpy(labels).to(self.device)
        frames = lambda t: 1 + int(t.shape[1]) // hop  # noqa: E731
        self.voice_active = []
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for v in self.voices:
                act = torch.empty(frames(v), device=self.device, dtype=torch.float32)
                N.check(N.lib().iris_mix_wave_frame_active(v.data_ptr(), self.channels, int(v.shape[1]), n_fft, hop,
                                                           act.data_ptr(), stream), "iris_mix_wave_frame_active")
                self.voice_active.append(act)
        ptrs = lambda ts: np.array([t.data_ptr() for t in ts], np.uint64)  # noqa: E731
        lens = lambda ts: np.array([int(t.shape[1]) for t in ts], np.int64)  # noqa: E731
        self._bg_ptr, self._bg_L = ptrs(self.backgrounds), lens(self.backgrounds)
        self._v_ptr, self._v_L = ptrs(self.voices), lens(self.voices)
        self._v_act = ptrs(self.voice_active)
        self._n_ptr = ptrs(self.noises) if self.noises is not None else None
        self._n_L = lens(self.noises) if self.noises is not None else None
        self._bg_T, self._v_T = 1 + self._bg_L // hop, 1 + self._v_L // hop
        self._n_T = 1 + self._n_L // hop if self.noises is not None else None
        self._b = _Stream(len(self.backgrounds), self.rng)
        self._v = _Stream(len(self.voices), self.rng)
        self._n = _Stream(len(self.noises), self.rng) if self.noises is not None else None

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
        check_speed_range(lo, hi)
        if getattr(self, "_sp", None) is not None:
            raise RuntimeError("enable_speed was already called on this mixer")
        from . import frontend as _fe
        orig, orig_L = list(self.voices), self._v_L.copy()
        cap = np.array([_fe.speed_len(int(n), lo) for n in orig_L], np.int64)
        if cap.max() > 2 ** 31 - 1:
            raise ValueError(f"enable_speed: a voice at rate {lo} would have {cap.max()} samples (> 2^31 - 1)")
        bufs = [torch.zeros(self.channels * int(c), device=self.device, dtype=torch.float32) for c in cap]
        acts = [torch.zeros(1 + int(c) // self.hop, device=self.device, dtype=torch.float32) for c in cap]
        table = np.zeros(len(orig), _fe.SPEED_SRC)
        table["src"], table["dst"] = [t.data_ptr() for t in orig], [b.data_ptr() for b in bufs]
        table["len_in"] = orig_L
        act_ptr = np.array([a.data_ptr() for a in acts], np.uint64)
        self._sp = {"lo": float(lo), "hi": float(hi), "orig": orig, "orig_L": orig_L, "cap": cap, "bufs": bufs, "acts": acts,
                    "table": table, "rates": None,
                    "table_dev": torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=self.device),
                    "act_ptr_dev": torch.from_numpy(act_ptr.astype(np.int64)).to(self.device)}
        self.voice_active = acts
        self._v_ptr = np.array([b.data_ptr() for b in bufs], np.uint64)
        self._v_act = act_ptr
        dd = getattr(self, "_dd", None)
        if dd is not None:
            dd["voice_arrays"]["src"].copy_(torch.from_numpy(self._v_ptr.astype(np.int64)))
            dd["voice_arrays"]["act"].copy_(torch.from_numpy(self._v_act.astype(np.int64)))
        self.respeed(np.ones(len(orig)))

    def respeed(self, rates=None) -> np.ndarray:
        """Resample every ORIGINAL voice anew into its buffer: rate_i ~ U[lo, hi) from the mixer's own NumPy generator (or the
        given `rates`, one per voice, each >= lo so that the result fits its buffer), ONE `iris_speed_perturb` launch over the
        whole voice corpus and ONE `iris_mix_wave_frame_active_batch` launch for the frame activity of the results (the labels
        follow the perturbed voice; a silent tail stays exactly zero).  The voices' lengths change to L' = ceil(L_i / rate_i)
        and their frame counts to 1 + L' // hop, on the host (`_v_L`, `_v_T`, `voices`) and in place in the device corpus of
        `enable_device_draw`.  Call it outside any graph capture.  Backgrounds and noises are not perturbed.  Returns the rates
        used."""
        sp = getattr(self, "_sp", None)
        if sp is None:
            raise RuntimeError("respeed needs enable_speed() first")
        from . import frontend as _fe
        n_voice = len(sp["orig"])
        if rates is None:
            rates = stretch_rates(self.rng, n_voice, sp["lo"], sp["hi"])
        rates = np.asarray(rates, np.float64).reshape(-1)
        if rates.shape[0] != n_voice:
            raise ValueError(f"respeed: {rates.shape[0]} rates for {n_voice} voices")
        n_out = np.array([_fe.speed_len(int(n), r) for n, r in zip(sp["orig_L"], rates)], np.int64)
        if np.any(n_out > sp["cap"]):
            i = int(np.argmax(n_out > sp["cap"]))
            raise ValueError(f"respeed: voice {i} at rate {rates[i]} needs {n_out[i]} samples but its buffer holds "
                             f"{sp['cap'][i]} (rates below lo = {sp['lo']} do not fit)")
        table = sp["table"]
        table["len_out"], table["rate"] = n_out, rates
        table_dev = _fe.speed_perturb_launch(table, self.channels, int(sp["cap"].max()), self.device, sp["table_dev"])
        with torch.cuda.device(self.device):
            rc = N.lib().iris_mix_wave_frame_active_batch(table_dev.data_ptr(), n_voice, self.channels, self.n_fft, self.hop,
                                                          sp["act_ptr_dev"].data_ptr(), 1 + int(sp["cap"].max()) // self.hop,
                                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        N.check(rc, "iris_mix_wave_frame_active_batch")
        self._v_L, self._v_T = n_out, 1 + n_out // self.hop
        self.voices = [b[:self.channels * int(n)].view(self.channels, int(n)) for b, n in zip(sp["bufs"], n_out)]
        dd = getattr(self, "_dd", None)
        if dd is not None:
            dd["voice_arrays"]["T"].copy_(torch.from_numpy(self._v_T.astype(np.int32)))
            dd["voice_arrays"]["len"].copy_(torch.from_numpy(n_out.astype(np.int32)))
        sp["rates"] = rates.copy()
        return sp["rates"]

    def mix(self, batch: int, draws=None):
        """One batch of (waveforms [B, C, (n_frame - 1) * hop], labels [B, max_voices, n_frame, n_classes])."""
        dev = self.device
        on_device = draws is None and getattr(self, "_dd", None) is not None
        if on_device:
            table_d, first_d, n_srcs = self._draw_on_device(batch)
        else:
            draws = self.draw_arrays(batch) if draws is None else draws
            batch = len(draws)
            table, first = self.table(draws)
            n_srcs = int(table.shape[0])
            table_d = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev, non_blocking=True)
            first_d = torch.from_numpy(first).to(dev, non_blocking=True)
        wav = torch.empty((batch, self.channels, (self.n_frame - 1) * self.hop), device=dev, dtype=torch.float32)
        label = torch.empty((batch, self.max_voices, self.n_frame, self.n_classes), device=dev, dtype=torch.float32)
        ws_floats = int(N.lib().iris_mix_workspace(n_srcs, self.n_frame))
        ws = torch.empty(max(ws_floats, 1), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = N.lib().iris_mix_waves(table_d.data_ptr(), n_srcs, first_d.data_ptr(), self.label_vecs.data_ptr(),
                                        wav.data_ptr(), label.data_ptr(), batch, self.channels, self.hop, self.n_frame,
                                        self.max_voices, self.n_classes, ws.data_ptr(), ws_floats,
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        N.check(rc, "iris_mix_waves")
        for t in ((ws,) if on_device else (table_d, first_d, ws)):
            t.record_stream(torch.cuda.current_stream(dev))
        return wav, label
