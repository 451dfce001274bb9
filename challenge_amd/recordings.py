"""Training windows from LABELLED RECORDINGS: wav files plus an answer JSON in `sample_answer.json`'s schema - what
`metrics.evaluate`, `python -m challenge_amd.eval` and `detect --score / --tune` already read - as a source of training batches.

    waves, events = load_recordings("recordings", "recordings/answer.json", device)
    sampler = RecordingSampler(waves, events, n_frame=512, hop=256, device=device, seed=0)
    sampler.enable_device_draw(seed=0)
    wav, y = sampler.sample(32)          # [32, C, 511 * 256], [32, 512, 3]: two launches, no host round trip

The recordings stay resident in ONE flat device buffer; `sample` draws B windows, every window of the corpus equally likely
(`iris_crop_draw`), and gathers them and their frame labels (`iris_crop_windows`).  `sj_train.make_wave_dataset(...,
recordings=sampler)` puts such windows in front of the synthetic samples of every training batch."""
from __future__ import annotations

import json
import os
from glob import glob
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import data_utils as _du
from . import frontend as _fe

_ROW_ALIGN = 64   # floats: every channel row starts on a 256-byte boundary


def events_to_frames(rows, n_frames: int, resolution: float = 16000 / 256, n_classes: int = 3) -> np.ndarray:
    """Answer rows [[class, start s, end s], ...] -> int32 [n, 3] of (class, start frame, end frame), end exclusive, with
    `eval.second2frame`'s own rounding `int(np.round(x * resolution))` and both ends clipped to [0, n_frames]: the table
    rasterised (`+= 1` over start:end of the class column) is `second2frame(rows, n_frames, resolution)`.  Rows that come out
    empty are dropped; a class outside [0, n_classes) is a ValueError.  n_frames of a file is 1 + samples // hop, the frame
    count `load_wav` gives it."""
    n_frames = int(n_frames)
    if n_frames < 0:
        raise ValueError(f"events_to_frames: n_frames = {n_frames} is negative")
    out = []
    for row in rows:
        if len(row) != 3:
            raise ValueError(f"events_to_frames: a row is [class, start s, end s], got {row!r}")
        k = int(row[0])
        if k != row[0] or not 0 <= k < n_classes:
            raise ValueError(f"events_to_frames: class {row[0]!r} is outside [0, {n_classes})")
        start = min(max(int(np.round(row[1] * resolution)), 0), n_frames)
        end = min(max(int(np.round(row[2] * resolution)), 0), n_frames)
        if start < end:
            out.append((k, start, end))
    return np.asarray(out, np.int32).reshape(-1, 3)


def load_recordings(wav_dir: str, answer_path: Optional[str] = None, device=None, sample_rate: int = 16000, hop: int = 256,
                    n_classes: int = 3):
    """(waves, events) of sorted(glob(wav_dir/*.wav)) for `RecordingSampler`: every file read by `data_utils.read_wav_file`,
    brought to `sample_rate` by `frontend.resample` and scaled by `data_utils.normalize` over the whole file - the
    wav / (10 rms) `load_wav` applies before evaluation, so training windows sit at the scale evaluation windows have - as
    [chan, samples] float32 tensors on `device`; its events from `task2_answer[name]` of the answer file (default
    wav_dir/answer.json; `name` = the file name without '.wav') as `events_to_frames` tables at sample_rate / hop frames per
    second.  A wav without an entry is a ValueError (an unlabelled recording would train as silence; an explicit [] is
    accepted); entries without a wav are ignored.  Everything that can be refused is refused before the device is touched."""
    answer_path = os.path.join(wav_dir, "answer.json") if answer_path is None else answer_path
    paths = sorted(glob(os.path.join(wav_dir, "*.wav")))
    if not paths:
        raise ValueError(f"load_recordings: no *.wav in {wav_dir!r}")
    with open(answer_path) as f:
        answer = json.load(f)["task2_answer"]
    missing = [os.path.basename(p) for p in paths if os.path.basename(p)[:-4] not in answer]
    if missing:
        raise ValueError(f"load_recordings: {answer_path!r} has no 'task2_answer' entry for {missing}: an unlabelled recording "
                         "would train as silence (give it an explicit [] if it has no events)")
    host, events = [], []
    for path in paths:
        data, sr = _du.read_wav_file(path)
        if data.shape[1] < 1:
            raise ValueError(f"load_recordings: {path!r} is empty")
        n = int(data.shape[1]) if sr == sample_rate else int(N.lib().iris_resample_len(int(data.shape[1]), int(sr), int(sample_rate)))
        try:
            events.append(events_to_frames(answer[os.path.basename(path)[:-4]], 1 + n // hop, sample_rate / hop, n_classes))
        except ValueError as exc:
            raise ValueError(f"load_recordings: {path!r}: {exc}") from None
        host.append((data, sr))
    if len({d.shape[0] for d, _ in host}) != 1:
        raise ValueError(f"load_recordings: the files of {wav_dir!r} differ in their channel counts")
    device = _du._default_device() if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_recordings needs a ROCm device (no CPU fallback)")
    waves = []
    for data, sr in host:
        wav = torch.from_numpy(data).to(device)
        if sr != sample_rate:
            wav = _fe.resample(wav, sr, sample_rate)
        waves.append(_du.normalize(wav))
    return waves, events


def _channels_of(waves) -> int:
    """The common channel count of [chan, samples] arrays / tensors (ValueError when they disagree or are not 2-D)."""
    shapes = [tuple(w.shape) for w in waves]
    if not shapes:
        raise ValueError("recordings: at least one recording is needed")
    if any(len(s) != 2 or s[1] < 1 for s in shapes) or len({s[0] for s in shapes}) != 1:
        raise ValueError("recordings: every recording must be [chan, samples >= 1] with equal chan")
    return int(shapes[0][0])


class RecordingSampler:
    """B random windows of a ragged set of labelled recordings, and their frame labels, as a batch on the device.

    waves: [chan, samples] float32 arrays or tensors with equal channel counts (1 or 2); events: per recording an integer
    [m, 3] table of (class, start frame, end frame) as `events_to_frames` gives it (frames of `hop` samples; an empty list
    for none).  The waveforms are copied into ONE flat device buffer (`storage`) in which every channel row starts on a
    256-byte boundary, so `iris_crop_windows` moves 16 bytes per lane whenever hop % 4 == 0; the event table, the record table
    (`frontend.CROP_REC`) and the int64 prefix sums of the position counts max((len - L) // hop, 0) + 1 are built once.  A
    recording shorter than a window has the one position 0; its tail comes out as zeros.

    `sample(batch, draws=None)` -> (wav [B, C, (n_frame - 1) * hop], y [B, n_frame, n_classes]).  `draws`: int32 [B, 2] of
    (recording, first frame), host or device; without them they come from the sampler's NumPy Generator (host, uploaded) or -
    after `enable_device_draw(seed)` - from `iris_crop_draw`: then a batch is two launches with no host synchronisation and no
    device-to-host copy.  The outputs (and `last_draws()`) are long-lived buffers that the next call of the same batch size
    overwrites, as the draws of `DeviceAugmentDraw` are: copy what must survive it."""

    def __init__(self, waves: Sequence, events: Sequence, n_frame: int, hop: int, n_classes: int = 3, device=None, seed=None):
        waves = list(waves)
        self.n_frame, self.hop, self.n_classes = int(n_frame), int(hop), int(n_classes)
        if self.n_frame < 2 or self.hop <= 0 or self.n_classes <= 0:
            raise ValueError(f"RecordingSampler: n_frame = {n_frame} must be at least 2, hop = {hop} and n_classes = {n_classes} positive")
        self.channels = _channels_of(waves)
        if self.channels not in (1, 2):
            raise ValueError(f"RecordingSampler: recordings have {self.channels} channels (1 or 2)")
        events = list(events)
        if len(events) != len(waves):
            raise ValueError(f"RecordingSampler: {len(waves)} recordings but {len(events)} event tables")
        tables = []
        for i, ev in enumerate(events):
            t = np.asarray(ev)
            if t.size and (t.ndim != 2 or t.shape[1] != 3 or not np.all(t == np.round(t))):
                raise ValueError(f"RecordingSampler: events[{i}] must be an integer [m, 3] table of (class, start frame, end frame)")
            t = t.astype(np.int64).reshape(-1, 3)
            if t.size and (t[:, 0].min() < 0 or t[:, 0].max() >= self.n_classes):
                raise ValueError(f"RecordingSampler: events[{i}] names a class outside [0, {self.n_classes})")
            tables.append(np.clip(t, -2**31, 2**31 - 1).astype(np.int32))
        self.length = (self.n_frame - 1) * self.hop
        lens = np.array([int(w.shape[1]) for w in waves], np.int64)
        if lens.max() > 2**31 - 1:
            raise ValueError("RecordingSampler: a recording has more than 2^31 - 1 samples per channel")
        self.lens = lens
        self.n_pos = np.maximum((lens - self.length) // self.hop, 0) + 1
        prefix = np.concatenate([[0], np.cumsum(self.n_pos)]).astype(np.int64)
        strides = (lens + _ROW_ALIGN - 1) // _ROW_ALIGN * _ROW_ALIGN
        offsets = np.concatenate([[0], np.cumsum(strides * self.channels)]).astype(np.int64)
        counts = np.array([len(t) for t in tables], np.int64)
        ev_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if ev_first[-1] > 2**31 - 1:
            raise ValueError("RecordingSampler: more than 2^31 - 1 events")
        table = np.concatenate(tables) if ev_first[-1] else np.zeros((1, 3), np.int32)   # (one unused row: a valid address)

        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("RecordingSampler needs a ROCm device (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RecordingSampler needs a ROCm device (no CPU fallback)")
        N.lib()
        self.storage = torch.zeros(int(offsets[-1]), dtype=torch.float32, device=self.device)
        for w, off, stride, n in zip(waves, offsets[:-1], strides, lens):
            w = w.detach() if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float32)))
            self.storage[int(off):int(off + self.channels * stride)].view(self.channels, int(stride))[:, :int(n)].copy_(w)
        self.recs = np.zeros(len(waves), _fe.CROP_REC)
        self.recs["base"] = self.storage.data_ptr() + 4 * offsets[:-1]
        self.recs["row_stride"], self.recs["len"] = strides, lens
        self.recs["ev_first"], self.recs["ev_count"] = ev_first[:-1], counts
        self._recs_dev = torch.from_numpy(self.recs.view(np.uint8).reshape(-1).copy()).to(self.device)
        self.events = torch.from_numpy(table).to(self.device)
        self._prefix_host = prefix
        self.prefix = torch.from_numpy(prefix).to(self.device)
        self.rng = np.random.default_rng(seed)
        self._dd = None
        self._bufs = {}
        self._last = None

    def __len__(self) -> int:
        return len(self.recs)

    @property
    def n_windows(self) -> int:
        """Window positions of the whole corpus (what a draw is uniform over)."""
        return int(self._prefix_host[-1])

    def enable_device_draw(self, seed: int = 0) -> None:
        """Draw every later `sample(batch)` ON THE DEVICE (`iris_crop_draw`): Philox keyed by `seed`, the call counter in a
        device word of this sampler's own, so a captured `sample` replays with fresh draws."""
        self._dd = {"seed": int(seed) & 0xFFFFFFFFFFFFFFFF, "state": torch.zeros(1, dtype=torch.int64, device=self.device)}

    def draw(self, batch: int) -> np.ndarray:
        """Host draws int32 [batch, 2] from the sampler's NumPy Generator: a uniform window index, then (recording, frame)."""
        u = self.rng.integers(0, self.n_windows, size=int(batch), dtype=np.int64)
        i = np.searchsorted(self._prefix_host, u, side="right") - 1
        return np.stack([i, u - self._prefix_host[i]], axis=1).astype(np.int32)

    def sample(self, batch: int, draws=None):
        batch = int(batch)
        if batch not in self._bufs:   # long-lived: a captured graph keeps their addresses
            self._bufs[batch] = (torch.zeros((batch, 2), dtype=torch.int32, device=self.device),
                                 torch.empty((batch, self.channels, self.length), dtype=torch.float32, device=self.device),
                                 torch.empty((batch, self.n_frame, self.n_classes), dtype=torch.float32, device=self.device))
        d, wav, y = self._bufs[batch]
        if draws is None and self._dd is not None:
            _fe.crop_draw(self.prefix, batch, self._dd["seed"], self._dd["state"], out=d)
        else:
            if draws is None:
                draws = self.draw(batch)
            if isinstance(draws, torch.Tensor) and draws.is_cuda:
                if tuple(draws.shape) != (batch, 2) or draws.dtype != torch.int32:
                    raise ValueError(f"RecordingSampler.sample: draws must be int32 [batch = {batch}, 2]")
            else:
                host = np.asarray(draws.cpu() if isinstance(draws, torch.Tensor) else draws)
                if host.shape != (batch, 2) or not np.issubdtype(host.dtype, np.integer):
                    raise ValueError(f"RecordingSampler.sample: draws must be an integer [batch = {batch}, 2] array")
                if batch and (host[:, 0].min() < 0 or host[:, 0].max() >= len(self) or host[:, 1].min() < 0 or
                              np.any(host[:, 1] >= self.n_pos[host[:, 0]])):
                    raise ValueError("RecordingSampler.sample: a draw names no window (recording outside the corpus, or a first "
                                     "frame beyond its positions)")
                draws = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32)))
            d.copy_(draws)
        self._last = d
        return _fe.crop_windows(self._recs_dev, self.events, d, self.channels, self.hop, self.n_frame, self.n_classes, out=(wav, y))

    def last_draws(self) -> torch.Tensor:
        """The device tensor int32 [B, 2] of the latest `sample`'s draws (long-lived: the next call of that batch size
        overwrites it)."""
        if self._last is None:
            raise RuntimeError("RecordingSampler.last_draws: nothing has been sampled yet")
        return self._last
