"""Event detection on recordings without labels, and the challenge's answer file.

    python -m challenge_amd.detect --name <run name> [--p] [--path DIR] [--wav_dir .] [--out answer.json]
                                   [--overlap_hop 512] [--score ANSWER.json]

`detect` runs a trained model over wav files (or in-memory recordings) and returns, per file, the events it finds in the
forms of the reference's helpers: frame events (Challenge_Metric.get_start_end_frame), the (class, middle second) rows
`get_er` scores (output_to_metric) and the (class, start s, end s) rows of the answer (Challenge_Metric.get_start_end_time).
`write_answer` writes them as {"task2_answer": {name: [[class, start_s, end_s], ...]}}, the schema of sample_answer.json.

The front end is metrics.evaluate's (data_utils.load_wav, inference.features_for_eval: per-file min-max over the whole
recording).  The windows of all files of a group are cut with inference.frame, stacked and run through `model.predict` in
batches that cross file boundaries; `decode_events` then turns every window prediction of the group into events in one
call: on GPU tensors the iris_decode_events launches (csrc/k_detect.h) and one copy back, on CPU tensors the restatement
below, which follows the kernel's arithmetic bit for bit:
  1. p[t]: overlap-add average - fp32 sum from 0 over the covering windows in ascending order, / (float) count
  2. a[t]: AveragePooling1D(31, 1, 'same') - fp32 sum of the in-range p in frame order, / (float) frames in range
  3. d[t]: MaxPooling1D(124, 1, 'same') then >= 0.5, as "some a[u] >= 0.5 in the window and no NaN a[u]"
  4. the maximal runs of d as (first, last) frames.
inference.predict_frames computes the same function with torch ops whose fp32 rounding differs in the last bits (the
overlap-add's index_add_ order, avg_pool1d's sum / 31 * 31 / n): the two agree wherever no a[t] sits within rounding of
the threshold."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from glob import glob
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import data_utils as D
from . import metrics as M
from .inference import features_for_eval, frame

SR, HOP = 16000, 256
AVG_POOL = int(0.5 * SR) // HOP     # metrics.py:76-78: 31 frames
MAX_POOL = 4 * AVG_POOL             # 124 frames
THRESHOLD = 0.5
MAX_K = 16


def _check(preds_shape, win_off: np.ndarray, frame_lens: np.ndarray, n_frame: int, overlap_hop: int, avg_pool: int,
           max_pool: int) -> None:
    if len(preds_shape) != 3:
        raise ValueError(f"decode_events: preds must be [windows, n_out, K], got {tuple(preds_shape)}")
    n_win, n_out, k = preds_shape
    f = len(frame_lens)
    if f < 1 or win_off.shape != (f + 1,):
        raise ValueError(f"decode_events: {f} files need {f + 1} window offsets, got {win_off.shape}")
    if n_frame < 1 or overlap_hop < 1 or n_out < 1 or k < 1:
        raise ValueError(f"decode_events: n_frame {n_frame}, overlap_hop {overlap_hop}, preds {tuple(preds_shape)}")
    if overlap_hop > n_frame:
        raise ValueError(f"decode_events: overlap_hop {overlap_hop} > n_frame {n_frame} leaves frames no window covers")
    if n_frame % n_out != 0:
        raise ValueError(f"decode_events: n_frame {n_frame} is not a multiple of the model's {n_out} output frames")
    if k > MAX_K:
        raise ValueError(f"decode_events: {k} classes (at most {MAX_K})")
    if not (1 <= avg_pool <= 127 and 1 <= max_pool <= 256):
        raise ValueError(f"decode_events: avg_pool {avg_pool} (1..127), max_pool {max_pool} (1..256)")
    nwin = np.diff(win_off)
    if win_off[0] < 0 or (nwin < 0).any() or (frame_lens < 0).any() or win_off[-1] > n_win:
        raise ValueError(f"decode_events: window offsets {win_off.tolist()} / frame lengths {frame_lens.tolist()} do not fit "
                         f"{n_win} windows")
    bad = np.flatnonzero((frame_lens > 0) & (frame_lens > (nwin - 1) * overlap_hop + n_frame))
    if bad.size:
        f0 = int(bad[0])
        raise ValueError(f"decode_events: file {f0}: {int(frame_lens[f0])} frames > ({int(nwin[f0])} - 1) * {overlap_hop} + "
                         f"{n_frame}: frames no window covers")


def _pairs(frame_lens: np.ndarray) -> np.ndarray:
    return (frame_lens + 1) // 2 + 1      # event capacity of one (file, class): ceil(T / 2) + 1


def _decode_file_host(preds: torch.Tensor, w0: int, n_win: int, t_len: int, n_frame: int, hop: int, avg_pool: int,
                      max_pool: int, threshold: float) -> Tuple[np.ndarray, ...]:
    """Steps 1-4 for one file on CPU fp32 tensors, in the kernel's order."""
    n_out, k = preds.shape[1], preds.shape[2]
    if t_len == 0:
        return tuple(np.zeros((0, 2), np.int64) for _ in range(k))
    up = n_frame // n_out
    t = torch.arange(t_len)
    w_hi = torch.clamp(t // hop, max=n_win - 1)
    w_lo = torch.where(t >= n_frame, torch.div(t - n_frame, hop, rounding_mode='floor') + 1, torch.zeros_like(t))
    s = torch.zeros(t_len, k, dtype=torch.float32)
    for r in range(int((w_hi - w_lo).max()) + 1):   # the r-th covering window of every frame: ascending w
        w = w_lo + r
        ok = w <= w_hi
        w = torch.where(ok, w, w_lo)
        v = preds[w0 + w, torch.div(t - w * hop, up, rounding_mode='floor')]
        s = s + torch.where(ok[:, None], v, torch.zeros((), dtype=torch.float32))   # (+0 is exact: s is never -0)
    p = s / (w_hi - w_lo + 1).to(torch.float32)[:, None]
    al, ar = (avg_pool - 1) // 2, avg_pool - 1 - ((avg_pool - 1) // 2)
    pp = torch.nn.functional.pad(p.t(), (al, ar)).t()
    acc = torch.zeros(t_len, k, dtype=torch.float32)
    for j in range(avg_pool):                         # frame order; the zero padding adds exactly nothing
        acc = acc + pp[j:j + t_len]
    n = (torch.clamp(t + ar, max=t_len - 1) - torch.clamp(t - al, min=0) + 1).to(torch.float32)
    a = acc / n[:, None]
    ml, mr = (max_pool - 1) // 2, max_pool - 1 - ((max_pool - 1) // 2)
    on = (a >= threshold).numpy()
    isn = torch.isnan(a).numpy()
    lo = np.clip(np.arange(t_len) - ml, 0, t_len)
    hi = np.clip(np.arange(t_len) + mr + 1, 0, t_len)
    out = []
    for c in range(k):
        c_on = np.concatenate([[0], np.cumsum(on[:, c], dtype=np.int64)])
        c_nan = np.concatenate([[0], np.cumsum(isn[:, c], dtype=np.int64)])
        d = ((c_on[hi] - c_on[lo]) > 0) & ((c_nan[hi] - c_nan[lo]) == 0)
        e = np.diff(np.concatenate([[0], d.astype(np.int8), [0]]))
        out.append(np.stack([np.flatnonzero(e == 1), np.flatnonzero(e == -1) - 1], 1).astype(np.int64))
    return tuple(out)


class DecodeLayout:
    """Host-side layout of one iris_decode_events call: `meta` = int32 [win_off (F + 1), frame_len (F)] (uploaded once), and
    the output buffer `out` = int32 [n_ev (F K), ev (2 pairs)] with (file f, class k) at pair K sum_{g<f} cap_g + k cap_f."""

    def __init__(self, win_off, frame_lens, n_classes: int):
        self.win_off = np.ascontiguousarray(np.asarray(win_off, dtype=np.int64)).astype(np.int32)
        self.frame_lens = np.ascontiguousarray(np.asarray(frame_lens, dtype=np.int64)).astype(np.int32)
        self.k = int(n_classes)
        f = len(self.frame_lens)
        cap = _pairs(self.frame_lens.astype(np.int64))
        self.cap = cap
        self.pair_base = self.k * np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)
        self.n_words = int(self.k * ((self.frame_lens.astype(np.int64) + 63) // 64).sum())
        self.n_pairs = int(self.k * cap.sum())
        self.out_len = f * self.k + 2 * self.n_pairs
        self.meta = np.concatenate([self.win_off, self.frame_lens]).astype(np.int32)

    def buffers(self, device):
        """(meta on the device, bit-word workspace, output buffer)."""
        meta = torch.from_numpy(self.meta).to(device)
        bits = torch.empty(max(self.n_words, 1), dtype=torch.int64, device=device)
        out = torch.empty(self.out_len, dtype=torch.int32, device=device)
        return meta, bits, out

    def parse(self, out_host: np.ndarray) -> List[Tuple[np.ndarray, ...]]:
        f, k = len(self.frame_lens), self.k
        n_ev = out_host[:f * k].reshape(f, k)
        ev = out_host[f * k:].reshape(-1, 2)
        res = []
        for i in range(f):
            cls = []
            for c in range(k):
                b = int(self.pair_base[i] + c * self.cap[i])
                cls.append(ev[b:b + int(n_ev[i, c])].astype(np.int64))
            res.append(tuple(cls))
        return res


def launch_decode(preds: torch.Tensor, layout: DecodeLayout, meta: torch.Tensor, bits: torch.Tensor, out: torch.Tensor,
                  n_frame: int, overlap_hop: int, avg_pool: int = AVG_POOL, max_pool: int = MAX_POOL,
                  threshold: float = THRESHOLD) -> None:
    """The iris_decode_events launches on the current stream into `out` (no host sync: capturable once the buffers exist)."""
    f = len(layout.frame_lens)
    if not (preds.is_cuda and preds.dtype == torch.float32 and preds.is_contiguous()):
        raise ValueError("launch_decode: preds must be a contiguous fp32 GPU tensor")
    for name, t, n in (("meta", meta, 2 * f + 1), ("out", out, layout.out_len)):
        if t.dtype != torch.int32 or t.device != preds.device or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"launch_decode: {name} must be a contiguous int32 [{n}] tensor on {preds.device}")
    if bits.dtype != torch.int64 or bits.device != preds.device or bits.numel() < max(layout.n_words, 1):
        raise ValueError(f"launch_decode: bits must be an int64 tensor of >= {layout.n_words} words on {preds.device}")
    wo_h, fl_h = layout.win_off, layout.frame_lens
    ptr = meta.data_ptr()
    N.check(N.lib().iris_decode_events(preds.data_ptr(), ptr, ptr + 4 * (f + 1), wo_h.ctypes.data, fl_h.ctypes.data, f,
                                       int(n_frame), int(overlap_hop), preds.shape[1], preds.shape[2], int(avg_pool),
                                       int(max_pool), float(threshold), bits.data_ptr(), out.data_ptr() + 4 * f * layout.k,
                                       out.data_ptr(), torch.cuda.current_stream(preds.device).cuda_stream),
            "iris_decode_events")


def decode_events(preds: torch.Tensor, win_off, frame_lens, n_frame: int, overlap_hop: int, avg_pool: int = AVG_POOL,
                  max_pool: int = MAX_POOL, threshold: float = THRESHOLD) -> List[Tuple[np.ndarray, ...]]:
    """Window predictions [W_total, n_out, K] of F files (file f owns windows win_off[f] .. win_off[f + 1] - 1 and has
    frame_lens[f] frames) -> per file, per class [n, 2] int64 (first, last) frame events, as get_start_end_frame returns them.
    GPU tensors: the iris_decode_events launches and one copy back; CPU tensors: the restatement of the module doc."""
    wo = np.asarray(win_off.cpu() if torch.is_tensor(win_off) else win_off, dtype=np.int64).reshape(-1)
    fl = np.asarray(frame_lens.cpu() if torch.is_tensor(frame_lens) else frame_lens, dtype=np.int64).reshape(-1)
    _check(tuple(preds.shape), wo, fl, int(n_frame), int(overlap_hop), int(avg_pool), int(max_pool))
    if not preds.is_cuda:
        p = preds.detach().to(torch.float32).contiguous()
        return [_decode_file_host(p, int(wo[i]), int(wo[i + 1] - wo[i]), int(fl[i]), int(n_frame), int(overlap_hop),
                                  int(avg_pool), int(max_pool), float(threshold)) for i in range(len(fl))]
    p = preds.detach().to(torch.float32).contiguous()
    layout = DecodeLayout(wo, fl, p.shape[2])
    meta, bits, out = layout.buffers(p.device)
    launch_decode(p, layout, meta, bits, out, n_frame, overlap_hop, avg_pool, max_pool, threshold)
    return layout.parse(out.cpu().numpy())


# ---------------------------------------------------------------------------
# detection over recordings
# ---------------------------------------------------------------------------
@dataclass
class Detection:
    name: str
    n_frames: int
    events: Tuple[np.ndarray, ...]     # per class [n, 2] int64 (first, last) frames   (get_start_end_frame)
    metric: np.ndarray                 # [N, 2] int32 (class, middle second)             (output_to_metric)
    answer: Tuple[np.ndarray, ...]     # per class [n, 2] int32 (start s, end s)        (get_start_end_time)


class _FromEvents(M.Challenge_Metric):
    """Challenge_Metric whose frame events are already decoded: get_start_end_time's rounding and de-duplication run on them."""

    def __init__(self, events):
        super().__init__(SR, HOP)
        self._events = events

    def get_start_end_frame(self, data):
        return self._events


def _items(wavs_or_paths, sample_rate: int):
    """-> [(name, path or None, wav or None, sample rate)]."""
    out = []
    for i, it in enumerate(wavs_or_paths):
        if isinstance(it, (str, os.PathLike)):
            p = os.fspath(it)
            out.append((os.path.splitext(os.path.basename(p))[0], p, None, sample_rate))
        elif isinstance(it, tuple):
            out.append((str(it[0]), None, it[1], int(it[2]) if len(it) > 2 else sample_rate))
        else:
            out.append((str(i), None, it, sample_rate))
    return out


def _model_device(model, device):
    if device is not None:
        return torch.device(device)
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration):
        return torch.device('cuda', 0) if torch.cuda.is_available() else torch.device('cpu')


def _predict(model, windows: torch.Tensor, batch_size: int) -> torch.Tensor:
    if hasattr(model, 'predict'):   # CustomModel: on a GPU through its cached InferenceEngine
        return model.predict(windows, batch_size=batch_size)
    model.eval()
    return torch.cat([model(windows[i:i + batch_size]) for i in range(0, windows.shape[0], batch_size)])


@torch.no_grad()
def detect(model, wavs_or_paths: Sequence, config, overlap_hop: int = 512, batch_size: int = 32, sample_rate: int = SR,
           device=None, max_windows: int = 1024) -> List[Detection]:
    """Events of `model` in each recording: a wav path, a (name, [chan, samples] array[, sample rate]) tuple or a bare array
    (named by its position).  Files are handled in groups of at most `max_windows` windows (a longer file forms a group of
    its own); each window's prediction does not depend on the grouping."""
    dev = _model_device(model, device)
    items = _items(wavs_or_paths, sample_rate)
    results: List[Detection] = []
    group, n_group = [], 0

    def flush():
        nonlocal group, n_group
        if group:
            results.extend(_detect_group(model, group, config, overlap_hop, batch_size))
        group, n_group = [], 0

    for name, path, wav, sr in items:
        spec = D.load_wav(path, dev) if path is not None else D.load_wav_array(wav, sr, dev)
        feats = features_for_eval(spec, config)
        del spec
        t_len = int(feats.shape[-2])
        windows = frame(feats, config.n_frame, overlap_hop, pad_end=True, axis=-2)   # [M, W, n_frame, C']
        windows = windows.permute(1, 0, 2, 3)[..., :config.n_chan].contiguous()
        if group and n_group + windows.shape[0] > max_windows:
            flush()
        group.append((name, t_len, windows))
        n_group += windows.shape[0]
    flush()
    return results


def _detect_group(model, group, config, overlap_hop: int, batch_size: int) -> List[Detection]:
    windows = torch.cat([w for _, _, w in group]) if len(group) > 1 else group[0][2]
    preds = _predict(model, windows, batch_size)
    del windows
    win_off = np.concatenate([[0], np.cumsum([w.shape[0] for _, _, w in group])])
    events = decode_events(preds.to(torch.float32), win_off, [t for _, t, _ in group], config.n_frame, overlap_hop)
    out = []
    for (name, t_len, _), ev in zip(group, events):
        metric = M.output_to_metric(HOP, SR)(*ev)
        out.append(Detection(name, t_len, ev, metric, _FromEvents(ev).get_start_end_time(None)))
    return out


def answer_rows(det: Detection) -> List[List[int]]:
    """[[class, start_s, end_s], ...]: classes in order, times ascending."""
    return [[c, int(s), int(e)] for c, rows in enumerate(det.answer) for s, e in np.asarray(rows).reshape(-1, 2)]


def write_answer(results: Sequence[Detection], path: str) -> dict:
    """{"task2_answer": {name: [[class, start_s, end_s], ...]}} as sample_answer.json holds it."""
    answer = {"task2_answer": {d.name: answer_rows(d) for d in results}}
    with open(path, 'w') as f:
        json.dump(answer, f, indent=4)
    return answer


def main(argv=None):
    from .eval import load_model, parse_name
    from .sj_train import ARGS
    config = ARGS()
    config.args.add_argument('--p', help='parsing name', action='store_true')
    config.args.add_argument('--path', type=str, default='')
    config.args.add_argument('--wav_dir', type=str, default='.')
    config.args.add_argument('--out', type=str, default='answer.json')
    config.args.add_argument('--overlap_hop', type=int, default=512)
    config.args.add_argument('--score', type=str, default=None, help='sample_answer.json to print per-file ER against')
    config = config.get(argv)
    if config.p:
        parse_name(config)
    model = load_model(config, config.path)
    paths = sorted(glob(os.path.join(config.wav_dir, '*.wav')))
    results = detect(model, paths, config, overlap_hop=config.overlap_hop)
    write_answer(results, config.out)
    print(f"{len(results)} files, {sum(len(d.metric) for d in results)} events -> {config.out}")
    if config.score:
        with open(config.score) as f:
            gt = json.load(f)['task2_answer']
        scores = []
        for d in results:
            er = M.get_er(gt[d.name], d.metric)
            scores.append(er)
            print(f"ER {d.name} {er!r}")
        print('FINAL SCORE:', np.mean(scores))
        return scores
    return results


if __name__ == "__main__":
    main()
