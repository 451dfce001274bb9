"""CPU tests of challenge_amd.detect: decode_events' restatement against an independent fp64 NumPy restatement of the
reference chain (metrics.py:56-81 from the model outputs on, then get_start_end_frame :111-137), its argument checks (in
Python and at the C ABI), write_answer and the answer rows' rounding."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from challenge_amd import _native as N
from challenge_amd import detect as DT
from challenge_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# fp64 reference: tf.signal.frame / overlap_and_add, Keras 'same' pooling, >= 0.5, get_start_end_frame
# ---------------------------------------------------------------------------
def ref_smoothed(preds, n_frame, hop, t_len, avg=31, mx=124):
    """One file's window predictions [W, n_out, K] -> (a [T, K] fp64 average-pooled, m [T, K] max-pooled)."""
    p = np.asarray(preds, np.float64)
    w, n_out, k = p.shape
    p = np.repeat(p, n_frame // n_out, axis=1)                       # UpSampling1D
    out_len = (w - 1) * hop + n_frame
    acc = np.zeros((out_len, k))
    cnt = np.zeros((out_len, 1))
    for i in range(w):                                              # tf.signal.overlap_and_add
        acc[i * hop:i * hop + n_frame] += p[i]
        cnt[i * hop:i * hop + n_frame] += 1
    x = acc[:t_len] / cnt[:t_len]
    al, ar = (avg - 1) // 2, avg - 1 - (avg - 1) // 2
    a = np.empty_like(x)
    for t in range(t_len):                                          # AveragePooling1D(avg, 1, 'same'): padding not counted
        a[t] = x[max(t - al, 0):t + ar + 1].mean(0)
    ml, mr = (mx - 1) // 2, mx - 1 - (mx - 1) // 2
    m = np.empty_like(a)
    for t in range(t_len):                                          # MaxPooling1D(mx, 1, 'same'): NaN propagates
        m[t] = np.max(a[max(t - ml, 0):t + mr + 1], axis=0)
    return a, m


def ref_start_end_frame(data):
    """metrics.py:111-137 for any number of classes."""
    k = data.shape[1]
    prev = np.concatenate([np.zeros([1, k]), data[:-1, :]], 0)
    diff = np.argwhere(prev != data)
    out = []
    for c in range(k):
        idx = diff[diff[:, 1] == c][:, 0]
        if idx.shape[0] % 2 != 0:
            idx = np.concatenate([idx, [len(data)]])
        idx = idx.reshape(-1, 2)
        out.append(np.stack([idx[:, 0], idx[:, 1] - 1], 1).astype(np.int64))
    return out


def ref_events(preds, win_off, frame_lens, n_frame, hop):
    res, margin = [], np.inf
    for f, t_len in enumerate(frame_lens):
        a, m = ref_smoothed(preds[win_off[f]:win_off[f + 1]], n_frame, hop, t_len)
        fin = a[np.isfinite(a)]
        if fin.size:
            margin = min(margin, float(np.abs(fin - 0.5).min()))
        res.append(ref_start_end_frame((m >= 0.5).astype(np.float32)) if t_len else [np.zeros((0, 2), np.int64)] * preds.shape[2])
    return res, margin


def run_preds(rng, frame_lens, n_frame, hop, n_out, k=3, mean_run=120.0, noise=0.03):
    """Window predictions of files whose frames follow random on / off runs (levels 0.12 / 0.88 plus noise per window)."""
    up = n_frame // n_out
    chunks, win_off = [], [0]
    for t_len in frame_lens:
        n_win = max(-(-t_len // hop), 1)
        span = (n_win - 1) * hop + n_frame
        flips = rng.random((span, k)) < 1.0 / mean_run
        level = np.where(np.cumsum(flips, 0) % 2 == 1, 0.88, 0.12)
        idx = np.arange(n_win)[:, None] * hop + np.arange(n_out)[None, :] * up
        chunks.append(level[idx] + noise * rng.standard_normal((n_win, n_out, k)))
        win_off.append(win_off[-1] + n_win)
    return np.concatenate(chunks).astype(np.float32), np.asarray(win_off)


def margin_case(seed, frame_lens, n_frame, hop, n_out, k=3, need=1e-4, **kw):
    """Inputs whose fp64 smoothed values all keep `need` from 0.5 (drawn again until they do), with their reference events."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        preds, win_off = run_preds(rng, frame_lens, n_frame, hop, n_out, k, **kw)
        ref, margin = ref_events(preds, win_off, frame_lens, n_frame, hop)
        if margin >= need:
            return preds, win_off, ref
    raise AssertionError("no input with the margin found")


def assert_same_events(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for gc, wc in zip(g, w):
            assert gc.dtype == np.int64 and gc.shape == wc.shape
            assert np.array_equal(gc, wc), (gc, wc)


@pytest.mark.parametrize("hop", [128, 256, 512])
@pytest.mark.parametrize("n_out", [512, 16])
def test_decode_matches_fp64_reference(hop, n_out):
    frame_lens = [1000, 300, 2049, 513]   # T < n_frame, T not a multiple of 64 or of the hop
    preds, win_off, ref = margin_case(hop + n_out, frame_lens, 512, hop, n_out)
    got = DT.decode_events(torch.from_numpy(preds), win_off, frame_lens, 512, hop)
    assert_same_events(got, ref)


def test_decode_edge_cases():
    n_frame, hop = 512, 256
    # all on, all off, single-frame files, an empty file
    frame_lens = [700, 700, 1, 1, 0]
    win_off = np.array([0, 3, 6, 7, 8, 8])
    preds = np.full((8, 16, 3), 0.1, np.float32)
    preds[0:3] = 0.9
    preds[6] = 0.9
    got = DT.decode_events(torch.from_numpy(preds), win_off, frame_lens, n_frame, hop)
    assert [g.tolist() for g in got[0]] == [[[0, 699]]] * 3
    assert all(g.shape == (0, 2) for g in got[1])
    assert [g.tolist() for g in got[2]] == [[[0, 0]]] * 3
    assert all(g.shape == (0, 2) for g in got[3])
    assert all(g.shape == (0, 2) for g in got[4])
    ref, _ = ref_events(preds, win_off, frame_lens, n_frame, hop)
    assert_same_events(got, ref)


def test_decode_runs_touching_both_ends():
    n_frame, hop, t_len = 512, 512, 900
    sig = np.full((1024, 3), 0.1, np.float32)
    sig[:200, 0] = 0.9           # from frame 0
    sig[700:, 1] = 0.9           # to frame T - 1
    sig[300:400, 2] = 0.9        # inside
    preds = sig.reshape(2, 512, 3)
    win_off = [0, 2]
    got = DT.decode_events(torch.from_numpy(preds), win_off, [t_len], n_frame, hop)
    ref, margin = ref_events(preds, np.asarray(win_off), [t_len], n_frame, hop)
    assert margin > 1e-4
    assert_same_events(got, ref)
    assert got[0][0][0, 0] == 0 and got[0][1][-1, 1] == t_len - 1


def test_decode_nan_switches_off_its_window():
    n_frame, hop, t_len = 512, 512, 1500
    preds = np.full((3, 512, 3), 0.9, np.float32)
    preds[1, 100, 1] = np.nan                 # frame 612, class 1
    got = DT.decode_events(torch.from_numpy(preds), [0, 3], [t_len], n_frame, hop)
    ref, _ = ref_events(preds, np.array([0, 3]), [t_len], n_frame, hop)
    assert_same_events(got, ref)
    # a is NaN on frames 597..627; every frame within (-62, +61) of those is off
    assert got[0][1].tolist() == [[0, 534], [689, t_len - 1]]
    assert got[0][0].tolist() == [[0, t_len - 1]]


def test_decode_matches_predict_frames_chain():
    """The restatement and inference.predict_frames' torch chain (+ get_start_end_frame) agree away from the threshold."""
    from challenge_amd import inference as I
    frame_lens = [1700]
    for hop in (128, 512):
        preds, win_off, ref = margin_case(7 + hop, frame_lens, 512, hop, 16)
        x = torch.from_numpy(preds).repeat_interleave(32, dim=1).permute(2, 0, 1)
        counts = I.overlap_and_add(torch.ones_like(x), hop)[..., :1700]
        d = (I.smooth((I.overlap_and_add(x, hop)[..., :1700] / counts).t()) >= 0.5).float()
        want = M.Challenge_Metric().get_start_end_frame(d.numpy())
        got = DT.decode_events(torch.from_numpy(preds), win_off, frame_lens, 512, hop)[0]
        assert_same_events([got], [want])


@pytest.mark.parametrize("kw,msg", [
    (dict(overlap_hop=600), "overlap_hop"),
    (dict(n_frame=520), "multiple"),
    (dict(k=17), "classes"),
    (dict(frame_lens=[1100]), "no window covers"),
])
def test_decode_rejects(kw, msg):
    n_frame = kw.get("n_frame", 512)
    k = kw.get("k", 3)
    preds = torch.zeros(2, 16, k)
    with pytest.raises(ValueError, match=msg):
        DT.decode_events(preds, [0, 2], kw.get("frame_lens", [900]), n_frame, kw.get("overlap_hop", 512))


@pytest.mark.parametrize("args,code", [
    (dict(overlap_hop=600), -1),
    (dict(n_frame=520), -1),
    (dict(k=17), -2),
    (dict(frame_len=1100), -1),
])
def test_c_abi_rejects(args, code):
    """The same checks at the C ABI: they fail before any device work (host pointers stand in for device buffers)."""
    lib = N.lib()
    buf = (C.c_int * 64)()
    win_off = (C.c_int * 2)(0, 2)
    frame_len = (C.c_int * 1)(args.get("frame_len", 900))
    p = C.cast(buf, C.c_void_p)
    st = lib.iris_decode_events(p, p, p, C.cast(win_off, C.c_void_p), C.cast(frame_len, C.c_void_p), 1,
                                args.get("n_frame", 512), args.get("overlap_hop", 512), 16, args.get("k", 3), 31, 124, 0.5,
                                p, p, p, None)
    assert st == code
    assert lib.iris_last_error().startswith(b"iris_decode_events")


def _detection(name, events, n_frames=20000):
    metric = M.output_to_metric(256, 16000)(*events)
    return DT.Detection(name, n_frames, events, metric, DT._FromEvents(events).get_start_end_time(None))


def test_answer_rows_round_half_even_and_unique():
    ev = (np.array([[10, 40], [12, 41], [3000, 3100]], np.int64),     # the first two round to the same seconds
          np.zeros((0, 2), np.int64),
          np.array([[94, 156], [1, 1]], np.int64))
    det = _detection("x", ev)
    for c, rows in enumerate(det.answer):
        sec = np.asarray([[np.round(v * 256 / 16000) for v in r] for r in ev[c]]).reshape(-1, 2)   # half to even
        want = np.unique(sec, axis=0) if len(sec) else sec
        assert np.array_equal(rows, want)
    assert det.answer[0].tolist() == [[0, 1], [48, 50]]
    assert det.answer[2].tolist() == [[0, 0], [2, 2]]
    assert np.round(2.5) == 2.0   # numpy's round is tf.round's half to even


def test_write_answer_schema(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "sample_answer.json")) as f:
        sample = json.load(f)
    names = list(sample["task2_answer"])[:3]
    rng = np.random.default_rng(3)
    dets = []
    for n in names:
        ev = []
        for _ in range(3):
            s = np.sort(rng.choice(14000, 6, replace=False)).reshape(-1, 2)
            ev.append(s.astype(np.int64))
        dets.append(_detection(n, tuple(ev)))
    path = tmp_path / "answer.json"
    DT.write_answer(dets, str(path))
    with open(path) as f:
        got = json.load(f)
    assert list(got) == list(sample) == ["task2_answer"]
    assert list(got["task2_answer"]) == names
    for n, d in zip(names, dets):
        rows = got["task2_answer"][n]
        assert all(isinstance(v, int) for r in rows for v in r) and all(len(r) == 3 for r in rows)
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)
        for c in range(3):
            mine = [r[1:] for r in rows if r[0] == c]
            assert mine == sorted(mine) == d.answer[c].tolist()
    for rows in sample["task2_answer"].values():   # the shipped file has the same shape
        assert all(len(r) == 3 and all(isinstance(v, int) for v in r) for r in rows)
