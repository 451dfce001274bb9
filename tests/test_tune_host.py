"""CPU tests of the decoder tuning in challenge_amd.detect: get_er as a sum of per-class terms, sweep_decoder's restatement
against the chain decode_events -> output_to_metric -> per-class greedy at every grid point, choose_settings on a case whose
answer is known, DecoderSettings, per-class settings in decode_events, and the --tune / --decoder plumbing of the command."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from challenge_amd import _native as N
from challenge_amd import detect as DT
from challenge_amd import metrics as M
from test_detect_host import run_preds

HOP, SR = 256, 16000


# ---------------------------------------------------------------------------
# an independent statement of the per-class greedy rule
# ---------------------------------------------------------------------------
def greedy_class(gt_rows, pred_rows, c):
    """(n_pred, matched, n_gt) of class c: ground truth by ascending start (stable); each row takes the first prediction of the
    class, in time order, that no earlier row took and whose second lies in [start, end]."""
    gt = [r for r in np.asarray(gt_rows).reshape(-1, 3).tolist() if r[0] == c]
    gt.sort(key=lambda r: r[1])                                          # list.sort is stable
    sec = sorted(r[1] for r in np.asarray(pred_rows).reshape(-1, 2).tolist() if r[0] == c)
    used = [False] * len(sec)
    m = 0
    for _, s, e in gt:
        for i, v in enumerate(sec):
            if not used[i] and s <= v <= e:
                used[i] = True
                m += 1
                break
    return len(sec), m, len(gt)


def chain_counts(preds, win_off, frame_lens, gt, n_frame, hop, point):
    """decode_events(setting) -> output_to_metric -> greedy per class: (n_pred [F, 3], matched [F, 3])."""
    thr, avg, mx = point
    ev = DT.decode_events(preds, win_off, frame_lens, n_frame, hop, avg, mx, thr)
    n_pred = np.zeros((len(frame_lens), 3), np.int64)
    matched = np.zeros_like(n_pred)
    for f, e in enumerate(ev):
        metric = M.output_to_metric(HOP, SR)(*e)
        for c in range(3):
            n_pred[f, c], matched[f, c], _ = greedy_class(gt[f], metric, c)
    return n_pred, matched


def random_gt(rng, frame_lens, k=3, rows=(0, 7)):
    """Per file [[class, start_s, end_s], ...]: overlapping and repeated rows, classes left out, a few empty intervals."""
    out = []
    for t_len in frame_lens:
        dur = max(int(t_len * HOP / SR), 1)
        g = []
        for c in range(k):
            if rng.random() < 0.2:
                continue
            for _ in range(int(rng.integers(*rows))):
                s = int(rng.integers(0, dur + 1))
                g.append([c, s, s + int(rng.integers(-1, 9))])
            if g and rng.random() < 0.3:
                g.append(list(g[-1]))
        order = rng.permutation(len(g))
        out.append([g[i] for i in order])
    return out


PLANT = (0.25, 0.3)


def plant_info(frame_lens, n_frame, hop, plant=PLANT):
    """Where sweep_case plants: in the last file, from the start q0 of its last window on, everything is quiet except blocks of
    32 frames at q0 + 32 (2 i + 1) holding the fp32 value plant[i] in class 0 -> [(value, first frame, last frame)] of those
    that fit inside the file."""
    t_len = frame_lens[-1]
    q0 = (max(-(-t_len // hop), 1) - 1) * hop
    out = []
    for i, v in enumerate(plant):
        first = q0 + 32 * (2 * i + 1)
        if first + 32 < t_len and 32 * (2 * i + 2) <= min(hop, n_frame):
            out.append((float(np.float32(v)), first, first + 31))
    return q0, out


def sweep_case(seed, frame_lens, n_frame=512, hop=512, n_out=16, k=3, plant=PLANT):
    """Window predictions of ragged files (random on / off runs plus noise), with one window of NaN in file 0, and a quiet
    stretch at the end of the last file holding frames whose smoothed value equals a threshold exactly (plant_info: every
    window that covers such a frame holds the value there, and v + v = 2 v, 2 v / 2 = v are exact, so with avg_pool 1
    a[t] = p[t] = v whatever the overlap); and random ground truth."""
    rng = np.random.default_rng(seed)
    preds, win_off = run_preds(rng, frame_lens, n_frame, hop, n_out, k=k, noise=0.25, mean_run=90.0)
    if win_off[1] - win_off[0] > 2:
        preds[win_off[0] + 1, :, k - 1] = np.nan
    up = n_frame // n_out
    assert 32 % up == 0 and hop % 32 == 0
    q0, blocks = plant_info(frame_lens, n_frame, hop, plant)
    w0, n_win = win_off[-2], win_off[-1] - win_off[-2]
    value = np.zeros((n_win - 1) * hop + n_frame, np.float32)          # class 0 of the quiet stretch, frame by frame
    for v, first, last in blocks:
        value[first:last + 1] = v
    for w in range(n_win):
        for j in range(n_out):
            t = w * hop + j * up
            if t >= q0:
                preds[w0 + w, j, :] = 0.0
                preds[w0 + w, j, 0] = value[t]
    return torch.from_numpy(preds), win_off, random_gt(rng, frame_lens, k)


SMALL_GRID = [(t, a, m) for a in (1, 15, 31) for t in (0.25, 0.3, 0.5, 0.7) for m in (1, 31, 124)]   # 36 points


# ---------------------------------------------------------------------------
# 1. get_er is a sum of per-class terms
# ---------------------------------------------------------------------------
def test_get_er_decomposes_by_class():
    rng = np.random.default_rng(0)
    n_cases = 0
    for case in range(260):
        gt, pred = [], []
        for c in range(3):
            if rng.random() > 0.15:
                for _ in range(int(rng.integers(1, 7))):
                    s = int(rng.integers(0, 30))
                    gt.append([c, s, s + int(rng.integers(-1, 12))])      # overlapping rows, now and then an empty one
            if rng.random() > 0.15:
                pred += [[c, int(v)] for v in np.sort(rng.integers(0, 40, int(rng.integers(1, 9))))]   # repeated seconds
        if not gt:
            continue
        if case % 3 == 0 and gt:
            gt.append(list(gt[0]))
        gt = [gt[i] for i in rng.permutation(len(gt))]
        want = M.get_er(gt, np.asarray(pred, np.int32).reshape(-1, 2))
        terms = [greedy_class(gt, pred, c) for c in range(3)]
        mine = sum(p + g - 2 * m for p, m, g in terms) / len(gt)
        assert mine == want, (gt, pred)
        n_pred, matched, n_gt = DT.class_counts(gt, pred, 3)
        assert [tuple(x) for x in zip(n_pred, matched, n_gt)] == terms
        assert DT.er_from_counts(n_pred, matched, n_gt) == want
        assert DT.er_from_counts(*DT.class_counts(gt, pred)) == want      # K from the rows
        n_cases += 1
    assert n_cases >= 200


# ---------------------------------------------------------------------------
# 2. the sweep against the chain, grid point by grid point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n_out", [(512, 16), (256, 512)])
def test_sweep_matches_brute_force(hop, n_out):
    frame_lens = [1700, 300, 513, 64, 2200]          # T < n_frame, one window, T not a multiple of 64 or of the hop
    preds, win_off, gt = sweep_case(3 + hop, frame_lens, hop=hop, n_out=n_out)
    assert win_off[4] - win_off[3] == 1 and torch.isnan(preds).any()
    _, blocks = plant_info(frame_lens, 512, hop)     # the planted values landed: on at their own threshold, off just above it
    assert [v for v, _, _ in blocks] == [float(np.float32(0.25)), float(np.float32(0.3))]
    assert {v for v, _, _ in blocks} <= {float(np.float32(t)) for t, _, _ in SMALL_GRID}
    for v, first, last in blocks:
        at = DT.decode_events(preds, win_off, frame_lens, 512, hop, 1, 1, v)[4][0].tolist()
        above = DT.decode_events(preds, win_off, frame_lens, 512, hop, 1, 1, float(np.nextafter(np.float32(v), np.float32(1))))
        assert [first, last] in at and [first, last] not in above[4][0].tolist()
    assert len(SMALL_GRID) >= 24 and {1} <= {a for _, a, _ in SMALL_GRID} and {1} <= {m for _, _, m in SMALL_GRID}
    n_pred, matched, n_gt = DT.sweep_decoder(preds, win_off, frame_lens, gt, SMALL_GRID, 512, hop)
    assert n_pred.shape == matched.shape == (len(SMALL_GRID), 5, 3) and n_gt.shape == (5, 3)
    assert n_pred.dtype.kind == matched.dtype.kind == n_gt.dtype.kind == 'i'
    for g, point in enumerate(SMALL_GRID):
        want_p, want_m = chain_counts(preds, win_off, frame_lens, gt, 512, hop, point)
        assert np.array_equal(n_pred[g], want_p), point
        assert np.array_equal(matched[g], want_m), point
    assert np.array_equal(n_gt, [[sum(r[0] == c for r in g) for c in range(3)] for g in gt])
    assert matched.sum() > 0 and (matched <= np.minimum(n_pred, n_gt[None])).all()


def test_sweep_threshold_is_inclusive():
    """Frames whose smoothed value equals the threshold bit for bit are on: with avg_pool 1 and max_pool 1 a planted value is
    an event at its own threshold and none just above it."""
    frame_lens = [1024]
    preds = torch.zeros(2, 16, 3)
    t03 = float(np.float32(0.3))
    preds[1, 3, 0] = t03                 # frames 608..639 of class 0
    up = float(np.nextafter(np.float32(0.3), np.float32(1)))
    gt = [[[0, 9, 10]]]                  # (608 + 639) / 2 * 256 / 16000 = 9.97 -> second 9
    grid = [(0.3, 1, 1), (up, 1, 1), (0.25, 1, 1)]
    n_pred, matched, _ = DT.sweep_decoder(preds, [0, 2], frame_lens, gt, grid, 512, 512)
    assert n_pred[:, 0, 0].tolist() == [1, 0, 1] and matched[:, 0, 0].tolist() == [1, 0, 1]
    assert DT.decode_events(preds, [0, 2], frame_lens, 512, 512, 1, 1, 0.3)[0][0].tolist() == [[608, 639]]


def test_sweep_grid_order_and_repeats_do_not_matter():
    frame_lens = [900, 1500]
    preds, win_off, gt = sweep_case(11, frame_lens)
    grid = SMALL_GRID[:12]
    base = DT.sweep_decoder(preds, win_off, frame_lens, gt, grid, 512, 512)
    perm = np.random.default_rng(1).permutation(len(grid))
    twice = [grid[i] for i in perm] + [grid[0]]
    got = DT.sweep_decoder(preds, win_off, frame_lens, gt, twice, 512, 512)
    for b, g in zip(base[:2], got[:2]):
        assert np.array_equal(g[:-1], b[perm]) and np.array_equal(g[-1], b[0])


# ---------------------------------------------------------------------------
# 3. a case with a known answer
# ---------------------------------------------------------------------------
def known_case():
    """Three files whose predictions are their ground-truth frames (events of 220..600 frames, gaps of at least 400), scaled
    to a peak of 0.4 for class 0 and 0.9 for classes 1 and 2; n_out = n_frame, no overlap: the predictions are the frames."""
    rng = np.random.default_rng(5)
    frame_lens, chunks, win_off, gt = [4000, 2600, 5100], [], [0], []
    for t_len in frame_lens:
        n_win = -(-t_len // 512)
        sig = np.zeros((n_win * 512, 3), np.float32)
        rows = []
        for c in range(3):
            t = int(rng.integers(150, 300))
            while True:
                n = int(rng.integers(220, 600))
                if t + n + 150 > t_len:
                    break
                sig[t:t + n, c] = 0.4 if c == 0 else 0.9
                rows.append([c, int(t * HOP / SR), int(np.ceil((t + n - 1) * HOP / SR))])
                t += n + int(rng.integers(400, 700))
        assert {r[0] for r in rows} == {0, 1, 2}
        chunks.append(sig.reshape(n_win, 512, 3))
        win_off.append(win_off[-1] + n_win)
        gt.append(rows)
    return torch.from_numpy(np.concatenate(chunks)), np.asarray(win_off), frame_lens, gt


def test_choose_settings_known_answer():
    preds, win_off, frame_lens, gt = known_case()
    grid = DT.decoder_grid()
    assert grid[0] == (0.5, 31, 124) and len(grid) == 1 + 17 * 5 * 6
    thr = sorted({t for t, _, _ in grid[1:]})
    assert len(thr) == 17 and np.allclose(thr, np.arange(0.1, 0.91, 0.05)) and all(t == float(np.float32(t)) for t in thr)
    assert {a for _, a, _ in grid[1:]} == {1, 15, 31, 47, 63} and {m for _, _, m in grid[1:]} == {1, 31, 62, 124, 186, 248}
    n_pred, matched, n_gt = DT.sweep_decoder(preds, win_off, frame_lens, gt, grid, 512, 512)
    tuned = DT.choose_settings(n_pred, matched, n_gt, grid)
    s = tuned.settings
    assert s.threshold[0] < 0.4
    assert s.points()[1] == s.points()[2] == (0.5, 31, 124) and tuned.index[1:] == (0, 0)      # the tie rule
    assert tuned.mean_er_chosen == 0.0
    # the brute-force path agrees, at the reference point and at the chosen one
    ref_ev = DT.decode_events(preds, win_off, frame_lens, 512, 512)
    new_ev = DT.decode_events(preds, win_off, frame_lens, 512, 512, settings=s)
    ref_er, new_er = [], []
    for f in range(3):
        ref_metric = M.output_to_metric(HOP, SR)(*ref_ev[f])
        assert not (ref_metric[:, 0] == 0).any()                          # class 0 entirely missed at the reference point
        n0 = sum(r[0] == 0 for r in gt[f])
        ref_er.append(M.get_er(gt[f], ref_metric))
        assert ref_er[-1] == n0 / len(gt[f])                              # ... and that is all that is missed
        new_er.append(M.get_er(gt[f], M.output_to_metric(HOP, SR)(*new_ev[f])))
    assert new_er == [0.0, 0.0, 0.0]
    assert tuned.mean_er_reference == float(np.mean(ref_er)) > 0.0
    # the table the settings carry is the one they were chosen from
    score = np.asarray(s.score)
    assert score.shape == (len(grid), 3) and s.grid == grid
    assert all(score[tuned.index[c], c] == score[:, c].min() == 0.0 for c in range(3))
    assert all((score[:tuned.index[c], c] > 0.0).all() for c in range(3))   # the earliest of the minima


def test_choose_settings_is_the_minimum_over_all_combinations():
    """G^K combinations scored with get_er's expression: the per-class choice attains the minimum mean."""
    rng = np.random.default_rng(2)
    g, f, k = 5, 4, 3
    n_gt = rng.integers(0, 4, (f, k))
    n_gt[:, 0] += 1
    n_pred = rng.integers(0, 6, (g, f, k))
    matched = np.minimum(rng.integers(0, 6, (g, f, k)), np.minimum(n_pred, n_gt[None]))
    grid = [(0.5, 31, 124)] + [(0.1 * i, 15, 31) for i in range(1, g)]
    tuned = DT.choose_settings(n_pred, matched, n_gt, grid)
    cls = np.arange(k)
    best = min(float(np.mean([DT.er_from_counts(n_pred[np.asarray(ix), i, cls], matched[np.asarray(ix), i, cls], n_gt[i])
                              for i in range(f)]))
               for ix in np.ndindex(g, g, g))
    assert abs(tuned.mean_er_chosen - best) <= 1e-12 and tuned.mean_er_chosen <= tuned.mean_er_reference


def test_empty_ground_truth_is_refused():
    n_pred = np.zeros((2, 3, 3), np.int64)
    n_gt = np.array([[1, 0, 0], [0, 0, 0], [0, 2, 0]])
    with pytest.raises(ValueError, match="clip_b"):
        DT.choose_settings(n_pred, n_pred, n_gt, [(0.5, 31, 124), (0.3, 31, 124)], names=["clip_a", "clip_b", "clip_c"])
    with pytest.raises(ValueError, match="file 1 "):
        DT.choose_settings(n_pred, n_pred, n_gt, [(0.5, 31, 124), (0.3, 31, 124)])


# ---------------------------------------------------------------------------
# 4. settings, decode_events(settings=...), limits, the command line
# ---------------------------------------------------------------------------
def test_settings_round_trip(tmp_path):
    s = DT.DecoderSettings([0.35, 0.5, 0.1], [15, 31, 1], [62, 124, 248], grid=DT.decoder_grid()[:4],
                           score=[[0.1, 0.2, 0.3]] * 4)
    path = tmp_path / "decoder.json"
    s.save(str(path))
    back = DT.DecoderSettings.load(str(path))
    assert back == s and back.grid == s.grid and back.score == s.score
    assert back.threshold[0] == float(np.float32(0.35)) and isinstance(back.avg_pool[0], int)
    with open(path) as f:
        doc = json.load(f)

    def only_numbers(x):
        return all(only_numbers(v) for v in x) if isinstance(x, list) else isinstance(x, (int, float))
    assert sorted(doc) == ["avg_pool", "grid", "max_pool", "score", "threshold"] and all(only_numbers(v) for v in doc.values())
    d = DT.DecoderSettings.default(3)
    assert d.points() == [(DT.THRESHOLD, DT.AVG_POOL, DT.MAX_POOL)] * 3 == [(0.5, 31, 124)] * 3
    d.save(str(path))
    assert DT.DecoderSettings.load(str(path)) == d and DT.DecoderSettings.load(str(path)).grid is None
    with pytest.raises(ValueError):
        DT.DecoderSettings([0.5], [31, 31], [124])
    with pytest.raises(ValueError):
        DT.DecoderSettings([0.5], [128], [124])


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert u.dtype == v.dtype == np.int64 and np.array_equal(u, v)


def test_decode_events_with_settings():
    frame_lens = [1700, 300, 2049]
    preds, win_off, _ = sweep_case(8, frame_lens, hop=256)
    _same(DT.decode_events(preds, win_off, frame_lens, 512, 256, settings=DT.DecoderSettings.default(3)),
          DT.decode_events(preds, win_off, frame_lens, 512, 256))
    s = DT.DecoderSettings([0.3, 0.5, 0.7], [15, 31, 15], [62, 124, 1])
    mixed = DT.decode_events(preds, win_off, frame_lens, 512, 256, settings=s)
    single = [DT.decode_events(preds, win_off, frame_lens, 512, 256, a, m, t) for t, a, m in s.points()]
    _same(mixed, [tuple(single[c][f][c] for c in range(3)) for f in range(3)])
    assert len({tuple(map(len, f)) for f in mixed}) > 1
    with pytest.raises(ValueError, match="classes"):
        DT.decode_events(preds, win_off, frame_lens, 512, 256, settings=DT.DecoderSettings.default(2))


def test_sweep_limits_are_errors():
    preds = torch.zeros(2, 16, 3)
    ok = dict(win_off=[0, 2], frame_lens=[900], gt=[[[0, 1, 2]]], grid=[(0.5, 31, 124)])

    def run(**kw):
        a = dict(ok, **kw)
        return DT.sweep_decoder(a.get("preds", preds), a["win_off"], a["frame_lens"], a["gt"], a["grid"], 512, 512)
    run()
    with pytest.raises(ValueError, match="grid points"):
        run(grid=[(0.001 * i, 31, 124) for i in range(DT.MAX_GRID + 1)])
    with pytest.raises(ValueError, match="distinct thresholds"):
        run(grid=[(0.001 * i, 31, 124) for i in range(DT.MAX_GROUP_THRESHOLDS + 1)])
    with pytest.raises(ValueError, match="words"):
        run(preds=torch.zeros(50, 16, 3), win_off=[0, 50], frame_lens=[25000], grid=DT.decoder_grid())
    with pytest.raises(ValueError, match="ground-truth events"):
        run(gt=[[[1, i, i + 1] for i in range(DT.MAX_GT_ROWS + 1)]])
    with pytest.raises(ValueError, match="class"):
        run(gt=[[[3, 1, 2]]])
    with pytest.raises(ValueError, match="max_pool"):
        run(grid=[(0.5, 31, 257)])
    with pytest.raises(ValueError, match="files"):
        run(gt=[])
    n = DT.MAX_SWEEP_FILES + 1                       # zero-length files: the count alone is refused
    with pytest.raises(ValueError, match="65536 files in one call"):
        run(win_off=[0] * n + [2], frame_lens=[0] * n, gt=[[]] * n)
    with pytest.raises(ValueError, match="too many counts"):
        run(preds=torch.zeros(2, 16, 16), win_off=[0] * (n - 1) + [2], frame_lens=[0] * (n - 1), gt=[[]] * (n - 1),
            grid=[(0.5, 31, 1 + i % 256) for i in range(DT.MAX_GRID)])
    with pytest.raises(ValueError, match="frames x 3 classes"):
        DT.SweepLayout([0, 2 ** 22], [2 ** 30], 3, [[]], [(0.5, 31, 124)])


@pytest.mark.parametrize("kw,code,msg", [
    (dict(k=17), -2, b"K 17"),
    (dict(avg=[31, 128]), -2, b"avg_pool 128"),
    (dict(mx=[124, 257]), -2, b"max_pool 257"),
    (dict(n_grid=4097), -2, b"grid points"),
    (dict(thr=[0.001 * i for i in range(257)]), -2, b"distinct thresholds"),
    (dict(frame_len=25000, win=50, thr=[0.05 * i for i in range(17)]), -2, b"words"),
    (dict(gt_off=[0, 65, 65, 65]), -2, b"ground-truth events"),
    (dict(files=65536), -2, b"65536 files"),
    (dict(frame_len=2 ** 30, win=2 ** 22), -2, b"frames x 3 classes"),
    (dict(files=65535, k=16, n_grid=4096), -2, b"too many counts"),
    (dict(avg=[31, 15, 31]), -1, b"not adjacent"),
    (dict(thr=[0.5, 0.3, 0.5]), -1, b"not adjacent"),
    (dict(overlap_hop=600), -1, b"overlap_hop"),
])
def test_c_abi_limits(kw, code, msg):
    """Every cap of iris_decode_sweep at the C ABI: the checks run on the host copies, before any device work (host pointers
    stand in for the device buffers) and nothing is written."""
    lib = N.lib()
    thr = kw.get("thr", [0.5] * max(len(kw.get("avg", [])), len(kw.get("mx", [])), 1))
    n = kw.get("n_grid", len(thr))
    avg = kw.get("avg", [31] * len(thr))
    mx = kw.get("mx", [124] * len(thr))
    k = kw.get("k", 3)
    a_thr = (C.c_float * max(n, len(thr)))(*thr)
    a_avg = (C.c_int * max(n, len(avg)))(*avg)
    a_max = (C.c_int * max(n, len(mx)))(*mx)
    n_files = kw.get("files", 1)                     # more than one: zero-length files, the last one owning the windows
    win_off = (C.c_int * (n_files + 1))(*([0] * n_files + [kw.get("win", 2)]))
    frame_len = (C.c_int * n_files)(*([0] * (n_files - 1) + [kw.get("frame_len", 900 if n_files == 1 else 0)]))
    gt_off = (C.c_int * (n_files * k + 1))(*kw.get("gt_off", [0] * (n_files * k + 1)))
    buf = (C.c_int * 64)(*([-7] * 64))
    p = C.cast(buf, C.c_void_p)
    vp = lambda x: C.cast(x, C.c_void_p)
    st = lib.iris_decode_sweep(p, p, p, vp(win_off), vp(frame_len), n_files, 512, kw.get("overlap_hop", 512), 16, k,
                               p, p, p, vp(a_thr), vp(a_avg), vp(a_max), n, p, p, vp(gt_off), HOP, SR, p, p, p, None)
    assert st == code
    err = lib.iris_last_error()
    assert err.startswith(b"iris_decode_sweep") and msg in err
    assert list(buf) == [-7] * 64


class _Stub(torch.nn.Module):
    """Class c is 0.3 + 0.25 c where the window's feature exceeds 0.5, else 0.05: class 0 never reaches 0.5."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        on = (x.mean(dim=(1, 3)).reshape(x.shape[0], 16, -1).mean(-1) > 0.5).float()      # [W, 16]
        return torch.stack([0.05 + on * (0.25 + 0.25 * c) for c in range(3)], -1)


def test_cli_tune_and_decoder(tmp_path, monkeypatch, capsys):
    """--tune / --decoder_out / --decoder / --score through detect.main, with the model and the front end replaced by CPU
    stand-ins (the real ones need a GPU): a 'recording' is a text file of on / off flags per block of 32 frames."""
    from challenge_amd import eval as E
    rng = np.random.default_rng(4)
    answer = {}
    for i in range(3):
        n_blocks = 40 + 16 * i
        flags = np.zeros(n_blocks, np.int64)
        rows, b = [], 3
        while b + 12 < n_blocks:
            n = int(rng.integers(6, 10))
            flags[b:b + n] = 1
            rows += [[c, int(b * 32 * HOP / SR), int(np.ceil((b + n) * 32 * HOP / SR))] for c in range(3)]
            b += n + int(rng.integers(8, 12))
        np.savetxt(tmp_path / f"rec{i}.wav", flags, fmt="%d")
        answer[f"rec{i}"] = rows
    with open(tmp_path / "answer_gt.json", "w") as f:
        json.dump({"task2_answer": answer}, f)
    monkeypatch.setattr(E, "load_model", lambda config, path='', device=None: _Stub())
    monkeypatch.setattr(DT.D, "load_wav", lambda path, device=None: torch.from_numpy(np.loadtxt(path)).float())
    monkeypatch.setattr(DT, "features_for_eval",
                        lambda spec, config: spec.repeat_interleave(32)[None, :, None].expand(4, -1, 1).contiguous())
    base = ["--name", "run", "--v", "9", "--n_mels", "64", "--n_frame", "512", "--n_chan", "1", "--wav_dir", str(tmp_path),
            "--out", str(tmp_path / "answer.json"), "--score", str(tmp_path / "answer_gt.json")]
    plain = DT.main(base)
    out = capsys.readouterr().out
    assert "MEAN ER" not in out and all(er > 0 for er in plain)          # class 0 stays under 0.5: missed
    tuned = DT.main(base + ["--tune", str(tmp_path / "answer_gt.json"), "--decoder_out", str(tmp_path / "decoder.json")])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("MEAN ER")][0].split()
    assert float(line[3]) == float(np.mean(plain)) and float(line[5]) == float(np.mean(tuned)) == 0.0
    s = DT.DecoderSettings.load(str(tmp_path / "decoder.json"))
    assert s.threshold[0] < 0.3 + 1e-6 and s.points()[1] == s.points()[2] == (0.5, 31, 124) and len(s.grid) == 511
    again = DT.main(base + ["--decoder", str(tmp_path / "decoder.json")])
    assert again == tuned
    with open(tmp_path / "answer.json") as f:
        ans = json.load(f)["task2_answer"]
    assert all({r[0] for r in rows} == {0, 1, 2} for rows in ans.values())
    with pytest.raises(ValueError, match="one of the two"):
        DT.main(base + ["--tune", "x.json", "--decoder", "y.json"])
