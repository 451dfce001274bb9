"""CPU tests of the segment- and event-based detection counts (metrics.sed_counts_host / SedEval / sed_eval / sed_metrics), of what
`fit`, `sj_train` and `evaluate` do with them, and of the argument checks iris_sed_counts makes before any launch.  Counts are
integers: every comparison with tests/sedeval_ref.py (plain loops over rows, frames and events) is for EQUALITY."""
import csv
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import sedeval_ref as R
from challenge_amd import _native as N
from challenge_amd import metrics as M

F32 = np.float32
HOP, COLLAR = 256, 3200     # 200 ms at 16 kHz = 12.5 frames


def block_labels(rng, b, t, k, block=8, p=0.4):
    return np.repeat(rng.random((b, (t + block - 1) // block, k)) < p, block, axis=1)[:, :t].astype(F32)


def random_case(rng, b, t, k):
    """Block labels and sigmoid-like scores that follow them loosely."""
    yt = block_labels(rng, b, t, k)
    logits = (yt * 2 - 1) * 1.5 + rng.standard_normal((b, t, k)) * 2.0
    return yt, (1.0 / (1.0 + np.exp(-logits))).astype(F32)


def host(yt, yp, thresholds=(0.5,), **kw):
    return M.sed_counts_host(torch.from_numpy(np.asarray(yt, F32)), torch.from_numpy(np.asarray(yp, F32)), thresholds, **kw).numpy()


def row(t, *events):
    """[1, t, 1] with the frames of every (first, last) event set."""
    y = np.zeros((1, t, 1), F32)
    for s, e in events:
        y[0, s:e + 1, 0] = 1
    return y


def event_counts(ref_events, pred_events, t=400, **kw):
    yt, yp = row(t, *ref_events), row(t, *pred_events)
    got = host(yt, yp, **kw)
    assert np.array_equal(got, R.counts(yt, yp, (0.5,), **kw))
    return tuple(int(v) for v in got[0, 0, 3:])          # (ev_tp, ev_fp, ev_fn)


# ---------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_host_counts_equal_the_definition_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    b, t, k = int(rng.integers(1, 4)), int(rng.choice([1, 2, 63, 64, 65, 130, 301])), int(rng.integers(1, 5))
    thr = sorted({float(F32(h)) for h in rng.random(int(rng.integers(1, 5)))})
    yt, yp = random_case(rng, b, t, k)
    yp[rng.random(yp.shape) < 0.05] = F32(thr[0])          # scores exactly at a threshold
    yp[rng.random(yp.shape) < 0.02] = np.nan
    yt[rng.random(yt.shape) < 0.02] = np.nan
    for kw in ({}, dict(hop=100, segment=0.1, collar=0.05, offset_pct=0), dict(hop=8192, segment=1.0, offset_pct=100)):
        assert np.array_equal(host(yt, yp, thr, **kw), R.counts(yt, yp, thr, **kw)), kw


def test_constructed_rows():
    t = 130
    cases = {"all active": np.ones((1, t, 1), F32), "all inactive": np.zeros((1, t, 1), F32),
             "alternating": (np.arange(t) % 2 == 0).astype(F32).reshape(1, t, 1),
             "from frame 0, across 64, open at the end": row(t, (0, 3), (60, 70), (120, t - 1))}
    for name, yt in cases.items():
        for other in cases.values():
            got = host(yt, other * F32(0.5), (0.25, 0.5, 0.75))
            assert np.array_equal(got, R.counts(yt, other * F32(0.5), (0.25, 0.5, 0.75))), name
    got = host(cases["alternating"], cases["alternating"])
    assert got[0, 0, 3:].tolist() == [65, 0, 0]            # T / 2 events, each matched with itself


def test_onset_collar_edge():
    """hop 256, collar 3200 samples: 12 frames (3072) are within, 13 (3328) are not."""
    assert event_counts([(100, 199)], [(112, 199)]) == (1, 0, 0)
    assert event_counts([(100, 199)], [(88, 199)]) == (1, 0, 0)
    assert event_counts([(100, 199)], [(113, 199)]) == (0, 1, 1)
    assert event_counts([(100, 199)], [(87, 199)]) == (0, 1, 1)


def test_offset_collar_edge_and_the_fallback_to_the_collar():
    """A 100-frame reference event: 50 % of its length is 50 frames.  A 4-frame one: 2 frames < the 200 ms collar (12 frames)."""
    assert event_counts([(100, 199)], [(100, 249)]) == (1, 0, 0)
    assert event_counts([(100, 199)], [(100, 149)]) == (1, 0, 0)
    assert event_counts([(100, 199)], [(100, 250)]) == (0, 1, 1)
    assert event_counts([(100, 199)], [(100, 148)]) == (0, 1, 1)
    assert event_counts([(100, 103)], [(100, 115)]) == (1, 0, 0)
    assert event_counts([(100, 103)], [(100, 116)]) == (0, 1, 1)
    assert event_counts([(100, 199)], [(100, 211)], offset_pct=0) == (1, 0, 0)     # the collar alone
    assert event_counts([(100, 199)], [(100, 212)], offset_pct=0) == (0, 1, 1)


def test_greedy_takes_the_earliest_compatible_prediction():
    """One reference event, two predictions that may both match it: the earlier is taken, the later is an ev_fp; and a
    prediction that fails the offset condition is passed over, not used up."""
    assert event_counts([(100, 103)], [(95, 98), (100, 103)]) == (1, 1, 0)
    yt, yp = row(400, (100, 103)), row(400, (95, 98), (100, 103))
    ref_ev, pred_ev = R.runs(list(yt[0, :, 0] > 0)), R.runs(list(yp[0, :, 0] > 0))
    assert all(R.may_match(p, ref_ev[0], HOP, COLLAR, 50) for p in pred_ev)
    # a prediction within the onset collar that ends too early is passed over for the next one ...
    assert event_counts([(100, 199)], [(95, 100), (102, 199)]) == (1, 1, 0)
    # ... and stays free: it is within the onset collar of both reference events, ends too late for the first, suits the second
    assert event_counts([(100, 103), (110, 209)], [(108, 180)]) == (1, 0, 1)
    assert event_counts([(100, 199), (201, 204)], [(100, 120), (122, 199), (201, 204)]) == (1, 2, 1)


def three_class_example(frames_per_segment):
    """Four segments: a substitution (class 0 in the labels, class 1 predicted), a deletion, an insertion, a hit; then a
    partial fifth segment of 3 frames with a hit."""
    n = frames_per_segment
    yt, yp = np.zeros((1, 4 * n + 3, 3), F32), np.zeros((1, 4 * n + 3, 3), F32)
    yt[0, 1, 0] = yp[0, n - 1, 1] = 1            # segment 0: labels {0}, prediction {1}
    yt[0, n + 2, 2] = 1                          # segment 1: labels {2}, prediction {}
    yp[0, 2 * n, 0] = 1                          # segment 2: labels {}, prediction {0}
    yt[0, 3 * n:4 * n, 1] = yp[0, 4 * n - 1, 1] = 1   # segment 3: both {1}
    yt[0, 4 * n + 2, 2] = yp[0, 4 * n, 2] = 1    # partial segment 4: both {2}
    return yt, yp


def test_segment_bookkeeping_by_hand():
    # seg_samples 1600 at hop 100: 16 frames per segment; seg_samples 16000 at hop 256: 62.5 frames - segments of 63, 62, 63, 62
    # frames (frame f is in (f * 256) // 16000), so the example is laid out from the true boundaries
    yt, yp = three_class_example(16)
    got = host(yt, yp, hop=100, segment=0.1)
    assert np.array_equal(got, R.counts(yt, yp, (0.5,), hop=100, segment=0.1))
    assert got[0, 3].tolist() == [1, 1, 1, 5, 0, 0]                       # S, D, I, segments (the partial one counts)
    assert got[0, :3, :3].tolist() == [[0, 1, 1], [1, 1, 0], [1, 0, 1]]   # per class tp, fp, fn
    first = [0, 63, 125, 188, 250, 313]                                   # ceil(62.5 s)
    assert [(f * 256) // 16000 for f in first] == [0, 1, 2, 3, 4, 5] and [((f - 1) * 256) // 16000 for f in first[1:]] == [0, 1, 2, 3, 4]
    t = first[4] + 3
    yt, yp = np.zeros((1, t, 3), F32), np.zeros((1, t, 3), F32)
    yt[0, first[1] - 1, 0] = yp[0, 0, 1] = 1                              # segment 0, its last and first frame
    yt[0, first[1], 2] = 1                                                # segment 1, its first frame
    yp[0, first[3] - 1, 0] = 1                                            # segment 2, its last frame
    yt[0, first[3], 1] = yp[0, first[4] - 1, 1] = 1                       # segment 3
    yt[0, t - 1, 2] = yp[0, first[4], 2] = 1                              # partial segment 4
    got = host(yt, yp)
    assert np.array_equal(got, R.counts(yt, yp, (0.5,)))
    assert got[0, 3].tolist() == [1, 1, 1, 5, 0, 0]
    assert got[0, :3, :3].tolist() == [[0, 1, 1], [1, 1, 0], [1, 0, 1]]
    # segments restart with every clip: two clips of 70 frames are 2 + 2 segments, one clip of 140 frames is 3
    assert host(np.zeros((2, 70, 1), F32), np.zeros((2, 70, 1), F32))[0, 1, 3] == 4
    assert host(np.zeros((1, 140, 1), F32), np.zeros((1, 140, 1), F32))[0, 1, 3] == 3


def test_event_counts_agree_with_get_start_end_frame():
    """Anchor to existing code: per class, ev_tp + ev_fp is the number of runs Challenge_Metric.get_start_end_frame finds in the
    same decisions (and ev_tp + ev_fn in the labels)."""
    rng = np.random.default_rng(8)
    yt, yp = random_case(rng, 1, 500, 3)
    got = host(yt, yp)
    runs = M.Challenge_Metric().get_start_end_frame((yp[0] >= 0.5).astype(F32))
    assert [int(got[0, k, 3] + got[0, k, 4]) for k in range(3)] == [len(r) for r in runs]
    runs = M.Challenge_Metric().get_start_end_frame(yt[0])
    assert [int(got[0, k, 3] + got[0, k, 5]) for k in range(3)] == [len(r) for r in runs]
    assert min(len(r) for r in runs) > 3


def test_greedy_never_beats_an_optimal_matching():
    """The definition is greedy; sed_eval's default is an optimal bipartite matching.  greedy <= optimal on random rows with short
    events packed within a collar of each other (scripts/sed_greedy_vs_optimal.py runs the large sample DESIGN.md quotes)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    rng = np.random.default_rng(0)
    for _ in range(300):
        t = 120
        ref = R.runs(list(rng.random(t) < rng.choice([0.3, 0.5, 0.7])))
        pred = R.runs(list(rng.random(t) < rng.choice([0.3, 0.5, 0.7])))
        if not ref or not pred:
            continue
        graph = np.array([[R.may_match(p, r, HOP, COLLAR, 50) for p in pred] for r in ref], dtype=np.int8)
        optimal = int((maximum_bipartite_matching(csr_matrix(graph), perm_type='column') >= 0).sum())
        assert R.greedy_matches(ref, pred, HOP, COLLAR, 50) <= optimal


# ---------------------------------------------------------------------------
# ratios
# ---------------------------------------------------------------------------
def test_sed_metrics_on_hand_made_counts():
    nan = float('nan')
    counts = np.array([[[6, 2, 2, 3, 1, 2], [0, 0, 0, 0, 0, 0], [1, 0, 3, 0, 2, 1], [1, 2, 1, 10, 0, 0]],
                       [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 10, 0, 0]]], np.int64)
    out = M.sed_metrics(counts, (0.25, 0.5))
    seg, ev = out['per_threshold'][0]['segment'], out['per_threshold'][0]['event']
    assert seg['f1'] == 14 / (14 + 2 + 5) and seg['precision'] == 7 / 9 and seg['recall'] == 7 / 12
    assert seg['per_class']['f1'][0] == 12 / 16 and math.isnan(seg['per_class']['f1'][1]) and seg['per_class']['f1'][2] == 2 / 5
    assert seg['macro_f1'] == (12 / 16 + 2 / 5) / 2
    assert seg['er'] == 4 / 12 and seg['substitution_rate'] == 1 / 12 and seg['deletion_rate'] == 2 / 12 and seg['insertion_rate'] == 1 / 12
    assert seg['n_ref'] == 12 and seg['n_segments'] == 10
    assert ev['f1'] == 6 / (6 + 3 + 3) and ev['precision'] == 3 / 6 and ev['recall'] == 3 / 6 and ev['er'] == 6 / 6
    assert ev['per_class']['f1'] == [6 / 9, pytest.approx(nan, nan_ok=True), 0.0] and ev['macro_f1'] == (6 / 9 + 0.0) / 2
    assert ev['n_ref'] == 6 and ev['n_pred'] == 6
    empty = out['per_threshold'][1]
    for kind in ('segment', 'event'):
        assert all(math.isnan(empty[kind][n]) for n in ('f1', 'precision', 'recall', 'macro_f1', 'er'))
    assert math.isnan(empty['segment']['substitution_rate']) and empty['segment']['n_segments'] == 10
    assert out['thresholds'] == [0.25, 0.5] and out['best_event_f1_threshold'] == 0.25 and out['best_segment_f1_threshold'] == 0.25
    none = M.sed_metrics(counts[1:], (0.5,))
    assert math.isnan(none['best_event_f1_threshold']) and math.isnan(none['best_segment_f1_threshold'])
    two = np.stack([counts[1], counts[0]])
    assert M.sed_metrics(two, (0.25, 0.5))['best_event_f1_threshold'] == 0.5
    json.dumps(out)
    for bad in (counts.astype(np.float64), counts[:, :, :5], counts[0]):
        with pytest.raises(ValueError):
            M.sed_metrics(bad, (0.25, 0.5))
    with pytest.raises(ValueError):
        M.sed_metrics(counts, (0.5,))


# ---------------------------------------------------------------------------
# SedEval, sed_eval, MetricSet
# ---------------------------------------------------------------------------
def test_sed_eval_object_accumulates_and_refuses():
    rng = np.random.default_rng(4)
    yt, yp = random_case(rng, 2, 100, 3)
    thr = (0.3, 0.5, 0.7)
    sed = M.SedEval(3, thr)
    sed.update(torch.from_numpy(yt), torch.from_numpy(yp))
    sed.update(torch.from_numpy(yt[:1]).double(), torch.from_numpy(yp[:1]))
    want = R.counts(yt, yp, thr) + R.counts(yt[:1], yp[:1], thr)
    assert np.array_equal(sed.counts().numpy(), want) and sed.counts().dtype == torch.int64
    assert json.dumps(sed.compute()) == json.dumps(M.sed_metrics(want, sed.thresholds))      # (as text: NaN != NaN)
    sed.update(torch.zeros(0, 100, 3), torch.zeros(0, 100, 3))                      # an empty batch counts nothing
    assert np.array_equal(sed.counts().numpy(), want)
    for bad in ((torch.zeros(2, 100, 3), torch.zeros(2, 99, 3)), (torch.zeros(2, 100, 2), torch.zeros(2, 100, 2)),
                (torch.zeros(2, 100), torch.zeros(2, 100)), (torch.zeros(2, 100, 3, dtype=torch.int64), torch.zeros(2, 100, 3))):
        with pytest.raises(ValueError):
            sed.update(*bad)
    assert np.array_equal(sed.counts().numpy(), want)
    sed.reset()
    assert int(sed.counts().abs().sum()) == 0
    for kw in (dict(thresholds=()), dict(thresholds=tuple(i / 32 for i in range(17))), dict(thresholds=(0.5, 0.5)),
               dict(thresholds=(0.6, 0.5)), dict(thresholds=(0.5, float('nan'))), dict(thresholds=(float('inf'),)),
               dict(thresholds=(0.5, 0.5 + 1e-9)),                                   # equal as fp32
               dict(offset_pct=101), dict(offset_pct=-1), dict(offset_pct=12.5), dict(hop=0), dict(hop=256, segment=0.01),
               dict(collar=-0.1), dict(thresholds=0.5)):
        with pytest.raises(ValueError):
            M.SedEval(3, **kw)
        with pytest.raises(ValueError):
            M.sed_eval(**kw)
    for k in (0, 17):
        with pytest.raises(ValueError):
            M.SedEval(k)
    assert M.SedEval(16, tuple(i / 32 for i in range(16))).state('cpu').shape == (16, 17, 6)


def test_metric_set_feeds_the_counts_in_the_val_phase_only():
    rng = np.random.default_rng(3)
    yt, yp = random_case(rng, 4, 40, 3)
    yt, yp = torch.from_numpy(yt), torch.from_numpy(yp)
    sed = M.sed_eval((0.5, 0.7), hop=1600)
    ms = M.MetricSet([M.cos_sim, sed, M.er_score(smoothing=False), M.score_curves(64)])
    assert ms.sed is sed and sed not in ms.others
    out = ms(yt, yp, 'train')
    assert set(out) == {'cos_sim', 'er'} and sed.counter is None                        # nothing made, nothing counted
    assert set(ms.sed_values('val_')) == {'val_seg_f1', 'val_seg_er', 'val_event_f1'}
    assert all(math.isnan(v) for v in ms.sed_values('val_').values())
    assert set(ms(yt, yp, 'val')) == {'cos_sim', 'er'}                              # no per-step value
    ms(yt, yp, 'train')
    want = R.counts(yt.numpy(), yp.numpy(), (0.5, 0.7), hop=1600)
    assert np.array_equal(sed.counter.counts().numpy(), want)
    assert not any(t is s for t in ms.state_tensors() for s in sed.counter.states.values())
    first = M.sed_metrics(want, (0.5, 0.7))['per_threshold'][0]
    assert ms.sed_values('val_') == {'val_seg_f1': first['segment']['f1'], 'val_seg_er': first['segment']['er'],
                                     'val_event_f1': first['event']['f1']}
    assert M.SED_NAMES == ('seg_f1', 'seg_er', 'event_f1')
    ms.reset('train')
    assert int(sed.counter.counts().sum()) == int(want.sum())
    ms.reset()
    assert int(sed.counter.counts().sum()) == 0
    assert M.MetricSet([M.cos_sim]).sed_values('val_') == {}
    with pytest.raises(ValueError, match="sed_eval"):
        M.MetricSet([M.sed_eval(), M.sed_eval((0.3,))])
    with pytest.raises(TypeError):
        sed(yt, yp)


def test_iris_sed_counts_refuses_before_any_launch():
    lib = N.lib()
    p = C.c_void_p(64)
    INVALID, UNSUPPORTED = -1, -2
    big = C.c_size_t(1 << 40)

    def levels(*values):
        return (C.c_float * len(values))(*values)

    def call(yt=p, yp=p, b=1, t=64, k=3, thr=levels(0.5), n=1, hop=256, seg=16000, collar=3200, pct=50, ws=p, ws_bytes=big, counts=p):
        return lib.iris_sed_counts(yt, yp, b, t, k, thr, n, hop, seg, collar, pct, ws, ws_bytes, counts, None)

    def refused(rc, code):
        assert rc == code, (rc, lib.iris_last_error())
        assert lib.iris_last_error().startswith(b"iris_sed_"), lib.iris_last_error()
    for kw in (dict(yt=None), dict(yp=None), dict(thr=None), dict(ws=None), dict(counts=None), dict(b=0), dict(t=0), dict(k=0),
               dict(b=-1), dict(n=0), dict(n=17), dict(hop=0), dict(seg=255), dict(pct=-1), dict(pct=101), dict(collar=-1),
               dict(thr=levels(0.5, 0.5), n=2), dict(thr=levels(0.6, 0.5), n=2), dict(thr=levels(0.5, float('nan')), n=2),
               dict(thr=levels(float('inf')), n=1), dict(thr=levels(float('nan')), n=1), dict(ws=C.c_void_p(66)),
               dict(ws_bytes=C.c_size_t(0))):
        refused(call(**kw), INVALID)
    need = lib.iris_sed_workspace_bytes(1, 64, 3, 1, 256, 16000)
    # 3 rows x 2 lists: a count, 33 starts and 33 ends each (int32); 2 segments of 16-bit words per row
    assert need == 3 * 2 * 4 * (1 + 2 * 33) + 3 * 2 * 2
    refused(call(ws_bytes=C.c_size_t(need - 1)), INVALID)
    refused(call(k=17), UNSUPPORTED)
    refused(call(t=2 ** 20 + 1), UNSUPPORTED)
    refused(call(b=2 ** 12, t=2 ** 19), UNSUPPORTED)                                 # 2^31 frames
    assert lib.iris_sed_workspace_bytes(1, 64, 17, 1, 256, 16000) == 0 and lib.iris_sed_workspace_bytes(1, 64, 3, 0, 256, 16000) == 0
    assert lib.iris_sed_workspace_bytes(1, 64, 3, 1, 256, 255) == 0
    assert lib.iris_sed_workspace_bytes(64, 512, 3, 9, 256, 16000) == 192 * 10 * 4 * (1 + 2 * 257) + 192 * 9 * 2
    assert "iris_sed_counts" in N.SIGNATURES and lib.iris_abi_version() == 1


# ---------------------------------------------------------------------------
# fit, sj_train, evaluate
# ---------------------------------------------------------------------------
def _small(seed=3):
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(seed)
    return S, cfg, S.get_model(cfg)


def _batches(n, seed, rows=6):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 32, 64, 1, generator=g), (torch.rand(rows, 2, 3, generator=g) > 0.5).float()) for _ in range(n)]


def test_fit_rows_gain_exactly_the_three_names(tmp_path):
    from challenge_amd.dataset import Dataset
    hists, kept = {}, {}
    for tag in ("plain", "sed"):
        S, cfg, model = _small(seed=5)
        metric = M.sed_eval((0.5, 0.6), hop=S.output_hop(cfg)) if tag == "sed" else None
        model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                      metrics=[metric] if metric else None)
        train, val = _batches(3, 11), _batches(2, 12)

        class Keep:
            def on_epoch_end(self, epoch, m):
                m.eval()
                with torch.no_grad():
                    kept[(tag, epoch)] = torch.cat([m(x) for x, _ in val])
                m.train()
        hists[tag] = S.fit(model, Dataset.from_generator(lambda: iter(train)).repeat(), epochs=2, steps_per_epoch=2,
                           validation_data=Dataset.from_generator(lambda: iter(val)).repeat(), validation_steps=2,
                           csv_path=str(tmp_path / f"{tag}.csv"), verbose=False, callbacks=[Keep()])
    with open(tmp_path / "plain.csv") as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss']       # without it: the header of before
    with open(tmp_path / "sed.csv") as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss', 'val_seg_f1', 'val_seg_er', 'val_event_f1']
    yt = torch.cat([y for _, y in _batches(2, 12)]).numpy()
    for e, (r, base) in enumerate(zip(hists["sed"], hists["plain"])):
        assert set(r) - set(base) == {'val_seg_f1', 'val_seg_er', 'val_event_f1'}
        assert r['loss'] == base['loss'] and r['val_loss'] == base['val_loss']          # nothing else moved
        first = M.sed_metrics(R.counts(yt, kept[("sed", e)].numpy(), (0.5, 0.6), hop=8192), (0.5, 0.6))['per_threshold'][0]
        want = (first['segment']['f1'], first['segment']['er'], first['event']['f1'])
        got = (r['val_seg_f1'], r['val_seg_er'], r['val_event_f1'])
        assert all(g == w or (g != g and w != w) for g, w in zip(got, want)), (got, want)


def test_monitors_and_flags():
    from challenge_amd import fit as Fit
    from challenge_amd import sj_train as S
    assert Fit.monitor_maximised('val_event_f1') and Fit.monitor_maximised('val_seg_f1') and Fit.monitor_maximised('val_ema_event_f1')
    assert not Fit.monitor_maximised('val_seg_er') and not Fit.monitor_maximised('val_ema_seg_er')
    plain = S.ARGS().get([])
    assert plain.sed_eval == () and S.row_names(plain) == ['loss', 'val_loss']
    cfg = S.ARGS().get(['--sed_eval', '0.3,0.5', '--checkpoint_monitor', 'val_event_f1'])
    assert cfg.sed_eval == (float(F32(0.3)), 0.5) and cfg.checkpoint_monitor == 'val_event_f1'
    assert S.row_names(cfg) == ['loss', 'val_loss', 'val_seg_f1', 'val_seg_er', 'val_event_f1']
    assert S.run_name(cfg) == S.run_name(plain)                                          # not part of the run name
    both = S.ARGS().get(['--sed_eval', '0.5', '--curves', '64', '--ema', '0.9', '--checkpoint_monitor', 'val_seg_er'])
    assert S.row_names(both)[-6:] == ['val_ema_auc', 'val_ema_map', 'val_ema_best_f1', 'val_ema_seg_f1', 'val_ema_seg_er', 'val_ema_event_f1']
    assert S.ARGS().get(['--sed_eval', '0.5', '--checkpoint_monitor', 'val_seg_f1']).checkpoint_monitor == 'val_seg_f1'
    for bad in (['--sed_eval', '0.5,0.5'], ['--sed_eval', '0.7,0.5'], ['--sed_eval', 'half'], ['--sed_eval', ','.join(['0.5'] * 17)]):
        with pytest.raises(SystemExit):
            S.ARGS().get(bad)
    for bad in (['--checkpoint_monitor', 'val_event_f1'], ['--sed_eval', '0.5', '--checkpoint_monitor', 'val_ema_event_f1']):
        with pytest.raises(ValueError, match="checkpoint_monitor"):
            S.ARGS().get(bad)
    assert S.output_hop(S.ARGS().get(['--v', '9'])) == 8192 and S.output_hop(S.ARGS().get(['--v', '1'])) == 256


def test_main_with_sed_eval_logs_the_columns_and_checkpoints_on_them(tmp_path, monkeypatch):
    """`sj_train.main --sed_eval 0.5 --checkpoint_monitor val_event_f1 --ema 0.9` on the CPU (fixed batches stand in for the
    synthesis pipeline, which needs a device); without the flag the header is the one of before."""
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(S, "make_dataset", lambda config, training=True: Dataset.from_generator(
        lambda: iter(_batches(2, 20 + int(training), rows=2))).repeat())
    base = ['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--synthetic', '--epochs', '2', '--steps_per_epoch', '1',
            '--validation_steps', '1', '--batch_size', '2']
    S.main(['--name', 'sed'] + base + ['--sed_eval', '0.5', '--checkpoint_monitor', 'val_event_f1', '--ema', '0.9'])
    S.main(['--name', 'plain'] + base)
    name = S.run_name(S.ARGS().get(['--name', 'sed'] + base))
    with open(name.replace('.h5', '.csv')) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ['epoch', 'loss', 'lr', 'time', 'val_loss', 'val_seg_f1', 'val_seg_er', 'val_event_f1', 'val_ema_loss',
                             'val_ema_seg_f1', 'val_ema_seg_er', 'val_ema_event_f1']
    assert len(rows) == 2
    for k in ('val_seg_f1', 'val_event_f1', 'val_ema_seg_f1', 'val_ema_event_f1'):
        assert all(r[k] == 'nan' or 0.0 <= float(r[k]) <= 1.0 for r in rows), k
    assert all(r['val_seg_er'] == 'nan' or float(r['val_seg_er']) >= 0.0 for r in rows)
    assert os.path.exists(name.replace('.h5', '.pt')) or all(r['val_event_f1'] in ('nan', '0.0') for r in rows)
    with open(S.run_name(S.ARGS().get(['--name', 'plain'] + base)).replace('.h5', '.csv')) as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss']


def test_checkpoint_follows_event_f1_upwards_and_seg_er_downwards(tmp_path):
    from types import SimpleNamespace
    from challenge_amd import fit as Fit
    from challenge_amd.dataset import Dataset
    y = row(400, (100, 199))[0:1].repeat(3, axis=2)
    shifts = [30, 20, 20, 30, 5, 0]                     # onset error in frames (the collar is 12.5): event F1 0, 0, 0, 0, 1, 1

    class Stub:
        def __init__(self):
            self._ema = self._ddp = None
            self.optimizer = SimpleNamespace(param_groups=[{'lr': 0.1}])
            self._metrics = M.MetricSet([M.sed_eval((0.5,))])
            self.epoch, self.saved = 0, []

        def train_step(self, data):
            return {'loss': torch.tensor(1.0)}

        def test_step(self, data):
            s = shifts[self.epoch]
            yp = torch.from_numpy(row(400, (100 + s, 199 + 4 * s)).repeat(3, axis=2))
            out = {'loss': torch.tensor(float(self.epoch + 1)), **self._metrics(torch.from_numpy(y), yp, 'val')}
            self.epoch += 1
            return out

        def state_dict(self):
            self.saved.append(self.epoch - 1)
            return {'epoch': torch.tensor(self.epoch - 1)}
    ds = Dataset.from_generator(lambda: iter([(torch.zeros(1), torch.zeros(1))])).repeat()

    def run(monitor):
        stub = Stub()
        hist = Fit.fit(stub, ds, epochs=len(shifts), steps_per_epoch=1, validation_data=ds, validation_steps=1, graph=False,
                       checkpoint_path=str(tmp_path / "stub.pt"), checkpoint_monitor=monitor, verbose=False)
        return stub, hist
    stub, hist = run('val_event_f1')                   # the loss gets worse all along: only the monitor can cause a save
    assert [r['val_event_f1'] for r in hist] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    assert stub.saved == [0, 4]                         # strictly larger only
    # the labels cover segments 1 .. 3 (frames 100 .. 199, boundaries at 63, 125, 188, 250, 313): a shift of 30 loses segment 1
    # and adds segments 4 and 5, a shift of 20 adds segment 4, shifts of 5 and 0 cover the same segments
    stub, hist = run('val_seg_er')
    assert [r['val_seg_er'] for r in hist] == [1.0, 1 / 3, 1 / 3, 1.0, 0.0, 0.0]
    assert stub.saved == [0, 1, 4]                      # strictly smaller only


def test_eval_takes_a_file_for_sed_eval():
    from challenge_amd import eval as E
    cfg = E.build_args().get(['--name', 'run', '--sed_eval', 'out.json'])
    assert cfg.sed_eval == 'out.json' and cfg.sed_thresholds == (0.5,) and cfg.curves is None
    assert E.build_args().get(['--name', 'run']).sed_eval is None
    assert E.build_args().get(['--name', 'run', '--sed_eval', 'o.json', '--sed_thresholds', '0.25,0.5']).sed_thresholds == (0.25, 0.5)


def test_evaluate_feeds_the_posteriors_and_the_answer_labels(tmp_path, monkeypatch):
    """A stub in place of the recording -> features -> model chain (known posteriors per file): the counts are those of the
    posteriors against second2frame's labels, one [1, T, 3] update per file, and the scores are the ones of a run without `sed`;
    `eval --sed_eval OUT.json` writes compute()."""
    from challenge_amd import data_utils as D
    from challenge_amd import eval as E
    from challenge_amd import inference as I
    from challenge_amd import sj_train as S
    rng = np.random.default_rng(5)
    t = 188                                                # 3 s at 62.5 frames per second
    post = {f"clip{i}": torch.from_numpy(rng.random((t, 3)).astype(F32)) for i in range(2)}
    post["clip0"][:70, 0] = 0.9
    answers = {"clip0": [[0, 0, 1], [1, 1, 2], [1, 1, 3]], "clip1": [[2, 0, 3]]}
    for n in post:
        (tmp_path / f"{n}.wav").write_bytes(b"")
    with open(tmp_path / "sample_answer.json", "w") as f:
        json.dump({"task2_answer": answers}, f)
    monkeypatch.setattr(D, "load_wav", lambda path, device=None: os.path.basename(path)[:-4])
    monkeypatch.setattr(I, "features_for_eval", lambda spec, config: spec)

    def predict_frames(model, features, config, overlap_hop=512, batch_size=32, smoothing=True, threshold=True):
        p = post[features]
        return (p >= 0.5).to(torch.float32) if threshold else p
    monkeypatch.setattr(I, "predict_frames", predict_frames)
    cfg = S.ARGS().get(['--v', '9'])
    kw = dict(wav_dir=str(tmp_path), answer_path=str(tmp_path / "sample_answer.json"), device=torch.device("cpu"))
    plain = M.evaluate(cfg, None, **kw)
    thr = (0.25, 0.5)
    sed, hist = M.SedEval(3, thr), M.ScoreHistogram(3, 64)
    assert M.evaluate(cfg, None, sed=sed, **kw) == plain
    want = sum(R.counts(E.second2frame(answers[n], t, 16000 / 256).numpy()[None], post[n].numpy()[None], thr) for n in sorted(post))
    assert np.array_equal(sed.counts().numpy(), want) and int(want[0, 3, 3]) == 2 * 3    # 188 frames: frame 187 starts at 2.992 s
    sed.reset()
    assert M.evaluate(cfg, None, sed=sed, curves=hist, **kw) == plain                    # both at once
    assert np.array_equal(sed.counts().numpy(), want) and int(hist.counts().sum()) == 2 * t * 3
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(E, "load_model", lambda config, path='', device=None: None)
    monkeypatch.setattr(E, "evaluate", lambda config, model, **k: M.evaluate(config, model, **k, **kw))
    assert E.main(['--name', 'run', '--v', '9', '--sed_eval', 'out.json', '--sed_thresholds', '0.25,0.5']) == plain
    with open(tmp_path / "out.json") as f:
        out = json.load(f)
    assert json.dumps(out) == json.dumps(M.sed_metrics(want, thr)) and len(out['per_threshold']) == 2
    assert not os.path.exists(tmp_path / "curves.json")
