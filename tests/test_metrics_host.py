"""CPU tests of challenge_amd.metrics / challenge_amd.eval (the reference's metrics.py and eval.py) and of the compiled
metrics in the training surface.  `ref_er` below restates the reference's er_score op by op in NumPy (np.argwhere for
tf.where, stable argsorts by class then clip, the [:, ::2] (clip, class) equality, the time window, reduce_max over the
predictions); the GPU tests import it too."""
import json
import math
import os

import numpy as np
import pytest
import torch

from challenge_amd import metrics as M
from challenge_amd import sj_train as S
from challenge_amd import trainer as TR
from challenge_amd.dataset import Dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------
# independent restatement of reference metrics.py:217-274
# ---------------------------------------------------------------------------
def ref_avg_pool_same(x, k):
    """AveragePooling1D(k, padding='same'), stride k, on [B, T, K] fp32: mean over the in-range frames, summed in order."""
    b, t, c = x.shape
    out = -(-t // k)
    pad_before = max((out - 1) * k + k - t, 0) // 2
    y = np.zeros((b, out, c), np.float32)
    for i in range(out):
        lo, hi = max(i * k - pad_before, 0), min(i * k - pad_before + k, t)
        acc = np.zeros((b, c), np.float32)
        for f in range(lo, hi):
            acc = (acc + x[:, f, :]).astype(np.float32)
        y[:, i, :] = acc / np.float32(hi - lo)
    return y


def _events(x):
    starts = np.clip(x - np.pad(x, [[0, 0], [1, 0], [0, 0]])[:, :-1], 0, 1)
    ends = np.clip(x - np.pad(x, [[0, 0], [0, 1], [0, 0]])[:, 1:], 0, 1)
    n = starts.astype(np.float32).sum((1, 2), dtype=np.float32)

    def order(a):
        a = a[np.argsort(a[:, -1], kind="stable")]   # tf.gather(x, argsort(x[:, -1]), -1): -1 is validate_indices
        return a[np.argsort(a[:, 0], kind="stable")]
    return n, order(np.argwhere(starts)), order(np.argwhere(ends))


def ref_er(y_true, y_pred, threshold=0.5, smoothing=True):
    thr = np.float32(threshold)
    y_true = np.asarray(y_true, np.float32)
    y_pred = np.asarray(y_pred, np.float32)
    yt = (y_true >= thr).astype(np.int32)
    if smoothing:
        y_pred = ref_avg_pool_same(y_pred, int(0.5 * 16000) // 256)
    yp = (y_pred >= thr).astype(np.int32)
    n_true, true_starts, true_ends = _events(yt)
    n_pred, pred_starts, pred_ends = _events(yp)
    middle = ((pred_starts + pred_ends) / 2).astype(np.int64)
    correct = true_starts[:, ::2, None] == middle.T[None, ::2]
    correct = correct.astype(np.float32).min(axis=1)
    mid_time = middle[:, 1:2].T
    correct = correct * (true_starts[:, 1:2] <= mid_time).astype(np.float32)
    correct = correct * (true_ends[:, 1:2] >= mid_time).astype(np.float32)
    correct = np.pad(correct, [[0, 0], [0, 1]]).max(-1)
    per_sample = (np.eye(y_true.shape[0], dtype=np.float32)[true_starts[:, 0]] * correct[:, None]).sum(0, dtype=np.float32)
    score = (n_true + n_pred - np.float32(2) * per_sample).astype(np.float32)
    m = n_true.max() if n_true.size else np.float32(0)
    return (score / np.maximum(np.minimum(n_true, m), np.float32(1))).astype(np.float32)   # clip_by_value(n, 1, max n)


def adversarial_cases(rng, b, t, k):
    """(y_true, y_pred) pairs covering the edge cases of the event matching."""
    cases = []
    cases.append(((rng.random((b, t, k)) > 0.6).astype(np.float32), rng.random((b, t, k)).astype(np.float32)))
    yt = np.zeros((b, t, k), np.float32)
    yt[:, : max(1, t // 4)] = 1
    yt[:, t - max(1, t // 5):] = 1                                     # runs touching frame 0 and frame T-1
    cases.append((yt, yt[:, ::-1].copy()))
    cases.append((np.ones((b, t, k), np.float32), np.ones((b, t, k), np.float32)))        # all ones
    cases.append((np.zeros((b, t, k), np.float32), np.zeros((b, t, k), np.float32)))      # no events anywhere
    alt = np.zeros((b, t, k), np.float32)
    alt[:, ::2] = 1                                                                         # alternating frames
    cases.append((alt, alt[:, ::-1].copy()))
    cases.append((alt, 1 - alt))
    yt = np.zeros((b, t, k), np.float32)
    yt[0, t // 3: 2 * t // 3 + 1, 0] = 1                                                   # one clip has events, others none
    yp = np.zeros((b, t, k), np.float32)
    yp[0, t // 3: 2 * t // 3 + 1, k - 1] = 1                                               # ... predicted in another class
    if b > 1:
        yp[1, t // 3: 2 * t // 3 + 1, 0] = 1                                               # ... and in another clip
    cases.append((yt, yp))
    yt = np.zeros((b, t, k), np.float32)
    yt[:, 0:t] = 1
    yp = np.zeros((b, t, k), np.float32)
    yp[:, 1: max(2, t // 4)] = 1
    yp[:, t // 2: t // 2 + 2] = 1                                                          # two middles in one true run
    cases.append((yt, yp))
    y = rng.random((b, t, k)).astype(np.float32)                                           # values on the threshold, NaN
    y[:, ::7] = 0.5
    y[:, 3::11] = 0.3
    yp = y.copy()
    yp[:, 5::13] = np.nan
    cases.append(((y > 0.45).astype(np.float32), yp))
    return cases


def test_reference_kat():
    kat = json.load(open(os.path.join(GOLDEN, "metrics_kat.json")))
    gt = np.zeros([2, kat["n_frame"], 3], np.float32)
    pred = np.zeros([2, kat["n_frame"], 3], np.float32)
    for c, s, e in kat["gt"]:
        gt[:, s:e, c] = 1
    for c, m in kat["predict"]:
        pred[:, m - 2:m + 2, c] = 1
    er = M.er_score(smoothing=False)(torch.from_numpy(gt), torch.from_numpy(pred))
    assert er.dtype == torch.float32 and er.shape == (2,)
    assert er.tolist() == pytest.approx([kat["expected_mean_er"]] * 2, abs=1e-6)
    assert float(er.mean()) == pytest.approx(1.2, abs=1e-6)
    assert np.array_equal(ref_er(gt, pred, smoothing=False), er.numpy())


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("smoothing", [False, True])
def test_er_host_matches_restatement_bitwise(k, threshold, smoothing):
    rng = np.random.default_rng(10 * k + int(threshold * 10) + smoothing)
    for b, t in ((1, 1), (3, 40), (4, 97), (2, 200)):
        for yt, yp in adversarial_cases(rng, b, t, k):
            if smoothing:   # pooled-rate patterns too (smoothing compares pooled middles with full-rate frames)
                yp = np.repeat(yp, 31, axis=1)[:, : t]
            got = M.er_score(threshold, smoothing)(torch.from_numpy(yt), torch.from_numpy(yp)).numpy()
            ref = ref_er(yt, yp, threshold, smoothing)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32)), (b, t, got, ref)


def test_er_accepts_predictions_at_another_rate():
    rng = np.random.default_rng(3)
    yt = (rng.random((3, 62, 3)) > 0.5).astype(np.float32)
    yp = rng.random((3, 5, 3)).astype(np.float32)
    assert np.array_equal(M.er_host(torch.from_numpy(yt), torch.from_numpy(yp)).numpy(), ref_er(yt, yp, smoothing=False))


def test_f1_score_is_cumulative_and_strict():
    f1 = M.f1_score()
    yt = torch.tensor([[[1., 0., 1.], [0., 1., 0.]]])
    yp = torch.tensor([[[0.9, 0.5, 0.2], [0.6, 0.7, 0.1]]])   # 0.5 is not positive (tfa: y_pred > threshold)
    v1 = float(f1(yt, yp))
    tp, fp, fn = 2.0, 1.0, 1.0
    assert v1 == pytest.approx(2 * tp / (2 * tp + fp + fn), abs=1e-7)
    yt2 = torch.tensor([[[0., 0., 1.], [1., 1., 0.]]])
    yp2 = torch.tensor([[[0.1, 0.2, 0.9], [0.1, 0.2, 0.8]]])   # tp 1, fp 1, fn 2
    v2 = float(f1(yt2, yp2))
    tp, fp, fn = 3.0, 2.0, 3.0
    p, r = tp / (tp + fp), tp / (tp + fn)
    assert v2 == pytest.approx(2 * p * r / (p + r), abs=1e-7)
    assert M.f1_score()(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3)).item() == 0.0   # div-no-nan


def test_cos_sim_is_trainer_cos_sim():
    rng = np.random.default_rng(4)
    yt = torch.from_numpy((rng.random((4, 16, 3)) > 0.5).astype(np.float32))
    yt[1, :, 2] = 0
    yp = torch.from_numpy(rng.random((4, 16, 3)).astype(np.float32))
    assert torch.equal(M.cos_sim(yt, yp), TR.cos_sim(yt, yp))
    assert M.cos_sim is TR.cos_sim


def test_get_start_end_frame_odd_toggles():
    d = np.zeros((10, 3), np.float32)
    d[2:5, 0] = 1
    d[7:, 0] = 1          # open at the end: closes at the last frame
    d[0:1, 2] = 1
    c0, c1, c2 = M.Challenge_Metric().get_start_end_frame(d)
    assert c0.tolist() == [[2, 4], [7, 9]]
    assert c1.shape == (0, 2)
    assert c2.tolist() == [[0, 0]]


def test_output_to_metric_truncates():
    rows = M.output_to_metric(256, 16000)(np.array([[2, 4]]), np.zeros((0, 2)), np.array([[100, 131], [62, 63]]))
    assert rows.dtype == np.int32
    assert rows.tolist() == [[0, int(3 * 256 / 16000)], [2, int(115.5 * 256 / 16000)], [2, int(62.5 * 256 / 16000)]]
    assert rows.tolist() == [[0, 0], [2, 1], [2, 1]]


def test_get_er_greedy_and_class_mismatch():
    gt = [[0, 10, 20], [0, 12, 18]]
    assert M.get_er(gt, [[0, 15]]) == (3 - 2) / 2               # one prediction cannot match two events
    assert M.get_er(gt, [[0, 15], [0, 16]]) == 0.0
    assert M.get_er([[1, 10, 20]], [[0, 15]]) == 2.0             # class mismatch
    assert M.get_er([[2, 5, 8]], [[2, 8], [2, 5]]) == 1.0        # boundaries inclusive; the earliest match is taken
    with pytest.raises(ZeroDivisionError):
        M.get_er(np.zeros((0, 3)), [[0, 1]])


def test_reference_kat_through_the_scoring_helpers():
    kat = json.load(open(os.path.join(GOLDEN, "metrics_kat.json")))
    assert M.get_er(kat["gt"], kat["predict"]) == pytest.approx((10 - 2 * 2) / 5)   # two events matched
    answers = json.load(open(os.path.join(GOLDEN, "sample_answer.json")))["task2_answer"]
    assert all(len(e) == 3 for v in answers.values() for e in v)


def test_extract_middle_order():
    y = np.zeros((2, 10, 2), np.float32)
    y[0, 6:9, 0] = 1
    y[0, 1:3, 1] = 1
    y[0, 0:2, 0] = 1
    y[1, 4:5, 1] = 1
    assert M.extract_middle(y).tolist() == [[0, 0, 0], [0, 7, 0], [0, 1, 1], [1, 4, 1]]


def test_second2frame():
    from challenge_amd.eval import parse_name, second2frame
    f = second2frame([[1, 0.5, 1.0], [1, 0.75, 1.5]], 8, 4).numpy()
    assert f[:, 1].tolist() == [0, 0, 1, 2, 1, 1, 0, 0] and f[:, [0, 2]].sum() == 0
    cfg = S.ARGS().get(['--name', 'vad_v8_lr0.001_batch12_opt_adam_mel80_chan2_BCE_framelen512'])
    parse_name(cfg)
    assert (cfg.model_type, cfg.v, cfg.n_mels, cfg.n_chan, cfg.n_frame) == ('vad', 8, 80, 2, 512)


def test_iris_event_metrics_rejects_bad_arguments():
    from challenge_amd import _native as N
    lib = N.lib()
    x = torch.zeros(64)
    p = x.data_ptr()
    o = torch.zeros(8)
    for b, t, tp, k in ((1, 4, 4, 0), (1, 4, 4, 17), (1, 0, 4, 3), (1, 8193, 8193, 3), (0, 4, 4, 3), (1, 4, 8193, 3)):
        st = lib.iris_event_metrics(p, p, b, t, tp, k, 0.5, 0, 0.5, o.data_ptr(), None, None, None, None, None, None, None)
        assert st < 0, (b, t, tp, k)
        assert b"iris_event_metrics" in lib.iris_last_error()
    assert lib.iris_event_metrics(None, p, 1, 4, 4, 3, 0.5, 0, 0.5, o.data_ptr(), None, None, None, None, None, None, None) < 0
    assert lib.iris_event_metrics(p, p, 1, 4, 4, 3, 0.5, 0, 0.5, None, None, None, None, None, None, None, None) < 0
    s3 = torch.zeros(3, dtype=torch.float64)
    st = lib.iris_event_metrics(p, p, 1, 4, 4, 3, 0.5, 0, 0.5, o.data_ptr(), None, s3.data_ptr(), o.data_ptr(), None, None,
                                None, None)   # F1 state without slab / ticket
    assert st < 0 and b"slab" in lib.iris_last_error()
    st = lib.iris_event_metrics(p, p, 1, 4, 5, 3, 0.5, 0, 0.5, o.data_ptr(), o.data_ptr(), None, None, None, None, None, None)
    assert st < 0 and b"label rate" in lib.iris_last_error()
    with pytest.raises(ValueError):
        N.check(lib.iris_event_metrics(p, p, 1, 4, 4, 17, 0.5, 0, 0.5, o.data_ptr(), None, None, None, None, None, None, None),
                "iris_event_metrics")


def test_sj_train_metrics_flag():
    assert S.ARGS().get([]).metrics == 'none'
    assert S.ARGS().get(['--metrics', 'reference']).metrics == 'reference'
    with pytest.raises(SystemExit):
        S.ARGS().get(['--metrics', 'all'])


# ---------------------------------------------------------------------------
# training surface
# ---------------------------------------------------------------------------
def _small_cfg():
    return S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '2'])


def test_train_and_test_step_return_metrics_from_the_loss_predictions():
    torch.manual_seed(0)
    cfg = _small_cfg()
    m = S.get_model(cfg)
    f1 = M.f1_score()
    m.compile(S.make_optimizer(cfg, m.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
              metrics=[M.cos_sim, f1, M.er_score(smoothing=False)])
    x, y = torch.randn(3, 32, 64, 1), (torch.rand(3, 2, 3) > 0.5).float()
    m.eval()
    with torch.no_grad():
        y_pred = m(x)
    r = m.test_step((x, y))
    assert list(r) == ['loss', 'cos_sim', 'f1_score', 'er']
    assert torch.equal(r['er'], M.er_host(y, y_pred)) and torch.equal(r['cos_sim'], TR.cos_sim(y, y_pred))
    assert torch.equal(f1.states[torch.device('cpu')], M.f1_counts_host(y, y_pred))
    t = m.train_step((x, y))
    assert set(t) == {'loss', 'cos_sim', 'f1_score', 'er'} and t['er'].shape == (3,)


def test_fit_rows_and_checkpoint_monitor(tmp_path):
    torch.manual_seed(1)
    cfg = _small_cfg()
    m = S.get_model(cfg)
    m.compile(S.make_optimizer(cfg, m.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
              metrics=[M.cos_sim, M.f1_score(), M.er_score(smoothing=False)])
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 32, 64, 1, generator=g), (torch.rand(4, 2, 3, generator=g) > 0.5).float()) for _ in range(3)]
    ds = Dataset.from_generator(lambda: iter(batches)).repeat()
    vb = [(torch.randn(4, 32, 64, 1, generator=g), (torch.rand(4, 2, 3, generator=g) > 0.5).float()) for _ in range(2)]
    vds = Dataset.from_generator(lambda: iter(vb)).repeat()
    snaps = []

    class Snap:
        def on_epoch_end(self, epoch, model):
            snaps.append({k: v.clone() for k, v in model.state_dict().items()})
    hist = S.fit(m, ds, epochs=6, steps_per_epoch=2, validation_data=vds, validation_steps=2, csv_path=str(tmp_path / 'log.csv'),
                 checkpoint_path=str(tmp_path / 'm.pt'), patience=2, verbose=False, checkpoint_monitor='val_er',
                 callbacks=[Snap()])
    for row in hist:
        for key in ('er', 'val_er', 'f1_score', 'val_f1_score', 'cos_sim', 'val_cos_sim', 'loss', 'val_loss'):
            assert key in row and math.isfinite(row[key]), (key, row)
    header = open(tmp_path / 'log.csv').readline().strip().split(',')
    assert {'er', 'val_er', 'f1_score', 'cos_sim'} <= set(header)
    # checkpoint: the last epoch whose val_er beat every earlier one (strictly)
    best, want = math.inf, None
    for i, row in enumerate(hist):
        if row['val_er'] < best:
            best, want = row['val_er'], i
    saved = torch.load(tmp_path / 'm.pt')
    assert all(torch.equal(saved[k], snaps[want][k]) for k in saved)
    # early stopping still follows val_loss (patience 2)
    best, bad, stop_at = math.inf, 0, None
    for i, row in enumerate(hist):
        if row['val_loss'] < best:
            best, bad = row['val_loss'], 0
        else:
            bad += 1
            if bad >= 2:
                stop_at = i
                break
    assert len(hist) == (stop_at + 1 if stop_at is not None else 6)


def test_fit_val_er_is_the_clip_weighted_mean():
    torch.manual_seed(2)
    cfg = _small_cfg()
    m = S.get_model(cfg)
    er = M.er_score(smoothing=False)
    m.compile(S.make_optimizer(cfg, m.parameters()), S.binary_crossentropy, metrics=[er])
    g = torch.Generator().manual_seed(6)
    vb = [(torch.randn(n, 32, 64, 1, generator=g), (torch.rand(n, 2, 3, generator=g) > 0.5).float()) for n in (3, 1)]
    vds = Dataset.from_generator(lambda: iter(vb)).repeat()
    hist = S.fit(m, vds, epochs=1, steps_per_epoch=1, validation_data=vds, validation_steps=2, verbose=False)
    m.eval()
    with torch.no_grad():
        vals = torch.cat([M.er_host(y, m(x)) for x, y in vb])
    assert hist[0]['val_er'] == pytest.approx(float(vals.double().mean()), abs=1e-12)


def test_fit_without_metrics_keeps_todays_row():
    torch.manual_seed(0)
    cfg = _small_cfg()
    m = S.get_model(cfg)
    m.compile(S.make_optimizer(cfg, m.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue)
    x, y = torch.randn(2, 32, 64, 1), (torch.rand(2, 2, 3) > 0.8).float()
    ds = Dataset.from_generator(lambda: iter([(x, y)])).repeat()
    hist = S.fit(m, ds, epochs=1, steps_per_epoch=1, validation_data=ds, validation_steps=1, verbose=False)
    assert list(hist[0]) == ['epoch', 'loss', 'lr', 'time', 'val_loss']
    assert set(m.train_step((x, y))) == {'loss'} and set(m.test_step((x, y))) == {'loss'}


def test_metric_names_must_be_unique():
    with pytest.raises(ValueError, match="unique"):
        M.MetricSet([M.er_score(smoothing=False), M.er_score(threshold=0.3)])
    with pytest.raises(ValueError, match="unique"):
        M.MetricSet([M.f1_score(), M.f1_score()])


# ---------------------------------------------------------------------------
# the count states of the validation pass: one contract for ScoreHistogram, SedEval and Psds
# ---------------------------------------------------------------------------
_LEVELS = (0.3, 0.6)
COUNTERS = {   # public name -> (a fresh object for 3 classes, the class's host rule with the same parameters)
    'ScoreHistogram': (lambda: M.ScoreHistogram(3, 16), lambda yt, yp: M.score_hist_host(yt, yp, 16)),
    'SedEval': (lambda: M.SedEval(3, _LEVELS, hop=1600), lambda yt, yp: M.sed_counts_host(yt, yp, _LEVELS, hop=1600)),
    'Psds': (lambda: M.Psds(3, 2, _LEVELS), lambda yt, yp: M.psds_counts_host(yt, yp, _LEVELS, dtc_pct=10, gtc_pct=10, cttc_pct=30)),
}


def _count_case():
    """B = 2, T = 16, K = 3: block labels (events of 4 frames) and scores that follow them loosely."""
    g = torch.Generator().manual_seed(3)
    yt = (torch.rand(2, 4, 3, generator=g) < 0.5).float().repeat_interleave(4, dim=1)
    yp = (0.6 * yt + 0.5 * torch.rand(2, 16, 3, generator=g)).clamp(0, 1)
    return yt, yp


@pytest.mark.parametrize("name", sorted(COUNTERS))
def test_count_states_share_one_contract(name):
    make, host_rule = COUNTERS[name]
    yt, yp = _count_case()
    want = host_rule(yt, yp)
    assert want.dtype == torch.int64 and int(want.sum()) > 0
    c, other = make(), make()
    assert type(c).__name__ == name and int(c.counts().sum()) == 0 and not c.states
    c.update(yt[:1], yp[:1])
    c.update(yt[1:], yp[1:])                                      # two updates = one on the concatenation
    assert torch.equal(c.counts(), want) and tuple(c.counts().shape) == tuple(want.shape)
    assert torch.equal(c.total(), want)
    assert int(other.counts().sum()) == 0 and not other.states    # a second object shares nothing
    other.update(yt, yp)
    assert torch.equal(other.counts(), want) and torch.equal(c.counts(), want)
    bad = [(yt[0], yp[0]),                                        # rank
           (yt, yp[:, :8]),                                       # shape
           (yt[:, :, :2], yp[:, :, :2]),                          # class count
           (yt.long(), yp),                                       # dtype
           (yt.to('meta'), yp)]                                   # device
    for a, b in bad:
        with pytest.raises(ValueError) as exc:
            c.update(a, b)
        assert str(exc.value).startswith(name + ".update: "), exc.value
        assert torch.equal(c.counts(), want)                      # the state is left untouched
    c.update(yt[:0], yp[:0])                                      # an empty batch: nothing
    assert torch.equal(c.counts(), want)
    with pytest.raises(ValueError) as exc:
        type(c)(17)
    assert str(exc.value).startswith(name + ": n_classes")
    c.reset()
    assert int(c.counts().abs().sum()) == 0 and torch.equal(other.counts(), want)
    c.update(yt, yp)
    assert torch.equal(c.counts(), want) and c.compute() == other.compute() == c.metrics(want)


def test_val_values_is_the_union_of_the_three_readers_in_row_order():
    """All three count metrics compiled in REVERSE order: the rows keep curves, sed, psds."""
    def same(a, b):
        return list(a) == list(b) and all(x == y or (x != x and y != y) for x, y in zip(a.values(), b.values()))
    score, sed, curves = M.psds(2, _LEVELS, hop=1600), M.sed_eval(_LEVELS, hop=1600), M.score_curves(16)
    ms = M.MetricSet([score, M.cos_sim, sed, curves])
    assert ms.counted == [curves, sed, score] and (ms.curves, ms.sed, ms.psds) == (curves, sed, score) and ms.others == []
    keys = ['val_auc', 'val_map', 'val_best_f1', 'val_seg_f1', 'val_seg_er', 'val_event_f1', 'val_psds']
    assert keys == ['val_' + n for n in M.CURVE_NAMES + M.SED_NAMES + M.PSDS_NAMES]
    yt, yp = _count_case()
    for _ in range(2):                                            # before the first 'val' call, and after 'train' calls: all NaN
        vals = ms.val_values('val_')
        assert list(vals) == keys and all(math.isnan(v) for v in vals.values())
        assert set(ms(yt, yp, 'train')) == {'cos_sim'} and all(m.counter is None for m in ms.counted)
    assert set(ms(yt, yp, 'val')) == {'cos_sim'}
    vals = ms.val_values('val_')
    union = {**ms.curve_values('val_'), **ms.sed_values('val_'), **ms.psds_values('val_')}
    assert list(vals) == keys and same(vals, union) and any(math.isfinite(v) for v in vals.values())
    assert vals['val_psds'] == score.counter.compute()['psds'] and vals['val_auc'] == curves.counter.compute()['auc']
    assert vals['val_seg_er'] == sed.counter.compute()['per_threshold'][0]['segment']['er']
    ms(yt, 1 - yp, 'train')                                       # a 'train' call counts nothing
    assert same(ms.val_values('val_'), vals)
    assert same(ms.val_values('val_ema_'), {'val_ema_' + k[4:]: v for k, v in vals.items()})
    assert M.MetricSet([M.cos_sim]).val_values('val_') == {}
    ms.reset('train')
    assert same(ms.val_values('val_'), vals)
    ms.reset('val')
    assert all(int(m.counter.counts().sum()) == 0 for m in ms.counted)


def test_main_with_reference_metrics_needs_the_answer_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IRIS_FORCE_PG"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(FileNotFoundError, match="sample_answer.json"):
        S.main(['--metrics', 'reference', '--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--synthetic',
                '--epochs', '1', '--steps_per_epoch', '1'])
