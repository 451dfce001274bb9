"""CPU tests of the polyphonic sound detection score (metrics.psds_counts_host / Psds / psds / psds_metrics) and of what `fit` and
`sj_train` do with it.  Counts are integers: every comparison with tests/psds_ref.py (plain loops over event lists and interval
intersections) is for EQUALITY."""
import csv
import json
import math

import numpy as np
import pytest
import torch

import psds_ref as R
from challenge_amd import metrics as M

F32 = np.float32
SCENARIOS = {1: dict(dtc_pct=70, gtc_pct=70, cttc_pct=None), 2: dict(dtc_pct=10, gtc_pct=10, cttc_pct=30)}


def block_case(rng, b, t, k, block=8, p=0.4, hold=4):
    """Block labels and sigmoid-like scores that follow them loosely and are HELD for `hold` frames (independent noise per frame
    would give one-frame runs only)."""
    yt = np.repeat(rng.random((b, (t + block - 1) // block, k)) < p, block, axis=1)[:, :t].astype(F32)
    noise = np.repeat(rng.standard_normal((b, (t + hold - 1) // hold, k)), hold, axis=1)[:, :t]
    mixed = np.roll(yt, 1, axis=2) if k > 1 else 0.0            # some weight on the neighbouring class: cross-triggers
    logits = (yt * 2 - 1) * 1.5 + mixed * 1.5 + noise * 2.0
    return yt, (1.0 / (1.0 + np.exp(-logits))).astype(F32)


def host(yt, yp, thr, **kw):
    return M.psds_counts_host(torch.from_numpy(np.asarray(yt, F32)), torch.from_numpy(np.asarray(yp, F32)), thr, **kw).numpy()


def worked_example():
    yt, yp = np.zeros((1, 20, 2), F32), np.zeros((1, 20, 2), F32)
    yt[0, 2:12, 0] = 1
    yt[0, 14:18, 1] = 1
    yp[0, 3:7, 0] = yp[0, 8:13, 0] = 0.9
    yp[0, 15:19, 0] = 0.6
    yp[0, :, 1] = 0.3
    yp[0, 14:17, 1] = 0.8
    return yt, yp, (0.25, 0.5, 0.7)


WORKED = {1: [[[1, 0, 1, 3], [0, 0, 1, 1]], [[1, 0, 1, 3], [0, 1, 0, 1]], [[1, 0, 0, 2], [0, 1, 0, 1]]],
          2: [[[1, 1, 1, 3], [0, 1, 0, 1]], [[1, 1, 1, 3], [0, 1, 0, 1]], [[1, 0, 0, 2], [0, 1, 0, 1]]]}
WORKED_TOTALS = [[1, 10, 20, 0], [1, 4, 0, 0]]                   # n_gt, gt_frames per class; n_frames at [0][K]


# ---------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", [1, 2])
def test_worked_example(scenario):
    yt, yp, thr = worked_example()
    want = np.asarray(WORKED[scenario] + [WORKED_TOTALS], np.int64)
    assert np.array_equal(R.counts(yt, yp, thr, **SCENARIOS[scenario]), want)
    assert np.array_equal(host(yt, yp, thr, **SCENARIOS[scenario]), want)
    p = M.Psds(2, scenario, thr)
    p.update(torch.from_numpy(yt), torch.from_numpy(yp))
    assert np.array_equal(p.counts().numpy(), want) and p.counts().dtype == torch.int64


@pytest.mark.parametrize("seed", range(8))
def test_host_counts_equal_the_definition_on_random_rows(seed):
    rng = np.random.default_rng(seed)
    b, t, k = int(rng.integers(1, 4)), int(rng.choice([1, 2, 16, 63, 64, 65, 130, 301])), int(rng.integers(1, 5))
    thr = sorted({float(F32(h)) for h in rng.random(int(rng.integers(1, 7)))})
    yt, yp = block_case(rng, b, t, k)
    yp[rng.random(yp.shape) < 0.05] = F32(thr[0])          # scores exactly at a threshold
    yp[rng.random(yp.shape) < 0.02] = np.nan
    yt[rng.random(yt.shape) < 0.02] = np.nan
    for kw in (SCENARIOS[1], SCENARIOS[2], dict(dtc_pct=100, gtc_pct=1, cttc_pct=100), dict(dtc_pct=1, gtc_pct=100, cttc_pct=1)):
        want = R.counts(yt, yp, thr, **kw)
        assert np.array_equal(host(yt, yp, thr, **kw), want), kw
        assert want.shape == (len(thr) + 1, k, k + 2) and int(want[-1, 0, R.frames_column(k)]) == b * t


def test_constructed_rows():
    t = 130
    yt = np.zeros((1, t, 3), F32)
    yt[0, 10:20, 0] = yt[0, 30:40, 0] = yt[0, 50:60, 0] = 1      # three events under one detection
    yt[0, 0:100, 1] = 1                                          # one long event under three detections
    yt[0, 100:t, 2] = 1                                          # open at the end
    yp = np.zeros((1, t, 3), F32)
    yp[0, 10:60, 0] = 0.9                                        # 30 of 50 frames on class 0: passes DTC 10 %, fails 70 %
    yp[0, 0:30, 1] = yp[0, 35:65, 1] = yp[0, 70:95, 1] = 0.9     # 30 + 30 + 25 = 85 of 100 frames: GTC 70 % only jointly
    yp[0, 20:28, 2] = 0.9                                        # only on class 1's event: a cross-trigger
    yp[0, 101:t, 2] = 0.5                                        # equal to the threshold: active
    thr = (0.5,)
    one, two = R.counts(yt, yp, thr, **SCENARIOS[1]), R.counts(yt, yp, thr, **SCENARIOS[2])
    assert one[0].tolist() == [[0, 0, 0, 1, 1], [0, 1, 0, 0, 3], [0, 0, 1, 1, 2]]
    assert two[0].tolist() == [[3, 0, 0, 0, 1], [0, 1, 0, 0, 3], [0, 1, 1, 1, 2]]
    assert one[1].tolist() == [[3, 30, 0, t, 0], [1, 100, 0, 0, 0], [1, 30, 0, 0, 0]]
    assert np.array_equal(host(yt, yp, thr, **SCENARIOS[1]), one) and np.array_equal(host(yt, yp, thr, **SCENARIOS[2]), two)
    nan = np.full((1, t, 3), np.nan, F32)
    assert int(host(yt, nan, thr)[0].sum()) == 0 and int(host(nan, yp, thr)[1, :, :2].sum()) == 0


def test_updates_add_up_and_arguments_are_refused():
    rng = np.random.default_rng(7)
    yt, yp = block_case(rng, 3, 100, 3)
    thr = (0.3, 0.5, 0.7)
    p = M.Psds(3, 2, thr)
    p.update(torch.from_numpy(yt), torch.from_numpy(yp))
    p.update(torch.from_numpy(yt[:1]).double(), torch.from_numpy(yp[:1]))
    want = R.counts(yt, yp, thr, **SCENARIOS[2]) + R.counts(yt[:1], yp[:1], thr, **SCENARIOS[2])
    assert np.array_equal(p.counts().numpy(), want)
    both = M.Psds(3, 2, thr)
    both.update(torch.from_numpy(np.concatenate([yt, yt[:1]])), torch.from_numpy(np.concatenate([yp, yp[:1]])))
    assert np.array_equal(both.counts().numpy(), want)                              # clips are independent
    assert json.dumps(p.compute()) == json.dumps(M.psds_metrics(want, p.thresholds, alpha_ct=0.5, alpha_st=1.0))
    p.update(torch.zeros(0, 100, 3), torch.zeros(0, 100, 3))                        # an empty batch counts nothing
    assert np.array_equal(p.counts().numpy(), want)
    for bad in ((torch.zeros(2, 100, 3), torch.zeros(2, 99, 3)), (torch.zeros(2, 100, 2), torch.zeros(2, 100, 2)),
                (torch.zeros(2, 100), torch.zeros(2, 100)), (torch.zeros(2, 100, 3, dtype=torch.int64), torch.zeros(2, 100, 3))):
        with pytest.raises(ValueError):
            p.update(*bad)
    assert np.array_equal(p.counts().numpy(), want)
    p.reset()
    assert int(p.counts().abs().sum()) == 0
    for kw in (dict(thresholds=()), dict(thresholds=tuple(i / 128 for i in range(65))), dict(thresholds=(0.5, 0.5)),
               dict(thresholds=(0.6, 0.5)), dict(thresholds=(0.5, float('nan'))), dict(thresholds=(float('inf'),)),
               dict(thresholds=(0.5, 0.5 + 1e-9)), dict(thresholds=0.5),
               dict(scenario=0), dict(scenario=3), dict(scenario='1'), dict(scenario=dict(dtc_pct=70)),
               dict(scenario=dict(dtc_pct=0, gtc_pct=70)), dict(scenario=dict(dtc_pct=70, gtc_pct=101)),
               dict(scenario=dict(dtc_pct=70, gtc_pct=70, cttc_pct=101)), dict(scenario=dict(dtc_pct=70, gtc_pct=70, cttc_pct=-1)),
               dict(scenario=dict(dtc_pct=12.5, gtc_pct=70)), dict(scenario=dict(dtc_pct=70, gtc_pct=70, colour=1)),
               dict(hop=0), dict(e_max=0.0), dict(e_max=float('inf'))):
        with pytest.raises(ValueError):
            M.Psds(3, **kw)
        with pytest.raises(ValueError):
            M.psds(**kw)
    for kw in (dict(dtc_pct=0), dict(gtc_pct=101), dict(cttc_pct=101), dict(dtc_pct=0.7)):
        with pytest.raises(ValueError):
            M.check_psds_params(**kw)
        with pytest.raises(ValueError):
            M.psds_counts_host(torch.zeros(1, 4, 1), torch.zeros(1, 4, 1), (0.5,), **kw)
    for k in (0, 17):
        with pytest.raises(ValueError):
            M.Psds(k)
    default = M.Psds(16)
    assert default.state('cpu').shape == (51, 16, 18)
    assert default.thresholds == tuple(float(h) for h in np.linspace(0.01, 0.99, 50).astype(F32))
    assert M.Psds(3, 1, tuple(i / 128 for i in range(1, 65))).state('cpu').shape == (65, 3, 5)
    assert (M.Psds(3, 2).dtc_pct, M.Psds(3, 2).cttc_pct, M.Psds(3, 2).alpha_ct, M.Psds(3, 1).cttc_pct) == (10, 30, 0.5, None)


# ---------------------------------------------------------------------------
# the score
# ---------------------------------------------------------------------------
def _hand(ct=0, gt_frames1=0):
    thr = (0.3, 0.5, 0.7)
    c = np.zeros((4, 2, 4), np.int64)
    for j, ((fp0, tp0), (fp1, tp1)) in enumerate(zip(((200, 10), (50, 8), (0, 4)), ((100, 6), (20, 6), (0, 0)))):
        c[j, 0, 0], c[j, 0, 2], c[j, 1, 1], c[j, 1, 2] = tp0, fp0, tp1, fp1
    c[1, 0, 1] = ct
    c[3, :, 0] = 10
    c[3, 1, 1] = gt_frames1
    c[3, 0, 2] = 225000                                          # one hour at hop 256, 16 kHz
    return c, thr


def test_hand_worked_scores():
    c, thr = _hand()
    assert M.psds_metrics(c, thr, 256, 16000, alpha_ct=0.0, alpha_st=0.0)['psds'] == pytest.approx(0.54, abs=1e-12)
    res = M.psds_metrics(c, thr, 256, 16000, alpha_ct=0.0, alpha_st=1.0)
    assert res['psds'] == pytest.approx(0.42, abs=1e-12)
    assert res['curves'][0] == {'efpr': [0.0, 50.0, 200.0], 'tpr': [0.4, 0.8, 1.0]}
    assert res['curves'][1] == {'efpr': [0.0, 20.0, 100.0], 'tpr': [0.0, 0.6, 0.6]}
    assert res['tpr_at_e_max'] == [0.8, 0.6] and res['classes_scored'] == [0, 1] and res['classes_without_gt'] == []
    assert res['n_frames'] == 225000 and res['n_gt'] == [10, 10]
    c, thr = _hand(ct=5, gt_frames1=22500)
    res = M.psds_metrics(c, thr, 256, 16000, alpha_ct=0.5, alpha_st=0.0)
    assert res['psds'] == pytest.approx(0.49, abs=1e-12)
    assert res['cross_triggers'] == {'threshold': 0.5, 'matrix': [[0, 5], [0, 0]]}
    assert M.psds_metrics(c, thr, 256, 16000, alpha_ct=0.0, alpha_st=0.0)['psds'] == pytest.approx(0.54, abs=1e-12)
    assert M.psds_metrics(torch.from_numpy(c), thr, 256, 16000, alpha_ct=0.5, alpha_st=0.0)['psds'] == res['psds']
    # half the range: [0, 20) 0.2, [20, 50) 0.5 -> 19 / 50
    assert M.psds_metrics(_hand()[0], thr, 256, 16000, alpha_ct=0.0, alpha_st=0.0, e_max=50.0)['psds'] == pytest.approx(0.38, abs=1e-12)
    for bad in (c[:3], c[:, :, :3], c.astype(np.float64)):
        with pytest.raises(ValueError):
            M.psds_metrics(bad, thr)


def test_perfect_empty_and_missing_classes():
    rng = np.random.default_rng(1)
    yt, _ = block_case(rng, 4, 200, 3)
    assert yt.sum((0, 1)).min() > 0
    for scenario in (1, 2):
        p = M.Psds(3, scenario)
        p.update(torch.from_numpy(yt), torch.from_numpy(yt))
        assert p.compute()['psds'] == 1.0
        p.reset()
        p.update(torch.from_numpy(yt), torch.zeros(4, 200, 3))
        assert p.compute()['psds'] == 0.0
        p.reset()
        gone = yt.copy()
        gone[:, :, 1] = 0                                        # class 1 has no ground truth: left out, the others still perfect
        p.update(torch.from_numpy(gone), torch.from_numpy(gone))
        res = p.compute()
        assert res['psds'] == 1.0 and res['classes_without_gt'] == [1] and res['classes_scored'] == [0, 2]
        assert math.isnan(res['tpr_at_e_max'][1]) and set(res['curves']) == {0, 2}
        p.reset()
        p.update(torch.zeros(4, 200, 3), torch.from_numpy(yt))
        res = p.compute()
        assert math.isnan(res['psds']) and res['classes_without_gt'] == [0, 1, 2]
        json.dumps(res)
    assert math.isnan(M.Psds(3).compute()['psds'])               # nothing seen


@pytest.mark.parametrize("seed", range(6))
def test_a_pure_false_positive_never_raises_the_score(seed):
    """One more detection of class 0 at every threshold, in a stretch without labels or scores: FP[.][0] grows by one and nothing
    else moves, so class 0's curve moves right and its TPR at every eFPR can only fall.  With alpha_st = 0 the score is the mean
    of the curves and cannot rise for any K.  With alpha_st = 1 that holds for K <= 2 (mean - std of two values is their minimum)
    but NOT for K >= 3, where lowering the largest of the values can shrink the deviation by more than the mean: those settings
    are the ones asserted."""
    rng = np.random.default_rng(seed)
    for k, alpha_st in ((3, 0.0), (2, 1.0), (2, 0.0), (1, 1.0)):
        yt, yp = block_case(rng, 2, 200, k)
        yt[:, 150:], yp[:, 150:] = 0, 0
        more = yp.copy()
        more[0, 170:180, 0] = 0.995
        for sc in (1, 2):
            kw = dict(SCENARIOS[sc])
            thr = M.psds_default_thresholds()
            a, b = R.counts(yt, yp, thr, **kw), R.counts(yt, more, thr, **kw)
            diff = b - a
            assert (diff[:50, 0, k] == 1).all() and (diff[:50, 0, k + 1] == 1).all() and int(diff.sum()) == 100
            args = dict(hop=256, sr=16000, alpha_ct=0.5 if sc == 2 else 0.0, alpha_st=alpha_st)
            before, after = M.psds_metrics(a, thr, **args)['psds'], M.psds_metrics(b, thr, **args)['psds']
            assert after <= before, (k, alpha_st, sc, before, after)


# ---------------------------------------------------------------------------
# MetricSet, fit, sj_train
# ---------------------------------------------------------------------------
def test_metric_set_feeds_the_counts_in_the_val_phase_only():
    rng = np.random.default_rng(3)
    yt, yp = block_case(rng, 4, 40, 3)
    yt, yp = torch.from_numpy(yt), torch.from_numpy(yp)
    score = M.psds(2, hop=1600)
    ms = M.MetricSet([M.cos_sim, score, M.er_score(smoothing=False), M.sed_eval((0.5,), hop=1600)])
    assert ms.psds is score and score not in ms.others
    out = ms(yt, yp, 'train')
    assert set(out) == {'cos_sim', 'er'} and score.counter is None                      # nothing made, nothing counted
    assert set(ms.psds_values('val_')) == {'val_psds'} and math.isnan(ms.psds_values('val_')['val_psds'])
    assert set(ms(yt, yp, 'val')) == {'cos_sim', 'er'}                               # no per-step value
    ms(yt, yp, 'train')
    want = R.counts(yt.numpy(), yp.numpy(), M.psds_default_thresholds(), **SCENARIOS[2])
    assert np.array_equal(score.counter.counts().numpy(), want)
    assert not any(t is s for t in ms.state_tensors() for s in score.counter.states.values())
    value = M.psds_metrics(want, M.psds_default_thresholds(), 1600, 16000, 0.5, 1.0)['psds']
    assert ms.psds_values('val_') == {'val_psds': value} and 0.0 <= value <= 1.0
    ms.reset('train')
    assert int(score.counter.counts().sum()) == int(want.sum())
    ms.reset()
    assert int(score.counter.counts().sum()) == 0
    assert M.MetricSet([M.cos_sim]).psds_values('val_') == {}
    with pytest.raises(ValueError, match="psds"):
        M.MetricSet([M.psds(1), M.psds(2)])
    with pytest.raises(TypeError):
        score(yt, yp)


def test_monitors_and_flags():
    from challenge_amd import fit as Fit
    from challenge_amd import sj_train as S
    assert Fit.monitor_maximised('val_psds') and Fit.monitor_maximised('val_ema_psds')
    plain = S.ARGS().get([])
    assert plain.psds == 0 and S.row_names(plain) == ['loss', 'val_loss']
    cfg = S.ARGS().get(['--psds', '2', '--checkpoint_monitor', 'val_psds'])
    assert cfg.psds == 2 and cfg.checkpoint_monitor == 'val_psds'
    assert S.row_names(cfg) == ['loss', 'val_loss', 'val_psds']
    assert S.run_name(cfg) == S.run_name(plain)                                      # a flag, not a run-name token
    both = S.ARGS().get(['--psds', '1', '--sed_eval', '0.5', '--ema', '0.9', '--checkpoint_monitor', 'val_ema_psds'])
    assert S.row_names(both)[-5:] == ['val_ema_loss', 'val_ema_seg_f1', 'val_ema_seg_er', 'val_ema_event_f1', 'val_ema_psds']
    for bad in (['--psds', '3'], ['--psds', 'one'], ['--psds', '-1']):
        with pytest.raises(SystemExit):
            S.ARGS().get(bad)
    for bad in (['--checkpoint_monitor', 'val_psds'], ['--psds', '1', '--checkpoint_monitor', 'val_ema_psds']):
        with pytest.raises(ValueError, match="checkpoint_monitor"):
            S.ARGS().get(bad)


def _batches(n, seed, rows=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 32, 64, 1, generator=g), (torch.rand(rows, 2, 3, generator=g) > 0.5).float()) for _ in range(n)]


def test_main_with_psds_logs_the_column_and_checkpoints_on_it(tmp_path, monkeypatch):
    """`sj_train.main --psds 1 --checkpoint_monitor val_psds --ema 0.9` on the CPU (fixed batches stand in for the synthesis
    pipeline, which needs a device); without the flag the header is the one of before."""
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(S, "make_dataset", lambda config, training=True: Dataset.from_generator(
        lambda: iter(_batches(2, 20 + int(training)))).repeat())
    base = ['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--synthetic', '--epochs', '2', '--steps_per_epoch', '1',
            '--validation_steps', '1', '--batch_size', '2']
    S.main(['--name', 'scored'] + base + ['--psds', '1', '--checkpoint_monitor', 'val_psds', '--ema', '0.9'])
    S.main(['--name', 'plain'] + base)
    name = S.run_name(S.ARGS().get(['--name', 'scored'] + base))
    with open(name.replace('.h5', '.csv')) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ['epoch', 'loss', 'lr', 'time', 'val_loss', 'val_psds', 'val_ema_loss', 'val_ema_psds']
    assert len(rows) == 2
    for key in ('val_psds', 'val_ema_psds'):
        assert all(r[key] == 'nan' or -1.0 <= float(r[key]) <= 1.0 for r in rows), key
    with open(S.run_name(S.ARGS().get(['--name', 'plain'] + base)).replace('.h5', '.csv')) as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss']


def test_checkpoint_follows_psds_upwards(tmp_path):
    from types import SimpleNamespace
    from challenge_amd import fit as Fit
    from challenge_amd.dataset import Dataset
    y = np.zeros((1, 400, 3), F32)
    y[0, 100:200] = 1
    cover = [20, 10, 10, 20, 80, 100]                   # frames of the event that are detected: GTC 70 % from 70 on

    class Stub:
        def __init__(self):
            self._ema = self._ddp = None
            self.optimizer = SimpleNamespace(param_groups=[{'lr': 0.1}])
            self._metrics = M.MetricSet([M.psds(1)])
            self.epoch, self.saved = 0, []

        def train_step(self, data):
            return {'loss': torch.tensor(1.0)}

        def test_step(self, data):
            yp = np.zeros((1, 400, 3), F32)
            yp[0, 100:100 + cover[self.epoch]] = 1
            out = {'loss': torch.tensor(float(self.epoch + 1)), **self._metrics(torch.from_numpy(y), torch.from_numpy(yp), 'val')}
            self.epoch += 1
            return out

        def state_dict(self):
            self.saved.append(self.epoch - 1)
            return {'epoch': torch.tensor(self.epoch - 1)}
    ds = Dataset.from_generator(lambda: iter([(torch.zeros(1), torch.zeros(1))])).repeat()
    stub = Stub()
    hist = Fit.fit(stub, ds, epochs=len(cover), steps_per_epoch=1, validation_data=ds, validation_steps=1, graph=False,
                   checkpoint_path=str(tmp_path / "stub.pt"), checkpoint_monitor='val_psds', verbose=False)
    assert [r['val_psds'] for r in hist] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]          # (the loss gets worse all along)
    assert stub.saved == [0, 4]                                                       # strictly larger only
