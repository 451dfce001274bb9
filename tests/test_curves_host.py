"""CPU tests of the threshold-free validation numbers (metrics.curve_metrics / ScoreHistogram / score_curves, iris_score_hist's
argument checks, `fit`'s val_auc / val_map / val_best_f1 columns and maximised monitors, sj_train's flags, evaluate(curves=)).
The oracle is tests/curves_ref.py: the definitions from scratch, no histogram inside.

Tolerance of every float comparison with the oracle: bins * 2^-52 absolute - the rounding of a sum of `bins` terms of size <= 1
in fp64 (the oracle itself is exact rational arithmetic rounded once)."""
import copy
import csv
import ctypes as C
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import curves_ref as R
from challenge_amd import _native as N
from challenge_amd import metrics as M

F32 = np.float32


def tol(bins):
    return bins * 2.0 ** -52


def special_predictions(bins):
    """(value, slot) pairs: the bin edges and the floats just below them, the ends, the values outside [0, 1), NaN, a subnormal."""
    out = []
    for j in sorted({1, 2, bins // 2, bins - 1}):
        edge = F32(j) / F32(bins)
        out += [(edge, j), (np.nextafter(edge, F32(0), dtype=F32), j - 1)]
    out += [(F32(0), 0), (F32(-0.0), 0), (F32(1), bins - 1), (np.nextafter(F32(1), F32(0), dtype=F32), bins - 1), (F32(-1), 0),
            (F32(2), bins - 1), (F32(np.inf), bins - 1), (F32(-np.inf), 0), (F32(np.nan), bins), (F32(1e-40), 0), (F32(-1e-40), 0),
            (F32(3e38), bins - 1), (F32(-3e38), 0)]
    return out


SPECIAL_LABELS = [(F32(0.5), 1), (np.nextafter(F32(0.5), F32(0), dtype=F32), 0), (F32(2.0), 1), (F32(np.nan), 0), (F32(0), 0), (F32(1), 1)]


def special_batch(bins, k):
    """[1, T, k] labels and predictions holding every (special prediction, special label) pair in every class, and the counts
    they must give, built from the stated slots (not from any code under test)."""
    preds, labs = special_predictions(bins), SPECIAL_LABELS
    t = len(preds) * len(labs)
    yp, yt = np.empty((1, t, k), F32), np.empty((1, t, k), F32)
    want = np.zeros((k, 2, bins + 1), np.int64)
    i = 0
    for p, slot in preds:
        for y, lab in labs:
            yp[0, i, :], yt[0, i, :] = p, y
            want[:, lab, slot] += 1
            i += 1
    return yt, yp, want


def random_case(rng, n, k, bins, sharp=False):
    yt = (rng.random((n, k)) < 0.3).astype(F32)
    if sharp:   # sigmoid-like: piled up at the ends
        z = rng.standard_normal((n, k)) * 6 + (yt * 2 - 1) * 2
        yp = (1 / (1 + np.exp(-z))).astype(F32)
    else:
        yp = np.clip(rng.random((n, k)) * 0.7 + yt * rng.random((n, k)) * 0.5, 0, 1).astype(F32)
    return yt, yp


def assert_matches_ref(got, ref, bins):
    for name in ('auroc', 'ap', 'best_f1', 'ece'):
        for g, r in zip(got['per_class'][name], ref['per_class'][name]):
            assert (math.isnan(g) and math.isnan(r)) or abs(g - r) <= tol(bins), (name, g, r)
    for name in ('best_threshold', 'n_pos', 'n_neg', 'n_nan'):
        for g, r in zip(got['per_class'][name], ref['per_class'][name]):
            assert g == r or (isinstance(r, float) and math.isnan(g) and math.isnan(r)), (name, g, r)
    for name in ('auc', 'map', 'best_f1'):
        g, r = got[name], ref[name]
        assert (math.isnan(g) and math.isnan(r)) or abs(g - r) <= tol(bins), (name, g, r)


# ---------------------------------------------------------------------------
# curve_metrics against the definitions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bins,n,sharp", [(16, 300, False), (64, 500, True), (4096, 400, False), (4096, 400, True)])
def test_curve_metrics_matches_the_definitions(bins, n, sharp):
    rng = np.random.default_rng(bins + n)
    yt, yp = random_case(rng, n, 3, bins, sharp)
    yp[5, 1] = np.nan                                     # a NaN prediction is counted apart and excluded from the curves
    counts = R.counts(yt, yp, bins)
    got = M.curve_metrics(counts)
    assert got['bins'] == bins and got['per_class']['n_nan'] == [0, 1, 0]
    assert_matches_ref(got, R.metrics(yt, yp, bins), bins)
    again = M.curve_metrics(torch.from_numpy(counts))     # a tensor is taken too
    assert again == got or all(again[k] == got[k] for k in ('auc', 'map', 'best_f1'))


def test_curve_metrics_degenerate_classes():
    bins = 64
    rng = np.random.default_rng(1)
    n = 200
    yt = np.zeros((n, 4), F32)
    yp = rng.random((n, 4)).astype(F32)
    yt[:, 1] = 1                                          # class 0: no positives; class 1: no negatives
    yt[:, 2] = rng.random(n) < 0.4
    yp[:, 2] = 0.37                                       # class 2: all scores equal
    yt[:, 3] = rng.random(n) < 0.5
    yp[:, 3] = np.where(yt[:, 3] > 0, 0.6 + 0.3 * rng.random(n), 0.4 * rng.random(n))   # class 3: perfect separation
    got = M.curve_metrics(R.counts(yt, yp, bins))
    per = got['per_class']
    assert math.isnan(per['auroc'][0]) and math.isnan(per['ap'][0]) and math.isnan(per['best_f1'][0]) and math.isnan(per['best_threshold'][0])
    assert math.isnan(per['auroc'][1]) and per['ap'][1] == 1.0 and per['best_f1'][1] == 1.0 and per['best_threshold'][1] == 0.0
    assert per['auroc'][2] == 0.5 and per['best_threshold'][2] == 0.0
    assert per['auroc'][3] == 1.0 and per['ap'][3] == 1.0 and per['best_f1'][3] == 1.0
    assert_matches_ref(got, R.metrics(yt, yp, bins), bins)
    empty = M.curve_metrics(np.zeros((2, 2, 17), np.int64))
    assert all(math.isnan(empty[k]) for k in ('auc', 'map', 'best_f1')) and math.isnan(empty['per_class']['ece'][0])
    with pytest.raises(ValueError):
        M.curve_metrics(np.zeros((2, 2, 17), np.float32))
    with pytest.raises(ValueError):
        M.curve_metrics(np.zeros((2, 3, 17), np.int64))


def test_curve_metrics_is_exact_beyond_int64_products():
    """Counts whose products pass 2^63 (a long validation set over many ranks): the numerators are Python integers."""
    c = np.zeros((1, 2, 17), np.int64)
    c[0, 1, 12] = c[0, 0, 3] = 2 ** 33
    c[0, 1, 3] = c[0, 0, 12] = 2 ** 31
    got = M.curve_metrics(c)
    p = n = 2 ** 33 + 2 ** 31
    want = (2 ** 33 * (2 * 2 ** 33 + 2 ** 31) + 2 ** 31 * 2 ** 33) / (2 * p * n)
    assert got['per_class']['auroc'][0] == want and 0.5 < want < 1


@pytest.mark.parametrize("bins", [16, 64, 4096])
def test_curve_metrics_agrees_with_sklearn_on_the_bin_centres(bins):
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(7 + bins)
    yt, yp = random_case(rng, 600, 2, bins, sharp=True)
    got = M.curve_metrics(R.counts(yt, yp, bins))
    for c in range(2):
        centres = (R.quantise(yp[:, c], bins) + 0.5) / bins
        assert abs(got['per_class']['auroc'][c] - sk.roc_auc_score(yt[:, c], centres)) <= tol(bins)
        assert abs(got['per_class']['ap'][c] - sk.average_precision_score(yt[:, c], centres)) <= tol(bins)


# ---------------------------------------------------------------------------
# ScoreHistogram on CPU tensors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [16, 1024, 4096])
def test_cpu_update_places_every_special_value(bins):
    yt, yp, want = special_batch(bins, 3)
    assert np.array_equal(R.counts(yt, yp, bins), want)   # the from-scratch rule agrees with the stated slots
    h = M.ScoreHistogram(3, bins)
    h.update(torch.from_numpy(yt), torch.from_numpy(yp))
    got = h.counts()
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 2, bins + 1)
    assert np.array_equal(got.numpy(), want) and int(got.sum()) == yp.size
    h.update(torch.from_numpy(yt), torch.from_numpy(yp))  # cumulative
    assert np.array_equal(h.counts().numpy(), 2 * want)
    assert h.compute()['per_class']['n_nan'] == [2 * len(SPECIAL_LABELS)] * 3
    h.reset()
    assert int(h.counts().sum()) == 0
    other = M.ScoreHistogram(3, bins)                     # no shared state
    other.update(torch.from_numpy(yt), torch.from_numpy(yp))
    assert int(h.counts().sum()) == 0 and np.array_equal(other.counts().numpy(), want)


def test_cpu_update_refuses_what_it_cannot_count():
    h = M.ScoreHistogram(3, 64)
    y = torch.zeros(2, 8, 3)
    for bad_t, bad_p in [(y, torch.zeros(2, 4, 3)), (torch.zeros(2, 8, 4), torch.zeros(2, 8, 4)), (y.long(), y), (y, y.long()),
                         (y[0], y[0]), (torch.zeros(1, 8, 3), y)]:
        with pytest.raises(ValueError):
            h.update(bad_t, bad_p)
    assert int(h.counts().sum()) == 0
    h.update(y.double(), y.half())                        # any floating type is taken
    assert int(h.counts().sum()) == 48
    for bins in (0, 8, 1000, 8192):
        with pytest.raises(ValueError):
            M.ScoreHistogram(3, bins)
        with pytest.raises(ValueError):
            M.score_curves(bins)
    with pytest.raises(ValueError):
        M.ScoreHistogram(17, 64)


def test_iris_score_hist_refuses_before_any_launch():
    lib = N.lib()
    p = C.c_void_p(64)
    INVALID, UNSUPPORTED = -1, -2

    def refused(rc, code):
        assert rc == code, rc
        assert lib.iris_last_error().startswith(b"iris_score_hist:"), lib.iris_last_error()
    refused(lib.iris_score_hist(None, p, 1, 4, 3, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, None, 1, 4, 3, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, p, 1, 4, 3, 64, None, None), INVALID)
    refused(lib.iris_score_hist(p, p, 0, 4, 3, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, p, 1, 0, 3, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, p, 1, 4, 0, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, p, -1, 4, 3, 64, p, None), INVALID)
    refused(lib.iris_score_hist(p, p, 1, 4, 17, 64, p, None), UNSUPPORTED)
    for bins in (0, 8, 15, 48, 1000, 4097, 8192, -16):
        refused(lib.iris_score_hist(p, p, 1, 4, 3, bins, p, None), UNSUPPORTED)
    refused(lib.iris_score_hist(p, p, 65536, 32768, 3, 64, p, None), UNSUPPORTED)       # 2^31 frames
    refused(lib.iris_score_hist(p, p, 2 ** 31 - 1, 2, 3, 64, p, None), UNSUPPORTED)
    assert "iris_score_hist" in N.SIGNATURES and lib.iris_abi_version() == 1


# ---------------------------------------------------------------------------
# MetricSet
# ---------------------------------------------------------------------------
def test_metric_set_feeds_the_histogram_in_the_val_phase_only():
    rng = np.random.default_rng(3)
    yt, yp = random_case(rng, 4 * 8, 3, 64)
    yt, yp = torch.from_numpy(yt).view(4, 8, 3), torch.from_numpy(yp).view(4, 8, 3)
    curves = M.score_curves(64)
    ms = M.MetricSet([M.cos_sim, curves, M.er_score(smoothing=False)])
    assert ms.curves is curves and curves not in ms.others
    out = ms(yt, yp, 'train')
    assert set(out) == {'cos_sim', 'er'} and curves.counter is None           # nothing made, nothing counted
    assert all(math.isnan(v) for v in ms.curve_values('val_').values())
    assert set(ms(yt, yp, 'val')) == {'cos_sim', 'er'}                     # no per-step value
    ms(yt, yp, 'train')
    assert np.array_equal(curves.counter.counts().numpy(), R.counts(yt.numpy(), yp.numpy(), 64))
    assert not any(t is s for t in ms.state_tensors() for s in curves.counter.states.values())
    vals = ms.curve_values('val_')
    ref = R.metrics(yt.numpy(), yp.numpy(), 64)
    assert set(vals) == {'val_auc', 'val_map', 'val_best_f1'}
    assert all(abs(vals['val_' + k] - ref[k]) <= tol(64) for k in ('auc', 'map', 'best_f1'))
    ms.reset('train')
    assert int(curves.counter.counts().sum()) == 96
    ms.reset()
    assert int(curves.counter.counts().sum()) == 0
    assert M.MetricSet([M.cos_sim]).curve_values('val_') == {}
    with pytest.raises(ValueError):
        M.MetricSet([M.score_curves(64), M.score_curves(16)])
    with pytest.raises(TypeError):
        curves(yt, yp)


# ---------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------
def _small(seed=3):
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(seed)
    return S, cfg, S.get_model(cfg)


def _batches(n, seed, rows=6):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 32, 64, 1, generator=g), (torch.rand(rows, 2, 3, generator=g) > 0.5).float()) for _ in range(n)]


class _Keep:
    """A fit callback: the weights as each epoch's validation pass saw them."""

    def __init__(self, ema=None):
        self.states, self.ema_states, self.ema = [], [], ema

    def on_epoch_end(self, epoch, model):
        self.states.append(copy.deepcopy(model.state_dict()))
        if self.ema is not None:
            self.ema_states.append(copy.deepcopy(self.ema.state_dict()))


def _fit(tmp_path, tag, curves, with_ema=False, monitor=None, epochs=2):
    from challenge_amd.dataset import Dataset
    from challenge_amd.ema import WeightEMA
    S, cfg, model = _small(seed=5)
    ema = None
    if with_ema:
        ema = WeightEMA(model, 0.9)
        ema.compile(S.binary_crossentropy, metrics=[M.score_curves(curves)] if curves else None)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  metrics=[M.score_curves(curves)] if curves else None, ema=ema)
    train, val = _batches(3, 11), _batches(2, 12)
    keep = _Keep(ema)
    (tmp_path / tag).mkdir()
    extra = {"ema": ema, "ema_checkpoint_path": str(tmp_path / tag / "model_EMA.pt")} if with_ema else {}
    hist = S.fit(model, Dataset.from_generator(lambda: iter(train)).repeat(), epochs=epochs, steps_per_epoch=2,
                 validation_data=Dataset.from_generator(lambda: iter(val)).repeat(), validation_steps=2,
                 checkpoint_path=str(tmp_path / tag / "model.pt"), csv_path=str(tmp_path / f"{tag}.csv"), checkpoint_monitor=monitor,
                 verbose=False, callbacks=[keep], **extra)
    return hist, keep, val, tmp_path / f"{tag}.csv"


def _replayed(state, val, bins):
    """curves_ref on the validation batches under the given weights (eval mode, as test_step runs them)."""
    _, _, model = _small(seed=9)
    model.load_state_dict(state)
    model.eval()
    with torch.no_grad():
        yp = torch.cat([model(x) for x, _ in val]).numpy()
    yt = torch.cat([y for _, y in val]).numpy()
    return R.metrics(yt, yp, bins)


def test_fit_logs_the_curve_columns_and_they_are_the_definitions(tmp_path):
    bins = 64
    plain, _, _, plain_csv = _fit(tmp_path, "plain", 0)
    hist, keep, val, curve_csv = _fit(tmp_path, "curves", bins, with_ema=True)
    with open(plain_csv) as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss']          # without curves: the header of before
    with open(curve_csv) as f:
        assert next(csv.reader(f)) == ['epoch', 'loss', 'lr', 'time', 'val_loss', 'val_auc', 'val_map', 'val_best_f1',
                                       'val_ema_loss', 'val_ema_auc', 'val_ema_map', 'val_ema_best_f1']
    assert len(hist) == len(plain) == 2
    for e, (row, base) in enumerate(zip(hist, plain)):
        assert row['loss'] == base['loss'] and row['val_loss'] == base['val_loss']          # nothing else moved
        ref, eref = _replayed(keep.states[e], val, bins), _replayed(keep.ema_states[e], val, bins)
        for k in ('auc', 'map', 'best_f1'):
            assert 0.0 <= row['val_' + k] <= 1.0 and 0.0 <= row['val_ema_' + k] <= 1.0
            assert abs(row['val_' + k] - ref[k]) <= tol(bins), (e, k, row['val_' + k], ref[k])
            assert abs(row['val_ema_' + k] - eref[k]) <= tol(bins), (e, k, row['val_ema_' + k], eref[k])


class _StubModel:
    """What `fit` touches of a compiled model, with crafted validation predictions per epoch."""

    def __init__(self, wrong, losses, bins=16):
        self._ema = self._ddp = None
        self.optimizer = SimpleNamespace(param_groups=[{'lr': 0.1}])
        self._metrics = M.MetricSet([M.score_curves(bins)])
        self.wrong, self.losses, self.epoch, self.saved = wrong, losses, 0, []
        self.y = (torch.arange(48).view(2, 8, 3) % 2).float()

    def train_step(self, data):
        return {'loss': torch.tensor(1.0)}

    def test_step(self, data):
        yp = self.y.clone().view(-1)
        yp[:self.wrong[self.epoch]] = 1 - yp[:self.wrong[self.epoch]]
        yp = yp.view_as(self.y) * 0.8 + 0.1
        out = {'loss': torch.tensor(float(self.losses[self.epoch])), **self._metrics(self.y, yp, 'val')}
        self.epoch += 1
        return out

    def state_dict(self):
        self.saved.append(self.epoch - 1)
        return {'epoch': torch.tensor(self.epoch - 1)}


def test_checkpoint_monitor_on_a_curve_name_is_maximised(tmp_path):
    from challenge_amd import fit as F
    from challenge_amd.dataset import Dataset
    assert F.monitor_maximised('val_map') and F.monitor_maximised('val_ema_auc') and F.monitor_maximised('val_best_f1')
    assert not any(F.monitor_maximised(n) for n in (None, 'val_loss', 'val_er', 'loss', 'val_f1_score', 'val_ema_loss'))
    wrong = [6, 3, 3, 5, 0, 0]                           # val_map: up, equal, down, up, equal
    ds = Dataset.from_generator(lambda: iter([(torch.zeros(1), torch.zeros(1))])).repeat()

    def run(monitor, losses):
        stub = _StubModel(wrong, losses)
        hist = F.fit(stub, ds, epochs=len(wrong), steps_per_epoch=1, validation_data=ds, validation_steps=1, graph=False,
                     checkpoint_path=str(tmp_path / "stub.pt"), checkpoint_monitor=monitor, verbose=False)
        return stub, hist
    stub, hist = run('val_map', [1, 2, 3, 4, 5, 6])      # the loss gets worse all along: only the monitor can cause a save
    maps = [r['val_map'] for r in hist]
    assert maps[0] < maps[1] == maps[2] > maps[3] < maps[4] == maps[5] == 1.0
    assert stub.saved == [0, 1, 4]                        # strictly larger only
    stub, _ = run('val_loss', [3, 2, 2, 1, 4, 0.5])      # every other name keeps `<`
    assert stub.saved == [0, 1, 3, 5]
    stub, _ = run(None, [3, 2, 2, 1, 4, 0.5])
    assert stub.saved == [0, 1, 3, 5]


# ---------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------
def test_args_take_curves_and_a_checkpoint_monitor():
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get([])
    assert cfg.curves == 0 and cfg.checkpoint_monitor is None
    cfg = S.ARGS().get(['--curves', '1024', '--checkpoint_monitor', 'val_map', '--ema', '0.99'])
    assert cfg.curves == 1024 and cfg.checkpoint_monitor == 'val_map'
    assert 'val_ema_best_f1' in S.row_names(cfg) and 'val_er' not in S.row_names(cfg)
    assert S.run_name(cfg) == S.run_name(S.ARGS().get([]))                                  # not part of the run name
    for bad in (['--curves', '1000'], ['--curves', '8'], ['--curves', '8192'], ['--curves', 'many']):
        with pytest.raises(SystemExit):
            S.ARGS().get(bad)
    for bad in (['--checkpoint_monitor', 'val_map'], ['--curves', '64', '--checkpoint_monitor', 'val_er'],
                ['--curves', '64', '--checkpoint_monitor', 'val_ema_map'], ['--checkpoint_monitor', 'nonsense']):
        with pytest.raises(ValueError, match="checkpoint_monitor"):
            S.ARGS().get(bad)
    assert S.ARGS().get(['--metrics', 'reference', '--checkpoint_monitor', 'val_cos_sim']).checkpoint_monitor == 'val_cos_sim'


def test_main_with_curves_logs_the_columns_and_checkpoints_on_them(tmp_path, monkeypatch):
    """`sj_train.main --curves 64 --checkpoint_monitor val_map --ema 0.9` on the CPU: with --metrics none the histogram is the
    only metric, the EMA gets its own, and both checkpoints appear.  (The synthesis pipeline needs a device: fixed batches stand
    in for it.)"""
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(S, "make_dataset", lambda config, training=True: Dataset.from_generator(
        lambda: iter(_batches(2, 20 + int(training), rows=2))).repeat())
    S.main(['--name', 'cv', '--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--synthetic', '--epochs', '2',
            '--steps_per_epoch', '1', '--validation_steps', '1', '--batch_size', '2', '--curves', '64', '--checkpoint_monitor', 'val_map',
            '--ema', '0.9'])
    name = S.run_name(S.ARGS().get(['--name', 'cv', '--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '2']))
    with open(name.replace('.h5', '.csv')) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for k in ('val_auc', 'val_map', 'val_best_f1', 'val_ema_auc', 'val_ema_map', 'val_ema_best_f1'):
        assert all(r[k] == 'nan' or 0.0 <= float(r[k]) <= 1.0 for r in rows), k
    assert os.path.exists(name.replace('.h5', '.pt')) or all(r['val_map'] == 'nan' for r in rows)


def test_eval_takes_a_file_for_curves():
    """`python -m challenge_amd.eval --curves OUT.json`: there the flag names a file (the trainer's takes a bin count)."""
    from challenge_amd import eval as E
    cfg = E.build_args().get(['--name', 'run', '--curves', 'out.json'])
    assert cfg.curves == 'out.json' and cfg.curve_bins == 1024 and cfg.p is False and cfg.n_mels == 80
    assert E.build_args().get(['--name', 'run']).curves is None
    assert E.build_args().get(['--name', 'run', '--curves', 'o.json', '--curve_bins', '256']).curve_bins == 256


# ---------------------------------------------------------------------------
# evaluate(curves=)
# ---------------------------------------------------------------------------
def test_evaluate_feeds_the_posteriors_and_the_answer_labels(tmp_path, monkeypatch):
    """A stub in place of the recording -> features -> model chain (known posteriors per file): the histogram holds those
    posteriors against second2frame's labels, and the scores are the ones of a run without `curves`."""
    from challenge_amd import data_utils as D
    from challenge_amd import eval as E
    from challenge_amd import inference as I
    from challenge_amd import sj_train as S
    rng = np.random.default_rng(5)
    t = 188                                                # 3 s at 62.5 frames per second
    post = {f"clip{i}": torch.from_numpy(rng.random((t, 3)).astype(F32)) for i in range(2)}
    post["clip0"][:70, 0] = 0.9
    answers = {"clip0": [[0, 0, 1], [1, 1, 2], [1, 1, 3]], "clip1": [[2, 0, 3]]}            # (overlapping events: a label of 2)
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
    hist = M.ScoreHistogram(3, 256)
    assert M.evaluate(cfg, None, curves=hist, **kw) == plain
    yt = np.concatenate([E.second2frame(answers[n], t, 16000 / 256).numpy() for n in sorted(post)])
    yp = np.concatenate([post[n].numpy() for n in sorted(post)])
    assert yt.max() == 2.0
    assert np.array_equal(hist.counts().numpy(), R.counts(yt, yp, 256)) and int(hist.counts().sum()) == 2 * t * 3
    assert_matches_ref(hist.compute(), R.metrics(yt, yp, 256), 256)
    json.dumps(hist.compute())                             # what `python -m challenge_amd.eval --curves OUT.json` writes
