"""GPU tests of the intersection-count launches (iris_psds_counts, csrc/k_psds.h) behind metrics.Psds / psds.  Counts are
integers: every comparison - with tests/psds_ref.py (plain loops over event lists and interval intersections), with the CPU path
and between two runs - is for EQUALITY."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import psds_ref as R
from challenge_amd import _native as N
from challenge_amd import metrics as M
from test_psds_host import SCENARIOS, WORKED, WORKED_TOTALS, block_case, worked_example

pytestmark = pytest.mark.gpu
F32 = np.float32

# (B, T, K, n_thr): one frame; the validation shape (T = 16); around the 64-frame step; several steps; the most classes; many
# rows; more (row, threshold) items (19,200) and more rows (17,600) than the grid has waves (16,384: the grid-stride loops of both
# kernels); and (in a test of its own) one long recording.  1, 50 (the default) and 64 (the most) thresholds.
SHAPES = [(1, 1, 1, 64), (2, 16, 3, 50), (3, 63, 3, 1), (3, 64, 2, 64), (3, 65, 3, 50), (5, 130, 3, 64), (5, 130, 3, 1),
          (2, 700, 16, 50), (64, 512, 3, 50), (128, 16, 3, 50), (1100, 3, 16, 1)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def thresholds(n):
    if n == 50:
        return M.psds_default_thresholds()
    return tuple(float(F32((i + 1) / (n + 1))) for i in range(n))


def _gpu_counts(yt, yp, thr, dev, scenario):
    p = M.Psds(yt.shape[2], scenario, thr)
    p.update(torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev))
    return p.counts().numpy()


def _cpu_counts(yt, yp, thr, scenario):
    return M.psds_counts_host(torch.from_numpy(yt), torch.from_numpy(yp), thr, **SCENARIOS[scenario]).numpy()


@pytest.fixture(scope="module")
def cases():
    """Inputs and the reference counts per shape, made once: scores held for several frames against block labels, some scores
    exactly at a threshold, some NaN on both sides."""
    out = {}
    for b, t, k, n in SHAPES:
        rng = np.random.default_rng(b * 1000 + t + n)
        thr = thresholds(n)
        yt, yp = block_case(rng, b, t, k, block=8 if t < 512 else 24, hold=4 if t < 512 else 12)
        at = rng.random(yp.shape) < 0.02
        yp[at] = np.asarray(thr, F32)[rng.integers(0, n, int(at.sum()))]
        yp[rng.random(yp.shape) < 0.005] = np.nan
        yt[rng.random(yt.shape) < 0.005] = np.nan
        out[(b, t, k, n)] = (yt, yp, thr, {sc: R.counts(yt, yp, thr, **SCENARIOS[sc]) for sc in (1, 2)})
    return out


@pytest.mark.parametrize("scenario", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_the_definition_and_the_cpu_path(shape, scenario, cases):
    dev = _dev()
    yt, yp, thr, want = cases[shape]
    b, t, k, n = shape
    got = _gpu_counts(yt, yp, thr, dev, scenario)
    assert got.shape == (n + 1, k, k + 2) and np.array_equal(got, want[scenario]), np.argwhere(got != want[scenario])[:8]
    assert np.array_equal(got, _cpu_counts(yt, yp, thr, scenario))
    assert np.array_equal(got, _gpu_counts(yt, yp, thr, dev, scenario))              # two runs: equal bits
    assert int(got[n, 0, R.frames_column(k)]) == b * t


@pytest.mark.parametrize("scenario", [1, 2])
def test_worked_example(scenario):
    yt, yp, thr = worked_example()
    assert _gpu_counts(yt, yp, thr, _dev(), scenario).tolist() == WORKED[scenario] + [WORKED_TOTALS]


@pytest.mark.parametrize("t", [64, 65, 130, 700])
def test_crafted_rows(t):
    """All active, all inactive, alternating (T / 2 events: the ground-truth list's capacity), one run from frame 0 to T - 1
    across every step, runs that end at frame 63 and start at 64, a detection over three ground-truth events, one event under
    three detections that pass GTC only jointly, a detection lying only on another class's event, NaN scores - each as labels
    against each as scores, the scores EXACTLY at the thresholds."""
    dev = _dev()
    rows = [np.ones(t, F32), np.zeros(t, F32), (np.arange(t) % 2 == 0).astype(F32), (np.arange(t) % 2 == 1).astype(F32)]
    edge = np.zeros(t, F32)
    edge[50:64] = 1
    edge[[i for i in (127, 128, 130, t - 1) if i < t]] = 1
    rows += [edge, 1 - edge]
    three = np.zeros(t, F32)                      # three events of 10 frames with gaps of 8 ...
    three[4:14] = three[22:32] = three[40:50] = 1
    over = np.zeros(t, F32)                       # ... under one run of 50: 30 / 50 on it - and three runs of 12, 12, 20 = 44 of 50
    over[2:52] = 1
    parts = np.zeros(t, F32)
    parts[2:14] = parts[18:30] = parts[32:52] = 1
    tail = np.zeros(t, F32)                       # open at frame T - 1, begun in the first step
    tail[t // 3:] = 1
    rows += [three, over, parts, tail]
    k = len(rows)
    labels = np.stack(rows, 1)[None]              # [1, T, 10]
    thr = (0.25, 0.5, 0.75)
    for shift in range(k):
        scores = np.roll(labels, shift, axis=2) * F32(thr[shift % 3])       # active at the thresholds up to its own, exactly
        holes = scores.copy()
        holes[0, 5::17] = np.nan
        yt, yp = np.concatenate([labels, labels]), np.concatenate([scores, holes])
        for sc in (1, 2):
            want = R.counts(yt, yp, thr, **SCENARIOS[sc])
            got = _gpu_counts(yt, yp, thr, dev, sc)
            assert np.array_equal(got, want), (shift, sc, np.argwhere(got != want)[:8])
    alt = rows[2].reshape(1, t, 1)
    got = _gpu_counts(alt, alt, (0.5,), dev, 1)
    assert got[0, 0].tolist() == [(t + 1) // 2, 0, (t + 1) // 2] and got[1, 0].tolist() == [(t + 1) // 2, (t + 1) // 2, t]
    # the three events under one detection, and the event under three detections, by hand
    yt = np.stack([three, over], 1)[None]
    yp = np.stack([over, parts], 1)[None]
    assert _gpu_counts(yt, yp, (0.5,), dev, 1)[0].tolist() == [[0, 0, 1, 1], [0, 1, 0, 3]]    # 60 % < DTC 70 %; 88 % >= GTC 70 %
    assert _gpu_counts(yt, yp, (0.5,), dev, 2)[0].tolist() == [[3, 0, 0, 1], [0, 1, 0, 3]]
    yp = np.stack([np.zeros(t, F32), three], 1)[None]                                        # class 1 fires on class 0's events only
    assert _gpu_counts(np.stack([three, np.zeros(t, F32)], 1)[None], yp, (0.5,), dev, 2)[0].tolist() == [[0, 0, 0, 0], [3, 0, 3, 3]]


def test_one_long_recording():
    """The `evaluate` shape: one file of 40000 frames (10 min 40 s), 3 classes, the default thresholds."""
    dev = _dev()
    rng = np.random.default_rng(40000)
    yt, yp = block_case(rng, 1, 40000, 3, block=50, p=0.3, hold=10)
    yt[0, 3000:9000, 1] = 1                        # events and detections across a hundred steps
    yp[0, 2900:9100, 1] = 0.97
    thr = M.psds_default_thresholds()
    for sc in (1, 2):
        want = R.counts(yt, yp, thr, **SCENARIOS[sc])
        got = _gpu_counts(yt, yp, thr, dev, sc)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert int(np.trace(want[25, :, :3])) > 50 and int(want[25, 1, 4]) > 0        # true positives and false positives
        assert np.array_equal(got, _cpu_counts(yt, yp, thr, sc))
    assert int(want[25, :, :3].sum() - np.trace(want[25, :, :3])) > 0                 # and cross-triggers


def test_state_accumulates_adds_over_devices_and_resets(cases):
    dev = _dev()
    yt, yp, thr, want = cases[SHAPES[4]]
    p, other = M.Psds(3, 2, thr), M.Psds(3, 2, thr)
    gt, gp = torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)
    p.update(gt[:1], gp[:1])
    p.update(gt[1:], gp[1:])                                                          # two updates = one on the concatenation
    assert np.array_equal(p.counts().numpy(), want[2])
    assert int(other.counts().sum()) == 0                                             # a second object shares nothing
    p.update(torch.from_numpy(yt), torch.from_numpy(yp))                              # a second device's state (the host's): they add up
    assert len(p.states) == 2 and np.array_equal(p.counts().numpy(), 2 * want[2])
    p.update(gt.double(), gp)                                                         # (any floating label type)
    assert np.array_equal(p.counts().numpy(), 3 * want[2])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other.update(gt, gp)
    other.update(gt, gp)                                                              # two streams: a workspace each
    side.synchronize()
    assert np.array_equal(other.counts().numpy(), 2 * want[2]) and len(other._workspaces) == 2
    big = cases[SHAPES[8]]
    grown = M.Psds(3, 2, thr)
    grown.update(gt, gp)
    grown.update(torch.from_numpy(big[0]).to(dev), torch.from_numpy(big[1]).to(dev))  # a larger batch: the workspace grows
    grown.update(gt, gp)                                                              # ... and serves the smaller one again
    assert np.array_equal(grown.counts().numpy(), 2 * want[2] + big[3][2]) and len(grown._retired) == 1
    p.reset()
    assert int(p.counts().abs().sum()) == 0
    with pytest.raises(ValueError):
        p.update(gt, gp[:, :10])
    with pytest.raises(ValueError):
        p.update(gt, gp.cpu())
    assert int(p.counts().abs().sum()) == 0
    p.update(gt, gp)
    assert np.array_equal(p.counts().numpy(), want[2])


def test_iris_psds_counts_refuses_before_any_launch():
    lib = N.lib()
    p = C.c_void_p(64)
    INVALID, UNSUPPORTED = -1, -2
    big = C.c_size_t(1 << 40)

    def levels(*values):
        return (C.c_float * len(values))(*values)

    def call(yt=p, yp=p, b=1, t=64, k=3, thr=levels(0.5), n=1, dtc=70, gtc=70, cttc=0, ws=p, ws_bytes=big, counts=p):
        return lib.iris_psds_counts(yt, yp, b, t, k, thr, n, dtc, gtc, cttc, ws, ws_bytes, counts, None)

    def refused(rc, code):
        assert rc == code, (rc, lib.iris_last_error())
        assert lib.iris_last_error().startswith(b"iris_psds_"), lib.iris_last_error()
    for kw in (dict(yt=None), dict(yp=None), dict(thr=None), dict(ws=None), dict(counts=None), dict(b=0), dict(t=0), dict(k=0),
               dict(b=-1), dict(n=0), dict(dtc=0), dict(dtc=101), dict(gtc=0), dict(gtc=101), dict(cttc=-1), dict(cttc=101),
               dict(thr=levels(0.5, 0.5), n=2), dict(thr=levels(0.6, 0.5), n=2), dict(thr=levels(0.5, float('nan')), n=2),
               dict(thr=levels(float('inf')), n=1), dict(thr=levels(float('nan')), n=1), dict(ws=C.c_void_p(68)),
               dict(ws_bytes=C.c_size_t(0))):
        refused(call(**kw), INVALID)
    need = lib.iris_psds_workspace_bytes(1, 64, 3, 1)
    # 3 rows x 1 threshold x 2 words of 8 + 4 bytes; per row 65 prefix counts, an event count, 33 starts and 33 ends (int32)
    assert need == 3 * 2 * 12 + 3 * 4 * (65 + 1 + 2 * 33)
    refused(call(ws_bytes=C.c_size_t(need - 1)), INVALID)
    refused(call(k=17), UNSUPPORTED)
    refused(call(n=65, thr=levels(*[i / 100 for i in range(65)])), UNSUPPORTED)
    refused(call(t=2 ** 20 + 1), UNSUPPORTED)
    refused(call(b=2 ** 12, t=2 ** 19), UNSUPPORTED)                                  # 2^31 frames
    assert lib.iris_psds_workspace_bytes(1, 64, 17, 1) == 0 and lib.iris_psds_workspace_bytes(1, 64, 3, 0) == 0
    assert lib.iris_psds_workspace_bytes(1, 64, 3, 65) == 0
    assert lib.iris_psds_workspace_bytes(64, 512, 3, 50) == 192 * 50 * 9 * 12 + 192 * 4 * (513 + 1 + 2 * 257)
    assert "iris_psds_counts" in N.SIGNATURES and lib.iris_abi_version() == 1


def test_fit_with_psds_logs_a_finite_val_psds():
    """psds() compiled into a GPU model: test_step feeds the counts (two launches), a 'train'-phase call leaves them alone, the
    row of `fit` gains a finite val_psds, and the counts are those of the definition on the same predictions."""
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    dev = _dev()
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(5)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    seen = []

    def recorder(y_true, y_pred):
        seen.append((y_true.detach().cpu(), y_pred.detach().cpu()))
        return y_pred.new_zeros(())
    hop = S.output_hop(cfg)
    score = M.psds(2, hop=hop)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue, metrics=[score, recorder])
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(4, 32, 64, 1, generator=g).to(dev), (torch.rand(4, 2, 3, generator=g) > 0.5).float().to(dev)) for _ in range(2)]
    assert 'psds' not in model.test_step(batches[0])
    ms = model._metrics
    before = score.counter.counts()
    ms(batches[0][1], torch.rand(4, 2, 3, device=dev), 'train')                       # no train-phase launch: the state is untouched
    assert torch.equal(score.counter.counts(), before) and int(before[50, 0, 3]) == 8    # 4 clips of 2 output frames
    assert not any(t is s for t in ms.state_tensors() for s in score.counter.states.values())
    want = R.counts(seen[0][0].numpy(), seen[0][1].numpy(), M.psds_default_thresholds(), **SCENARIOS[2])
    assert np.array_equal(before.numpy(), want)
    value = ms.psds_values('val_')['val_psds']
    assert value == M.psds_metrics(want, M.psds_default_thresholds(), hop, 16000, 0.5, 1.0)['psds'] and math.isfinite(value)
    hist = S.fit(model, Dataset.from_generator(lambda: iter(batches)).repeat(), epochs=1, steps_per_epoch=1,
                 validation_data=Dataset.from_generator(lambda: iter(batches)).repeat(), validation_steps=2, verbose=False, graph=False)
    assert math.isfinite(hist[0]['val_psds']) and -1.0 <= hist[0]['val_psds'] <= 1.0
    assert int(score.counter.counts()[50, 0, 3]) == 16                                   # reset, then the two validation batches


def test_eval_writes_the_scores_of_the_recordings(tmp_path, monkeypatch):
    """`challenge_amd.eval --psds OUT.json` on two synthetic recordings in the sample layout: the ER scores are those of a run
    without the flag, and the file holds compute() per scenario of counts with one [1, T, 3] update per file."""
    from scipy.io import wavfile
    from challenge_amd import eval as E
    from challenge_amd import sj_train as S
    dev = _dev()
    flags = ['--v', '9', '--n_mels', '64', '--n_frame', '128', '--n_chan', '1']
    cfg = S.ARGS().get(flags)
    torch.manual_seed(0)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    torch.save(model.state_dict(), tmp_path / "run.pt")
    rng = np.random.default_rng(5)
    for i in range(2):
        wav = (rng.standard_normal((48000, 2)) * 0.1).astype(F32)
        wav[16000:24000] *= 8
        wavfile.write(str(tmp_path / f"clip{i}.wav"), 16000, wav)
    with open(tmp_path / "sample_answer.json", "w") as f:
        json.dump({"task2_answer": {"clip0": [[0, 0, 1], [1, 1, 2]], "clip1": [[2, 0, 3]]}}, f)
    monkeypatch.chdir(tmp_path)
    argv = ['--name', 'run', '--path', str(tmp_path)] + flags
    plain = E.main(argv)
    assert E.main(argv + ['--psds', 'out.json']) == plain
    with open(tmp_path / "out.json") as f:
        out = json.load(f)
    assert set(out) == {'1', '2'}
    for sc, res in out.items():
        # one window of 128 frames per recording is decoded and scored; the answers put one event per class into them
        assert res['n_gt'] == [1, 1, 1] and res['n_frames'] >= 2 * 126 and len(res['thresholds']) == 50
        assert math.isfinite(res['psds']) and res['classes_without_gt'] == []
        assert res['alpha_ct'] == (0.5 if sc == '2' else 0.0)
    E.main(argv + ['--psds', 'one.json', '--psds_scenario', '2'])
    with open(tmp_path / "one.json") as f:
        assert json.load(f) == {'2': out['2']}
    psds = M.Psds(3, 1)
    assert M.evaluate(cfg, E.load_model(S.ARGS().get(['--name', 'run'] + flags), str(tmp_path)), psds=psds) == plain
    assert json.loads(json.dumps(psds.compute())) == out['1']
