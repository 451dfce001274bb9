"""GPU tests of the detection-count launches (iris_sed_counts, csrc/k_sedeval.h) behind metrics.SedEval / sed_eval.  Counts are
integers: every comparison - with tests/sedeval_ref.py (plain loops over rows, frames and events), with the CPU path and between
two runs - is for EQUALITY."""
import numpy as np
import pytest
import torch

import sedeval_ref as R
from challenge_amd import metrics as M
from test_sedeval_host import block_labels, random_case

pytestmark = pytest.mark.gpu
F32 = np.float32

# (B, T, K, n_thr): every T in {1, 63, 64, 65, 130, 512, 1000} (one frame; around the 64-frame step; several steps), B in
# {1, 2, 5}, K and n_thr in {1, 3, 16}, and T = 65 with the most classes and thresholds together
SHAPES = [(1, 1, 1, 1), (2, 63, 3, 3), (5, 64, 1, 16), (1, 65, 16, 16), (2, 130, 16, 1), (5, 512, 3, 3), (2, 1000, 3, 1)]
# the defaults (62.5 frames per segment); 16 frames per segment, a short collar and no length share; the model's output frames
# (1.95 frames per segment); segments longer than two steps (187.5 frames) with the widest offset share; a collar of 200 frames
# (up to 101 candidate predictions per event: more than the matching walk's 64-bit mask of taken ones holds)
PARAMS = [{}, dict(hop=100, segment=0.1, collar=0.05, offset_pct=0), dict(hop=8192), dict(segment=3.0, offset_pct=100),
          dict(hop=16, segment=0.05)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def thresholds(n):
    return tuple(float(F32((i + 1) / (n + 1))) for i in range(n))


def _gpu_counts(yt, yp, thr, dev, **kw):
    sed = M.SedEval(yt.shape[2], thr, **kw)
    sed.update(torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev))
    return sed.counts().numpy()


def _cpu_counts(yt, yp, thr, **kw):
    return M.sed_counts_host(torch.from_numpy(yt), torch.from_numpy(yp), thr, **kw).numpy()


@pytest.fixture(scope="module")
def cases():
    """Inputs per shape, made once: sigmoid-like scores against block labels, some scores exactly at a threshold, some NaN on
    both sides."""
    out = {}
    for b, t, k, n in SHAPES:
        rng = np.random.default_rng(b * 1000 + t)
        thr = thresholds(n)
        yt, yp = random_case(rng, b, t, k)
        at = rng.random(yp.shape) < 0.1
        yp[at] = np.asarray(thr, F32)[rng.integers(0, n, int(at.sum()))]
        yp[rng.random(yp.shape) < 0.02] = np.nan
        yt[rng.random(yt.shape) < 0.02] = np.nan
        out[(b, t, k, n)] = (yt, yp, thr)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_the_definition_and_the_cpu_path(shape, cases):
    dev = _dev()
    yt, yp, thr = cases[shape]
    b, t, k, n = shape
    for kw in PARAMS:
        want = R.counts(yt, yp, thr, **kw)
        got = _gpu_counts(yt, yp, thr, dev, **kw)
        assert got.shape == (n, k + 1, 6) and np.array_equal(got, want), (kw, np.argwhere(got != want)[:8])
        assert np.array_equal(got, _cpu_counts(yt, yp, thr, **kw))
        assert np.array_equal(got, _gpu_counts(yt, yp, thr, dev, **kw))              # two runs: equal bits


@pytest.mark.parametrize("t", [64, 65, 130])
def test_rows_that_stress_the_run_extraction(t):
    """All active, all inactive, alternating (T / 2 events: the lists' capacity), runs from frame 0, open at the end, across and
    touching the 64-frame steps - each as labels against each as scores, scores EXACTLY at the thresholds."""
    dev = _dev()
    rows = [np.ones(t, F32), np.zeros(t, F32), (np.arange(t) % 2 == 0).astype(F32), (np.arange(t) % 2 == 1).astype(F32)]
    marks = np.zeros(t, F32)
    for s, e in ((0, 2), (60, 66), (t - 3, t - 1)):
        marks[max(s, 0):e + 1] = 1
    rows.append(marks)
    edge = np.zeros(t, F32)                       # a run that ends at frame 63, one that starts at 64, single frames at 127 / 128
    edge[50:64] = 1
    edge[[i for i in (127, 128, 130, t - 1) if i < t]] = 1
    rows.append(edge)
    rows.append(1 - edge)
    k = len(rows)
    labels = np.stack(rows, 1)[None]                                        # [1, T, 7]
    thr = (0.25, 0.5, 0.75)
    for shift in range(k):
        scores = np.roll(labels, shift, axis=2) * F32(thr[shift % 3])       # active at the thresholds up to its own, exactly
        both_t = np.concatenate([labels, labels]), np.concatenate([scores, np.roll(scores, 1, axis=2)])
        for kw in (PARAMS[0], PARAMS[1], PARAMS[4]):
            want = R.counts(*both_t, thr, **kw)
            got = _gpu_counts(*both_t, thr, dev, **kw)
            assert np.array_equal(got, want), (shift, kw, np.argwhere(got != want)[:8])
    alt = rows[2].reshape(1, t, 1)
    assert _gpu_counts(alt, alt, (0.5,), dev)[0, 0, 3:].tolist() == [(t + 1) // 2, 0, 0]


def test_one_long_recording():
    """The `evaluate` shape: one file of 40000 frames (10 min 40 s), 3 classes."""
    dev = _dev()
    rng = np.random.default_rng(40000)
    yt = block_labels(rng, 1, 40000, 3, block=50, p=0.3)
    logits = (yt * 2 - 1) * 2.0 + np.repeat(rng.standard_normal((1, 4000, 3)), 10, axis=1) * 1.5
    yp = (1.0 / (1.0 + np.exp(-logits))).astype(F32)
    want = R.counts(yt, yp, (0.5,))
    got = _gpu_counts(yt, yp, (0.5,), dev)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert want[0, 3, 3] == 640 and want[0, :3, 3].min() > 50                       # segments; matched events in every class
    assert np.array_equal(got, _cpu_counts(yt, yp, (0.5,)))


def test_state_accumulates_is_reproducible_and_resets(cases):
    dev = _dev()
    (yt, yp, thr), (yt2, yp2, _) = cases[SHAPES[5]], cases[SHAPES[1]]
    one, two = R.counts(yt, yp, thr), R.counts(yt2, yp2, thr)
    sed, other = M.SedEval(3, thr), M.SedEval(3, thr)
    gt, gp = torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)
    sed.update(gt, gp)
    sed.update(torch.from_numpy(yt2).to(dev), torch.from_numpy(yp2).to(dev))        # a smaller batch in the same workspace
    assert np.array_equal(sed.counts().numpy(), one + two)
    assert int(other.counts().sum()) == 0                                            # a second object shares nothing
    sed.update(gt.double(), gp)                                                      # (any floating label type)
    assert np.array_equal(sed.counts().numpy(), 2 * one + two)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other.update(gt, gp)
    other.update(gt, gp)                                                             # two streams: a workspace each
    side.synchronize()
    assert np.array_equal(other.counts().numpy(), 2 * one) and len(other._workspaces) == 2
    small = torch.from_numpy(yt2).to(dev), torch.from_numpy(yp2).to(dev)
    grown = M.SedEval(3, thr)
    grown.update(*small)
    grown.update(gt, gp)                                                             # a larger batch: the workspace grows
    grown.update(*small)                                                             # ... and serves the smaller one again
    assert np.array_equal(grown.counts().numpy(), one + 2 * two) and len(grown._retired) == 1
    sed.reset()
    assert int(sed.counts().abs().sum()) == 0
    with pytest.raises(ValueError):
        sed.update(gt, gp[:, :10])
    with pytest.raises(ValueError):
        sed.update(gt, gp.cpu())
    assert int(sed.counts().abs().sum()) == 0
    sed.update(gt, gp)
    assert np.array_equal(sed.counts().numpy(), one)


def test_metric_set_through_test_step_equals_the_cpu_path():
    """sed_eval() compiled into a GPU model: test_step feeds the counts (two launches), a 'train'-phase call leaves them alone,
    and the values are those of sed_counts_host on the same predictions."""
    from challenge_amd import sj_train as S
    dev = _dev()
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '2'])
    torch.manual_seed(5)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    seen = []

    def recorder(y_true, y_pred):
        seen.append((y_true.detach().cpu(), y_pred.detach().cpu()))
        return y_pred.new_zeros(())
    thr, hop = (0.4, 0.5), S.output_hop(cfg)
    sed = M.sed_eval(thr, hop=hop)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue, metrics=[sed, recorder])
    g = torch.Generator().manual_seed(12)
    batch = (torch.randn(2, 32, 64, 1, generator=g).to(dev), (torch.rand(2, 2, 3, generator=g) > 0.5).float().to(dev))
    assert 'sed_eval' not in model.test_step(batch)
    ms = model._metrics
    before = sed.counter.counts()
    ms(batch[1], torch.rand(2, 2, 3, device=dev), 'train')                           # no train-phase launch: the state is untouched
    model.train_step(batch)
    assert torch.equal(sed.counter.counts(), before) and int(before[0, 3, 3]) == 2    # 2 clips; a clip's 2 output frames (0 s, 0.512 s) share a segment
    assert not any(t is s for t in ms.state_tensors() for s in sed.counter.states.values())
    want = M.sed_counts_host(*seen[0], thr, hop=hop)
    assert torch.equal(before, want) and np.array_equal(want.numpy(), R.counts(seen[0][0].numpy(), seen[0][1].numpy(), thr, hop=hop))
    first = M.sed_metrics(want, thr)['per_threshold'][0]
    vals = ms.sed_values('val_')
    for name, value in (('val_seg_f1', first['segment']['f1']), ('val_seg_er', first['segment']['er']), ('val_event_f1', first['event']['f1'])):
        assert vals[name] == value or (vals[name] != vals[name] and value != value), (name, vals, first)
    ms.reset()
    assert int(sed.counter.counts().sum()) == 0


def test_eval_writes_the_measures_of_the_recordings(tmp_path, monkeypatch):
    """`challenge_amd.eval --sed_eval OUT.json` on two synthetic recordings in the sample layout: the scores are those of a run
    without the flag, and the file holds compute() of counts with one [1, T, 3] update per file."""
    import json
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
    assert E.main(argv + ['--sed_eval', 'out.json', '--sed_thresholds', '0.3,0.5']) == plain
    with open(tmp_path / "out.json") as f:
        out = json.load(f)
    assert out['thresholds'] == [float(F32(0.3)), 0.5] and len(out['per_threshold']) == 2
    for res in out['per_threshold']:
        # one window of 128 frames per recording is decoded and scored: frames 0 .. 127 lie in segments 0, 1, 2; the answers
        # put one event per class into them: [0 s, 1 s) class 0 = frames 0 .. 61, one segment; [1 s, 2 s) class 1 = frames
        # 62 .. 124 (second2frame rounds 62.5 to 62, and frame 62 starts at 0.992 s), two segments; [0 s, 3 s) class 2, three
        assert res['segment']['n_segments'] == 2 * 3 and res['segment']['n_ref'] == 1 + 2 + 3 and res['event']['n_ref'] == 3
        assert res['event']['n_pred'] >= 0 and len(res['event']['per_class']['f1']) == 3
    assert out['per_threshold'][0]['event']['n_pred'] >= 0
