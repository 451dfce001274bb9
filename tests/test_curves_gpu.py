"""GPU tests of the score histogram launch (iris_score_hist, csrc/k_curves.h) behind metrics.ScoreHistogram / score_curves.
Counts are integers: every comparison - with the CPU path (torch ops, same rule), with tests/curves_ref.py (a plain loop over
the elements) and between two runs - is for EQUALITY."""
import numpy as np
import pytest
import torch

import curves_ref as R
from challenge_amd import metrics as M
from test_curves_host import SPECIAL_LABELS, random_case, special_batch, tol

pytestmark = pytest.mark.gpu
F32 = np.float32

# (B, T, K, bins): the smallest; a wave tail with K not dividing a vector; one class per LDS tile at the widest histogram and the
# most classes; the validation shape
SHAPES = [(1, 1, 1, 16), (3, 65, 3, 64), (2, 130, 16, 4096), (64, 512, 3, 1024)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gpu_counts(yt, yp, k, bins, dev):
    h = M.ScoreHistogram(k, bins)
    h.update(torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev))
    return h.counts().numpy()


def _cpu_counts(yt, yp, k, bins):
    h = M.ScoreHistogram(k, bins)
    h.update(torch.from_numpy(yt), torch.from_numpy(yp))
    return h.counts().numpy()


@pytest.fixture(scope="module")
def uniform_cases():
    """Inputs and from-scratch reference counts per shape, computed once."""
    out = {}
    for b, t, k, bins in SHAPES:
        rng = np.random.default_rng(b * 1000 + t)
        yt, yp = random_case(rng, b * t, k, bins)
        yt, yp = yt.reshape(b, t, k), yp.reshape(b, t, k)
        out[(b, t, k, bins)] = (yt, yp, R.counts(yt, yp, bins))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_the_cpu_path_and_the_definition(shape, uniform_cases):
    b, t, k, bins = shape
    dev = _dev()
    yt, yp, want = uniform_cases[shape]
    got = _gpu_counts(yt, yp, k, bins, dev)
    assert got.sum() == b * t * k
    assert np.array_equal(got, want)
    assert np.array_equal(got, _cpu_counts(yt, yp, k, bins))
    assert np.array_equal(got, _gpu_counts(yt, yp, k, bins, dev))          # two runs: equal bits


def test_every_prediction_exactly_one_is_still_exact():
    """The worst contention: every score in one slot.  Also everything at 0, and sigmoid-like scores piled up at both ends."""
    b, t, k, bins = SHAPES[-1]
    dev = _dev()
    rng = np.random.default_rng(5)
    yt = (rng.random((b, t, k)) < 0.3).astype(F32)
    n_pos = yt.reshape(-1, k).sum(0).astype(np.int64)
    for value, slot in ((1.0, bins - 1), (0.0, 0)):
        got = _gpu_counts(yt, np.full((b, t, k), value, F32), k, bins, dev)
        want = np.zeros((k, 2, bins + 1), np.int64)
        want[:, 1, slot], want[:, 0, slot] = n_pos, b * t - n_pos
        assert np.array_equal(got, want)
    _, sharp = random_case(rng, b * t, k, bins, sharp=True)
    sharp = sharp.reshape(b, t, k)
    got = _gpu_counts(yt, sharp, k, bins, dev)
    assert np.array_equal(got, _cpu_counts(yt, sharp, k, bins)) and np.array_equal(got, _gpu_counts(yt, sharp, k, bins, dev))
    # the case is what it claims to be: logits N(+-2, 6^2) pass +-ln(1023) = +-6.93 with probability Phi(-0.82) + Phi(-1.49) =
    # 0.206 + 0.068 = 27 % - that share of the 98,304 scores sits in the two end slots (binomial spread 0.14 %)
    assert got[:, :, 0].sum() + got[:, :, bins - 1].sum() > 0.25 * b * t * k


@pytest.mark.parametrize("k,bins", [(3, 16), (3, 1024), (16, 4096), (5, 2048)])
def test_special_values_land_in_their_slots(k, bins):
    dev = _dev()
    yt, yp, want = special_batch(bins, k)
    got = _gpu_counts(yt, yp, k, bins, dev)
    assert got.sum() == yp.size
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[:, :, bins].sum() == k * len(SPECIAL_LABELS)                  # the NaN predictions, kept apart
    assert np.array_equal(got, _gpu_counts(yt, yp, k, bins, dev))


def test_state_accumulates_per_object_and_follows_the_stream(uniform_cases):
    dev = _dev()
    b, t, k, bins = SHAPES[1]
    yt, yp, want = uniform_cases[SHAPES[1]]
    gt, gp = torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)
    h, other = M.ScoreHistogram(k, bins), M.ScoreHistogram(k, bins)
    h.update(gt, gp)
    h.update(gt, gp)
    assert np.array_equal(h.counts().numpy(), 2 * want)
    assert int(other.counts().sum()) == 0                                    # a second object shares nothing
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other.update(gt, gp)
        other.update(gt.double(), gp.half().float())                         # (any floating label type; fp32 predictions again)
    side.synchronize()
    assert np.array_equal(other.counts().numpy(), want + R.counts(yt, gp.half().float().cpu().numpy(), bins))
    h.reset()
    assert int(h.counts().sum()) == 0
    with pytest.raises(ValueError):
        h.update(gt, gp[:, :10])
    with pytest.raises(ValueError):
        h.update(gt, gp.cpu())
    assert int(h.counts().sum()) == 0


def test_metric_set_through_test_step_equals_the_cpu_path():
    """score_curves() compiled into a GPU model: test_step feeds the histogram (one launch), a 'train'-phase call leaves it alone,
    and the values are those of the CPU path on the same predictions."""
    from challenge_amd import sj_train as S
    dev = _dev()
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(5)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    seen = []

    def recorder(y_true, y_pred):
        seen.append((y_true.detach().cpu(), y_pred.detach().cpu()))
        return y_pred.new_zeros(())
    curves = M.score_curves(64)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue, metrics=[curves, recorder])
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(6, 32, 64, 1, generator=g).to(dev), (torch.rand(6, 2, 3, generator=g) > 0.5).float().to(dev)) for _ in range(2)]
    for batch in batches:
        out = model.test_step(batch)
        assert 'score_curves' not in out
    ms = model._metrics
    before = curves.counter.counts()
    ms(batches[0][1], torch.rand(6, 2, 3, device=dev), 'train')              # no train-phase launch: the histogram is untouched
    model.train_step(batches[0])
    assert torch.equal(curves.counter.counts(), before) and int(before.sum()) == 2 * 6 * 2 * 3
    assert not any(t is s for t in ms.state_tensors() for s in curves.counter.states.values())
    cpu = M.ScoreHistogram(3, 64)
    for yt, yp in seen[:2]:
        cpu.update(yt, yp)
    assert torch.equal(before, cpu.counts())
    vals, want = ms.curve_values('val_'), cpu.compute()
    assert vals == {'val_' + k: want[k] for k in ('auc', 'map', 'best_f1')}
    ref = R.metrics(torch.cat([a for a, _ in seen[:2]]).numpy(), torch.cat([b for _, b in seen[:2]]).numpy(), 64)
    assert all(abs(vals['val_' + k] - ref[k]) <= tol(64) for k in ('auc', 'map', 'best_f1'))
    ms.reset()
    assert int(curves.counter.counts().sum()) == 0


def test_eval_writes_the_curves_of_the_recordings(tmp_path, monkeypatch):
    """`challenge_amd.eval --curves OUT.json` on two synthetic recordings: the scores are those of a run without the flag, and
    the file holds compute() of a histogram with one count per frame and class."""
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
    assert E.main(argv + ['--curves', 'out.json', '--curve_bins', '256']) == plain
    with open(tmp_path / "out.json") as f:
        out = json.load(f)
    per = out['per_class']
    # predict_frames at the default overlap_hop of 512 frames covers a 188-frame recording with ONE window of n_frame = 128
    # frames: those are the frames that are decoded, scored and counted
    frames = [p + n + x for p, n, x in zip(per['n_pos'], per['n_neg'], per['n_nan'])]
    assert out['bins'] == 256 and frames == [2 * 128] * 3
    # second2frame at 62.5 frames per second: [0 s, 1 s) = frames 0..61 (round half to even), [1 s, 2 s) = 62..124, [0 s, 3 s) = all
    assert per['n_pos'] == [62, 63, 128] and per['n_nan'] == [0, 0, 0]
    assert all(0.0 <= v <= 1.0 for v in per['auroc'] + per['ap'] + per['best_f1'] + [out['auc'], out['map'], out['best_f1']])
