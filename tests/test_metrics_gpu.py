"""GPU tests of the fused metric launch (iris_event_metrics) and of the metrics in the graphed training step, evaluate()
and `python -m challenge_amd.eval`.  The oracle is test_metrics_host.ref_er (an op-by-op NumPy restatement of the
reference's er_score) plus the restatement of the scoring chain below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from challenge_amd import metrics as M
from challenge_amd import trainer as TR
from test_metrics_host import adversarial_cases, ref_er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _run_pattern(rng, b, t, k, mean_len):
    """0/1 labels made of runs (mean length `mean_len`) - few events per clip, so the O(N^2) restatement stays small."""
    p = 1.0 / max(mean_len, 1.0)
    flips = rng.random((b, t, k)) < p
    return (np.cumsum(flips, axis=1) % 2).astype(np.float32)


def _ref_er_per_clip(yt, yp, threshold=0.5, smoothing=False):
    return np.concatenate([ref_er(yt[i:i + 1], yp[i:i + 1], threshold, smoothing) for i in range(yt.shape[0])])


def _check(yt, yp, threshold=0.5, smoothing=False, ref=True):
    dev = _dev()
    gt, gp = torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)
    pool = M.SMOOTHING_POOL if smoothing else 0
    st = torch.zeros(3, dtype=torch.float64, device=dev)
    r = M.event_metrics(gt, gp, threshold, pool, want_cos=True, f1_state=st)
    r2 = M.event_metrics(gt, gp, threshold, pool, want_cos=True, f1_state=torch.zeros_like(st))
    er = r['er'].cpu().numpy()
    host = M.er_host(torch.from_numpy(yt), torch.from_numpy(yp), threshold, pool).numpy()
    assert np.array_equal(er.view(np.int32), host.view(np.int32))
    if ref:
        want = _ref_er_per_clip(yt, yp, threshold, smoothing)
        assert np.array_equal(er.view(np.int32), want.view(np.int32)), (er, want)
    for key in ('er', 'cos_sim', 'f1_score'):   # two launches: the same bits (NaN included)
        assert torch.equal(r[key].view(torch.int32), r2[key].view(torch.int32)), key
    counts = M.f1_counts_host(torch.from_numpy(yt), torch.from_numpy(yp))
    assert torch.equal(st.cpu(), counts)
    assert torch.equal(r['f1_score'].cpu(), M.f1_from_counts(counts))
    cs = TR.cos_sim(torch.from_numpy(yt), torch.from_numpy(yp))
    fin = torch.isfinite(cs)
    assert torch.allclose(r['cos_sim'].cpu()[fin], cs[fin], atol=1e-6, rtol=0)


@pytest.mark.parametrize("b", [1, 12, 64, 65])
@pytest.mark.parametrize("t", [1, 63, 64, 65, 512, 2048, 8192])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_kernel_matches_restatement(b, t, k):
    rng = np.random.default_rng(b * 100003 + t * 17 + k)
    yt = _run_pattern(rng, b, t, k, t / 6)
    yp = np.clip(_run_pattern(rng, b, t, k, t / 5) * 0.8 + rng.random((b, t, k)).astype(np.float32) * 0.15, 0, 1).astype(np.float32)
    yp[:, ::97] = 0.5   # on the threshold
    _check(yt, yp, 0.5, False)
    _check(yt, yp, 0.3, True)


@pytest.mark.parametrize("t", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("smoothing", [False, True])
def test_kernel_adversarial_patterns(t, k, smoothing):
    rng = np.random.default_rng(t * 7 + k)
    for yt, yp in adversarial_cases(rng, 12, t, k):
        if smoothing:
            yp = np.repeat(yp, 31, axis=1)[:, :t].copy()
        for thr in (0.5, 0.3):
            _check(yt, np.ascontiguousarray(yp), thr, smoothing)


def test_kernel_other_rate_and_large_adversarial():
    rng = np.random.default_rng(9)
    for yt, yp in adversarial_cases(rng, 65, 8192, 16):   # the bitwise CPU path as oracle at full size
        _check(yt, np.ascontiguousarray(yp), 0.5, False, ref=False)
        _check(yt, np.ascontiguousarray(yp), 0.5, True, ref=False)
    dev = _dev()
    yt = (rng.random((5, 300, 3)) > 0.5).astype(np.float32)
    yp = rng.random((5, 40, 3)).astype(np.float32)   # T' != T: er only
    er = M.er_score(smoothing=False)(torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)).cpu().numpy()
    assert np.array_equal(er, ref_er(yt, yp, smoothing=False))
    with pytest.raises(ValueError):
        M.event_metrics(torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev), want_cos=True)


def test_metric_callables_captured_in_a_graph():
    dev = _dev()
    rng = np.random.default_rng(11)

    def batch():
        return (torch.from_numpy(_run_pattern(rng, 16, 128, 3, 20)).to(dev),
                torch.from_numpy(rng.random((16, 128, 3)).astype(np.float32)).to(dev))
    er, f1 = M.er_score(smoothing=True), M.f1_score()
    ms = M.MetricSet([M.cos_sim, M.f1_score(), M.er_score(smoothing=False)])
    yt, yp = batch()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):   # warm-up (allocates the workspaces)
        er(yt, yp), f1(yt, yp), ms(yt, yp)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    f1.states[dev].zero_()
    ms.f1.states[dev].zero_()
    ms.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o_er, o_f1, o_ms = er(yt, yp), f1(yt, yp), ms(yt, yp)
    torch.cuda.synchronize()
    assert float(f1.states[dev].abs().sum()) == 0.0   # capturing ran nothing
    ref_f1, ref_ms_f1 = M.f1_score(), M.f1_score()
    sums = np.zeros(3)
    for i in range(3):
        nt, npd = batch()
        yt.copy_(nt)
        yp.copy_(npd)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_er, M.er_score(smoothing=True)(nt, npd))
        assert torch.equal(o_f1, ref_f1(nt, npd))
        assert torch.equal(f1.states[dev], ref_f1.states[dev])   # advanced once per replay
        e = M.event_metrics(nt, npd, want_cos=True)
        assert torch.equal(o_ms['er'], e['er']) and torch.equal(o_ms['cos_sim'], e['cos_sim'])
        assert torch.equal(o_ms['f1_score'], ref_ms_f1(nt, npd))
        sums += [float(o_ms['er'].double().sum()), float(o_ms['cos_sim'].double().sum()), float(o_ms['f1_score'])]
    acc = ms.accum(dev, 'train').cpu()
    assert acc[3].item() == 3 * 16 and acc[4].item() == 3
    assert acc[:3].numpy() == pytest.approx(sums, rel=1e-12, abs=1e-12)   # the sums fit logs: every clip, every replay


def _small_model(cfg, dev, seed=0):
    from challenge_amd import sj_train as S
    torch.manual_seed(seed)
    return S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)


def test_graphed_step_with_metrics():
    from challenge_amd import sj_train as S
    dev = _dev()
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_frame', '128', '--n_chan', '1', '--batch_size', '8'])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 64, 128, 1, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    y = (torch.rand(8, 4, 3, generator=g) < 0.4).float().to(dev)
    models, steps, f1s = [], [], []
    for with_metrics in (False, True):
        m = _small_model(cfg, dev)
        f1 = M.f1_score()
        m.compile(S.make_optimizer(cfg, m.parameters(), capturable=True), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  metrics=[M.cos_sim, f1, M.er_score(smoothing=False)] if with_metrics else None)
        st = S.GraphedTrainStep(m, (x, y), preserve_state=True)
        if with_metrics:
            assert float(f1.states[dev].abs().sum()) == 0.0          # the warm-up counted nothing
            assert float(m._metrics.accum(dev, 'train').abs().sum()) == 0.0
        models.append(m)
        steps.append(st)
        f1s.append(f1)
    ref_f1 = M.f1_score()
    sums = np.zeros(3)
    for _ in range(3):
        steps[0]((x, y))
        out = steps[1]((x, y))
        torch.cuda.synchronize()
        yp = steps[1].y_pred
        assert torch.equal(out['er'], M.er_score(smoothing=False)(y, yp))
        assert torch.equal(out['cos_sim'], M.event_metrics(y, yp, want_cos=True)['cos_sim'])
        assert torch.allclose(out['cos_sim'].cpu(), TR.cos_sim(y.cpu(), yp.cpu()), atol=1e-6, rtol=0)
        assert torch.equal(out['f1_score'], ref_f1(y, yp))
        sums += [float(out['er'].double().sum()), float(out['cos_sim'].double().sum()), float(out['f1_score'])]
    for a, b in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(a, b)
    acc = models[1]._metrics.accum(dev, 'train').cpu()
    assert acc[3].item() == 24 and acc[4].item() == 3
    assert acc[:3].numpy() == pytest.approx(sums, rel=1e-12, abs=1e-12)


def _write_wavs(tmp_path, rng, n_chan, seconds=3.0):
    from scipy.io import wavfile
    names = []
    for i in range(2):
        wav = (rng.standard_normal((int(16000 * seconds), n_chan)) * 0.1).astype(np.float32)
        wav[16000:24000] *= 8
        name = f"clip{i}"
        wavfile.write(str(tmp_path / f"{name}.wav"), 16000, wav)
        names.append(name)
    answers = {"task2_answer": {names[0]: [[0, 0, 1], [1, 1, 2]], names[1]: [[2, 0, 3]]}}
    with open(tmp_path / "sample_answer.json", "w") as f:
        json.dump(answers, f)
    return names, answers["task2_answer"]


def _restated_score(frames, gt, hop=256, sr=16000):
    """get_start_end_frame -> output_to_metric -> get_er, restated."""
    d = np.asarray(frames)
    events = []
    for c in range(3):
        col = np.concatenate([[0.0], d[:, c], [0.0]])
        on = np.flatnonzero(np.diff(col) > 0)
        off = np.flatnonzero(np.diff(col) < 0) - 1
        events += [(c, int(((s + e) / 2) * hop / sr)) for s, e in zip(on, off)]
    preds = sorted(events, key=lambda p: p[1])
    hits = 0
    for g in sorted(gt, key=lambda g: g[1]):
        for i, p in enumerate(preds):
            if g[1] <= p[1] <= g[2] and g[0] == p[0]:
                hits += 2
                del preds[i]
                break
    return (len(events) + len(gt) - hits) / len(gt)


def test_evaluate_matches_evaluate_wav_and_restatement(tmp_path):
    from challenge_amd import data_utils as D
    from challenge_amd import inference as I
    from challenge_amd import sj_train as S
    dev = _dev()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_frame', '128', '--n_chan', '1'])
    model = _small_model(cfg, dev).eval()
    rng = np.random.default_rng(21)
    names, gt = _write_wavs(tmp_path, rng, 2)
    scores = M.evaluate(cfg, model, wav_dir=str(tmp_path), answer_path=str(tmp_path / "sample_answer.json"))
    want = []
    for n in names:
        data, sr = D.read_wav_file(str(tmp_path / f"{n}.wav"))
        frames = I.evaluate_wav(model, data, cfg, sample_rate=sr, device=dev).cpu().numpy()
        want.append(_restated_score(frames, gt[n]))
    assert scores == pytest.approx(want, abs=0)


def test_eval_module_runs(tmp_path):
    from challenge_amd import sj_train as S
    dev = _dev()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_frame', '128', '--n_chan', '1'])
    model = _small_model(cfg, dev)
    torch.save(model.state_dict(), tmp_path / "run.pt")
    _write_wavs(tmp_path, np.random.default_rng(5), 2)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "challenge_amd.eval", "--name", "run", "--path", str(tmp_path), "--v", "9",
                        "--n_mels", "64", "--n_frame", "128", "--n_chan", "1"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "FINAL SCORE:" in r.stdout
