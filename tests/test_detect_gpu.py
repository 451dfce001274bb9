"""GPU tests of event detection: the iris_decode_events launches bitwise against detect.py's CPU restatement (ragged batches,
edge cases, repeat calls, graph replay), `detect` against the existing chain (inference.predict_frames ->
Challenge_Metric.get_start_end_frame) file by file, grouping, and `python -m challenge_amd.detect`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from challenge_amd import detect as DT
from challenge_amd import metrics as M
from test_detect_host import ref_smoothed, run_preds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE = 1e-5


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for gc, wc in zip(g, w):
            assert gc.dtype == np.int64 and gc.shape == wc.shape and np.array_equal(gc, wc)


def _kernel_vs_host(preds, win_off, frame_lens, n_frame, hop):
    p = torch.from_numpy(np.ascontiguousarray(preds))
    want = DT.decode_events(p, win_off, frame_lens, n_frame, hop)
    got = DT.decode_events(p.to(_dev()), win_off, frame_lens, n_frame, hop)
    _same(got, want)
    return got


@pytest.mark.parametrize("n_files,seed", [(1, 0), (7, 1), (40, 2)])
@pytest.mark.parametrize("hop,n_out", [(512, 16), (256, 512), (128, 16)])
def test_kernel_ragged_batches(n_files, seed, hop, n_out):
    rng = np.random.default_rng(seed * 10 + hop)
    frame_lens = [int(x) for x in rng.integers(1, 6000, n_files)]
    if n_files > 1:
        frame_lens[1] = 0
        frame_lens[-1] = 1
    preds, win_off = run_preds(rng, frame_lens, 512, hop, n_out, noise=0.3, mean_run=60.0)
    ev = _kernel_vs_host(preds, win_off, frame_lens, 512, hop)
    assert sum(len(c) for f in ev for c in f) > 0


def test_kernel_long_file_with_others():
    """One file of 225,000 frames (an hour at hop 256) between short ones: tiles, halos and joined runs."""
    rng = np.random.default_rng(9)
    frame_lens = [3000, 225_000, 777, 14_400]
    preds, win_off = run_preds(rng, frame_lens, 512, 512, 16, noise=0.4, mean_run=300.0)
    preds[win_off[1]:win_off[2], :, 2] = 0.9        # one run across every tile of the long file
    ev = _kernel_vs_host(preds, win_off, frame_lens, 512, 512)
    assert ev[1][2].tolist() == [[0, 224_999]]
    assert len(ev[1][0]) > 20


def test_kernel_edge_cases():
    n_frame = 512
    preds = np.full((8, 16, 3), 0.1, np.float32)
    preds[0:3] = 0.9
    preds[6] = 0.9
    _kernel_vs_host(preds, np.array([0, 3, 6, 7, 8, 8]), [700, 700, 1, 1, 0], n_frame, 256)   # all on / off, 1 frame, empty
    nan = np.full((3, 512, 3), 0.9, np.float32)
    nan[1, 100, 1] = np.nan
    ev = _kernel_vs_host(nan, [0, 3], [1500], n_frame, 512)
    assert ev[0][1].tolist() == [[0, 534], [689, 1499]]
    sig = np.full((1024, 3), 0.1, np.float32)
    sig[:200, 0] = 0.9
    sig[700:, 1] = 0.9
    _kernel_vs_host(sig.reshape(2, 512, 3), [0, 2], [900], n_frame, 512)   # runs touching frame 0 and frame T - 1
    rng = np.random.default_rng(4)
    for hop in (128, 256, 512):
        for n_out in (16, 512):
            lens = [300, 1000, 2049, 64, 65, 127]     # T < n_frame; T not a multiple of 64 or of the hop
            preds, win_off = run_preds(rng, lens, n_frame, hop, n_out, noise=0.3)
            _kernel_vs_host(preds, win_off, lens, n_frame, hop)


def test_kernel_rejects():
    dev = _dev()
    with pytest.raises(ValueError):
        DT.decode_events(torch.zeros(2, 16, 3, device=dev), [0, 2], [1100], 512, 512)
    lay = DT.DecodeLayout([0, 2], [1100], 3)
    meta, bits, out = lay.buffers(dev)
    with pytest.raises(ValueError, match="no window covers"):   # the C ABI's own check
        DT.launch_decode(torch.zeros(2, 16, 3, device=dev), lay, meta, bits, out, 512, 512)


def _launch_setup(seed=5):
    dev = _dev()
    rng = np.random.default_rng(seed)
    frame_lens = [int(x) for x in rng.integers(1, 20000, 12)]
    preds, win_off = run_preds(rng, frame_lens, 512, 256, 16, noise=0.3)
    p = torch.from_numpy(preds).to(dev)
    lay = DT.DecodeLayout(win_off, frame_lens, 3)
    return p, lay, lay.buffers(dev), preds, win_off, frame_lens


def test_kernel_two_calls_bitwise_equal():
    p, lay, (meta, bits, out), preds, win_off, frame_lens = _launch_setup()
    out.fill_(-7)   # (slots past each n_ev are never written)
    DT.launch_decode(p, lay, meta, bits, out, 512, 256)
    first = out.clone()
    out.fill_(-7)
    DT.launch_decode(p, lay, meta, bits, out, 512, 256)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert torch.equal(first, out)
    _same(lay.parse(host), DT.decode_events(torch.from_numpy(preds), win_off, frame_lens, 512, 256))


def test_kernel_graph_replay_equals_eager():
    p, lay, (meta, bits, out), preds, win_off, frame_lens = _launch_setup(6)
    out.fill_(-7)   # (slots past each n_ev are never written)
    DT.launch_decode(p, lay, meta, bits, out, 512, 256)   # warm-up (eager)
    torch.cuda.synchronize()
    eager = out.clone()
    out.fill_(-7)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            DT.launch_decode(p, lay, meta, bits, out, 512, 256)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    p.mul_(0.0)   # the graph reads the live inputs: everything off now
    g.replay()
    torch.cuda.synchronize()
    assert all(len(c) == 0 for f in lay.parse(out.cpu().numpy()) for c in f)


# ---------------------------------------------------------------------------
# detect() against the existing chain
# ---------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    """Deterministic, batch-independent (one window at a time) stand-in: per output frame the mean feature over (mel,
    channel, the frame's 32 input frames); class c is 0.91 where it exceeds the window's mean + (c - 1) / 2 std, else 0.13.
    With no overlap (hop = n_frame) every smoothed value is 0.13 + 0.78 h / n with n <= 31, never within 3e-4 of 0.5."""

    def __init__(self, n_out=16):
        super().__init__()
        self.n_out = n_out
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        outs = []
        for i in range(x.shape[0]):
            e = x[i].mean(dim=(0, 2)).reshape(self.n_out, -1).mean(-1)
            mu, sd = e.mean(), e.std()
            outs.append(torch.stack([torch.where(e > mu + (c - 1) * 0.5 * sd, 0.91, 0.13) for c in range(3)], -1))
        return torch.stack(outs).to(torch.float32)


def _wavs(seconds, seed=0, chans=2):
    rng = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(seconds):
        n = int(16000 * s)
        wav = (rng.standard_normal((chans, n)) * 0.05).astype(np.float32)
        env = np.repeat(rng.random(n // 4000 + 1) < 0.4, 4000)[:n] * 7.0 + 1.0      # bursts of 0.25 s
        wav *= env[None, :].astype(np.float32)
        out.append((f"f{i}", wav))
    return out


def _chain_events(model, items, cfg, hop, dev):
    """inference.predict_frames -> get_start_end_frame per file, and the fp64 smoothed values of the same window outputs."""
    from challenge_amd import data_utils as D
    from challenge_amd import inference as I
    events, margin = [], np.inf
    for _, wav in items:
        feats = I.features_for_eval(D.load_wav_array(wav, 16000, dev), cfg)
        d = I.predict_frames(model, feats, cfg, hop)
        events.append(M.Challenge_Metric().get_start_end_frame(d.cpu().numpy()))
        win = I.frame(feats, cfg.n_frame, hop, pad_end=True, axis=-2).permute(1, 0, 2, 3)[..., :cfg.n_chan].contiguous()
        preds = DT._predict(model, win, 32).float().cpu().numpy()
        a, _ = ref_smoothed(preds, cfg.n_frame, hop, feats.shape[-2])
        margin = min(margin, float(np.abs(a - 0.5).min()))
    return events, margin


def _cfg(*extra):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_frame', '512', '--n_chan', '1', *extra])


def _v9_model(cfg, dev, seed=0):
    """v9 CustomModel whose head leaves the tie band: class 0 on, class 1 off, class 2 off (bias +-4, small weights)."""
    from challenge_amd import sj_train as S
    torch.manual_seed(seed)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last).eval()
    with torch.no_grad():
        model.head.fc.weight.mul_(0.05)
        model.head.fc.bias.copy_(torch.tensor([4.0, -4.0, -4.0]))
    return model


@pytest.mark.parametrize("hop", [512, 256])
def test_detect_stub_matches_chain(hop):
    dev = _dev()
    cfg = _cfg()
    model = StubModel().to(dev)
    items = _wavs([37.3, 4.1, 21.0, 60.2, 12.5], seed=hop)
    want, margin = _chain_events(model, items, cfg, hop, dev)
    assert margin > TIE, margin          # the precondition: no smoothed value within rounding of the threshold
    res = DT.detect(model, items, cfg, overlap_hop=hop, batch_size=7)
    assert [r.name for r in res] == [n for n, _ in items]
    _same([r.events for r in res], want)
    assert sum(len(c) for r in res for c in r.events) > 10
    for r in res:
        assert np.array_equal(r.metric, M.output_to_metric(256, 16000)(*r.events))


def test_detect_v9_engine_matches_chain():
    dev = _dev()
    cfg = _cfg()
    model = _v9_model(cfg, dev)
    items = _wavs([25.0, 9.7, 40.1], seed=11)
    want, margin = _chain_events(model, items, cfg, 512, dev)
    assert margin > TIE, margin
    res = DT.detect(model, items, cfg)
    _same([r.events for r in res], want)
    assert [len(r.events[0]) for r in res] == [1, 1, 1]


def test_detect_grouping_and_order():
    dev = _dev()
    cfg = _cfg()
    model = StubModel().to(dev)
    items = _wavs([30.0, 8.2, 51.7], seed=3)
    together = DT.detect(model, items, cfg)
    grouped = DT.detect(model, items, cfg, max_windows=4)        # 4, 1 and 7 windows: three groups
    alone = [DT.detect(model, [it], cfg)[0] for it in items]
    rev = DT.detect(model, items[::-1], cfg)[::-1]
    for res in (grouped, alone, rev):
        assert [r.name for r in res] == [r.name for r in together]
        _same([r.events for r in res], [r.events for r in together])


def _write_named_wavs(tmp_path, seconds, seed):
    from scipy.io import wavfile
    with open(os.path.join(ROOT, "tests", "golden", "sample_answer.json")) as f:
        sample = json.load(f)
    names = list(sample["task2_answer"])[:len(seconds)]
    for (_, wav), name in zip(_wavs(seconds, seed), names):
        wavfile.write(str(tmp_path / f"{name}.wav"), 16000, wav.T.copy())
    gt = {"task2_answer": {n: sample["task2_answer"][n] for n in names}}
    with open(tmp_path / "sample_answer.json", "w") as f:
        json.dump(gt, f)
    return names


def test_cli_writes_answer_and_scores(tmp_path):
    dev = _dev()
    cfg = _cfg()
    model = _v9_model(cfg, dev)
    torch.save(model.state_dict(), tmp_path / "run.pt")
    names = _write_named_wavs(tmp_path, [20.0, 33.3, 12.0], seed=8)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "challenge_amd.detect", "--name", "run", "--path", str(tmp_path), "--v", "9",
                        "--n_mels", "64", "--n_frame", "512", "--n_chan", "1", "--wav_dir", str(tmp_path),
                        "--out", str(tmp_path / "answer.json"), "--score", str(tmp_path / "sample_answer.json")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "answer.json") as f:
        ans = json.load(f)
    assert list(ans) == ["task2_answer"] and sorted(ans["task2_answer"]) == sorted(names)
    for rows in ans["task2_answer"].values():
        assert all(len(x) == 3 and all(isinstance(v, int) for v in x) for x in rows)
        assert rows == sorted(rows)
        assert [x[0] for x in rows] == [0]       # the head: class 0 on over the whole file, the others off
    er = {ln.split()[1]: float(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("ER ")}
    want = M.evaluate(cfg, model, wav_dir=str(tmp_path), answer_path=str(tmp_path / "sample_answer.json"))
    assert [er[n] for n in sorted(names)] == want
