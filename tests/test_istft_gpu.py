"""GPU tests of the inverse STFT (iris_istft, csrc/k_istft.h): the error rule of tests/test_istft_host.py on every element,
ragged batches against single calls, canaries and skipped records, bit reproducibility (repeat, second stream, graph replay),
the device round trip, `sj_train.waves_from_specs`, `make_wave_dataset(spec_sources=...)` and `--wave_corpus pickles`.

Every test prints its figures; the kernel's own worst ratios are recorded in DESIGN.md (section 4, K3i)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import istft_ref as I
from test_istft_host import K

pytestmark = pytest.mark.gpu

_PLANS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _plan(dev, n_fft, hop, chan):
    from challenge_amd.frontend import FrontendPlan
    key = (n_fft, hop, chan)
    if key not in _PLANS:
        _PLANS[key] = FrontendPlan(n_fft, hop, 32, 16000, chan, 4, 40000, dev)
    return _PLANS[key]


# (n_fft, hop, frames, channels, len_out or None)
RULE_CASES = [(256, 128, 2, 1, None), (256, 128, 3, 1, None), (256, 128, 9, 1, None),
              (512, 256, 130, 2, None),        # several tiles, halo frames on both sides
              (1024, 256, 20, 1, None),        # four frames per sample
              (512, 96, 40, 2, None),          # a hop that does not divide n_fft
              (512, 256, 130, 2, 4096 + 37),   # len_out shorter than the default, ending inside the second tile
              (256, 128, 9, 1, 1),
              (2048, 512, 9, 2, None),
              (256, 32, 70, 2, None)]          # eight frames per sample, several passes per tile


@pytest.mark.parametrize("n_fft,hop,frames,chan,length", RULE_CASES)
def test_every_element_meets_the_rule(dev, n_fft, hop, frames, chan, length):
    plan = _plan(dev, n_fft, hop, chan)
    for n, kind in enumerate(I.KINDS):
        spec = I.make_spec(kind, chan, frames, n_fft, hop, 50 + n)
        ref, s = I.istft_ref(spec, n_fft, hop, length)
        out = plan.istft(torch.from_numpy(spec).to(dev)[None], length)[0].cpu().numpy()
        assert out.shape == ref.shape == (chan, length or (frames - 1) * hop) and out.dtype == np.float32
        ratio = I.rule_ratio(out, ref, s)   # (asserts the exact zeros where S == 0)
        print(f"k_istft n_fft {n_fft} hop {hop} T {frames} C {chan} len {length} {kind}: |y - ref| / (u S) <= {ratio:.2f} (K = {K}); "
              f"{int((s == 0).sum())} samples with S == 0")
        assert np.isfinite(out).all() and ratio <= K, (kind, ratio)
    # two adjacent zero frames at hop = n_fft / 2 (or more at smaller hops) silence whole samples: they must be exactly 0
    spec = I.make_spec("random", chan, frames, n_fft, hop, 99)
    span = -(-n_fft // hop)
    if frames > span + 1:
        spec[:, 1:1 + span + 1] = 0
        ref, s = I.istft_ref(spec, n_fft, hop, length)
        out = plan.istft(torch.from_numpy(spec).to(dev)[None], length)[0].cpu().numpy()
        if length is None:
            assert (s == 0).any()
        assert I.rule_ratio(out, ref, s) <= K
    # a NaN stays inside the samples its frame covers
    if frames >= 9 and length is None:
        spec = I.make_spec("random", chan, frames, n_fft, hop, 98)
        t_nan = frames // 2
        spec[3, t_nan, 0] = np.nan
        out = plan.istft(torch.from_numpy(spec).to(dev)[None])[0].cpu().numpy()
        p = np.arange(out.shape[1]) + n_fft // 2
        covered = (p - t_nan * hop >= 0) & (p - t_nan * hop < n_fft)
        assert np.isfinite(out[:, ~covered]).all() and np.isfinite(out[1:]).all() and np.isnan(out[0, covered]).any()


def _table(FE, dev, records):
    table = np.zeros(len(records), FE.ISTFT_SRC)
    for i, rec in enumerate(records):
        table[i] = rec
    return table, torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)


def test_ragged_batch_equals_single_calls_and_leaves_the_rest_alone(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    n_fft, hop, chan = 512, 256, 2
    plan = _plan(dev, n_fft, hop, chan)
    frames = [2, 3, 9, 130, 57]
    specs = [torch.from_numpy(I.make_spec(I.KINDS[i % 3], chan, t, n_fft, hop, 300 + i)).to(dev) for i, t in enumerate(frames)]
    batch = FE.istft_batch(plan, specs)
    singles = [FE.istft_batch(plan, [s])[0] for s in specs]
    for t, b, one, s in zip(frames, batch, singles, specs):
        assert b.shape == (chan, (t - 1) * hop) and torch.equal(b, one)
        assert torch.equal(b, plan.istft(s[None])[0])                  # the rectangular surface is the same launch
        ref, sc = I.istft_ref(s.cpu().numpy(), n_fft, hop)
        assert I.rule_ratio(b.cpu().numpy(), ref, sc) <= K
    # a canary behind each dst; skipped records leave their dst untouched; their neighbours are written
    lens = [(t - 1) * hop for t in frames]
    bufs = [torch.full((chan * n + 500,), -7.0, device=dev) for n in lens]
    skipped = [torch.full((chan * 2048,), -7.0, device=dev) for _ in range(5)]
    one_frame = specs[2][:, :1].contiguous()
    recs = [(s.data_ptr(), b.data_ptr(), t, n) for s, b, t, n in zip(specs, bufs, frames, lens)]
    recs += [(one_frame.data_ptr(), skipped[0].data_ptr(), 1, 256),          # n_frames < 2
             (specs[2].data_ptr(), skipped[1].data_ptr(), 9, 8 * hop + 1),    # len_out > (T - 1) hop
             (specs[2].data_ptr(), skipped[2].data_ptr(), 9, 0),              # len_out <= 0
             (0, skipped[3].data_ptr(), 9, 8 * hop),                          # NULL src
             (specs[3].data_ptr(), skipped[4].data_ptr(), 131, 1024)]         # n_frames > max_frames
    _, table_d = _table(FE, dev, recs)
    N.check(N.lib().iris_istft(plan._handle, table_d.data_ptr(), len(recs), 130, None), "iris_istft")
    torch.cuda.synchronize()
    for b, n, one in zip(bufs, lens, singles):
        assert torch.equal(b[:chan * n].view(chan, n), one) and bool((b[chan * n:] == -7.0).all())
    for i, b in enumerate(skipped):
        assert bool((b == -7.0).all()), i
    # max_frames below a record's frame count skips that record alone
    bufs2 = [torch.full((chan * n,), -7.0, device=dev) for n in lens]
    _, table_d = _table(FE, dev, [(s.data_ptr(), b.data_ptr(), t, n) for s, b, t, n in zip(specs, bufs2, frames, lens)])
    N.check(N.lib().iris_istft(plan._handle, table_d.data_ptr(), 5, 57, None), "iris_istft")
    torch.cuda.synchronize()
    for i, (b, n, one) in enumerate(zip(bufs2, lens, singles)):
        assert bool((b == -7.0).all()) if frames[i] > 57 else torch.equal(b.view(chan, n), one)
    # no sources: status 0, nothing launched
    assert N.lib().iris_istft(plan._handle, None, 0, 130, None) == 0


def test_argument_checks_with_a_plan(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    lib, p8 = N.lib(), C.c_void_p(8)
    plan = _plan(dev, 512, 256, 2)
    assert lib.iris_istft(plan._handle, p8, -1, 10, None) == -1
    assert lib.iris_istft(plan._handle, None, 1, 10, None) == -1
    assert lib.iris_istft(plan._handle, p8, 1, 1, None) == -1
    assert lib.iris_istft(plan._handle, p8, 70000, 10, None) == -2
    wide = FE.FrontendPlan(512, 384, 32, 16000, 2, 1, 4000, dev)          # hop > n_fft / 2
    assert lib.iris_istft(wide._handle, p8, 1, 10, None) == -2 and b"hop" in lib.iris_last_error()
    mel = FE.FrontendPlan.mel_only(8, 257, 2, 1, dev, np.ones((257, 8), np.float32))
    assert lib.iris_istft(mel._handle, p8, 1, 10, None) == -2
    with pytest.raises(ValueError):
        plan.istft(torch.zeros(1, 257, 9, 4, device=dev), 8 * 256 + 1)
    with pytest.raises(ValueError):
        plan.istft(torch.zeros(1, 257, 1, 4, device=dev))
    with pytest.raises(ValueError):
        FE.istft_batch(plan, [torch.zeros(129, 9, 4, device=dev)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plan.istft(torch.zeros(1, 257, 9, 4))


def test_repeat_second_stream_and_graph_replay_are_bitwise_equal(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    n_fft, hop, chan = 1024, 256, 1
    plan = _plan(dev, n_fft, hop, chan)
    frames = (40, 3, 21)
    specs = [torch.from_numpy(I.make_spec("noise", chan, t, n_fft, hop, 400 + i)).to(dev) for i, t in enumerate(frames)]
    a = FE.istft_batch(plan, specs)
    b = FE.istft_batch(plan, specs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = FE.istft_batch(plan, specs)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # the launch alone (table uploaded beforehand) captured into a graph and replayed: a single-branch graph
    outs = [torch.zeros_like(x) for x in a]
    _, table_d = _table(FE, dev, [(s.data_ptr(), o.data_ptr(), s.shape[1], o.shape[1]) for s, o in zip(specs, outs)])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        rc = N.lib().iris_istft(plan._handle, table_d.data_ptr(), 3, max(frames), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, outs))
    specs[0].copy_(specs[0].flip(1))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], FE.istft_batch(plan, [specs[0]])[0]) and torch.equal(outs[2], a[2])


def test_round_trip_on_the_device(dev):
    rng = np.random.default_rng(5)
    for n_fft, hop, chan, length in [(512, 256, 2, 20 * 256), (1024, 256, 1, 37 * 256), (256, 128, 1, 30 * 128)]:
        plan = _plan(dev, n_fft, hop, chan)
        x = (rng.standard_normal((3, chan, length)) * 0.3).astype(np.float32)
        y = plan.istft(plan.stft(torch.from_numpy(x).to(dev))).cpu().numpy()
        assert y.shape == x.shape and np.isfinite(y).all()
        xt = torch.from_numpy(x.reshape(-1, length))
        w = torch.from_numpy(I.hann(n_fft))
        z = torch.stft(xt, n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
        cpu = torch.istft(z, n_fft, hop_length=hop, window=w, center=True).numpy().reshape(x.shape)
        peak = np.abs(x).max()
        got, yard = np.abs(y - x).max() / peak, np.abs(cpu - x).max() / peak
        print(f"round trip n_fft {n_fft} hop {hop}: device {got:.3e} of max|x|, torch float32 on the CPU {yard:.3e} (bound 4 x)")
        assert got <= 4 * yard


def _spec_corpus(S, hop=256, n_fft=512):
    """Spectra made by the float64 oracle from `synthetic_wave_sources` waveforms, rounded to float32."""
    backgrounds, voices, labels, noises = S.synthetic_wave_sources(2, 3, hop, n_bg=2, n_voice=4, n_noise=3, seed=9)
    conv = lambda ws: [I.to_layout(I.stft64(w[:, :40 * hop + 13 * i], n_fft, hop)).astype(np.float32)   # noqa: E731
                       for i, w in enumerate(ws)]
    return conv(backgrounds), conv(voices), labels, conv(noises)


def test_waves_from_specs(dev):
    from challenge_amd import sj_train as S
    n_fft, hop = 512, 256
    sources = _spec_corpus(S, hop, n_fft)
    waves = S.waves_from_specs(sources, n_fft, hop, dev)
    assert waves[2] is sources[2]
    worst = 0.0
    for specs, ws in zip((sources[0], sources[1], sources[3]), (waves[0], waves[1], waves[3])):
        assert len(specs) == len(ws)
        for spec, w in zip(specs, ws):
            assert tuple(w.shape) == (2, (spec.shape[1] - 1) * hop) and w.dtype == torch.float32 and w.device == dev
            ref, s = I.istft_ref(spec, n_fft, hop)
            worst = max(worst, I.rule_ratio(w.cpu().numpy(), ref, s))
    print(f"waves_from_specs: worst |y - ref| / (u S) = {worst:.2f} (K = {K})")
    assert worst <= K
    with pytest.raises(ValueError, match="n_fft / 2 \\+ 1"):
        S.waves_from_specs(sources, 1024, 256, dev)


def test_make_wave_dataset_from_spec_sources(dev):
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
                        '--max_noises', '3', '--name', 'run'])
    sources = _spec_corpus(S)
    ds = S.make_wave_dataset(cfg, training=True, spec_sources=sources, device=dev, seed=4)
    assert [tuple(v.shape) for v in ds.mixer.voices] == [(2, (s.shape[1] - 1) * 256) for s in sources[1]]
    bx, by = next(iter(ds))
    assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3) and torch.isfinite(bx).all()


def test_sj_train_main_from_pickled_spectra(dev, tmp_path, monkeypatch):
    import csv
    from challenge_amd import sj_train as S
    monkeypatch.chdir(tmp_path)
    S.main(['--online_stft', '--wave_corpus', 'pickles', '--synthetic', '--epochs', '1', '--steps_per_epoch', '2',
            '--validation_steps', '1', '--batch_size', '8', '--n_frame', '128', '--v', '9', '--n_mels', '32', '--name', 'pyistft'])
    with open(tmp_path / 'pyistft_vad_v9_lr0.001_batch8_opt_adam_mel32_chan2_BCE_framelen128.csv') as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1 and math.isfinite(float(rows[0]['loss'])) and math.isfinite(float(rows[0]['val_loss']))
