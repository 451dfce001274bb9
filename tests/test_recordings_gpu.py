"""Training windows from labelled recordings on the GPU: `iris_crop_windows` and `iris_crop_draw` against their NumPy
restatement (tests/crop_ref.py) - they copy, count and draw integers, so every comparison is exact -, the draw's
distribution, the share of a `make_wave_dataset` batch cut from recordings, and `sj_train.main --recordings` end to end.

The corpus: four stereo recordings of 700 (shorter than a window), 960 (exactly one window), 4133 (no multiple of hop or 4)
and 1 sample at hop 64, n_frame 16 (L = 960): 1 + 1 + 50 + 1 = 53 window positions.  Events overlap across classes and
within a class, one ends past its file, one lies entirely in the zero-padded tail of the short recording."""
import csv
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from crop_ref import crop_draw_ref, crop_windows_ref, positions

pytestmark = pytest.mark.gpu

HOP, N_FRAME, K = 64, 16, 3
LENS = (700, 960, 4133, 1)
TABLES = [np.array([[0, 2, 6], [1, 4, 9], [0, 5, 8], [2, 12, 15], [1, 9, 40]], np.int32),   # (2, 12, 15): in the zero tail
          np.array([[2, 0, 16]], np.int32),
          np.array([[0, 3, 20], [0, 10, 30], [1, 15, 45], [2, 60, 80], [1, 64, 70], [2, 0, 1]], np.int32),
          np.array([[0, 0, 1], [0, 0, 3]], np.int32)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def waves():
    rng = np.random.default_rng(0)
    return [rng.standard_normal((2, n)).astype(np.float32) for n in LENS]


def _all_draws(hop, n_frame):
    n_pos, _ = positions(LENS, hop, n_frame)
    return np.array([(i, q) for i, n in enumerate(n_pos) for q in range(n)], np.int32)


def _sampler(dev, waves, n_frame=N_FRAME, **kw):
    from challenge_amd.recordings import RecordingSampler
    return RecordingSampler(waves, TABLES, n_frame, HOP, K, device=dev, **kw)


@pytest.mark.parametrize("chan", [2, 1])
def test_raw_abi_unaligned_rows_behind_nan(dev, waves, chan):
    """Rows at stride len + 1 from an odd float offset, every float that is not a sample NaN; hop 50, n_frame 5 (L = 200):
    the scalar path (and, where a row happens to start on 16 bytes, the wide one) and the `len` mask.  Every valid
    (recording, first frame) pair once."""
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    hop, n_frame = 50, 5
    waves = [w[:chan] for w in waves]
    draws = _all_draws(hop, n_frame)
    assert len(draws) == 11 + 16 + 79 + 1
    strides = [n + 1 for n in LENS]
    offsets = np.concatenate([[1], 1 + np.cumsum([chan * s for s in strides])])
    flat = np.full(int(offsets[-1]) + 8, np.nan, np.float32)
    for w, off, s in zip(waves, offsets, strides):
        for c in range(chan):
            flat[off + c * s:off + c * s + w.shape[1]] = w[c]
    assert np.isnan(flat).sum() == len(flat) - chan * sum(LENS)
    storage = torch.from_numpy(flat).to(dev)
    recs = np.zeros(len(LENS), FE.CROP_REC)
    recs["base"] = storage.data_ptr() + 4 * offsets[:-1]
    recs["row_stride"], recs["len"] = strides, LENS
    counts = [len(t) for t in TABLES]
    recs["ev_first"], recs["ev_count"] = np.concatenate([[0], np.cumsum(counts)[:-1]]), counts
    assert len({int(b) % 16 for b in recs["base"]}) > 1          # not all rows share an alignment; none is required
    recs_d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    events = torch.from_numpy(np.concatenate(TABLES)).to(dev)
    draws_d = torch.from_numpy(draws).to(dev)
    wav = torch.full((len(draws), chan, (n_frame - 1) * hop), 7.0, device=dev)
    y = torch.full((len(draws), n_frame, K), 7.0, device=dev)
    rc = N.lib().iris_crop_windows(recs_d.data_ptr(), len(LENS), events.data_ptr(), draws_d.data_ptr(), len(draws), chan, hop, n_frame,
                                   K, wav.data_ptr(), y.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, N.lib().iris_last_error()
    torch.cuda.synchronize()
    want_wav, want_y = crop_windows_ref(waves, TABLES, draws, hop, n_frame, K)
    assert torch.equal(wav.cpu(), torch.from_numpy(want_wav))
    assert torch.equal(y.cpu(), torch.from_numpy(want_y))
    assert float(want_y.max()) == 2.0 and (want_wav == 0).any()
    # the wrapper gives the same tensors; a draw that names no recording gives zeros
    wav2, y2 = FE.crop_windows(recs_d, events, draws_d, chan, hop, n_frame, K)
    assert torch.equal(wav2, wav) and torch.equal(y2, y)
    bad = torch.tensor([[4, 0], [-1, 0], [2, -1], [2, 3]], dtype=torch.int32, device=dev)
    wav3, y3 = FE.crop_windows(recs_d, events, bad, chan, hop, n_frame, K)
    assert not wav3[:3].any() and not y3[:3].any()
    assert torch.equal(wav3[3].cpu(), torch.from_numpy(crop_windows_ref(waves, TABLES, [[2, 3]], hop, n_frame, K)[0][0]))


@pytest.mark.parametrize("chan", [2, 1])
def test_sampler_aligned_path(dev, waves, chan):
    """Through `RecordingSampler`: rows on 256-byte boundaries, hop 64 - the 16-byte path - with the padding behind every row
    poisoned; all 53 windows, draws from the host and from a device tensor."""
    waves = [w[:chan] for w in waves]
    s = _sampler(dev, waves)
    assert s.n_windows == 53 and s.n_pos.tolist() == [1, 1, 50, 1] and s.channels == chan and len(s) == 4
    assert s.storage.data_ptr() % 256 == 0 and all(int(b) % 256 == 0 for b in s.recs["base"]) and all(s.recs["row_stride"] % 64 == 0)
    for r in s.recs:
        off = (int(r["base"]) - s.storage.data_ptr()) // 4
        for c in range(chan):
            s.storage[off + c * int(r["row_stride"]) + int(r["len"]):off + (c + 1) * int(r["row_stride"])] = float("nan")
    assert int(torch.isnan(s.storage).sum()) == chan * sum(int(r["row_stride"]) - int(r["len"]) for r in s.recs) > 0
    draws = _all_draws(HOP, N_FRAME)
    want_wav, want_y = crop_windows_ref(waves, TABLES, draws, HOP, N_FRAME, K)
    wav, y = s.sample(len(draws), draws)
    assert torch.equal(wav.cpu(), torch.from_numpy(want_wav)) and torch.equal(y.cpu(), torch.from_numpy(want_y))
    assert torch.equal(s.last_draws().cpu(), torch.from_numpy(draws))
    assert float(y[0, 13, 2]) == 1.0 and not wav[0, :, 700:].any()        # the event in the zero tail keeps its label
    assert y[52].sum(0).tolist() == [4.0, 0.0, 0.0] and float(y[52, 0, 0]) == 2.0   # the one-sample recording's two events
    perm = np.random.default_rng(1).permutation(len(draws))
    wav_p, y_p = s.sample(len(draws), torch.from_numpy(draws[perm]).to(dev))
    assert wav_p.data_ptr() == wav.data_ptr()                              # long-lived buffers, overwritten
    assert torch.equal(wav_p.cpu(), torch.from_numpy(want_wav[perm])) and torch.equal(y_p.cpu(), torch.from_numpy(want_y[perm]))
    with pytest.raises(ValueError, match="names no window"):
        s.sample(2, np.array([[0, 1], [2, 0]], np.int32))
    # the host generator: valid windows, the same for the same seed
    a, b = _sampler(dev, waves, seed=3), _sampler(dev, waves, seed=3)
    a.sample(64), b.sample(64)
    d = a.last_draws().cpu().numpy()
    assert np.array_equal(d, b.last_draws().cpu().numpy()) and np.all(d[:, 1] < a.n_pos[d[:, 0]]) and np.all(d >= 0)


def test_device_draw_is_the_restated_generator(dev, waves):
    s = _sampler(dev, waves)
    s.enable_device_draw(5)
    _, prefix = positions(LENS, HOP, N_FRAME)
    assert np.array_equal(s.prefix.cpu().numpy(), prefix)
    got = []
    for call in range(3):
        wav, y = s.sample(64)
        d = s.last_draws().cpu().numpy()
        assert np.array_equal(d, crop_draw_ref(5, call, 64, prefix)), call
        got.append(d)
    want_wav, want_y = crop_windows_ref(waves, TABLES, got[-1], HOP, N_FRAME, K)
    assert torch.equal(wav.cpu(), torch.from_numpy(want_wav)) and torch.equal(y.cpu(), torch.from_numpy(want_y))
    assert int(s._dd["state"].item()) == 3
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    same, other = _sampler(dev, waves), _sampler(dev, waves)
    same.enable_device_draw(5), other.enable_device_draw(6)
    for call in range(3):
        same.sample(64), other.sample(64)
        assert np.array_equal(same.last_draws().cpu().numpy(), got[call])
        assert not np.array_equal(other.last_draws().cpu().numpy(), got[call])
    # a key above 2^32 uses both key words
    big = _sampler(dev, waves)
    big.enable_device_draw((9 << 32) | 5)
    big.sample(64)
    assert np.array_equal(big.last_draws().cpu().numpy(), crop_draw_ref((9 << 32) | 5, 0, 64, prefix))


def test_device_draw_is_uniform_over_the_windows(dev):
    """21 calls of batch 1024 over the 53 positions: every one is drawn, and every count lies within 6 binomial standard
    deviations of n p (n = 21 * 1024 draws, p = 1 / 53; a deviation of 6 sigma has probability 2e-9 per position)."""
    from challenge_amd import frontend as FE
    _, prefix = positions(LENS, HOP, N_FRAME)
    prefix_d = torch.from_numpy(prefix).to(dev)
    state = torch.zeros(1, dtype=torch.int64, device=dev)
    calls, batch, total = 21, 1024, int(prefix[-1])
    counts = torch.zeros(total, dtype=torch.int64, device=dev)
    for _ in range(calls):
        d = FE.crop_draw(prefix_d, batch, seed=11, state=state).long()
        assert int(d[:, 0].min()) >= 0 and int(d[:, 0].max()) < len(LENS)
        counts += torch.bincount(prefix_d[d[:, 0]] + d[:, 1], minlength=total)
    counts = counts.cpu().numpy()
    n, p = calls * batch, 1.0 / total
    mean, sd = n * p, math.sqrt(n * p * (1.0 - p))
    print(f"window counts: min {counts.min()}, max {counts.max()}, mean {mean:.1f}, 6 sd {6 * sd:.1f}")
    assert total == 53 and counts.sum() == n and int(state.item()) == calls
    assert counts.min() > 0
    assert np.all(np.abs(counts - mean) <= 6 * sd), (counts.min(), counts.max(), mean, sd)


# The dataset cases run at n_frame 32, not 16: a TRAINING set draws SpecAugment time masks of up to 23 frames, which the
# existing draws (iris_augment_draw, transforms.mask_draw_batch) refuse on an axis shorter than 24 frames.  At hop 64 a window
# is then 1984 samples: the recordings of 700 and 960 samples are both shorter than it, 4133 has 34 positions.
DS_FRAME = 32


def _dataset_args(name="run_filter"):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--n_mels', '32', '--n_frame', str(DS_FRAME), '--n_chan', '2', '--batch_size', '4', '--max_voices', '4',
                         '--max_noises', '3', '--steps_per_epoch', '2', '--name', name])


def _expected(S, cfg, dev, seed, device_draw, wav, y):
    """What `make_wave_dataset` must yield for the batch `wav`, `y`: the features under the first bands of the same streams,
    the labels after `_label_tail`."""
    from challenge_amd import data_utils as D
    from challenge_amd import frontend as FE
    from challenge_amd.dataset import Dataset
    tokens = D.run_tokens(cfg)
    plan = FE.FrontendPlan(256, HOP, cfg.n_mels, 16000, 2, cfg.batch_size, (DS_FRAME - 1) * HOP, dev)
    tb, fb, gain = S.BatchDraws(tokens, True, dev, seed, device_draw, plan.n_bins)(cfg.batch_size, DS_FRAME, cfg.n_mels)
    assert tokens.filter and gain is None
    x = S.wave_features(plan, 'log', tokens.compression == 'minmax_log', wav.contiguous(), tb, fb, None, None, False)
    return next(iter(S._label_tail(Dataset.from_generator(lambda: iter([(x, y)])), cfg, compressed=True)))


@pytest.mark.parametrize("device_draw", [False, True])
def test_dataset_of_recordings_alone(dev, waves, device_draw, monkeypatch):
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    monkeypatch.setattr(Dataset, "prefetch", lambda self, buffer_size=-1: self)   # the batch read below is the sampler's latest
    cfg = _dataset_args()
    ds = S.make_wave_dataset(cfg, training=True, device=dev, seed=7, n_fft=256, hop=HOP, device_draw=device_draw,
                             recordings=(waves, TABLES), recordings_share=1.0)
    assert ds.mixer is None and ds.recordings.n_frame == DS_FRAME and ds.recordings.n_windows == 1 + 1 + 34 + 1
    it = iter(ds)
    for call in range(2):
        x, y = next(it)
        draws = ds.recordings.last_draws().cpu().numpy()
        if device_draw:
            assert np.array_equal(draws, crop_draw_ref(7, call, 4, positions(LENS, HOP, DS_FRAME)[1]))
        if call == 0:
            want_wav, want_y = crop_windows_ref(waves, TABLES, draws, HOP, DS_FRAME, K)
            want_x, want_y = _expected(S, cfg, dev, 7, device_draw, torch.from_numpy(want_wav).to(dev), torch.from_numpy(want_y).to(dev))
            assert x.shape == (4, 32, DS_FRAME, 2) and torch.isfinite(x).all()
            assert torch.equal(x, want_x) and torch.equal(y, want_y)
            first_y = y
            kept = y.clone()
    assert torch.equal(first_y, kept)          # the second batch did not overwrite what the first one handed out
    # a validation set is what it is without the recordings
    plain = S.make_wave_dataset(cfg, training=False, device=dev, seed=7, n_fft=256, hop=HOP, device_draw=device_draw)
    with_rec = S.make_wave_dataset(cfg, training=False, device=dev, seed=7, n_fft=256, hop=HOP, device_draw=device_draw,
                                   recordings=(waves, TABLES))
    assert with_rec.recordings is None and plain.recordings is None
    (xa, ya), (xb, yb) = next(iter(plain)), next(iter(with_rec))
    assert torch.equal(xa, xb) and torch.equal(ya, yb)


@pytest.mark.parametrize("device_draw", [False, True])
def test_dataset_half_recordings_half_mixer(dev, waves, device_draw, monkeypatch):
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    from challenge_amd.mixer import WaveMixer
    monkeypatch.setattr(Dataset, "prefetch", lambda self, buffer_size=-1: self)
    cfg = _dataset_args()
    sources = S.synthetic_wave_sources(2, 3, HOP, n_bg=3, n_voice=7, n_noise=4, seed=3)
    sampler = _sampler(dev, waves, n_frame=DS_FRAME, seed=9)
    if device_draw:
        sampler.enable_device_draw(9)
    ds = S.make_wave_dataset(cfg, training=True, sources=sources, device=dev, seed=7, n_fft=256, hop=HOP, device_draw=device_draw,
                             recordings=sampler, recordings_share=0.5)
    assert ds.recordings is sampler and ds.mixer is not None
    x, y = next(iter(ds))
    draws = sampler.last_draws().cpu().numpy()
    assert draws.shape == (2, 2)
    if device_draw:
        assert np.array_equal(draws, crop_draw_ref(9, 0, 2, positions(LENS, HOP, DS_FRAME)[1]))
    rec_wav, rec_y = crop_windows_ref(waves, TABLES, draws, HOP, DS_FRAME, K)
    backgrounds, voices, labels, noises = sources
    mixer = WaveMixer(backgrounds, voices, np.eye(3, dtype='float32')[np.asarray(labels)], noises, n_frame=DS_FRAME, n_fft=256, hop=HOP,
                      max_voices=cfg.max_voices, max_noises=cfg.max_noises, n_classes=3, device=dev, snr=cfg.snr, min_ratio=1, seed=7)
    if device_draw:
        mixer.enable_device_draw(7)
    syn_wav, syn_y = mixer.mix(2)
    wav = torch.cat([torch.from_numpy(rec_wav).to(dev), syn_wav])
    labels = torch.cat([torch.from_numpy(rec_y).to(dev), syn_y.sum(dim=-3)])
    want_x, want_y = _expected(S, cfg, dev, 7, device_draw, wav, labels)
    assert x.shape == (4, 32, DS_FRAME, 2)
    assert torch.equal(x[:2], want_x[:2]) and torch.equal(y[:2], want_y[:2])     # the reference crops
    assert torch.equal(x[2:], want_x[2:]) and torch.equal(y[2:], want_y[2:])     # the mixer's samples


def test_main_trains_on_recordings(dev, tmp_path, monkeypatch):
    """`sj_train.main --online_stft --synthetic --recordings DIR`: three stereo files (one at 8 kHz, one shorter than a
    window) with an answer file; the run finishes with a finite loss and both steps ran as the replayed graph where
    `graph_step_possible` says so.  (--v 9 and --n_mels 32 as the other end-to-end runs of the suite.)"""
    from scipy.io import wavfile
    from challenge_amd import sj_train as S
    rec = tmp_path / "rec"
    rec.mkdir()
    rng = np.random.default_rng(2)
    for name, sr, seconds in (("a", 16000, 2.0), ("b", 8000, 1.5), ("c", 16000, 0.5)):
        wavfile.write(str(rec / (name + ".wav")), sr, (rng.standard_normal((int(sr * seconds), 2)) * 2000).astype(np.int16))
    with open(rec / "answer.json", "w") as f:
        json.dump({"task2_answer": {"a": [[0, 0.2, 0.9], [1, 0.5, 1.4]], "b": [[2, 0.0, 3.0]], "c": [], "unused": [[0, 0, 1]]}}, f)
    monkeypatch.chdir(tmp_path)
    seen = {"replays": 0}
    inner_call, inner_fit = S.GraphedTrainStep.__call__, S.fit

    def counted(self, data):
        seen["replays"] += 1
        return inner_call(self, data)

    def fit(model, train_set, *args, **kwargs):
        seen["possible"] = S.graph_step_possible(model) and S.GRAPH_STEP
        seen["recordings"] = train_set.recordings
        return inner_fit(model, train_set, *args, **kwargs)
    monkeypatch.setattr(S.GraphedTrainStep, "__call__", counted)
    monkeypatch.setattr(S, "fit", fit)
    S.main(['--online_stft', '--synthetic', '--recordings', str(rec), '--epochs', '1', '--steps_per_epoch', '2', '--validation_steps', '1',
            '--batch_size', '8', '--n_frame', '64', '--v', '9', '--n_mels', '32', '--name', 'pyrec'])
    with open(tmp_path / 'pyrec_vad_v9_lr0.001_batch8_opt_adam_mel32_chan2_BCE_framelen64.csv') as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1 and math.isfinite(float(rows[0]['loss'])) and math.isfinite(float(rows[0]['val_loss']))
    sampler = seen["recordings"]
    assert len(sampler) == 3 and sampler.lens.tolist() == [32000, 24000, 8000] and sampler._dd is not None
    assert sampler.n_pos.tolist() == [(32000 - 63 * 256) // 256 + 1, (24000 - 63 * 256) // 256 + 1, 1]
    assert sampler.last_draws().shape == (4, 2) and int(sampler._dd["state"].item()) >= 2
    assert seen["replays"] == (2 if seen["possible"] else 0)
