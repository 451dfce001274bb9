"""GPU tests of the speed-perturbation augmentation (iris_speed_perturb and iris_mix_wave_frame_active_batch, csrc/k_speed.h):
parity with the float64 definition under the error rule of tests/test_speed_host.py, ragged batches, exact zeros and untouched
tails, bit reproducibility (repeat, second stream, graph replay), the batched frame activity, `WaveMixer.enable_speed` /
`respeed` against the oracle's waveform mixing, and the 'speed' run name.

Kernel's own worst ratio |out - ref| / (u S) on one MI355X over the cases of test_single_source_meets_the_rule: 1.859 (at
[2, 400000], rate 0.9) - beside the yardstick's 1.906 and K = 8 (profiles/speed/kernel_error_ratios.log).
The test prints every case."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import frontend_ref as R
from speed_ref import make_wave, rule_ratio, speed_len, speed_ref
from test_speed_host import K, RATES, random_rate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _perturb(dev, wav, rate):
    from challenge_amd import transforms as T
    return T.speed_perturb(torch.from_numpy(np.ascontiguousarray(wav)).to(dev), rate).cpu().numpy()


def _table(FE, dev, records):
    table = np.zeros(len(records), FE.SPEED_SRC)
    for i, rec in enumerate(records):
        table[i] = rec
    return table, torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)


def test_single_source_meets_the_rule(dev):
    sweep = RATES + [random_rate(0)]
    cases = [((2, 40000), sweep), ((1, 4096), sweep), ((2, 37), sweep), ((2, 1), sweep), ((3, 50), [77.0, 50.0, 49.5]),
             ((2, 400000), [0.9, 1.1, random_rate(1)]),          # one long recording over many tiles
             ((2, 30000), [5.0, 17.3]), ((5, 9000), [0.93, 3.1])]   # spans too long for the LDS buffer: the global-memory path
    worst, where = 0.0, None
    for n, (shape, rates) in enumerate(cases):
        w = make_wave(shape, 100 + n) if shape[1] > 1 else np.full(shape, 0.7, np.float32)
        for rate in rates:
            ref, s_abs = speed_ref(w, rate)
            out = _perturb(dev, w, rate)
            assert out.shape == ref.shape == (shape[0], math.ceil(shape[1] / rate)) and out.dtype == np.float32
            ratio = rule_ratio(out, ref, s_abs)
            print(f"k_speed_perturb {shape} rate {rate}: |out - ref| / (u S) <= {ratio:.3f} (K = {K})")
            if ratio > worst:
                worst, where = ratio, (shape, rate)
            assert ratio <= K, (shape, rate, ratio)
    assert math.ceil(50 / 77.0) == 1    # the rate larger than L gave a single sample
    print(f"k_speed_perturb: worst |out - ref| / (u S) = {worst:.3f} at {where}; K = {K}")


def test_ragged_batch_equals_single_calls(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(7)
    lengths = [int(t) for t in rng.permutation(np.arange(300, 300 + 24 * 173, 173))]
    rates = [float(r) for r in rng.uniform(0.5, 2.0, size=24)]
    rates[5], rates[9] = 1.0, 6.5
    waves = [torch.from_numpy(make_wave((2, t), 200 + i)).to(dev) for i, t in enumerate(lengths)]
    batch = FE.speed_perturb_batch(waves, rates)
    for w, r, b in zip(waves, rates, batch):
        single = FE.speed_perturb_batch([w], [r])[0]
        assert b.shape == (2, math.ceil(w.shape[1] / r)) and torch.equal(b, single)
    assert torch.equal(batch[5], waves[5]) and batch[5].data_ptr() != waves[5].data_ptr()   # rate 1: a bit-identical copy
    from challenge_amd import transforms as T   # a 1-D waveform goes through the same launch as [1, L]
    assert torch.equal(T.speed_perturb(waves[0][0], rates[0]), FE.speed_perturb_batch([waves[0][:1]], [rates[0]])[0][0])
    # no sources: status 0, nothing launched, nothing written
    dst = torch.full((2 * 400,), -7.0, device=dev)
    _, table_d = _table(FE, dev, [(waves[0].data_ptr(), dst.data_ptr(), lengths[0], 400, 1.0)])
    assert N.lib().iris_speed_perturb(table_d.data_ptr(), 0, 2, 400, None) == 0
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())


def test_zeros_silent_tails_the_floats_beyond_and_skipped_records(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    zero = torch.zeros((2, 777), device=dev)
    for rate in (0.9, 1.1):
        out = FE.speed_perturb_batch([zero], [rate])[0]
        assert out.shape[1] == math.ceil(777 / rate) and torch.count_nonzero(out) == 0
    length, silent_from = 3000, 2400
    w = make_wave((2, length), 3)
    assert not w[:, silent_from:].any() and w[:, :silent_from].all()
    wd = torch.from_numpy(w).to(dev)
    for rate in (0.5, 0.9, 0.93, 1.07, 1.1, 2.0):
        n = speed_len(length, rate)
        buf = torch.full((2 * n + 1000,), -7.0, device=dev)
        _, table_d = _table(FE, dev, [(wd.data_ptr(), buf.data_ptr(), length, n, rate)])
        assert N.lib().iris_speed_perturb(table_d.data_ptr(), 1, 2, n, None) == 0
        torch.cuda.synchronize()
        assert bool((buf[2 * n:] == -7.0).all())                       # the floats beyond C * n keep the sentinel
        got = buf[:2 * n].view(2, n).cpu().numpy()
        assert np.array_equal(got, _perturb(dev, w, rate))
        i0 = np.floor(np.arange(n, dtype=np.float64) * rate)
        h = math.ceil(6 / (0.99 * min(1.0, 1 / rate)))
        assert np.all(got[:, i0 - h >= silent_from] == 0) and (i0 - h >= silent_from).any()   # silence stays exactly silence
        assert np.all(np.abs(got[:, i0 + h + 1 < silent_from]).max(axis=0) > 0)
    # skipped records leave their destination untouched; their neighbours are written
    n = speed_len(length, 0.9)
    bufs = [torch.full((2 * n,), -7.0, device=dev) for _ in range(6)]
    recs = [(wd.data_ptr(), bufs[0].data_ptr(), 0, n, 0.9),            # len_in <= 0
            (wd.data_ptr(), bufs[1].data_ptr(), length, 0, 0.9),       # len_out <= 0
            (wd.data_ptr(), bufs[2].data_ptr(), length, n, 0.0),       # rate <= 0
            (wd.data_ptr(), bufs[3].data_ptr(), length, n, -1.1),
            (wd.data_ptr(), bufs[4].data_ptr(), length, n, 0.9),       # a good one
            (wd.data_ptr(), bufs[5].data_ptr(), length, n, 0.9)]       # len_out > max_out_len below
    _, table_d = _table(FE, dev, recs)
    assert N.lib().iris_speed_perturb(table_d.data_ptr(), 5, 2, n, None) == 0
    assert N.lib().iris_speed_perturb(table_d.data_ptr() + 5 * 32, 1, 2, n - 1, None) == 0
    torch.cuda.synchronize()
    for i in (0, 1, 2, 3, 5):
        assert bool((bufs[i] == -7.0).all()), i
    assert np.array_equal(bufs[4].view(2, n).cpu().numpy(), _perturb(dev, w, 0.9))


def test_repeat_second_stream_and_graph_replay_are_bitwise_equal(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    waves = [torch.from_numpy(make_wave((2, t), 300 + i)).to(dev) for i, t in enumerate((70000, 333, 15000))]
    rates = [0.9, 1.1, 0.93]
    a = FE.speed_perturb_batch(waves, rates)
    b = FE.speed_perturb_batch(waves, rates)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = FE.speed_perturb_batch(waves, rates)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # the launch alone (table uploaded beforehand) captured into a graph and replayed: a single-branch graph
    outs = [torch.zeros_like(x) for x in a]
    _, table_d = _table(FE, dev, [(w.data_ptr(), o.data_ptr(), w.shape[1], o.shape[1], r) for w, r, o in zip(waves, rates, outs)])
    max_out = max(int(o.shape[1]) for o in outs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        rc = N.lib().iris_speed_perturb(table_d.data_ptr(), 3, 2, max_out, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, outs))
    waves[0].copy_(waves[0].flip(1))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], FE.speed_perturb_batch([waves[0]], [rates[0]])[0]) and torch.equal(outs[2], a[2])


def _corpus(rng, chan=2, hop=64):
    def clip(n, silent_from=None):
        x = (rng.standard_normal((chan, n)) * 0.3).astype(np.float32)
        if silent_from is not None:
            x[:, silent_from:] = 0
        return x
    backgrounds = [clip(n) for n in (hop * 20 + 7, hop * 90, hop * 48 + 33)]
    voices = [clip(n, s) for n, s in ((hop * 30, hop * 20), (hop * 55 + 5, None), (hop * 41, hop * 5), (hop * 64, hop * 50),
                                      (hop * 25 + 60, None), (hop * 48, hop * 30), (hop * 36, None))]
    noises = [clip(n) for n in (hop * 18, hop * 90 + 9, hop * 40, hop * 52)]
    return backgrounds, voices, noises


def test_batched_frame_activity_equals_the_per_voice_entry_point(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    hop, n_fft = 64, 256
    _, voices, _ = _corpus(np.random.default_rng(17))
    rates = [0.9, 1.09, 1.0, 0.93, 1.07, 0.95, 1.1]
    out = FE.speed_perturb_batch([torch.from_numpy(v).to(dev) for v in voices], rates)
    frames = [1 + int(o.shape[1]) // hop for o in out]
    acts = [torch.full((f + 5,), -7.0, device=dev) for f in frames]
    _, table_d = _table(FE, dev, [(0, o.data_ptr(), 0, o.shape[1], 0.0) for o in out])   # only dst / len_out are read
    ptrs = torch.tensor([a.data_ptr() for a in acts], dtype=torch.int64, device=dev)
    N.check(N.lib().iris_mix_wave_frame_active_batch(table_d.data_ptr(), len(out), 2, n_fft, hop, ptrs.data_ptr(), max(frames), None),
            "iris_mix_wave_frame_active_batch")
    torch.cuda.synchronize()
    partial = 0
    for o, a, f in zip(out, acts, frames):
        single = torch.empty(f, device=dev)
        N.check(N.lib().iris_mix_wave_frame_active(o.data_ptr(), 2, int(o.shape[1]), n_fft, hop, single.data_ptr(), None), "active")
        torch.cuda.synchronize()
        assert torch.equal(a[:f], single) and bool((a[f:] == -7.0).all())
        assert np.array_equal(single.cpu().numpy(), R.wave_frame_active(o.cpu().numpy(), n_fft, hop))
        partial += int(0 < float(single.sum()) < f)
    assert partial >= 3                                        # the silent tails survived the perturbation
    # a record whose frame count exceeds max_frames is skipped
    acts2 = [torch.full((f,), -7.0, device=dev) for f in frames]
    ptrs2 = torch.tensor([a.data_ptr() for a in acts2], dtype=torch.int64, device=dev)
    small = sorted(frames)[2]
    assert N.lib().iris_mix_wave_frame_active_batch(table_d.data_ptr(), len(out), 2, n_fft, hop, ptrs2.data_ptr(), small, None) == 0
    torch.cuda.synchronize()
    for a, a2, f in zip(acts, acts2, frames):
        assert torch.equal(a2, a[:f]) if f <= small else bool((a2 == -7.0).all())


def _oracle_mix(draws, backgrounds, voices, labels, noises, n_frame, n_classes, hop, n_fft):
    return [R.mix_waves_apply(backgrounds[d["bg"]], [voices[k] for k in d["voices"]], labels[d["voices"]],
                              [noises[k] for k in d["noises"]], d, n_frame=n_frame, n_classes=n_classes, hop=hop, n_fft=n_fft,
                              min_ratio=1) for d in draws]


def test_wave_mixer_respeed(dev):
    from challenge_amd.mixer import WaveMixer
    rng = np.random.default_rng(11)
    hop, n_fft, n_frame, n_classes = 64, 256, 48, 3
    backgrounds, voices, noises = _corpus(rng)
    labels = np.eye(n_classes, dtype=np.float32)[rng.integers(0, n_classes, len(voices))]
    kw = dict(n_frame=n_frame, n_fft=n_fft, hop=hop, max_voices=4, max_noises=3, n_classes=n_classes, device=dev, min_ratio=1)
    L0 = np.array([v.shape[1] for v in voices])
    rates = np.array([0.9, 1.09, 1.0, 0.93, 1.07, 0.95, 1.1])

    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=5, **kw)
    mixer.enable_speed()
    assert np.array_equal(mixer._v_L, L0) and all(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(mixer.voices, voices))
    for v, act in zip(voices, mixer.voice_active):
        f = 1 + v.shape[1] // hop
        assert act.numel() == 1 + math.ceil(v.shape[1] / 0.9) // hop and np.array_equal(act[:f].cpu().numpy(), R.wave_frame_active(v, n_fft, hop))
    ptrs = (mixer._v_ptr.copy(), mixer._v_act.copy())
    used = mixer.respeed(rates)
    assert np.array_equal(used, rates)
    want_L = np.array([math.ceil(n / r) for n, r in zip(L0, rates)])
    assert np.array_equal(mixer._v_L, want_L) and np.array_equal(mixer._v_T, 1 + want_L // hop)
    assert [tuple(v.shape) for v in mixer.voices] == [(2, int(n)) for n in want_L]
    bank = [v.cpu().numpy() for v in mixer.voices]
    for v, s, r in zip(voices, bank, rates):   # what the buffers hold is the kernel's perturbation of the ORIGINAL voice
        assert np.array_equal(s, v if r == 1 else _perturb(dev, v, r))
    for s, act, n in zip(bank, mixer.voice_active, want_L):
        assert np.array_equal(act[:1 + int(n) // hop].cpu().numpy(), R.wave_frame_active(s, n_fft, hop))
    # mixing from the perturbed corpus == the oracle's mixing of the perturbed voices, bit for bit, labels included
    draws = mixer.draw(16)
    wav, lab = mixer.mix(16, draws)
    for i, (ref_wav, ref_lab) in enumerate(_oracle_mix(draws, backgrounds, bank, labels, noises, n_frame, n_classes, hop, n_fft)):
        assert np.array_equal(wav[i].cpu().numpy(), ref_wav) and np.array_equal(lab[i].cpu().numpy(), ref_lab), i
    assert float(lab.sum()) > 0
    # addresses never move: two more (random) calls
    r1, r2 = mixer.respeed().copy(), mixer.respeed().copy()
    assert np.all((r1 >= 0.9) & (r1 < 1.1)) and not np.array_equal(r1, r2)
    assert np.array_equal(mixer._v_ptr, ptrs[0]) and np.array_equal(mixer._v_act, ptrs[1])
    assert [v.data_ptr() for v in mixer.voices] == list(ptrs[0]) and [a.data_ptr() for a in mixer.voice_active] == list(ptrs[1])
    with pytest.raises(ValueError, match="voice 0"):
        mixer.respeed(np.full(7, 0.5))            # below lo: would not fit the buffers
    with pytest.raises(ValueError):
        mixer.respeed(np.ones(6))
    with pytest.raises(RuntimeError):
        mixer.enable_speed()
    with pytest.raises(RuntimeError):
        WaveMixer(backgrounds, voices, labels, noises, seed=5, **kw).respeed()

    # all rates 1 == a mixer on which enable_speed was never called, same seed
    plain = WaveMixer(backgrounds, voices, labels, noises, seed=21, **kw)
    ones = WaveMixer(backgrounds, voices, labels, noises, seed=21, **kw)
    ones.enable_speed()
    ones.respeed(np.ones(7))
    for _ in range(2):
        (wa, la), (wb, lb) = plain.mix(8), ones.mix(8)
        assert torch.equal(wa, wb) and torch.equal(la, lb)

    # with the draws on the device, in either call order: the T / len fields of the drawn records are the new ones
    for order in ("speed_first", "draw_first"):
        m = WaveMixer(backgrounds, voices, labels, noises, seed=5, **kw)
        if order == "speed_first":
            m.enable_speed()
            m.enable_device_draw(77)
        else:
            m.enable_device_draw(77)
            m.enable_speed()
        m.respeed(rates)
        va = m._dd["voice_arrays"]
        assert np.array_equal(va["len"].cpu().numpy(), want_L) and np.array_equal(va["T"].cpu().numpy(), 1 + want_L // hop)
        assert np.array_equal(va["src"].cpu().numpy().astype(np.uint64), m._v_ptr)
        assert np.array_equal(va["act"].cpu().numpy().astype(np.uint64), m._v_act)
        wav, lab = m.mix(16)
        table = m.last_table(16)
        dd = m.table_to_draws(table)
        bank = [v.cpu().numpy() for v in m.voices]
        for i, d in enumerate(dd):
            assert np.array_equal(table[i]["T"][1:5], (1 + want_L // hop)[d["voices"]]), (order, i)
            assert np.array_equal(table[i]["reserved"][1:5], want_L[d["voices"]]), (order, i)
            assert np.array_equal(table[i]["src"][1:5], m._v_ptr[d["voices"]]) and np.array_equal(table[i]["active"][1:5], m._v_act[d["voices"]])
        for i, (ref_wav, ref_lab) in enumerate(_oracle_mix(dd, backgrounds, bank, labels, noises, n_frame, n_classes, hop, n_fft)):
            assert np.array_equal(wav[i].cpu().numpy(), ref_wav) and np.array_equal(lab[i].cpu().numpy(), ref_lab), (order, i)

    # a captured mix replayed after a respeed reads the new contents through the unchanged addresses
    m.mix(16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        gw, gl = m.mix(16)
    for new_rates in (rates[::-1].copy(), None):
        m.respeed(new_rates)
        g.replay()
        torch.cuda.synchronize()
        dd = m.table_to_draws(m.last_table(16))
        bank = [v.cpu().numpy() for v in m.voices]
        for i, (ref_wav, ref_lab) in enumerate(_oracle_mix(dd, backgrounds, bank, labels, noises, n_frame, n_classes, hop, n_fft)):
            assert np.array_equal(gw[i].cpu().numpy(), ref_wav) and np.array_equal(gl[i].cpu().numpy(), ref_lab), i


def test_speed_run_name_in_make_wave_dataset(dev):
    from challenge_amd import sj_train as S
    args = ['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
            '--max_noises', '3', '--steps_per_epoch', '2']
    sources = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
    L0 = np.array([v.shape[1] for v in sources[1]])
    ds = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_speed']), training=True, sources=sources, device=dev, seed=4)
    first = ds.mixer._aug.rates.copy()
    assert not np.array_equal(ds.mixer._v_L, L0) and np.array_equal(ds.mixer._v_L, np.ceil(L0 / first).astype(np.int64))
    it = iter(ds)
    for _ in range(5):   # steps_per_epoch = 2 and a prefetch two batches deep: by the fifth batch a second respeed has run
        bx, by = next(it)
        assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3)
        assert torch.isfinite(bx).all() and float(by.min()) >= 0 and float(by.max()) <= 1
    assert not np.array_equal(ds.mixer._aug.rates, first)
    assert np.all(ds.mixer._v_L >= np.ceil(L0 / 1.1)) and np.all(ds.mixer._v_L <= np.ceil(L0 / 0.9))
    # validation sets are never perturbed; without the token the mixer has no speed state
    val = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_speed']), training=False, sources=sources, device=dev, seed=4)
    assert val.mixer._aug is None and np.array_equal(val.mixer._v_L, L0)
    plain = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run']), training=True, sources=sources, device=dev, seed=4)
    assert plain.mixer._aug is None and np.array_equal(plain.mixer._v_L, L0)
    bx, by = next(iter(plain))
    assert bx.shape == (6, 40, 64, 2) and torch.isfinite(bx).all()


def test_refusals(dev):
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    w = torch.from_numpy(make_wave((2, 200), 0)).to(dev)
    with pytest.raises(ValueError):
        FE.speed_perturb_batch([w], [0.0])
    with pytest.raises(ValueError):
        FE.speed_perturb_batch([w], [float("nan")])
    with pytest.raises(ValueError):
        FE.speed_perturb_batch([w, w[:1].contiguous()], [0.9, 0.9])
    with pytest.raises(ValueError):
        FE.speed_perturb_batch([w.view(-1)], [0.9])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.speed_perturb(w.cpu(), 0.9)
