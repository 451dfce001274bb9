"""GPU tests of the reverberation augmentation (iris_fir_batch, csrc/k_fir.h): parity with the float64 definition under the
rule |y - ref| <= (K + 2) u S of tests/reverb_ref.py on one ragged table, exact copies and zeros, bit reproducibility, untouched
tails, skipped records and refusals, unaligned rows, `WaveMixer.enable_reverb` / `rereverb` and the 'reverb' run name.

The accuracy test prints the ratio of every record and the worst one, which belongs in DESIGN.md (K2r); it is not entered
there yet: these tests had not run on an MI355X when they were written."""
import itertools

import numpy as np
import pytest
import torch

from reverb_ref import fir_ref, rule_ratio
from test_speed_gpu import _corpus

pytestmark = pytest.mark.gpu

LENGTHS = (1, 5, 255, 256, 257, 2049, 4100)
TAPS = (1, 2, 3, 63, 64, 65, 257, 4096)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test collected without a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ragged():
    """The ragged table of the accuracy test, every length crossed with every tap count (K > L and K < L both occur): inputs
    and NON-decaying taps ~ N(0, 1), one record scaled by 1e-4 and one by 1e3, and the float64 reference, computed once."""
    rng = np.random.default_rng(2017)
    cases = list(itertools.product(LENGTHS, TAPS))
    waves = [rng.standard_normal((2, n)).astype(np.float32) for n, _ in cases]
    taps = [rng.standard_normal((2, k)).astype(np.float32) for _, k in cases]
    small, large = cases.index((2049, 257)), cases.index((4100, 4096))
    waves[small] *= np.float32(1e-4)
    waves[large] *= np.float32(1e3)
    refs = [fir_ref(x, h) for x, h in zip(waves, taps)]
    return cases, waves, taps, refs


def _to(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def test_ragged_table_meets_the_rule(dev, ragged):
    from challenge_amd import frontend as FE
    cases, waves, taps, refs = ragged
    outs = FE.fir_batch(_to(dev, waves), _to(dev, taps))
    worst, where = 0.0, None
    for (n, k), out, (ref, s_abs) in zip(cases, outs, refs):
        assert out.shape == (2, n) and out.dtype == torch.float32
        ratio = rule_ratio(out.cpu().numpy(), ref, s_abs, k)
        print(f"k_fir_batch L = {n}, K = {k}: |y - ref| / ((K + 2) u S) <= {ratio:.4f}")
        if ratio > worst:
            worst, where = ratio, (n, k)
        assert ratio <= 1.0, (n, k, ratio)
    print(f"k_fir_batch: worst |y - ref| / ((K + 2) u S) = {worst:.4f} at (L, K) = {where}")


def test_a_record_alone_equals_the_record_in_the_table_and_repeats_bitwise(dev, ragged):
    from challenge_amd import frontend as FE
    cases, waves, taps, _ = ragged
    w, h = _to(dev, waves), _to(dev, taps)
    a, b = FE.fir_batch(w, h), FE.fir_batch(w, h)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in (cases.index((1, 4096)), cases.index((257, 65)), cases.index((2049, 3)), cases.index((4100, 4096))):
        assert torch.equal(FE.fir_batch([w[i]], [h[i]])[0], a[i]), cases[i]


def test_identity_taps_copy_and_zero_support_gives_zero(dev):
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 4100)).astype(np.float32)
    x[0, 17], x[1, 2048] = -0.0, 0.0
    xd = torch.from_numpy(x).to(dev)
    y = T.reverb(xd, np.ones((2, 1), np.float32))
    assert torch.equal(y.view(torch.int32), xd.view(torch.int32))             # bit for bit, the sign of a zero included
    assert torch.equal(T.reverb(xd[0].contiguous(), np.ones(1, np.float32)), xd[0])   # the [samples] form
    # a zero prefix longer than K: every output whose whole support is zero input is exactly 0
    k, prefix = 65, 300
    z = x.copy()
    z[:, :prefix] = 0
    h = rng.standard_normal((2, k)).astype(np.float32)
    out = FE.fir_batch(_to(dev, [z, np.zeros((2, 2049), np.float32)]), _to(dev, [h, rng.standard_normal((2, 4096)).astype(np.float32)]))
    assert bool((out[0][:, :prefix] == 0).all()) and bool((out[0][:, prefix:prefix + 50] != 0).all())
    assert bool((out[1] == 0).all())
    assert rule_ratio(out[0].cpu().numpy(), *fir_ref(z, h), k) <= 1.0


def _table(FE, dev, records):
    table = np.zeros(len(records), FE.FIR_SRC)
    for i, rec in enumerate(records):
        table[i] = rec
    return table


def test_tails_skipped_records_and_refusals(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(4)
    n, k, chan = 2049, 65, 2
    x, h = rng.standard_normal((chan, n)).astype(np.float32), rng.standard_normal((chan, k)).astype(np.float32)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    want = FE.fir_batch([xd], [hd])[0]
    fresh = lambda: torch.full((chan * n + 64,), SENTINEL, device=dev)  # noqa: E731
    good = fresh()
    bad = {"src NULL": (0, None, hd.data_ptr(), n, k), "taps NULL": (xd.data_ptr(), None, 0, n, k),
           "len 0": (xd.data_ptr(), None, hd.data_ptr(), 0, k), "len < 0": (xd.data_ptr(), None, hd.data_ptr(), -3, k),
           "n_taps 0": (xd.data_ptr(), None, hd.data_ptr(), n, 0), "n_taps < 0": (xd.data_ptr(), None, hd.data_ptr(), n, -1),
           "len > max_len": (xd.data_ptr(), None, hd.data_ptr(), n, k), "n_taps > max_taps": (xd.data_ptr(), None, hd.data_ptr(), n, k)}
    dsts = {name: fresh() for name in bad}
    records = [(xd.data_ptr(), good.data_ptr(), hd.data_ptr(), n, k), (xd.data_ptr(), 0, hd.data_ptr(), n, k)]   # (a NULL dst)
    records += [(r[0], dsts[name].data_ptr(), r[2], r[3], r[4]) for name, r in bad.items() if "max" not in name]
    FE.fir_launch(_table(FE, dev, records), chan, n, k, dev)
    # the two records that are malformed only against the launch's own maxima
    FE.fir_launch(_table(FE, dev, [(xd.data_ptr(), dsts["len > max_len"].data_ptr(), hd.data_ptr(), n, k)]), chan, n - 1, k, dev)
    FE.fir_launch(_table(FE, dev, [(xd.data_ptr(), dsts["n_taps > max_taps"].data_ptr(), hd.data_ptr(), n, k)]), chan, n, k - 1, dev)
    torch.cuda.synchronize()
    assert torch.equal(good[:chan * n].view(chan, n), want) and bool((good[chan * n:] == SENTINEL).all())   # the floats beyond: untouched
    for name, d in dsts.items():
        assert bool((d == SENTINEL).all()), name
    # the entry point's own refusals, and the empty table
    lib, t8 = N.lib(), xd.data_ptr()
    for args, code in (((None, 1, 2, 100, 16), -1), ((t8, -1, 2, 100, 16), -1), ((t8, 1, 0, 100, 16), -1), ((t8, 1, 2, 0, 16), -1),
                       ((t8, 1, 2, -1, 16), -1), ((t8, 1, 2, 100, 0), -1), ((t8, 1, 2, 100, -1), -1), ((t8, 65536, 2, 100, 16), -2)):
        assert lib.iris_fir_batch(*args, None) == code, args
        assert lib.iris_last_error().startswith(b"iris_fir_batch:")
    assert lib.iris_fir_batch(None, 0, 2, 100, 16, None) == 0 and FE.fir_batch([], []) == []
    torch.cuda.synchronize()
    # the Python surface
    for waves, taps in (([xd], [hd[:1].contiguous()]),                        # channel counts differ
                        ([xd, xd[:1].contiguous()], [hd, hd]),
                        ([xd], [hd[:, :0].contiguous()]),                     # an empty tap vector
                        ([xd], [torch.zeros((chan, 4097), device=dev)]),      # K > 4096
                        ([xd.cpu()], [hd]), ([xd], [hd.cpu()]),               # CPU tensors: no fallback
                        ([xd.view(-1)], [hd]), ([xd.double()], [hd]), ([xd, xd], [hd])):
        with pytest.raises(ValueError, match="fir_batch"):
            FE.fir_batch(waves, taps)
    from challenge_amd import transforms as T
    with pytest.raises(ValueError, match="no CPU fallback"):
        T.reverb(xd.cpu(), h)


def test_rows_off_16_bytes_meet_the_rule(dev):
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(5)
    chan, n, k = 2, 2051, 257                                    # len % 4 == 3: the second channel's rows shift again
    x, h = rng.standard_normal((chan, n)).astype(np.float32), rng.standard_normal((chan, k)).astype(np.float32)
    src, taps = torch.zeros(chan * n + 8, device=dev), torch.zeros(chan * k + 8, device=dev)
    dst = torch.full((chan * n + 8,), SENTINEL, device=dev)
    src[1:1 + chan * n].copy_(torch.from_numpy(x).view(-1))
    taps[1:1 + chan * k].copy_(torch.from_numpy(h).view(-1))
    for t in (src, dst, taps):
        assert t.data_ptr() % 16 == 0
    FE.fir_launch(_table(FE, dev, [(src.data_ptr() + 4, dst.data_ptr() + 4, taps.data_ptr() + 4, n, k)]), chan, n, k, dev)
    torch.cuda.synchronize()
    out = dst[1:1 + chan * n].view(chan, n)
    ratio = rule_ratio(out.cpu().numpy(), *fir_ref(x, h), k)
    print(f"k_fir_batch off 16 bytes, L = {n}, K = {k}: |y - ref| / ((K + 2) u S) <= {ratio:.4f}")
    assert ratio <= 1.0
    assert float(dst[0]) == SENTINEL and bool((dst[1 + chan * n:] == SENTINEL).all())
    # the same numbers through aligned rows: bit for bit
    assert torch.equal(out, FE.fir_batch(_to(dev, [x]), _to(dev, [h]))[0])


KW = dict(n_frame=48, n_fft=256, hop=64, max_voices=4, max_noises=3, n_classes=3, min_ratio=1)


def _sources(n_voice=6):
    rng = np.random.default_rng(11)
    backgrounds, voices, noises = _corpus(rng)
    voices = voices[:n_voice]
    labels = np.eye(3, dtype=np.float32)[rng.integers(0, 3, len(voices))]
    return backgrounds, voices, labels, noises


def _rirs(seed, n_voice=6):
    from challenge_amd.transforms import synth_rir
    rng = np.random.default_rng(seed)
    rirs = [synth_rir(rng, 2, rt60, drr) for rt60, drr in zip((0.02, 0.05, 0.1, 0.2, 0.3, 0.01), (-3.0, 0.0, 3.0, 6.0, 12.0, 9.0))]
    return rirs[:n_voice]


def test_wave_mixer_rereverb(dev):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()
    plain = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    assert mixer._aug is None
    acts = [a.clone() for a in mixer.voice_active]
    act_ptr, L0, T0 = mixer._v_act.copy(), mixer._v_L.copy(), mixer._v_T.copy()
    mixer.enable_reverb()
    # the identity response: the copies are the originals bit for bit, and so is a mix with the same draws
    assert all(torch.equal(a.view(torch.int32), torch.from_numpy(b).to(dev).view(torch.int32)) for a, b in zip(mixer.voices, voices))
    assert [v.data_ptr() for v in mixer.voices] == list(mixer._v_ptr) and mixer._v_ptr[0] != plain._v_ptr[0]
    draws = plain.draw(16)
    (wa, la), (wb, lb) = plain.mix(16, draws), mixer.mix(16, draws)
    assert torch.equal(wa, wb) and torch.equal(la, lb) and float(la.sum()) > 0
    # fresh responses: every voice is the kernel's convolution of the ORIGINAL voice
    ptrs = mixer._v_ptr.copy()
    rirs = _rirs(1)
    assert any(h.shape[1] > n for h, n in zip(rirs, L0)) and any(h.shape[1] < n for h, n in zip(rirs, L0))   # K > L and K < L
    for given in (_rirs(2), rirs):      # the second call starts from the originals again, not from the first call's result
        used = mixer.rereverb(given)
        assert all(np.array_equal(a, b) for a, b in zip(used, given))
    for i, (v, h, out) in enumerate(zip(voices, rirs, mixer.voices)):
        assert out.shape == v.shape
        ratio = rule_ratio(out.cpu().numpy(), *fir_ref(v, h), h.shape[1])
        print(f"rereverb voice {i}: L = {v.shape[1]}, K = {h.shape[1]}, |y - ref| / ((K + 2) u S) <= {ratio:.4f}")
        assert ratio <= 1.0, i
    # lengths, frame counts and the activity vectors (the labels) stay those of the dry voices; addresses never move
    assert np.array_equal(mixer._v_L, L0) and np.array_equal(mixer._v_T, T0) and np.array_equal(mixer._v_act, act_ptr)
    assert all(torch.equal(a, b) for a, b in zip(mixer.voice_active, acts)) and np.array_equal(mixer._v_ptr, ptrs)
    wc, lc = mixer.mix(16, draws)
    assert torch.equal(lc, la) and not torch.equal(wc, wa) and bool(torch.isfinite(wc).all())
    # random responses from the mixer's generator
    r1, r2 = mixer.rereverb(), mixer.rereverb()
    assert len(r1) == 6 and all(h.shape[0] == 2 and 1067 <= h.shape[1] <= 4096 for h in r1)      # rt60 in [0.1, 0.4)
    assert not all(np.array_equal(a, b) for a, b in zip(r1, r2)) and np.array_equal(mixer._v_ptr, ptrs)
    with pytest.raises(ValueError):
        mixer.rereverb(rirs[:5])
    with pytest.raises(ValueError):
        mixer.rereverb([h[:1] for h in rirs])
    with pytest.raises(ValueError):
        mixer.rereverb([np.zeros((2, 4097), np.float32)] * 6)
    # one voice augmentation per mixer
    with pytest.raises(RuntimeError, match="already called"):
        mixer.enable_reverb()
    with pytest.raises(RuntimeError, match="already called"):
        mixer.enable_speed()
    with pytest.raises(RuntimeError, match="enable_speed"):
        mixer.respeed()
    with pytest.raises(RuntimeError, match="enable_reverb"):
        plain.rereverb()
    plain.enable_speed()
    with pytest.raises(RuntimeError, match="already called"):
        plain.enable_reverb()
    with pytest.raises(RuntimeError, match="enable_reverb"):
        plain.rereverb()


@pytest.mark.parametrize("order", ["reverb_first", "draw_first"])
def test_captured_mix_replayed_after_rereverb_equals_the_eager_mix(dev, order):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()

    def make():
        m = WaveMixer(backgrounds, voices, labels, noises, seed=5, device=dev, **KW)
        if order == "reverb_first":
            m.enable_reverb()
            m.enable_device_draw(77)
        else:
            m.enable_device_draw(77)
            m.enable_reverb()
        assert np.array_equal(m._dd["voice_arrays"]["src"].cpu().numpy().astype(np.uint64), m._v_ptr)
        assert np.array_equal(m._dd["voice_arrays"]["act"].cpu().numpy().astype(np.uint64), m._v_act)
        m.rereverb(_rirs(1))
        m.mix(16)          # (warm-up: both mixers' device draw states move once)
        torch.cuda.synchronize()
        return m

    captured, eager = make(), make()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        gw, gl = captured.mix(16)
    for seed in (2, 3):     # replayed after a second (and third) rereverb: the new contents through unchanged addresses
        captured.rereverb(_rirs(seed))
        g.replay()
        eager.rereverb(_rirs(seed))
        ew, el = eager.mix(16)
        torch.cuda.synchronize()
        tc, te = captured.last_table(16), eager.last_table(16)      # the same draws (the buffers' addresses differ)
        assert all(np.array_equal(tc[f], te[f]) for f in ("T", "pad", "off", "gain", "kind", "slot", "label_row", "reserved"))
        assert torch.equal(gw, ew) and torch.equal(gl, el) and float(el.sum()) > 0


def test_reverb_run_name_in_make_wave_dataset(dev):
    from challenge_amd import sj_train as S
    args = ['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
            '--max_noises', '3', '--steps_per_epoch', '2']
    sources = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
    L0 = np.array([v.shape[1] for v in sources[1]])
    ds = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb']), training=True, sources=sources, device=dev, seed=4)
    first_rirs = ds.mixer._aug.rirs
    first = [v.clone() for v in ds.mixer.voices]
    assert len(first_rirs) == 7 and np.array_equal(ds.mixer._v_L, L0)
    assert not any(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(first, sources[1]))
    it = iter(ds)
    for _ in range(5):   # steps_per_epoch = 2 and a prefetch two batches deep: by the fifth batch a second rereverb has run
        bx, by = next(it)
        assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3)
        assert torch.isfinite(bx).all() and float(by.min()) >= 0 and float(by.max()) <= 1
    torch.cuda.synchronize()
    assert ds.mixer._aug.rirs is not first_rirs and np.array_equal(ds.mixer._v_L, L0)
    assert not any(torch.equal(a, b) for a, b in zip(first, ds.mixer.voices))
    # validation sets are never reverberated; without the token the mixer has no augmentation state
    val = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb']), training=False, sources=sources, device=dev, seed=4)
    assert val.mixer._aug is None
    plain = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run']), training=True, sources=sources, device=dev, seed=4)
    assert plain.mixer._aug is None
    bx, by = next(iter(plain))
    assert bx.shape == (6, 40, 64, 2) and torch.isfinite(bx).all()
