"""GPU tests of the partitioned FFT convolution (iris_fft_fir_batch, csrc/k_fft_fir.h): parity with the float64 convolution
under the norm-wise rule |y - ref| <= C u R of tests/fftconv_ref.py on one ragged table, exact zeros, bit reproducibility
(alone / in the table / across workspace groups), untouched tails, skipped records, unaligned rows, the tap-pitch layout, the
cross-check against the direct form, the long path of `WaveMixer.enable_reverb` and the 'reverb_long' run name.

The accuracy test prints the ratio of every record and the worst one, which DESIGN.md (K2f) quotes."""
import numpy as np
import pytest
import torch

import fftconv_ref as R
from reverb_ref import fir_ref
from reverb_ref import rule_ratio as fir_rule_ratio
from test_reverb_gpu import KW, _sources
from test_reverb_gpu import _to

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test collected without a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ragged():
    """The accuracy table of tests/fftconv_ref.py and its float64 reference, computed once."""
    cases, waves, taps = R.table()
    return cases, waves, taps, [R.fft_fir_ref(x, h) for x, h in zip(waves, taps)]


@pytest.fixture(scope="module")
def outs(dev, ragged):
    """The whole table through `fft_fir_batch` in ONE call (one group: the default budget holds it)."""
    from challenge_amd import frontend as FE
    _, waves, taps, _ = ragged
    assert sum(FE.fft_fir_workspace(2, x.shape[1], h.shape[1]) for x, h in zip(waves, taps)) < 256 << 20
    return FE.fft_fir_batch(_to(dev, waves), _to(dev, taps))


def test_ragged_table_meets_the_rule(ragged, outs):
    cases, _, _, refs = ragged
    worst, where = 0.0, None
    for (n, k), out, (ref, r_norm) in zip(cases, outs, refs):
        assert out.shape == (2, n) and out.dtype == torch.float32
        ratio = R.rule_ratio(out.cpu().numpy(), ref, r_norm)
        print(f"k_fft_fir L = {n}, K = {k}: |y - ref| / (u R) <= {ratio:.4f}")
        if ratio > worst:
            worst, where = ratio, (n, k)
    print(f"k_fft_fir: worst |y - ref| / (u R) = {worst:.4f} at (L, K) = {where} (the rule allows C = {R.C_RULE:g})")
    for (n, k), out, (ref, r_norm) in zip(cases, outs, refs):
        assert R.rule_ratio(out.cpu().numpy(), ref, r_norm) <= R.C_RULE, (n, k)


def test_zero_voice_alone_repeat_and_groups_are_bitwise(dev, ragged, outs):
    from challenge_amd import frontend as FE
    cases, waves, taps, _ = ragged
    w, h = _to(dev, waves), _to(dev, taps)
    # an all-zero voice gives exactly 0 everywhere
    zero = FE.fft_fir_batch([torch.zeros((2, 2049), device=dev)], [h[cases.index((2049, 4097))]])[0]
    assert bool((zero == 0).all())
    # two runs are bitwise equal
    again = FE.fft_fir_batch(w, h)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    # a record alone equals the same record inside the table
    for case in ((1, 9000), (1025, 2), (5000, 9000), (2049, 1025), R.LONG):
        i = cases.index(case)
        assert torch.equal(FE.fft_fir_batch([w[i]], [h[i]])[0], outs[i]), case
    # a tiny budget forces several groups (every record larger than the budget is a group of its own)
    table = np.zeros(len(cases), FE.FFT_FIR_SRC)
    table["len"], table["n_taps"] = [n for n, _ in cases], [k for _, k in cases]
    groups, largest = FE.fft_fir_groups(table, 2, 1 << 19)
    assert len(groups) == 10 and groups[0][1] - groups[0][0] > 1 and groups[-1] == (len(cases) - 1, len(cases))
    assert largest == FE.fft_fir_workspace(2, *R.LONG) > 1 << 19      # the last record alone exceeds the budget
    split = FE.fft_fir_batch(w, h, workspace_budget=1 << 19)
    assert all(torch.equal(a, b) for a, b in zip(outs, split))


def _table(FE, records):
    table = np.zeros(len(records), FE.FFT_FIR_SRC)
    for i, rec in enumerate(records):
        table[i] = rec
    return table


def test_tails_and_skipped_records(dev):
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(4)
    n, k, chan = 2049, 1500, 2
    x, h = rng.standard_normal((chan, n)).astype(np.float32), rng.standard_normal((chan, k)).astype(np.float32)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    want = FE.fft_fir_batch([xd], [hd])[0]
    need = FE.fft_fir_workspace(chan, n, k)
    fresh = lambda: torch.full((chan * n + 64,), SENTINEL, device=dev)  # noqa: E731
    xp, hp = xd.data_ptr(), hd.data_ptr()
    good = fresh()
    bad = {"src NULL": (0, hp, n, k, 0), "taps NULL": (xp, 0, n, k, 0), "len 0": (xp, hp, 0, k, 0), "len < 0": (xp, hp, -3, k, 0),
           "n_taps 0": (xp, hp, n, 0, 0), "n_taps < 0": (xp, hp, n, -1, 0), "slice beyond the workspace": (xp, hp, n, k, 2 * need),
           "slice does not fit": (xp, hp, n, k, need + 16), "slice off 16 bytes": (xp, hp, n, k, need + 8),
           "negative offset": (xp, hp, n, k, -16),
           "len > max_len": (xp, hp, n, k, 0), "n_taps > max_taps": (xp, hp, n, k, 0)}
    dsts = {name: fresh() for name in bad}
    ws = torch.empty(2 * need, dtype=torch.uint8, device=dev)
    records = [(xp, good.data_ptr(), hp, n, k, 0), (xp, 0, hp, n, k, need)]   # (the second: a NULL dst)
    records += [(r[0], dsts[name].data_ptr(), r[1], r[2], r[3], r[4]) for name, r in bad.items() if "max" not in name]
    FE.fft_fir_launch(_table(FE, records), chan, n, k, 0, ws, dev)
    # the two records that are malformed only against the launch's own maxima
    FE.fft_fir_launch(_table(FE, [(xp, dsts["len > max_len"].data_ptr(), hp, n, k, 0)]), chan, n - 1, k, 0, ws, dev)
    FE.fft_fir_launch(_table(FE, [(xp, dsts["n_taps > max_taps"].data_ptr(), hp, n, k, 0)]), chan, n, k - 1, 0, ws, dev)
    torch.cuda.synchronize()
    assert torch.equal(good[:chan * n].view(chan, n), want) and bool((good[chan * n:] == SENTINEL).all())   # the floats beyond: untouched
    for name, d in dsts.items():
        assert bool((d == SENTINEL).all()), name
    # the Python surface
    assert FE.fft_fir_batch([], []) == []
    for waves, taps in (([xd], [hd[:1].contiguous()]),                        # channel counts differ
                        ([xd, xd[:1].contiguous()], [hd, hd]),
                        ([xd], [hd[:, :0].contiguous()]),                     # an empty tap vector
                        ([xd], [torch.zeros((chan, 32769), device=dev)]),     # K > 32768
                        ([xd.cpu()], [hd]), ([xd], [hd.cpu()]),               # CPU tensors: no fallback
                        ([xd.view(-1)], [hd]), ([xd.double()], [hd]), ([xd, xd], [hd])):
        with pytest.raises(ValueError, match="fft_fir_batch"):
            FE.fft_fir_batch(waves, taps)
    from challenge_amd import transforms as T
    with pytest.raises(ValueError, match="no CPU fallback"):
        T.reverb_fft(xd.cpu(), h)
    assert torch.equal(T.reverb_fft(xd, h), want) and torch.equal(T.reverb_fft(xd[0].contiguous(), h[0]), want[0])


def test_rows_off_16_bytes_and_tap_pitch_equal_the_packed_layout(dev):
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(5)
    chan, n, k = 2, 2051, 1027                                   # len % 4 == 3: the second channel's rows shift again
    x, h = rng.standard_normal((chan, n)).astype(np.float32), rng.standard_normal((chan, k)).astype(np.float32)
    aligned = FE.fft_fir_batch(_to(dev, [x]), _to(dev, [h]))[0]
    src, taps = torch.zeros(chan * n + 8, device=dev), torch.zeros(chan * k + 8, device=dev)
    dst = torch.full((chan * n + 8,), SENTINEL, device=dev)
    src[1:1 + chan * n].copy_(torch.from_numpy(x).view(-1))
    taps[1:1 + chan * k].copy_(torch.from_numpy(h).view(-1))
    for t in (src, dst, taps):
        assert t.data_ptr() % 16 == 0
    ws = torch.empty(FE.fft_fir_workspace(chan, n, k), dtype=torch.uint8, device=dev)
    FE.fft_fir_launch(_table(FE, [(src.data_ptr() + 4, dst.data_ptr() + 4, taps.data_ptr() + 4, n, k, 0)]), chan, n, k, 0, ws, dev)
    torch.cuda.synchronize()
    out = dst[1:1 + chan * n].view(chan, n)
    ratio = R.rule_ratio(out.cpu().numpy(), *R.fft_fir_ref(x, h))
    print(f"k_fft_fir off 16 bytes, L = {n}, K = {k}: |y - ref| / (u R) <= {ratio:.4f}")
    assert ratio <= R.C_RULE
    assert float(dst[0]) == SENTINEL and bool((dst[1 + chan * n:] == SENTINEL).all())
    assert torch.equal(out, aligned)                             # the same numbers through aligned rows: bit for bit
    # the rows of the taps `pitch` floats apart, the floats between them poisoned
    pitch = 1100
    wide = torch.full((chan, pitch), float("nan"), device=dev)
    wide[:, :k] = torch.from_numpy(h).to(dev)
    xd, o = torch.from_numpy(x).to(dev), torch.full((chan, n), SENTINEL, device=dev)
    FE.fft_fir_launch(_table(FE, [(xd.data_ptr(), o.data_ptr(), wide.data_ptr(), n, k, 0)]), chan, n, k, pitch, ws, dev)
    torch.cuda.synchronize()
    assert torch.equal(o, aligned)


def test_cross_check_against_the_direct_form(dev, ragged, outs):
    """Where K <= 4096 both engines run on the same numbers: they differ by at most the sum of the two rules' bounds."""
    from challenge_amd import frontend as FE
    cases, waves, taps, refs = ragged
    idx = [i for i, (_, k) in enumerate(cases) if k <= FE.FIR_MAX_TAPS]
    assert len(idx) == 5 * len(R.LENGTHS)
    direct = FE.fir_batch(_to(dev, [waves[i] for i in idx]), _to(dev, [taps[i] for i in idx]))
    for i, d in zip(idx, direct):
        (n, k), (ref, r_norm) = cases[i], refs[i]
        _, s_abs = fir_ref(waves[i], taps[i])
        assert fir_rule_ratio(d.cpu().numpy(), ref, s_abs, k) <= 1.0, (n, k)
        bound = R.C_RULE * R.U * r_norm + (k + 2) * R.U * s_abs
        diff = np.abs(outs[i].cpu().numpy().astype(np.float64) - d.cpu().numpy().astype(np.float64))
        assert bool((diff <= bound).all()), (n, k, float((diff - bound).max()))


def _long_rirs(seed):
    rng = np.random.default_rng(seed)
    ks = (5000, 12000, 1, 300, 4097, 16384)
    return [(rng.standard_normal((2, k)) / np.sqrt(k)).astype(np.float32) for k in ks]


def test_wave_mixer_long_path(dev):
    from challenge_amd import frontend as FE
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()
    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    with pytest.raises(ValueError, match="shoebox"):
        mixer.enable_reverb(model="shoebox", max_taps=8192)
    with pytest.raises(ValueError, match="max_taps"):
        mixer.enable_reverb(max_taps=32769)
    assert mixer._aug is None
    acts = [a.clone() for a in mixer.voice_active]
    act_ptr, L0, T0 = mixer._v_act.copy(), mixer._v_L.copy(), mixer._v_T.copy()
    mixer.enable_reverb(rt60_lo=0.2, rt60_hi=1.0, max_taps=16384, workspace_budget=1 << 20)   # (a budget that splits 6 voices)
    aug = mixer._aug
    assert len(aug.groups) > 1 and all(t.shape == (2, 16384) for t in aug.taps) and aug.table.dtype == FE.FFT_FIR_SRC
    ws_ptr = aug.workspace.data_ptr()
    # the identity response: the copies equal the originals within the rule (not bit for bit on this path)
    one = np.ones((2, 1), np.float32)
    for i, (v, out) in enumerate(zip(voices, mixer.voices)):
        ratio = R.rule_ratio(out.cpu().numpy(), *R.fft_fir_ref(v, one))
        print(f"long path, identity, voice {i}: |y - x| / (u R) <= {ratio:.4f}")
        assert ratio <= R.C_RULE, i
    ptrs = mixer._v_ptr.copy()
    assert [v.data_ptr() for v in mixer.voices] == list(ptrs)
    # given responses of 5000, 12000, ... taps: every voice is the convolution of the ORIGINAL voice
    rirs = _long_rirs(1)
    for given in (_long_rirs(2), rirs):     # the second call starts from the originals again, not from the first call's result
        used = mixer.rereverb(given)
        assert all(np.array_equal(a, b) for a, b in zip(used, given))
    for i, (v, h, out) in enumerate(zip(voices, rirs, mixer.voices)):
        assert out.shape == v.shape
        ratio = R.rule_ratio(out.cpu().numpy(), *R.fft_fir_ref(v, h))
        print(f"long path, voice {i}: L = {v.shape[1]}, K = {h.shape[1]}, |y - ref| / (u R) <= {ratio:.4f}")
        assert ratio <= R.C_RULE, i
    # lengths, frame counts, the activity vectors (the labels) and every address stay
    assert np.array_equal(mixer._v_L, L0) and np.array_equal(mixer._v_T, T0) and np.array_equal(mixer._v_act, act_ptr)
    assert all(torch.equal(a, b) for a, b in zip(mixer.voice_active, acts)) and np.array_equal(mixer._v_ptr, ptrs)
    assert aug.workspace.data_ptr() == ws_ptr
    # random responses span K > 4096: rt60 in [0.2, 1.0) gives 2134 .. 10667 taps
    seen = [h.shape[1] for _ in range(3) for h in mixer.rereverb()]
    assert all(2134 <= k <= 10667 for k in seen) and max(seen) > 4096
    assert bool(torch.isfinite(mixer.mix(8)[0]).all())
    with pytest.raises(ValueError):
        mixer.rereverb([np.zeros((2, 16385), np.float32)] * 6)
    with pytest.raises(RuntimeError, match="already called"):
        mixer.enable_reverb(max_taps=16384)
    # a default mixer still stops at 4096 taps
    plain = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    plain.enable_reverb()
    assert plain._aug.groups is None and plain._aug.workspace is None and plain._aug.table.dtype == FE.FIR_SRC
    with pytest.raises(ValueError):
        plain.rereverb([np.zeros((2, 4097), np.float32)] * 6)


def test_wave_mixer_draws_from_measured_responses(dev):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()
    pool = _long_rirs(3)[:3]
    for bad in ([np.zeros((2, 16385), np.float32)], [np.zeros((1, 100), np.float32)], []):
        mixer = WaveMixer(backgrounds, voices, labels, noises, seed=8, device=dev, **KW)
        with pytest.raises(ValueError, match="rirs"):
            mixer.enable_reverb(max_taps=16384, rirs=bad)
        assert mixer._aug is None
    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=8, device=dev, **KW)
    mixer.enable_reverb(max_taps=16384, rirs=pool)
    picked = set()
    for _ in range(4):
        used = mixer.rereverb()
        assert len(used) == 6
        for h in used:
            which = [j for j, p in enumerate(pool) if np.array_equal(h, p)]
            assert len(which) == 1                      # only the given responses
            picked.add(which[0])
    assert picked == {0, 1, 2}
    for i, (v, h, out) in enumerate(zip(voices, used, mixer.voices)):
        assert R.rule_ratio(out.cpu().numpy(), *R.fft_fir_ref(v, h)) <= R.C_RULE, i


def test_captured_mix_replayed_after_long_rereverb_equals_the_eager_mix(dev):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()

    def make():
        m = WaveMixer(backgrounds, voices, labels, noises, seed=5, device=dev, **KW)
        m.enable_reverb(max_taps=16384)
        m.enable_device_draw(77)
        assert np.array_equal(m._dd["voice_arrays"]["src"].cpu().numpy().astype(np.uint64), m._v_ptr)
        m.rereverb(_long_rirs(1))
        m.mix(16)          # (warm-up: both mixers' device draw states move once)
        torch.cuda.synchronize()
        return m

    assert KW["n_frame"] == 48
    captured, eager = make(), make()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        gw, gl = captured.mix(16)
    for seed in (2, 3):     # replayed after a second (and third) rereverb: the new contents through unchanged addresses
        captured.rereverb(_long_rirs(seed))
        g.replay()
        eager.rereverb(_long_rirs(seed))
        ew, el = eager.mix(16)
        torch.cuda.synchronize()
        assert torch.equal(gw, ew) and torch.equal(gl, el) and float(el.sum()) > 0


def test_reverb_long_run_name_in_make_wave_dataset(dev):
    from challenge_amd import sj_train as S
    args = ['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
            '--max_noises', '3', '--steps_per_epoch', '2']
    sources = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
    L0 = np.array([v.shape[1] for v in sources[1]])
    ds = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb_long']), training=True, sources=sources, device=dev, seed=4)
    aug = ds.mixer._aug
    assert aug.max_taps == 16384 == S.RIR_MAX_TAPS and aug.rt60 == (0.2, 1.0) and aug.groups is not None
    first_rirs = aug.rirs
    first = [v.clone() for v in ds.mixer.voices]
    assert len(first_rirs) == 7 and all(2134 <= h.shape[1] <= 10667 for h in first_rirs) and np.array_equal(ds.mixer._v_L, L0)
    it = iter(ds)
    for _ in range(5):   # steps_per_epoch = 2 and a prefetch two batches deep: by the fifth batch a second rereverb has run
        bx, by = next(it)
        assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3)
        assert torch.isfinite(bx).all() and float(by.min()) >= 0 and float(by.max()) <= 1
    torch.cuda.synchronize()
    assert ds.mixer._aug.rirs is not first_rirs and np.array_equal(ds.mixer._v_L, L0)
    assert not any(torch.equal(a, b) for a, b in zip(first, ds.mixer.voices))
    # measured responses through the dataset: the pool is what the mixer draws from; validation sets are never reverberated
    pool = _long_rirs(4)[:2]
    ds = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb']), training=True, sources=sources, device=dev, seed=4, rirs=pool)
    assert ds.mixer._aug.max_taps == 16384 and all(any(np.array_equal(h, p) for p in pool) for h in ds.mixer._aug.rirs)
    val = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb_long']), training=False, sources=sources, device=dev, seed=4)
    assert val.mixer._aug is None
