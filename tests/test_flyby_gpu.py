"""GPU tests of the fly-by augmentation (iris_flyby, csrc/k_flyby.h): parity with the float64 definition of tests/flyby_ref.py
under the error rule |y - ref| <= K u S (K = 4, derived from the float32 yardstick in tests/test_flyby_host.py, never from the
kernel), exact zeros, the identity record, ragged batches against single calls, both staging paths, skipped records,
`WaveMixer.enable_flyby` / `reflyby`, and the 'flyby' run name.  The references are computed once per module.

Kernel's own worst ratio |out - ref| / (u S) on one MI355X over the cases of test_every_element_meets_the_rule: 1.531 (receding,
L = 4099, C = 3, beta = 0.6) - beside the yardstick's 1.650 and K = 4; 1.268 on the global-memory path.  The
tests print every case."""
import numpy as np
import pytest
import torch

import flyby_ref as FR
from flyby_ref import K, flyby_ref, geometry, line_mics, make_wave, rule_ratio
from oracle import frontend_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    """[(name, x, geometry, ref, S)] over `flyby_ref.gpu_cases()`, the float64 definition evaluated once."""
    return [(name, x, geom, *flyby_ref(x, geom)) for name, x, geom in FR.gpu_cases()]


@pytest.fixture(scope="module")
def batched(dev, cases):
    """The kernel's output for every case: one ragged launch per channel count."""
    from challenge_amd import frontend as FE
    out = [None] * len(cases)
    for chan in FR.CHANNELS:
        idx = [i for i, c in enumerate(cases) if c[1].shape[0] == chan]
        res = FE.flyby_batch([torch.from_numpy(cases[i][1]).to(dev) for i in idx], [cases[i][2] for i in idx])
        for i, r in zip(idx, res):
            out[i] = r
    return out


def test_every_element_meets_the_rule(cases, batched):
    worst, where = 0.0, None
    for (name, x, geom, ref, s_abs), out in zip(cases, batched):
        got = out.cpu().numpy()
        assert got.shape == x.shape and got.dtype == np.float32
        ratio = rule_ratio(got, ref, s_abs)        # (asserts that elements with S == 0 are exactly 0)
        covered = float((s_abs > 0).mean())
        print(f"k_flyby {name}: |out - ref| / (u S) <= {ratio:.3f} (K = {K}); S > 0 on {100 * covered:.1f} %")
        if x.shape[1] >= 255:
            assert covered >= 0.7, (name, covered)   # the rule cannot pass by leaving elements out
        if ratio > worst:
            worst, where = ratio, name
        assert ratio <= K, (name, ratio)
    print(f"k_flyby: worst |out - ref| / (u S) = {worst:.3f} at {where}; yardstick {FR.YARDSTICK_WORST}, K = {K}")


def test_batch_equals_single_calls_and_repeats_bitwise(dev, cases, batched):
    from challenge_amd import frontend as FE
    for chan in FR.CHANNELS:
        idx = [i for i, c in enumerate(cases) if c[1].shape[0] == chan]
        waves = [torch.from_numpy(cases[i][1]).to(dev) for i in idx]
        again = FE.flyby_batch(waves, [cases[i][2] for i in idx])
        for i, w, a in zip(idx, waves, again):
            assert torch.equal(a, batched[i]), cases[i][0]                                   # two runs
            assert torch.equal(FE.flyby_batch([w], [cases[i][2]])[0], batched[i]), cases[i][0]   # one record alone


def test_identity_record_and_the_single_voice_form(dev):
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    x = torch.from_numpy(make_wave((3, 4099), 7)).to(dev)
    geom = FR.case_geometry("overhead", 3, 4099, 0.6)
    out = FE.flyby_batch([x, x, x[:, :255].contiguous()], [None, geom, None])
    assert torch.equal(out[0], x) and out[0].data_ptr() != x.data_ptr() and torch.equal(out[2], x[:, :255])
    assert torch.equal(T.flyby(x, geom), out[1]) and not torch.equal(out[1], x)
    mono = FR.case_geometry("overhead", 1, 4099, 0.6)
    assert torch.equal(T.flyby(x[1], mono), FE.flyby_batch([x[1:2].contiguous()], [mono])[0][0])   # a 1-D voice is [1, L]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.flyby(x.cpu(), geom)
    with pytest.raises(ValueError):
        FE.flyby_batch([x], [geom, geom])
    with pytest.raises(ValueError):
        FE.flyby_batch([x], [FR.case_geometry("overhead", 2, 4099, 0.6)])      # two microphones for three channels


def test_global_memory_path_equals_the_staged_one(dev):
    """Eight channels with the ground path need more span than the LDS buffer holds, and so does a pair of microphones 60 m
    apart: these tiles read global memory.  Channel by channel as one-microphone records (staged) the bits are the same."""
    from challenge_amd import frontend as FE
    for chan, spacing, length in ((8, 0.1, 2500), (2, 60.0, 1500)):
        x = make_wave((chan, length), 40 + chan)
        geom = geometry((-1.0, 0.5, 5.0), (15.0, 0.0, 0.0), 1.5, 0.6, line_mics(chan, spacing))
        xd = torch.from_numpy(x).to(dev)
        out = FE.flyby_batch([xd], [geom])[0]
        ref, s_abs = flyby_ref(x, geom)
        ratio = rule_ratio(out.cpu().numpy(), ref, s_abs)
        print(f"k_flyby global path C = {chan}, spacing {spacing}: |out - ref| / (u S) <= {ratio:.3f} (K = {K})")
        assert ratio <= K
        # one microphone per record; the delays and gains stay referred to the whole array's reference distance
        table = FE.flyby_records([dict(geom, mics=geom["mics"][c:c + 1]) for c in range(chan)], [length] * chan, 1)
        table["r_ref"] = FE.flyby_r_ref(geom["p0"], geom["v"], geom["z_s"], geom["mics"], length)
        rows = torch.zeros_like(xd)
        table["src"] = [xd[c].data_ptr() for c in range(chan)]
        table["dst"] = [rows[c].data_ptr() for c in range(chan)]
        FE.flyby_launch(table, 1, length, dev)
        torch.cuda.synchronize()
        assert torch.equal(rows, out)


def test_skipped_records_leave_their_destination_alone(dev):
    from challenge_amd import frontend as FE
    length = 1500
    x = torch.from_numpy(make_wave((2, length), 9)).to(dev)
    geom = FR.case_geometry("overhead", 2, length, 0.6)
    good = FE.flyby_records([geom], [length], 2)[0]
    bufs = [torch.full((2 * length + 100,), -7.0, device=dev) for _ in range(10)]
    table = np.zeros(len(bufs), FE.FLYBY_SRC)
    table[:] = good
    table["src"], table["dst"] = x.data_ptr(), [b.data_ptr() for b in bufs]
    table["src"][0] = 0                      # NULL source
    table["len"][1] = 0                      # len <= 0
    table["len"][2] = length + 1             # len > max_len
    table["p0"][3, 1] = np.nan               # non-finite geometry
    table["mic"][4, 1, 2] = np.inf
    table["r_ref"][5] = 0.0                  # r_ref <= 0
    table["n_paths"][6] = 3                  # no such path count
    table["v"][7] = (400.0, 0.0, 0.0)        # faster than sound
    table["mic"][8, 5, 0] = np.nan           # (a microphone beyond `channels` is not read: a good record)
    FE.flyby_launch(table, 2, length, dev)
    torch.cuda.synchronize()
    want = FE.flyby_batch([x], [geom])[0]
    for i, b in enumerate(bufs):
        assert bool((b[2 * length:] == -7.0).all()), i               # the floats beyond [C, L] keep the sentinel
        if i < 8:
            assert bool((b == -7.0).all()), i
        else:
            assert torch.equal(b[:2 * length].view(2, length), want), i


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


def test_wave_mixer_reflyby(dev):
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    from challenge_amd.mixer import DeviceMixer, WaveMixer
    rng = np.random.default_rng(11)
    hop, n_fft, n_frame, n_classes = 64, 256, 48, 3
    backgrounds, voices, noises = _corpus(rng)
    labels = np.eye(n_classes, dtype=np.float32)[rng.integers(0, n_classes, len(voices))]
    kw = dict(n_frame=n_frame, n_fft=n_fft, hop=hop, max_voices=4, max_noises=3, n_classes=n_classes, device=dev, min_ratio=1)
    new = lambda seed: WaveMixer(backgrounds, voices, labels, noises, seed=seed, **kw)  # noqa: E731

    # before the first reflyby: bit-identical to a plain mixer of the same seed, also with the draws on the device
    plain, fly = new(21), new(21)
    fly.enable_flyby()
    for _ in range(2):
        (wa, la), (wb, lb) = plain.mix(8), fly.mix(8)
        assert torch.equal(wa, wb) and torch.equal(la, lb)
    plain_dd = new(5)
    plain_dd.enable_device_draw(77)
    want = [plain_dd.mix(8) for _ in range(2)]
    for order in ("flyby_first", "draw_first"):
        m = new(5)
        if order == "flyby_first":
            m.enable_flyby()
            m.enable_device_draw(77)
        else:
            m.enable_device_draw(77)
            m.enable_flyby()
        va = m._dd["voice_arrays"]
        assert np.array_equal(va["src"].cpu().numpy().astype(np.uint64), m._v_ptr)
        assert np.array_equal(va["act"].cpu().numpy().astype(np.uint64), m._v_act)
        for wa, la in want:
            wb, lb = m.mix(8)
            assert torch.equal(wa, wb) and torch.equal(la, lb), order

    # after reflyby(geometry): the resident voices are flyby_batch of the originals, the activity is the frame rule of the results
    mixer = fly
    originals = [torch.from_numpy(v).to(dev) for v in voices]
    assert all(torch.equal(a, b) for a, b in zip(mixer.voices, originals))
    ptrs = (mixer._v_ptr.copy(), mixer._v_act.copy())
    assert not set(ptrs[0]) & {int(v.data_ptr()) for v in mixer._aug.orig}
    grng = np.random.default_rng(2)
    geoms = [T.draw_flyby(grng, 2, v.shape[1] / 16000.0) for v in voices]
    geoms[2] = None                                                   # one voice left as it is
    used = mixer.reflyby(geoms)
    assert len(used) == len(geoms) and all(a is b for a, b in zip(used, geoms)) and mixer._aug.geometry is used
    want = FE.flyby_batch(originals, geoms)
    moved = 0
    for v, w, o, act in zip(mixer.voices, want, originals, mixer.voice_active):
        assert torch.equal(v, w) and v.shape == o.shape
        assert np.array_equal(act.cpu().numpy(), R.wave_frame_active(v.cpu().numpy(), n_fft, hop))
        moved += int(not torch.equal(v, o))
    assert moved == len(voices) - 1 and torch.equal(mixer.voices[2], originals[2])
    assert any(0 < float(a.sum()) < a.numel() for a in mixer.voice_active)     # silent tails stayed exactly silent
    assert np.array_equal(mixer._v_ptr, ptrs[0]) and np.array_equal(mixer._v_act, ptrs[1])
    assert [v.data_ptr() for v in mixer.voices] == list(ptrs[0]) and [a.data_ptr() for a in mixer.voice_active] == list(ptrs[1])
    assert np.array_equal(mixer._v_L, [v.shape[1] for v in voices]) and np.array_equal(mixer._v_T, [1 + v.shape[1] // hop for v in voices])
    wav, lab = mixer.mix(8)
    assert torch.isfinite(wav).all() and float(lab.sum()) > 0
    # two random redraws: other voices, the same addresses
    g1 = mixer.reflyby()
    first = [v.clone() for v in mixer.voices]
    g2 = mixer.reflyby()
    assert len(g1) == len(g2) == len(voices) and not np.array_equal(g1[0]["p0"], g2[0]["p0"])
    assert not any(torch.equal(a, b) for a, b in zip(first, mixer.voices))
    assert np.array_equal(mixer._v_ptr, ptrs[0]) and np.array_equal(mixer._v_act, ptrs[1])
    assert all(5 <= g["p0"][2] < 30 and np.linalg.norm(g["v"]) < 15 and 0 <= g["beta"] < 0.6 for g in g1 + g2)

    # refusals: one voice augmentation per mixer, in either order
    with pytest.raises(ValueError):
        mixer.reflyby(geoms[:3])
    with pytest.raises(RuntimeError, match="already called"):
        mixer.enable_flyby()
    for enable in (mixer.enable_speed, mixer.enable_reverb):
        with pytest.raises(RuntimeError, match="a mixer holds one voice augmentation"):
            enable()
    for first_call in ("enable_speed", "enable_reverb"):
        other = new(3)
        getattr(other, first_call)()
        with pytest.raises(RuntimeError, match="a mixer holds one voice augmentation"):
            other.enable_flyby()
        with pytest.raises(RuntimeError, match="enable_flyby"):
            other.reflyby()
    with pytest.raises(RuntimeError, match="enable_flyby"):
        new(3).reflyby()
    with pytest.raises(ValueError):
        new(3).enable_flyby(speed=(0.0, 400.0))
    with pytest.raises(NotImplementedError):
        DeviceMixer.enable_flyby(object())


def test_flyby_run_name_in_make_wave_dataset(dev):
    from challenge_amd import sj_train as S
    args = ['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
            '--max_noises', '3', '--steps_per_epoch', '2']
    backgrounds, voices, labels, noises = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
    mono = lambda ws: [np.repeat(w[:1], 2, axis=0) for w in ws]  # noqa: E731
    sources = (mono(backgrounds), mono(voices), labels, mono(noises))       # a mono corpus repeated over the two channels
    make = lambda name, training: S.make_wave_dataset(S.ARGS().get(args + ['--name', name]), training=training,  # noqa: E731
                                                      sources=sources, device=dev, seed=4)
    ds = make('run_flyby', True)
    assert ds.mixer._aug.geometry is not None and len(ds.mixer._aug.geometry) == 7
    first = [v.clone() for v in ds.mixer.voices]
    assert not any(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(first, sources[1]))
    it = iter(ds)
    for _ in range(5):   # steps_per_epoch = 2 and a prefetch two batches deep: by the fifth batch a second reflyby has run
        bx, by = next(it)
        assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3)
        assert torch.isfinite(bx).all() and float(by.min()) >= 0 and float(by.max()) <= 1
    assert not any(torch.equal(a, b) for a, b in zip(first, ds.mixer.voices))        # two epochs hold different voices
    assert [tuple(v.shape) for v in ds.mixer.voices] == [v.shape for v in sources[1]]
    # validation sets are never touched; without the token the mixer has no such state
    val, val_plain = make('run_flyby', False), make('run', False)
    assert val.mixer._aug is None and make('run', True).mixer._aug is None
    (xa, ya), (xb, yb) = next(iter(val)), next(iter(val_plain))
    assert torch.equal(xa, xb) and torch.equal(ya, yb)
    # with 'ipd': a mono-repeated corpus has the phase difference (cos, sin) = (1, 0) wherever there is sound; a voice heard
    # by two microphones 0.1 m apart does not
    still, _ = next(iter(make('run_ipd', True)))
    moving, _ = next(iter(make('run_flyby_ipd', True)))
    assert still.shape == moving.shape == (6, 40, 64, 4)
    assert float(still[..., 3].abs().max()) <= 1e-3
    off = (moving[..., 3].abs() > 1e-2).float().mean()
    print(f"'flyby' with 'ipd': |sin| > 0.01 on {100 * float(off):.1f} % of the (band, frame) cells; without: none")
    assert float(off) > 0.02
