"""CPU tests of the fly-by augmentation (iris_flyby, csrc/k_flyby.h): the float64 definition of tests/flyby_ref.py is held to
physics - Doppler shift, inter-channel delay, spreading level, the ground reflection - so that the GPU test (tests/test_flyby_gpu.py)
is not a comparison of two copies of one mistake; then the host side: the closed-form reference distance, the draws, the record
packing, the run-name token and the C entry point's argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import flyby_ref as FR
from flyby_ref import FS, SOUND, flyby_ref, geometry, line_mics, rule_ratio, yardstick32


def _cfg(name, *extra):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '2', '--batch_size', '2',
                         '--name', name, *extra])


# the pass of the Doppler and level tests: 5 m up, straight over the source (z_s = 1.5) at t = 1 s with 15 m/s, 2 s long
PASS = geometry((-15.0, 0.0, 5.0), (15.0, 0.0, 0.0), 1.5, 0.0)
PASS_LEN = 32000


def _tau(geom, t):
    """The emission time (seconds, up to a constant) of what microphone 0 receives at t."""
    return t - FR.distance(geom, 0, geom["z_s"], np.asarray(t, np.float64)) / SOUND


@pytest.fixture(scope="module")
def tone_pass():
    x = np.sin(2 * np.pi * 1000.0 * np.arange(PASS_LEN) / FS)[None, :]
    return flyby_ref(x, PASS)[0][0]


def test_yardstick_sets_k():
    """K is twice the float32 yardstick's worst ratio over the GPU test's inputs, rounded up - recomputed here."""
    worst = 0.0
    for name, x, geom in FR.gpu_cases():
        ref, s_abs = flyby_ref(x, geom)
        if x.shape[1] >= 255:   # the rule cannot pass by leaving elements out
            assert (s_abs > 0).mean() >= 0.7, name
        worst = max(worst, rule_ratio(yardstick32(x, geom), ref, s_abs))
    print(f"yardstick32 over gpu_cases(): worst |y32 - ref| / (u S) = {worst:.3f}; K = {FR.K}")
    assert abs(worst - FR.YARDSTICK_WORST) < 5e-3 and FR.K == math.ceil(2 * worst)


def test_doppler_shift_of_a_pass(tone_pass):
    y = tone_pass
    onset = (FR.distance(PASS, 0, 1.5, np.float64(0.0)) - FR.r_ref_closed(PASS, PASS_LEN)) / SOUND   # the first arrival, seconds
    shifts = []
    for t_a, t_b in ((0.0, 0.2), (1.8, 2.0)):
        a, b = int(round(max(t_a, onset + 20 / FS) * FS)), int(round(t_b * FS))
        seg = y[a:b]
        k = np.nonzero(seg[:-1] * seg[1:] < 0)[0]                          # a sign change between k and k + 1
        t_x = (a + k + seg[k] / (seg[k] - seg[k + 1])) / FS                # ... at this time, by linear interpolation
        measured = (len(t_x) - 1) / (2.0 * (t_x[-1] - t_x[0]))
        want = 1000.0 * (_tau(PASS, t_x[-1]) - _tau(PASS, t_x[0])) / (t_x[-1] - t_x[0])
        print(f"[{t_a}, {t_b}] s: {measured:.2f} Hz from the zero crossings, {want:.2f} Hz analytic")
        assert abs(measured - want) <= 2.5
        shifts.append(want - 1000.0)
    assert shifts[0] > 35 and shifts[1] < -35      # approaching: higher; receding: lower (about +-42 Hz)


def test_inter_channel_delay_of_a_hovering_pair():
    geom = geometry((20.0, 0.0, 1.5), (0.0, 0.0, 0.0), 1.5, 0.0, line_mics(2, 0.1))   # the path difference is the full 0.1 m
    rng = np.random.default_rng(3)
    x = np.repeat(rng.standard_normal((1, 8000)), 2, axis=0)
    y, _ = flyby_ref(x, geom)
    lags = np.arange(-48, 49)
    core = slice(64, 8000 - 64)
    xc = np.array([np.dot(y[0, core], np.roll(y[1], -lag)[core]) for lag in lags])
    # the correlation of white noise is as narrow as a sinc: a parabola through three whole lags is 0.12 samples off here.  So
    # the band-limited correlation is first evaluated on a grid 16 times finer (sinc interpolation), then the parabola is fitted
    fine = lags[int(np.argmax(xc))] + np.arange(-16, 17) / 16.0
    xf = np.array([np.dot(xc, np.sinc(t - lags)) for t in fine])
    k = int(np.argmax(xf))
    assert 0 < k < len(fine) - 1
    peak = fine[k] + (0.5 / 16.0) * (xf[k - 1] - xf[k + 1]) / (xf[k - 1] - 2 * xf[k] + xf[k + 1])
    print(f"inter-channel delay {peak:.4f} samples; 0.1 m is {0.1 * FS / SOUND:.4f}")
    assert abs(peak - 0.1 * FS / SOUND) <= 0.05


def test_level_follows_the_distance(tone_pass):
    y, n = tone_pass, np.arange(PASS_LEN)
    g = FR.r_ref_closed(PASS, PASS_LEN) / FR.distance(PASS, 0, 1.5, n / FS)
    near, far = slice(16000 - 800, 16000 + 800), slice(PASS_LEN - 1600, PASS_LEN)
    rms = lambda v: math.sqrt(float(np.mean(v * v)))  # noqa: E731
    measured, want = rms(y[near]) / rms(y[far]), float(g[near].mean() / g[far].mean())
    print(f"level ratio near / far: {measured:.4f} measured, {want:.4f} from the distances")
    assert want > 4 and abs(measured / want - 1) <= 0.02


def test_ground_reflection_is_the_image_source():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3000))
    both = geometry((-3.0, 2.0, 6.0), (12.0, -3.0, 0.0), 1.5, 0.5, line_mics(2))
    direct = dict(both, beta=0.0)
    image = dict(both, beta=0.0, z_s=-1.5)
    r_ref = FR.r_ref_closed(both, 3000)
    want = flyby_ref(x, direct)[0] + 0.5 * flyby_ref(x, image, r_ref=r_ref)[0]
    got = flyby_ref(x, both)[0]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(got - flyby_ref(x, direct)[0]).max() > 1e-2 * np.abs(want).max()   # (the reflection is there)


def test_reference_distance_closed_form():
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    rng = np.random.default_rng(11)
    length = 8000
    t = np.linspace(0.0, (length - 1) / FS, 100000)
    inside = 0
    for i in range(100):
        g = T.draw_flyby(rng, 1 + i % 3, (1 + 2 * (i % 2)) * length / FS)   # every other pass may peak after the clip
        closed = FE.flyby_r_ref(g["p0"], g["v"], g["z_s"], g["mics"], length)
        brute = min(float(FR.distance(g, c, g["z_s"], t).min()) for c in range(g["mics"].shape[0]))
        assert -1e-12 <= brute - closed <= 1e-9, (i, closed, brute)
        assert abs(closed - FR.r_ref_closed(g, length)) <= 1e-12 * closed     # the reference module's own closed form
        ends = min(float(FR.distance(g, c, g["z_s"], t[[0, -1]]).min()) for c in range(g["mics"].shape[0]))
        inside += closed < ends - 1e-6
    assert 20 <= inside <= 95                      # vertices inside the clip and clamped ones both occur
    hover = geometry((3.0, 4.0, 1.5), (0.0, 0.0, 0.0), 1.5)
    assert FE.flyby_r_ref(hover["p0"], hover["v"], 1.5, hover["mics"], 100) == 5.0


def _closest(g):
    """(time, horizontal distance) of the closest approach of the array centre to the source."""
    v, p = g["v"][:2], g["p0"][:2]
    t_c = -float(np.dot(p, v)) / float(np.dot(v, v))
    return t_c, float(np.linalg.norm(p + v * t_c))


def test_draw_flyby_ranges_seed_and_refusals():
    from challenge_amd import transforms as T
    rng = np.random.default_rng(0)
    seconds = 2.5
    seen = {"h": [], "s": [], "b": [], "t": [], "beta": []}
    for i in range(1000):
        chan = 1 + i % 4
        g = T.draw_flyby(rng, chan, seconds)
        assert set(g) == {"p0", "v", "z_s", "beta", "mics"} and g["z_s"] == 1.5
        assert g["p0"].shape == (3,) and g["v"].shape == (3,) and g["mics"].shape == (chan, 3) and g["v"][2] == 0
        assert np.allclose(g["mics"][:, 0], 0.1 * (np.arange(chan) - 0.5 * (chan - 1))) and not g["mics"][:, 1:].any()
        t_c, b = _closest(g)
        for key, val in zip(seen, (g["p0"][2], float(np.linalg.norm(g["v"])), b, t_c, g["beta"])):
            seen[key].append(val)
    for key, (lo, hi) in {"h": (5, 30), "s": (0, 15), "b": (0, 20), "t": (0, seconds), "beta": (0, 0.6)}.items():
        vals = np.array(seen[key])
        assert vals.min() >= lo - 1e-9 and vals.max() < hi + 1e-9, key
        assert vals.min() < lo + 0.05 * (hi - lo) and vals.max() > hi - 0.05 * (hi - lo), key   # the range is used
    a = T.draw_flyby(np.random.default_rng(42), 2, 1.0)
    b = T.draw_flyby(np.random.default_rng(42), 2, 1.0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    fixed = T.draw_flyby(rng, 2, 1.0, altitude=(7, 7), speed=(3, 3), miss=(0, 0), beta=(0, 0), mic_spacing=0.2, z_s=1.0)
    assert fixed["p0"][2] == 7 and abs(np.linalg.norm(fixed["v"]) - 3) < 1e-12 and fixed["beta"] == 0 and fixed["z_s"] == 1.0
    assert np.allclose(fixed["mics"][:, 0], [-0.1, 0.1])
    for bad in (dict(channels=0), dict(channels=9), dict(seconds=-1.0), dict(seconds=float("nan")), dict(mic_spacing=-0.1),
                dict(altitude=(1.0, 30.0)), dict(altitude=(30.0, 5.0)), dict(speed=(0.0, 400.0)), dict(speed=(-1.0, 5.0)),
                dict(miss=(-1.0, 2.0)), dict(beta=(0.0, 1.5)), dict(beta=(float("nan"), 0.5)), dict(z_s=-1.0), dict(speed=3.0)):
        kw = dict(channels=2, seconds=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            T.draw_flyby(rng, kw.pop("channels"), kw.pop("seconds"), **kw)


def test_record_packing_round_trips():
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    assert FE.FLYBY_SRC.itemsize == 288 and FE.FLYBY_SRC.fields["mic"][1] == 96
    rng = np.random.default_rng(1)
    geoms = [T.draw_flyby(rng, 3, 0.5), None, dict(T.draw_flyby(rng, 3, 0.5), beta=0.0), T.draw_flyby(rng, 3, 0.1)]
    lengths = [8000, 77, 8000, 1600]
    table = FE.flyby_records(geoms, lengths, 3)
    back = np.frombuffer(table.tobytes(), FE.FLYBY_SRC)
    assert list(back["len"]) == lengths and list(back["n_paths"]) == [2, 0, 1, 2] and not back["src"].any() and not back["dst"].any()
    for rec, g, n in zip(back, geoms, lengths):
        if g is None:
            assert rec["r_ref"] == 0 and not rec["mic"].any()
            continue
        assert np.array_equal(rec["p0"], g["p0"]) and np.array_equal(rec["v"], g["v"]) and rec["z_s"] == g["z_s"]
        assert rec["beta"] == g["beta"] and np.array_equal(rec["mic"][:3], g["mics"]) and not rec["mic"][3:].any()
        assert abs(rec["r_ref"] - FR.r_ref_closed(g, n)) <= 1e-12 * rec["r_ref"] and rec["r_ref"] > 0
    g = geoms[0]
    for bad in (dict(g, beta=1.0), dict(g, beta=-0.1), dict(g, z_s=-1.0), dict(g, v=np.array([400.0, 0, 0])),
                dict(g, p0=np.array([0.0, np.nan, 5.0])), dict(g, mics=g["mics"][:2]),
                dict(g, p0=np.array([0.0, 0.0, 1.5]), v=np.zeros(3), mics=np.zeros((3, 3)))):       # the array sits on the source
        with pytest.raises(ValueError):
            FE.flyby_records([bad], [8000], 3)
    with pytest.raises(ValueError):
        FE.flyby_records([g], [0], 3)
    with pytest.raises(ValueError):
        FE.flyby_records([g, g], [8000], 3)
    with pytest.raises(ValueError):
        FE.flyby_records([None], [10], 9)


def test_token_and_the_refusals():
    from challenge_amd import data_utils as D
    from challenge_amd import sj_train as S
    wants = lambda name: D.run_tokens(name).flyby  # noqa: E731
    assert wants("run_flyby") and wants("flyby") and wants("pcen_flyby_filter") and not wants("") and not wants(None)
    for name in ("stretch", "speed", "reverb", "reverb_long", "reverb_shoebox", "filtaug", "filtaug_linear", "ipd", "whiten", "pcen",
                 "pcen_learn", "filter", "nominmax"):
        assert not wants("run_" + name)
    assert D.RunTokens.__dataclass_fields__["flyby"].default is False
    t = D.run_tokens(_cfg("flyby_ipd_whiten_filtaug_pcen_filter"))                     # goes with every other token
    assert t.flyby and t.ipd and t.whiten and t.filtaug == 'step' and t.filter and t.compression == 'pcen'
    assert not (t.speed or t.reverb or t.stretch)
    assert D.model_in_channels(_cfg("run_flyby")) == 2
    for name in ("run_flyby_speed", "run_flyby_reverb", "reverb_shoebox_flyby", "flyby_reverb_long"):
        with pytest.raises(ValueError, match="'flyby'"):
            D.run_tokens(name)
    D.check_builder(D.run_tokens("run_flyby"), 'make_wave_dataset')
    for builder in ('make_dataset', 'make_device_dataset'):
        with pytest.raises(ValueError, match="asks for 'flyby'"):
            D.check_builder(D.run_tokens("run_flyby"), builder)
    cfg = S.ARGS().get(['--name', 'run_flyby', '--n_frame', '64', '--batch_size', '2'])
    spectra = S.synthetic_sources(2, 3, freq=33, n_bg=2, n_voice=3, n_noise=2)
    with pytest.raises(ValueError, match="make_wave_dataset"):
        S.make_dataset(cfg, training=True, sources=spectra)
    with pytest.raises(ValueError, match="make_wave_dataset"):
        S.make_device_dataset(cfg, training=True, sources=spectra)
    from challenge_amd.mixer import DeviceMixer, WaveMixer
    with pytest.raises(NotImplementedError, match="spectrum"):
        DeviceMixer.enable_flyby(object())
    with pytest.raises(RuntimeError, match="enable_flyby"):
        WaveMixer.reflyby(object())


def test_argument_validation_without_gpu():
    from challenge_amd import _native as N
    lib = N.lib()
    p8 = C.c_void_p(8)
    INVALID, UNSUPPORTED = -1, -2

    def refused(rc, code):
        assert rc == code, rc
        assert lib.iris_last_error().startswith(b"iris_flyby:"), lib.iris_last_error()

    refused(lib.iris_flyby(None, 1, 2, 100, None), INVALID)        # NULL table with n_src > 0
    refused(lib.iris_flyby(p8, 1, 0, 100, None), INVALID)          # channels
    refused(lib.iris_flyby(p8, 1, 9, 100, None), UNSUPPORTED)      # more microphones than a record holds
    refused(lib.iris_flyby(p8, -1, 2, 100, None), INVALID)         # n_src < 0
    refused(lib.iris_flyby(p8, 65536, 2, 100, None), UNSUPPORTED)  # more sources than the grid holds
    refused(lib.iris_flyby(p8, 1, 2, 0, None), INVALID)            # max_len
    assert lib.iris_flyby(None, 0, 2, 100, None) == 0              # no sources: nothing to do, no launch
    assert lib.iris_flyby(p8, 0, 8, 0, None) == 0
