"""Inter-channel phase features without a GPU: the float64 reference's properties and its sign convention on a delayed
channel, the torch restatement `transforms.mel_ipd` against it within the derived fp32 bound, the run-name token and its
refusals, and the token's way through the evaluation features, the model, the run name and the Keras weight import."""
import ctypes as C

import numpy as np
import pytest
import torch

from ipd_ref import U, band_counts, bound, mel_ipd_ref, user_matrix, worst_fraction


def _mel(m=80, f=257):
    from challenge_amd.frontend import mel_weight_matrix
    return mel_weight_matrix(m, f, 16000)


def _spec(rng, b=2, f=257, t=9):
    return (0.1 * rng.standard_normal((b, f, t, 4))).astype(np.float32)


def _cfg(name, *extra):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '2', '--batch_size', '2',
                         '--name', name, *extra])


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
def test_reference_properties():
    rng = np.random.default_rng(0)
    w = _mel()
    live = band_counts(w) > 0
    x = _spec(rng).astype(np.float64)
    # identical channels -> (1, 0)
    same = x.copy()
    same[..., 1], same[..., 3] = same[..., 0], same[..., 2]
    r = mel_ipd_ref(same, w)
    assert np.abs(r[:, live, :, 0] - 1).max() <= 1e-12 and np.abs(r[..., 1]).max() <= 1e-12
    # X1 = X0 e^{-i theta} -> (cos theta, sin theta)
    for theta in (0.3, -1.1, 2.5):
        rot = x.copy()
        x0 = x[..., 0] + 1j * x[..., 2]
        x1 = x0 * np.exp(-1j * theta)
        rot[..., 1], rot[..., 3] = x1.real, x1.imag
        r = mel_ipd_ref(rot, w)
        assert np.abs(r[:, live, :, 0] - np.cos(theta)).max() <= 1e-12
        assert np.abs(r[:, live, :, 1] - np.sin(theta)).max() <= 1e-12
    # swapping the channels flips sin only
    r = mel_ipd_ref(x, w)
    swapped = x[..., [1, 0, 3, 2]]
    rs = mel_ipd_ref(swapped, w)
    assert np.array_equal(rs[..., 0], r[..., 0]) and np.array_equal(rs[..., 1], -r[..., 1])
    # silence (a frame, a channel, everything) -> exact zeros
    quiet = x.copy()
    quiet[:, :, 3] = 0
    quiet[1, :, :, 1] = quiet[1, :, :, 3] = 0
    rq = mel_ipd_ref(quiet, w)
    assert not rq[:, :, 3].any() and not rq[1].any() and rq[0, live, 2].any()
    assert not mel_ipd_ref(np.zeros_like(x), w).any()
    # the length is a coherence: cos^2 + sin^2 <= 1, and a band without weights is (0, 0)
    assert ((r ** 2).sum(-1)).max() <= 1 + 1e-12
    assert not r[:, ~live].any()
    # a common positive scale cancels (FilterAugment's gains never reach these channels)
    assert np.abs(mel_ipd_ref(3.7 * x, w) - r).max() <= 1e-12


def _stft64(x, n_fft=512, hop=256):
    """Frames of a float64 signal under the periodic Hann window, no padding: [F, T] complex."""
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    n = 1 + (len(x) - n_fft) // hop
    frames = np.stack([x[i * hop:i * hop + n_fft] * win for i in range(n)], axis=1)
    return np.fft.rfft(frames, axis=0)


@pytest.mark.parametrize("d", [1, 3])
def test_delayed_channel_reads_the_delay(d):
    """Channel 1 = channel 0 (white noise, 1 s at 16 kHz) delayed by d samples, n_fft 512: bin k then holds the phase
    difference +2 pi k d / 512 (X0 conj X1 with X1 = X0 e^{-i 2 pi k d / N}: a LATER channel 1 gives a POSITIVE angle - the sign
    convention), and band m the a_k-weighted mean of (cos, sin) of those angles - up to the frame-edge effect of the delay (d
    samples enter and leave the window; a band that is quiet in a frame - one or two bins at the low end - takes that effect
    at full size, so the MAXIMUM is large while the MEAN is small).
    Measured here with the reference, float64, seed 0, over 80 bands x 61 frames x (cos, sin):
        d = 1: max |deviation| 9.45e-2 (band 7), mean 1.93e-3;   d = 3: max 6.90e-1 (band 4), mean 6.23e-3.
    Asserted: twice the measured maximum, and - the sharper check - twice the measured mean."""
    max_measured, mean_measured = {1: (9.45e-2, 1.93e-3), 3: (6.90e-1, 6.23e-3)}[d]
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(16000 + d)
    x0, x1 = noise[d:], noise[:-d]            # x1[n] = x0[n - d]
    s0, s1 = _stft64(x0), _stft64(x1)
    spec = np.stack([s0.real, s1.real, s0.imag, s1.imag], axis=-1)[None]
    w = _mel().astype(np.float64)
    got = mel_ipd_ref(spec, w)[0]              # [M, T, 2]
    a = np.abs(s0) * np.abs(s1)                # [F, T]
    ang = 2 * np.pi * np.arange(257) * d / 512
    den = w.T @ a + 1e-20
    want = np.stack([(w.T @ (a * np.cos(ang)[:, None])) / den, (w.T @ (a * np.sin(ang)[:, None])) / den], axis=-1)
    dev = np.abs(got - want)
    print(f"d = {d}: max deviation {dev.max():.3e}, mean {dev.mean():.3e}")
    assert dev.max() <= 2 * max_measured
    assert dev.mean() <= 2 * mean_measured
    low = band_counts(w) > 0
    assert (got[low][:8, :, 1].mean(axis=1) > 0).all()      # the lowest bands: small POSITIVE angles (the sign convention)


# ---------------------------------------------------------------------------
# the torch restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("f,m,user", [(257, 80, False), (129, 64, False), (257, 80, True), (129, 64, True)])
def test_torch_form_within_the_bound(f, m, user):
    """CPU fp32 `transforms.mel_ipd` against the float64 reference on the same fp32 spectrum: every element within
    (2 n_m + 16) u, with and without bands (a frequency band over a whole mel band, a time band, a band of size 0, bands on
    some samples only)."""
    from challenge_amd import transforms as T
    rng = np.random.default_rng(f + m + user)
    w = user_matrix(f, m) if user else _mel(m, f)
    x = _spec(rng, b=3, f=f, t=17)
    lo = int(np.flatnonzero(w[:, 5])[0])
    n5 = int(np.flatnonzero(w[:, 5])[-1]) - lo + 1
    fb = np.array([[[lo, n5], [0, 0]], [[0, 0], [0, 0]], [[3, 2], [f - 4, 4]]], np.int32)
    tb = np.array([[[2, 3]], [[0, 0]], [[16, 1]]], np.int32)
    for kw in ({}, {"t_bands": tb}, {"f_bands": fb}, {"t_bands": tb, "f_bands": fb}):
        got = T.mel_ipd(torch.from_numpy(x), w, **kw)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, m, 17, 2)
        ref = mel_ipd_ref(x, w, **kw)
        frac = worst_fraction(got.numpy(), ref, w)
        print(f"F {f} M {m} user {user} {sorted(kw)}: worst fraction of the bound {frac:.3f}")
        assert frac <= 1.0
        if "f_bands" in kw:
            assert not got[0, 5].any()                    # the whole band masked: exact zeros
        if "t_bands" in kw:
            assert not got[0, :, 2:5].any() and not got[2, :, 16].any() and got[1].any()
    if user:
        got = T.mel_ipd(torch.from_numpy(x), w)
        assert not got[:, 2].any()                        # the all-zero band: den = 0 -> exactly (0, 0)
    assert float(bound(w).max()) == (2 * band_counts(w).max() + 16) * U
    # [F, T, 4] in, [M, T, 2] out; a mono or magnitude-phase shaped input is refused
    assert torch.equal(T.mel_ipd(torch.from_numpy(x[0]), w), T.mel_ipd(torch.from_numpy(x), w)[0])
    with pytest.raises(ValueError):
        T.mel_ipd(torch.from_numpy(x[..., :2]), w)
    with pytest.raises(ValueError):
        T.mel_ipd(torch.from_numpy(x[:, :-1]), w)


# ---------------------------------------------------------------------------
# the token
# ---------------------------------------------------------------------------
def test_token_and_input_channels():
    from challenge_amd import data_utils as D
    wants = lambda name: D.run_tokens(name).ipd  # noqa: E731
    assert wants("run_ipd") and wants("ipd_filter_pcen") and not wants("run_filter_pcen_learn") and not wants("")
    assert wants("skipdrop") and not wants(None) and not D.run_tokens(type("NoName", (), {"n_chan": 2})()).ipd
    assert D.model_in_channels(_cfg("ipd")) == 4 and D.model_in_channels(_cfg("run")) == 2
    assert D.model_in_channels(_cfg("run", "--n_chan", "1")) == 1
    assert D.run_tokens(_cfg("ipd_pcen_filter_filtaug_reverb_shoebox")).ipd     # goes with every other token
    assert not D.run_tokens(_cfg("pcen_learn", "--n_chan", "1")).ipd             # no token: nothing to refuse


def test_which_builder_honours_which_token():
    """Every (builder, single token) pair of the refusal table is accepted or refused as stated here.  The grid was recorded
    from the three builders while each still held its own chain of refusals, not read off the table."""
    from challenge_amd import data_utils as D
    from challenge_amd import sj_train as S
    tokens = ('stretch', 'speed', 'reverb', 'filtaug', 'ipd')
    honoured = {'make_dataset':        (False, False, False, False, False),      # noqa: E241
                'make_device_dataset': (True,  False, False, True,  True),       # noqa: E241
                'make_wave_dataset':   (False, True,  True,  True,  True)}       # noqa: E241
    assert set(D.BUILDER_REFUSALS) == set(honoured)
    for builder, row in D.BUILDER_REFUSALS.items():
        assert tuple(row) == tokens
        for token, want in zip(row, honoured[builder]):
            cfg = _cfg("run_" + token)
            assert getattr(D.run_tokens(cfg), token)
            if want:
                D.check_builder(D.run_tokens(cfg), builder)
            else:
                with pytest.raises(ValueError, match=f"asks for '{token}'"):
                    D.check_builder(D.run_tokens(cfg), builder)
            # ... and the builder itself: a refusal is that ValueError, raised before any corpus or device is touched; an
            # honoured token gets past it (to a dataset on a GPU, to the mixer's demand for one without)
            if builder == 'make_wave_dataset':
                sources = S.synthetic_wave_sources(2, 3, n_bg=1, n_voice=2, n_noise=1)
            else:
                sources = S.synthetic_sources(2, 3, n_bg=1, n_voice=2, n_noise=1)
            try:
                getattr(S, builder)(cfg, training=True, sources=sources)
                refused = False
            except ValueError as exc:
                refused = f"asks for '{token}'" in str(exc)
            except RuntimeError:
                refused = False
            assert refused == (not want), (builder, token)


def test_refusals():
    from challenge_amd import sj_train as S
    for make in (S.make_device_dataset, S.make_wave_dataset):
        for chan in ("1", "3", "4"):
            with pytest.raises(ValueError, match="n_chan must be 2"):
                make(_cfg("ipd", "--n_chan", chan))
        with pytest.raises(ValueError, match="pcen_learn"):
            make(_cfg("ipd_pcen_learn"))
    with pytest.raises(ValueError, match="per-sample"):
        S.make_dataset(_cfg("ipd"), sources=S.synthetic_sources(2, 3, n_bg=1, n_voice=1, n_noise=1))
    with pytest.raises(ValueError, match="pcen_learn"):
        S.get_model(_cfg("ipd_pcen_learn"))


def test_c_abi_refuses_null_and_empty_before_any_launch():
    from challenge_amd import _native as N
    lib = N.lib()
    fake = C.c_void_p(64)
    assert lib.iris_spec_ipd(None, fake, fake, 2, 10, 0, None, 0, None, 0, None) == -1
    assert lib.iris_spec_ipd(fake, None, fake, 2, 10, 0, None, 0, None, 0, None) == -1
    assert lib.iris_spec_ipd(fake, fake, None, 2, 10, 0, None, 0, None, 0, None) == -1
    assert lib.iris_spec_ipd(fake, fake, fake, 0, 10, 0, None, 0, None, 0, None) == -1
    assert lib.iris_spec_ipd(fake, fake, fake, 2, -1, 0, None, 0, None, 0, None) == -1
    assert lib.iris_last_error().startswith(b"iris_spec_ipd:")


def test_features_for_eval_appends_two_channels(monkeypatch):
    """The wiring of `inference.features_for_eval` on the host: the stages that exist only as HIP kernels are replaced by torch
    stand-ins here (the GPU suite runs the real ones); with the token the result is [M, T, 4], its first two channels bitwise
    those without the token, its last two `mel_ipd` of the filtered spectrum."""
    from challenge_amd import data_utils as D
    from challenge_amd import inference as I
    from challenge_amd import transforms as T

    def to_mel_factory(n_mels, n_bins, *a, **k):
        w = _mel(n_mels, n_bins)

        def to_mel(x):
            return torch.einsum('ftc,fm->mtc', x[..., :x.shape[-1] // 2], torch.from_numpy(w))
        to_mel.mel_matrix = w
        return to_mel

    def magphase(x, y=None):
        c = x.shape[-1] // 2
        return torch.cat([torch.sqrt(x[..., :c] ** 2 + x[..., c:] ** 2), torch.atan2(x[..., c:], x[..., :c])], dim=-1)

    def minmax(x, y=None):
        mn, mx = x.amin(dim=(1, 2), keepdim=True), x.amax(dim=(1, 2), keepdim=True)
        return (x - mn) / (mx - mn).clamp_min(1e-8)

    monkeypatch.setattr(T, "magphase_to_mel", to_mel_factory)
    monkeypatch.setattr(T, "complex_to_magphase", magphase)
    monkeypatch.setattr(D, "minmax", minmax)
    monkeypatch.setattr(D, "log_on_mel", lambda mel, labels=None: torch.log(mel + 1e-8))
    spec = torch.from_numpy(_spec(np.random.default_rng(5), b=1, f=257, t=70)[0])
    plain = I.features_for_eval(spec, _cfg("run"))
    feats = I.features_for_eval(spec, _cfg("run_ipd"))
    assert tuple(plain.shape) == (32, 70, 2) and tuple(feats.shape) == (32, 70, 4)
    assert torch.equal(feats[..., :2], plain)
    filtered = spec.clone()
    filtered[1:17] = 0
    assert torch.equal(feats[..., 2:], T.mel_ipd(filtered, _mel(32, 257)))
    assert float(feats[..., 2:].abs().max()) <= 1 + 1e-6
    with pytest.raises(ValueError):
        I.features_for_eval(spec, _cfg("ipd", "--n_chan", "1"))
    with pytest.raises(ValueError):
        I.features_for_eval(spec[..., [0, 2]], _cfg("ipd"))       # a mono recording


def test_model_first_layer_and_keras_import():
    from challenge_amd import model as M
    from challenge_amd import sj_train as S
    torch.manual_seed(0)
    m4, m2 = S.get_model(_cfg("run_ipd")), S.get_model(_cfg("run"))
    c4, c2 = m4.features[0].convs[0][0], m2.features[0].convs[0][0]
    assert c4.in_channels == 4 and tuple(c4.weight.shape) == (32, 4, 3, 3) and c2.in_channels == 2
    m4.eval()
    with torch.no_grad():
        assert tuple(m4(torch.randn(2, 32, 64, 4)).shape) == (2, 2, 3)
    # a 2-channel checkpoint is refused by the first kernel's shape check, loudly: nothing is broadcast
    rng = np.random.default_rng(0)
    weights2 = [rng.standard_normal(s).astype(np.float32) for s in M.keras_weight_shapes(m2)]
    before = c4.weight.detach().clone()
    with pytest.raises(ValueError, match=r"\(3, 3, 4, 32\)"):
        M.load_keras_weights(m4, weights2)
    assert torch.equal(c4.weight, before)
    M.load_keras_weights(m2, weights2)                              # the same arrays fit the 2-channel model
    weights4 = [rng.standard_normal(s).astype(np.float32) for s in M.keras_weight_shapes(m4)]
    assert weights4[0].shape == (3, 3, 4, 32)
    M.load_keras_weights(m4, weights4)


def test_run_name_round_trips():
    from challenge_amd import data_utils as D
    from challenge_amd import eval as E
    from challenge_amd import fit as F
    for name in ("ipd", "run_ipd", "ipd_filter_pcen"):
        cfg = _cfg(name, "--n_mels", "40", "--n_frame", "128")
        full = F.run_name(cfg)[:-len('.h5')]      # (eval is given the name without the checkpoint suffix)
        assert D.run_tokens(full).ipd
        back = _cfg(full, "--n_mels", "80", "--n_frame", "512", "--n_chan", "1")
        back = E.parse_name(back)
        assert (back.v, back.n_mels, back.n_chan, back.n_frame) == (9, 40, 2, 128)
        assert D.model_in_channels(back) == 4
        assert D.run_tokens(back).ipd
