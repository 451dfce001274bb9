"""GPU tests of the shoebox room simulation (iris_ism_rir, csrc/k_ism.h): parity with the float64 image-source oracle of
tests/ism_ref.py under |h - ref| <= C_ISM u A_k + n_k 2^-33 on one ragged launch per channel count, the normalised form,
untouched tails, bit reproducibility, `WaveMixer.enable_reverb(model="shoebox")` / `rereverb`, the inter-channel lag of the
wet signal and the 'reverb shoebox' run name.

The accuracy tests print the ratio of every record, which belongs in DESIGN.md (K2s); it is not entered there yet: these tests
had not run on an MI355X when they were written."""
import numpy as np
import pytest
import torch

import ism_ref as R
from reverb_ref import fir_ref
from test_reverb_gpu import KW, _sources

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test collected without a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def refs():
    """The float64 references (h, A_k, n_k) of the ragged tables for C = 1, 2, 3, computed once."""
    return {chan: [R.ism_ref(**v) for v in R.cases(chan)] for chan in (1, 2, 3)}


def _arrays(cases):
    return dict(rooms=[v["room"] for v in cases], sources=[v["source"] for v in cases], mics=[v["mics"] for v in cases],
                betas=[v["beta"] for v in cases], n_taps=[v["n_taps"] for v in cases])


@pytest.mark.parametrize("chan", [1, 2, 3])
def test_ragged_launch_meets_the_rule(dev, refs, chan):
    from challenge_amd import frontend as FE
    cases = R.cases(chan)
    assert [v["n_taps"] for v in cases][:5] == [4096, 1, 8, 33, 257] and {v["beta"] for v in cases} >= {0.0, 0.9}
    outs = FE.shoebox_rir_batch(normalize=False, device=dev, **_arrays(cases))
    worst = 0.0
    for v, out, (h, A, n) in zip(cases, outs, refs[chan]):
        assert out.shape == (chan, v["n_taps"]) and out.dtype == torch.float32
        err = np.abs(out.cpu().numpy().astype(np.float64) - h)
        tol = R.rule(h, A, n)
        ratio = float(np.max(err[tol > 0] / tol[tol > 0])) if np.any(tol > 0) else 0.0
        print(f"k_ism_rir C = {chan}, K = {v['n_taps']}, beta = {v['beta']}: |h - ref| / (C_ISM u A_k + n_k 2^-33) <= {ratio:.4f}")
        worst = max(worst, ratio)
        assert np.all(err <= tol), (chan, v["n_taps"], ratio)
    print(f"k_ism_rir C = {chan}: worst ratio {worst:.4f}")
    # the nearest microphone's direct path is the unit tap at W, in every voice long enough to hold it
    for v, out in zip(cases, outs):
        if v["n_taps"] > R.W:
            assert abs(float(out[:, R.W].max()) - 1.0) <= 1e-6


def test_normalised_form_meets_its_rule(dev, refs):
    from challenge_amd import frontend as FE
    cases = R.cases(2)
    outs = FE.shoebox_rir_batch(normalize=True, device=dev, **_arrays(cases))
    for v, out, (h, A, n) in zip(cases, outs, refs[2]):
        g = R.gain(h)
        err = np.abs(out.cpu().numpy().astype(np.float64) - h * g)
        tol = (R.rule(h, A, n) + 4 * R.U * np.abs(h)) * g
        ratio = float(np.max(err[tol > 0] / tol[tol > 0])) if np.any(tol > 0) else 0.0
        print(f"k_ism_rir normalised K = {v['n_taps']}: ratio <= {ratio:.4f}, g = {g:.4f}")
        assert np.all(err <= tol), (v["n_taps"], ratio)
        if np.any(h != 0):   # white input keeps its mean power; the level difference between the channels is kept
            got = out.double().cpu().numpy()
            assert abs(np.mean(np.sum(got ** 2, axis=1)) - 1.0) < 1e-5
            e_ref = np.sum(h ** 2, axis=1)
            if np.all(e_ref > 0):
                assert np.allclose(np.sum(got ** 2, axis=1) / np.sum(got ** 2), e_ref / e_ref.sum(), rtol=1e-4)


def test_tails_survive_and_two_launches_give_equal_bits(dev):
    from challenge_amd import frontend as FE
    cases = R.cases(3)
    bufs = [torch.full((3, 4096), SENTINEL, device=dev) for _ in cases]
    a = FE.shoebox_rir_batch(out=bufs, normalize=True, **_arrays(cases))
    keep = [x.clone() for x in a]
    for v, buf, view in zip(cases, bufs, a):
        assert view.data_ptr() == buf.data_ptr() and view.shape == (3, v["n_taps"])
        assert bool((buf[:, v["n_taps"]:] == SENTINEL).all()) and bool((view != SENTINEL).all())
    b = FE.shoebox_rir_batch(normalize=True, device=dev, **_arrays(cases))      # a fresh buffer, rows max K apart
    c = FE.shoebox_rir_batch(out=bufs, normalize=True, **_arrays(cases))
    for x, y, z in zip(keep, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    one = FE.shoebox_rir_batch(normalize=True, device=dev, **_arrays(cases[:1]))[0]   # a record alone equals the record in the table
    assert torch.equal(one, keep[0])
    from challenge_amd import transforms as T
    h = T.shoebox_rir([3.1, 4.3, 2.6], [2.05, 3.12, 1.57], cases[0]["mics"], 0.2, dev)
    assert h.shape == (3, T.shoebox_taps(0.2)) and bool(torch.isfinite(h).all())
    with pytest.raises(ValueError, match="n_taps"):
        FE.shoebox_rir_batch(out=[torch.zeros((3, 100), device=dev)] * len(cases), **_arrays(cases))


def test_wave_mixer_shoebox_is_the_identity_until_the_first_rereverb(dev):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()
    plain = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    mixer.enable_reverb(model="shoebox")
    assert mixer._aug.model == "shoebox" and mixer._aug.geometry is None
    draws = plain.draw(16)
    (wa, la), (wb, lb) = plain.mix(16, draws), mixer.mix(16, draws)
    assert torch.equal(wa, wb) and torch.equal(la, lb) and float(la.sum()) > 0
    with pytest.raises(ValueError, match="bogus"):
        plain.enable_reverb(model="bogus")


def test_wave_mixer_shoebox_rereverb_equals_fir_of_the_oracle_response(dev):
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = _sources()
    mixer = WaveMixer(backgrounds, voices, labels, noises, seed=21, device=dev, **KW)
    acts = [a.clone() for a in mixer.voice_active]
    L0, T0 = mixer._v_L.copy(), mixer._v_T.copy()
    mixer.enable_reverb(rt60_lo=0.02, rt60_hi=0.06, model="shoebox")      # short rooms: the oracle stays quick
    ptrs, tap_ptrs = mixer._v_ptr.copy(), [t.data_ptr() for t in mixer._aug.taps]
    used = mixer.rereverb()
    first = [v.clone() for v in mixer.voices]
    geo = mixer._aug.geometry
    assert len(used) == len(geo) == 6 and all(0.02 <= g["rt60"] < 0.06 for g in geo)
    for i, (v, g, h_dev, out) in enumerate(zip(voices, geo, used, mixer.voices)):
        k = g["n_taps"]
        assert h_dev.shape == (2, k) and h_dev.data_ptr() == tap_ptrs[i] and out.shape == v.shape
        h, A, n = R.ism_ref(g["room"], g["source"], g["mics"], g["beta"], k)
        gn = R.gain(h)
        tap_tol = (R.rule(h, A, n) + 4 * R.U * np.abs(h)) * gn
        got_h = h_dev.cpu().numpy()
        assert np.all(np.abs(got_h.astype(np.float64) - h * gn) <= tap_tol), i
        # the convolution: iris_fir_batch's own bound on the kernel's taps, plus the tap bound pushed through it
        y_ref, _ = fir_ref(v, h * gn)
        _, s_abs = fir_ref(v, got_h)
        pushed, _ = fir_ref(np.abs(v), tap_tol)
        err = np.abs(out.cpu().numpy().astype(np.float64) - y_ref)
        tol = (k + 2) * R.U * s_abs + pushed
        print(f"shoebox rereverb voice {i}: K = {k}, worst |y - ref| / tol = {float(np.max(err / np.maximum(tol, 1e-300))):.4f}")
        assert np.all(err <= tol), i
    assert np.array_equal(mixer._v_L, L0) and np.array_equal(mixer._v_T, T0) and np.array_equal(mixer._v_ptr, ptrs)
    assert all(torch.equal(a, b) for a, b in zip(mixer.voice_active, acts))
    mixer.rereverb()          # fresh rooms: new contents behind the same addresses
    assert np.array_equal(mixer._v_ptr, ptrs) and [v.data_ptr() for v in mixer.voices] == list(ptrs)
    assert not any(torch.equal(a, b) for a, b in zip(first, mixer.voices))
    assert mixer._aug.geometry is not geo and [t.data_ptr() for t in mixer._aug.taps] == tap_ptrs
    # given responses keep working in this model
    given = [np.ones((2, 1), np.float32)] * 6
    mixer.rereverb(given)
    assert all(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(mixer.voices, voices))


def test_two_microphones_keep_the_lag_of_the_geometry(dev):
    from challenge_amd import transforms as T
    room, mics = [5.0, 4.0, 3.0], np.array([[2.45, 2.0, 1.5], [2.55, 2.0, 1.5]])
    source = [3.5, 2.0, 1.5]                                   # 1 m to the side of the array centre, on its axis
    want = (1.05 - 0.95) * 16000 / R.C_SOUND                   # 4.66 samples: channel 0 is later
    h = T.shoebox_rir(room, source, mics, 0.0, dev, n_taps=64, normalize=False)      # rt60 = 0: beta = 0
    x = np.random.default_rng(0).standard_normal(4000).astype(np.float32)
    wet = T.reverb(torch.from_numpy(np.stack([x, x])).to(dev), h).double().cpu().numpy()
    lags = np.arange(-20, 21)
    xc = [np.dot(wet[0, 40:3900], wet[1, 40 - l:3900 - l]) for l in lags]
    assert abs(int(lags[int(np.argmax(xc))]) - want) <= 1.0, (lags[int(np.argmax(xc))], want)


def test_reverb_shoebox_run_name_in_make_wave_dataset(dev):
    from challenge_amd import sj_train as S
    args = ['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '6', '--max_voices', '4',
            '--max_noises', '3', '--steps_per_epoch', '2']
    sources = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
    ds = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb_shoebox']), training=True, sources=sources, device=dev, seed=4)
    aug = ds.mixer._aug
    assert aug.model == "shoebox" and len(aug.geometry) == 7 and all(h.is_cuda and h.shape[0] == 2 for h in aug.rirs)
    assert not any(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(ds.mixer.voices, sources[1]))
    it = iter(ds)
    for _ in range(3):
        bx, by = next(it)
        assert bx.shape == (6, 40, 64, 2) and by.shape == (6, 2, 3) and torch.isfinite(bx).all()
    noise = S.make_wave_dataset(S.ARGS().get(args + ['--name', 'run_reverb']), training=True, sources=sources, device=dev, seed=4)
    assert noise.mixer._aug.model == "noise" and noise.mixer._aug.geometry is None and not torch.is_tensor(noise.mixer._aug.rirs[0])
