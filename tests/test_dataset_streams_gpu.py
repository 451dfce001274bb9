"""Which random stream each draw of a batch comes from, and that a batched dataset's batch is exactly the composition of its
parts: the mixer's batch (`seed`), the SpecAugment bands (`seed + 1`), the FilterAugment gains (`seed + 2`), the mel kernel,
PCEN and the phase channels - assembled here by hand and compared bitwise, on both batched builders, host and device draws."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAME, SEED = "run_ipd_pcen_filter_filtaug", 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _args(name):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--v', '9', '--n_mels', '40', '--n_frame', '64', '--n_chan', '2', '--batch_size', '2', '--max_voices', '4',
                         '--max_noises', '3', '--steps_per_epoch', '2', '--name', name])


@pytest.mark.parametrize("device_draw", [False, True])
@pytest.mark.parametrize("which", ["spectrum", "waveform"])
def test_first_batch_is_the_composition_of_its_parts(dev, which, device_draw):
    from challenge_amd import data_utils as D
    from challenge_amd import frontend as FE
    from challenge_amd import sj_train as S
    if which == "waveform":
        sources = S.synthetic_wave_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
        make = S.make_wave_dataset
    else:
        sources = S.synthetic_sources(2, 3, n_bg=3, n_voice=7, n_noise=4, seed=3)
        make = S.make_device_dataset

    def build(name):
        return make(_args(name), training=True, sources=sources, device=dev, seed=SEED, device_draw=device_draw)

    def first(name):
        x, y = next(iter(build(name)))
        torch.cuda.synchronize()
        return x.clone(), y.clone()

    x, y = first(NAME)
    assert tuple(x.shape) == (2, 40, 64, 4) and x.dtype == torch.float32
    assert torch.equal(y, first("run")[1])              # no token moves the mixer's stream: the labels of the plain name

    # the mixed batch: the mixer of a second construction (stream `seed`)
    mixed = build(NAME).mixer.mix(2)[0]
    # the bands: stream `seed + 1`, the 3-bin 'filter' band behind the SpecAugment frequency band
    if device_draw:
        tb, fb = D.DeviceAugmentDraw(dev, SEED + 1, 3)(2, 64, 257)
    else:
        tb, fb = D.augment_draw_batch(2, 64, 257, np.random.default_rng(SEED + 1))
        fb = np.concatenate([fb, np.tile(np.array([[[1, 3]]], np.int32), (2, 1, 1))], axis=1)
    assert tuple(tb.shape) == (2, 6, 2) and tuple(fb.shape) == (2, 2, 2)
    # the gains: stream `seed + 2`
    gain = D.FilterAugmentDraw(dev, 'step', SEED + 2, device_draw)(2, 40)
    assert tuple(gain.shape) == (2, 40) and not torch.equal(gain, torch.ones_like(gain))

    plan = FE.FrontendPlan(512, 256, 40, 16000, 2, 2, 63 * 256, dev)
    if which == "waveform":
        wav = mixed.contiguous()
        assert tuple(wav.shape) == (2, 2, 63 * 256)
        mel = plan.wav_to_logmel(wav, t_bands=tb, f_bands=fb, minmax=False, log=False, mel_gain=gain)
        spec = plan.stft(wav)
    else:
        spec = mixed
        mel = S.complex_to_mel(40, 257)(spec, None, t_bands=tb, f_bands=fb, mel_gain=gain)
    assert tuple(spec.shape) == (2, 257, 64, 4) and tuple(mel.shape) == (2, 40, 64, 2)
    want = torch.cat([FE.pcen(mel), plan.ipd(spec.float(), t_bands=tb, f_bands=fb)], dim=-1)
    torch.cuda.synchronize()
    assert torch.equal(x[..., 2:], want[..., 2:])       # the phase channels: the mixer's stream and the bands' stream
    assert torch.equal(x[..., :2], want[..., :2])       # the mel channels: those two and the gains' stream
    assert x[..., 2:].any() and (x[..., 2:].abs().sum(dim=(1, 3)) == 0).any()   # SpecAugment's time bands zero whole frames
