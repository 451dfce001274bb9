"""Drop-in counterpart of the reference's data_utils.py on torch tensors
(data_utils.py:9-148).  `load_wav`'s numeric tail (normalize + STFT), `minmax`,
`log_on_mel` and `augment` are the STFT and log ends of the hot path and run as HIP
kernels (ROCm device tensors, no CPU fallback); the channel / label helpers are cheap
device-agnostic torch glue."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import frontend as _fe
from . import transforms as _tr
from .transforms import mask
from .utils import EPSILON, safe_div  # noqa: F401

_SR = 16000


def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("load_wav needs a ROCm GPU: the STFT runs as a HIP kernel (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def read_wav_file(wav_fname: str):
    """[chan, samples] float32 in [-1, 1) and the sample rate, from a PCM / float WAV
    (the role of torchaudio.load in data_utils.py:19)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(wav_fname)
    if data.ndim == 1:
        data = data[:, None]
    if data.dtype == np.int16:
        data = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    return np.ascontiguousarray(data.T), int(sr)


def stft_array(wav: torch.Tensor, n_fft: int = 512, normalize: bool = False) -> torch.Tensor:
    """Spectrogram(n_fft, power=None) of wav [chan, samples] on a ROCm device, in the
    reference layout [freq, time, chan*2] (re block, im block) (data_utils.py:17-27); `normalize` folds
    data_utils.py:22-23's wav / (10 rms) into the transform (no normalised copy of the waveform)."""
    if wav.dim() != 2:
        raise ValueError("wav must be [chan, samples]")
    plan = _fe.get_plan(wav.device, n_fft, None, 80, _SR, int(wav.shape[0]), 1, int(wav.shape[1]))
    return plan.stft(wav.unsqueeze(0), normalize=normalize)[0]


def load_wav_array(wav, sample_rate: int = _SR, device=None) -> torch.Tensor:
    """The numeric part of load_wav on an in-memory [chan, samples] array."""
    device = _default_device() if device is None else torch.device(device)
    wav = torch.as_tensor(np.asarray(wav, dtype=np.float32) if not isinstance(wav, torch.Tensor) else wav)
    wav = wav.to(device=device, dtype=torch.float32)
    if sample_rate != _SR:   # data_utils.py:20-21: kaldi.resample_waveform(wav, r, 16000), on the device (iris_resample)
        wav = _fe.resample(wav, int(sample_rate), _SR)
    # normalize + STFT as ONE transform launch behind a partial-sums launch (iris_stft with IRIS_F_NORMALIZE): the
    # two-kernel iris_normalize pass over the waveform cost as much as the transform itself.  Equal to
    # stft_array(normalize(wav)) up to the fp32 rounding of the scaled samples (<= 2e-6 of the spectrum's peak)
    return stft_array(wav, 512, normalize=True)


def load_wav(wav_fname: str, device=None) -> torch.Tensor:
    """complex spectrogram [freq, time, chan*2] of a wav file (data_utils.py:9-29)."""
    data, sr = read_wav_file(wav_fname)
    return load_wav_array(data, sr, device)


def resample_waveform(wav: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """torchaudio.compliance.kaldi.resample_waveform as load_wav calls it (data_utils.py:20-21), on a ROCm device tensor."""
    return _fe.resample(wav, orig_freq, new_freq)


def normalize(wav: torch.Tensor) -> torch.Tensor:
    """wav / (10 * rms) with the rms over all channels jointly (data_utils.py:32-34)."""
    if wav.is_cuda:
        return _fe.normalize(wav)
    rms = torch.sqrt(torch.mean(torch.pow(wav, 2))) * 10
    return wav / rms


def minmax(x: torch.Tensor, y=None):
    """(x - min) / max(max - min, EPSILON) over every axis except 0 (data_utils.py:37-47)."""
    x = _fe.minmax_log(x, do_minmax=True, do_log=False)
    if y is not None:
        return x, y
    return x


def log_on_mel(mel: torch.Tensor, labels=None):
    """ln(mel + EPSILON) (data_utils.py:50-55)."""
    mel = _fe.minmax_log(mel, do_minmax=False, do_log=True)
    if labels is not None:
        return mel, labels
    return mel


def minmax_log_on_mel(mel: torch.Tensor, labels=None):
    """minmax + log in one kernel pass (trainer.py:63-77, eval.py:13-27)."""
    mel = _fe.minmax_log(mel, do_minmax=True, do_log=True)
    if labels is not None:
        return mel, labels
    return mel


def pcen_on_mel(mel: torch.Tensor, labels=None, **params):
    """Per-channel energy normalisation (`frontend.pcen`, one HIP launch) in place of min-max + log, with the calling
    convention of `minmax_log_on_mel` (it drops into `Dataset.map`); `params` are `frontend.pcen`'s (smooth, gain, bias,
    power, eps, time_axis).  PCEN runs along time over whatever the tensor holds, so where it is applied matters:
    training applies it per clip of n_frame (512) frames - the smoother starts afresh on every clip - while evaluation
    (`inference.features_for_eval`) applies it over the whole recording before it is cut into windows, as the reference
    does with min-max.  A window seen in evaluation therefore carries the smoother state of the audio before it; the
    same window seen in training does not."""
    mel = _fe.pcen(mel, **params)
    if labels is not None:
        return mel, labels
    return mel


@dataclass(frozen=True)
class RunTokens:
    """What a run name asks for, by the tokens in it (the reference's idiom for 'filter' / 'nominmax': a substring test, so
    'pcen' is found inside 'pcen_learn', 'filter' is not found inside 'filtaug', and a name such as 'skipdrop' holds 'ipd').
    `run_tokens` is the one parse; `check_builder` tells which dataset builder of sj_train honours what.

    compression: the stage behind the mel features - 'minmax_log' (the default), 'log' ('nominmax': log_on_mel alone), 'pcen'
        (pcen_on_mel, fixed parameters) or 'pcen_learn' (no stage: the datasets yield raw mel magnitudes and the model's own
        trainable `model.PCEN` layer follows).  'pcen' with 'nominmax' is refused: PCEN replaces the whole min-max / log stage.
    filter: the reference's `stft_filter` - the bins 1..3 (200 Hz) of every training and validation spectrum are zeroed.
    stretch, speed, reverb: ONE augmentation of the voice corpus, on training sets, at creation and again every
        config.steps_per_epoch batches.  stretch: time-stretched by rates ~ U[0.8, 1.2) (`DeviceMixer.enable_stretch` /
        `restretch`, one `iris_phase_vocoder` launch over the corpus).  speed: speed-perturbed by rates ~ U[0.9, 1.1)
        (`WaveMixer.enable_speed` / `respeed`: one `iris_speed_perturb` and one `iris_mix_wave_frame_active_batch` launch).
        reverb: convolved with fresh synthetic room impulse responses, rt60 ~ U[0.1, 0.4) s, direct-to-reverberant ratio ~
        U[-3, 12) dB (`WaveMixer.enable_reverb` / `rereverb`: one `iris_fir_batch` launch; the labels follow the dry voice).
    shoebox: the room model of a 'reverb' run - image-source simulations of random shoebox rooms that both channels share
        (`enable_reverb(model="shoebox")`: one `iris_ism_rir` and one `iris_fir_batch_pitch` launch per epoch, no tap upload),
        so the inter-channel delay and level of a voice are those of one room, instead of independent noise per channel.
        Refused without 'reverb': it only selects that augmentation's model.
    reverb_long: the 'reverb' run with long rooms ('reverb' is then true as well, as 'filtaug_linear' holds 'filtaug'): rt60 ~
        U[0.2, 1.0) s followed down to -40 dB without truncation - up to 10667 taps in [C, 16384] tap buffers - through the
        partitioned FFT convolution (`enable_reverb(rt60_lo=0.2, rt60_hi=1.0, max_taps=16384)`: one `iris_fft_fir_batch`
        launch pair per group of voices and epoch).  Refused with 'shoebox': the image-source kernel stops at 4096 taps.
    flyby: the fly-by augmentation of the voice corpus, on training sets of `make_wave_dataset`, at creation and again every
        config.steps_per_epoch batches - every voice as a moving microphone array hears it: one random level pass per voice
        (`transforms.draw_flyby`: altitude ~ U[5, 30) m, speed ~ U[0, 15) m/s, any heading, closest approach ~ U[0, 20) m at a
        time inside the voice, ground reflection ~ U[0, 0.6); choices, not measurements), per channel the time-varying delay of
        its microphone, the spreading level and one ground reflection (`WaveMixer.enable_flyby` / `reflyby`: one `iris_flyby`
        and one `iris_mix_wave_frame_active_batch` launch; the labels follow the delayed voice).  A mixer holds one voice
        augmentation: refused with 'speed' or 'reverb', and by the two other builders.  It goes with every other token, with
        recordings and with a corpus of wav files; validation sets, backgrounds and noises are never touched.
    filtaug: FilterAugment, None or the kind of its gain curve ('step'; 'linear' for 'filtaug_linear') - every training
        sample's mel magnitudes are multiplied by a fresh random piecewise gain curve over the mel bands inside the mel kernels,
        before any compression (`iris_magmel_gain`, `iris_wav_to_logmel_gain`: no extra launch, no extra pass; the draw is
        `iris_filter_draw` on the device, else `transforms.filter_augment_draw` on the host).  It touches neither the mixers
        nor the corpus, so it goes with every other token.
    ipd: the inter-channel phase features.  A FEATURE, not an augmentation: the batched datasets then yield [B, M, T, 4] on
        training and validation sets alike - channels 0-1 what they always were, channels 2-3 the (cos, sin) of the phase
        difference per mel band (`transforms.mel_ipd`, `FrontendPlan.ipd`) of the same mixed spectrum under the same
        SpecAugment / 'filter' bands, never min-maxed, logged, PCEN'd or gained (the definition is invariant to a band gain) -
        `inference.features_for_eval` appends the same two channels, and the model's first layer takes
        `model_in_channels(config)`.  Stereo only: n_chan must be 2 and the corpora stereo.  Refused with 'pcen_learn' (the
        trainable PCEN layer would have to skip the two phase channels); it goes with every other token.
    whiten: the spatially whitened energy channel, two-microphone noise nulling.  A FEATURE like 'ipd': the batched datasets
        append ONE channel, last (mel0, mel1, then the 'ipd' pair if named, then this one), on training and validation sets
        alike - ln(e + 1e-8) of the mel-band average e of x^H (R + d I)^-1 x (`transforms.mel_whiten`, `FrontendPlan.whiten`),
        with R the 2x2 inter-channel covariance of the clip's n_frame frames of the same mixed spectrum 'ipd' reads.  The
        batch's SpecAugment / 'filter' bands act on its output only (the covariance does not see them), and min-max, log,
        PCEN and the FilterAugment gain never touch it (the definition is invariant to a band gain).
        `inference.features_for_eval` appends the same channel with blocks of n_frame frames over the whole recording.
        Stereo only, refused with 'pcen_learn' (as 'ipd') and by `make_dataset`; it goes with every other token.
    A name without a token takes no code path of that token."""
    name: str
    compression: str
    filter: bool
    stretch: bool
    speed: bool
    reverb: bool
    shoebox: bool
    filtaug: Optional[str]
    ipd: bool
    reverb_long: bool = False
    flyby: bool = False
    whiten: bool = False


def run_tokens(config_or_name) -> RunTokens:
    """The tokens of a run name, given the name or a config (whose `name` may be missing or None).  Raises the refusals that
    the name alone decides and, given a config, 'ipd' or 'whiten' at n_chan != 2."""
    config = None if config_or_name is None or isinstance(config_or_name, str) else config_or_name
    name = (config_or_name if config is None else getattr(config, 'name', '')) or ''
    pcen, nominmax = 'pcen' in name, 'nominmax' in name
    if pcen and nominmax:
        raise ValueError(f"run name {name!r} asks for both 'pcen' and 'nominmax': PCEN replaces min-max + log, name one")
    tokens = RunTokens(
        name=name,
        compression='pcen_learn' if 'pcen_learn' in name else 'pcen' if pcen else 'log' if nominmax else 'minmax_log',
        filter='filter' in name, stretch='stretch' in name, speed='speed' in name, reverb='reverb' in name,
        shoebox='shoebox' in name,
        filtaug=('linear' if 'filtaug_linear' in name else 'step') if 'filtaug' in name else None,
        ipd='ipd' in name, reverb_long='reverb_long' in name, flyby='flyby' in name, whiten='whiten' in name)
    for other in ('speed', 'reverb'):
        if tokens.flyby and getattr(tokens, other):
            raise ValueError(f"run name {name!r} asks for both 'flyby' and {other!r}: the two cannot be combined yet (a mixer "
                             "holds one voice augmentation), name one")
    if tokens.reverb_long and tokens.shoebox:
        raise ValueError(f"run name {name!r} asks for both 'reverb_long' and 'shoebox': the image-source room model computes at "
                         "most 4096 taps, name one")
    if tokens.shoebox and not tokens.reverb:
        raise ValueError(f"run name {name!r} asks for 'shoebox' without 'reverb': the token selects the room model of the "
                         "reverberation augmentation, name both")
    if tokens.ipd and config is not None and config.n_chan != 2:
        raise ValueError(f"run name {name!r} asks for 'ipd' at n_chan = {config.n_chan}: the inter-channel phase difference is "
                         "that of a stereo pair, n_chan must be 2")
    if tokens.ipd and tokens.compression == 'pcen_learn':
        raise ValueError(f"run name {name!r} asks for both 'ipd' and 'pcen_learn': the trainable PCEN layer would have to skip "
                         "the two phase channels, which is not supported yet; name one (the fixed 'pcen' goes with 'ipd')")
    if tokens.whiten and config is not None and config.n_chan != 2:
        raise ValueError(f"run name {name!r} asks for 'whiten' at n_chan = {config.n_chan}: the inter-channel covariance is "
                         "that of a stereo pair, n_chan must be 2")
    if tokens.whiten and tokens.compression == 'pcen_learn':
        raise ValueError(f"run name {name!r} asks for both 'whiten' and 'pcen_learn': the trainable PCEN layer would have to skip "
                         "the whitened channel, which is not supported yet; name one (the fixed 'pcen' goes with 'whiten')")
    return tokens


# Which dataset builder of sj_train honours which token (None), and why the others refuse it
BUILDER_REFUSALS = {
    'make_dataset': {
        'stretch': "time stretching runs on the device-resident corpus (make_device_dataset); the per-sample host pipeline "
                   "does not stretch",
        'speed': "speed perturbation runs on the resident waveform corpus (make_wave_dataset); the per-sample host pipeline "
                 "does not resample",
        'reverb': "reverberation runs on the resident waveform corpus (make_wave_dataset); the per-sample host pipeline does "
                  "not convolve",
        'filtaug': "FilterAugment runs inside the batched mel kernels (make_device_dataset, make_wave_dataset); the per-sample "
                   "host pipeline has no gain stage",
        'ipd': "the inter-channel phase features are computed on whole batches (make_device_dataset, make_wave_dataset); the "
               "per-sample host pipeline has no such stage"},
    'make_device_dataset': {
        'stretch': None,
        'speed': "a spectrum corpus cannot be resampled in time (use make_wave_dataset; this path has 'stretch')",
        'reverb': "a spectrum corpus has no waveform to convolve (use make_wave_dataset; this path has 'stretch')",
        'filtaug': None,
        'ipd': None},
    'make_wave_dataset': {
        'stretch': "a waveform corpus has no spectra to stretch (use make_device_dataset)",
        'speed': None,
        'reverb': None,
        'filtaug': None,
        'ipd': None},
}


def check_builder(tokens: RunTokens, builder: str) -> None:
    """ValueError if `builder` (a key of BUILDER_REFUSALS) does not honour a token of the name, or - a mixer holds one voice
    augmentation - if the name asks it for both 'speed' and 'reverb'.  'whiten' is honoured by the two batched builders
    and refused by `make_dataset` here (the table keeps the rows it has); 'flyby' is honoured by `make_wave_dataset` alone, here
    as well."""
    for token, reason in BUILDER_REFUSALS[builder].items():
        if reason is not None and getattr(tokens, token):
            raise ValueError(f"run name {tokens.name!r} asks for {token!r}: {reason}")
    if tokens.whiten and builder == 'make_dataset':
        raise ValueError(f"run name {tokens.name!r} asks for 'whiten': the whitened channel is computed on whole batches "
                         "(make_device_dataset, make_wave_dataset); the per-sample host pipeline has no such stage")
    if tokens.flyby and builder != 'make_wave_dataset':
        raise ValueError(f"run name {tokens.name!r} asks for 'flyby': the fly-by runs on the resident waveform corpus "
                         f"(make_wave_dataset); " + ("the per-sample host pipeline has no such stage" if builder == 'make_dataset'
                                                     else "a spectrum corpus has no waveform to delay"))
    if tokens.speed and tokens.reverb:
        raise ValueError(f"run name {tokens.name!r} asks for both 'speed' and 'reverb': the two cannot be combined yet (a "
                         "mixer holds one voice augmentation), name one")


def feature_compression(name: str) -> str:
    """`run_tokens(name).compression`."""
    return run_tokens(name).compression


def model_in_channels(config) -> int:
    """Channels of the model's input: n_chan, plus the two (cos, sin) phase channels of an 'ipd' run name, plus the whitened
    energy channel of a 'whiten' one (in this order)."""
    tokens = run_tokens(config)
    return config.n_chan + 2 * tokens.ipd + tokens.whiten


class FilterAugmentDraw:
    """The FilterAugment gains of a batch, float32 [B, n_mel] on `device` (the paper's defaults: transforms.FILTAUG_*).
    device_draw=True: one `iris_filter_draw` launch (Philox keyed by `seed`, call counter in device memory: no host draw, no
    upload, replayable from a hipGraph) into a long-lived tensor that the next draw of the same shape overwrites; otherwise
    `transforms.filter_augment_draw` on the host from `rng`, evaluated by `filter_augment_gains` and uploaded."""

    def __init__(self, device, kind: str = "step", seed: int = 0, device_draw: bool = False,
                 rng: Optional[np.random.Generator] = None):
        if kind not in _tr.FILTAUG_KINDS:
            raise ValueError(f"FilterAugmentDraw: kind must be one of {_tr.FILTAUG_KINDS}, got {kind!r}")
        self.device, self.kind, self.device_draw = torch.device(device), kind, bool(device_draw)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rng = np.random.default_rng(seed) if rng is None else rng
        self.state = torch.zeros(1, dtype=torch.int64, device=self.device) if device_draw else None

    def __call__(self, batch: int, n_mel: int) -> torch.Tensor:
        if self.device_draw:
            return _fe.filter_draw(batch, n_mel, self.kind, seed=self.seed, state=self.state)[2]
        bounds, db, n_band = _tr.filter_augment_draw(self.rng, batch, n_mel, self.kind)
        return torch.from_numpy(_tr.filter_augment_gain_batch(bounds, db, n_band, n_mel, self.kind)).to(self.device)


def augment(specs: torch.Tensor, labels, time_axis: int = -2, freq_axis: int = -3):
    """6 time masks (< 24 frames) then 1 frequency mask (< 16 linear bins) on the complex
    spectrogram (data_utils.py:58-61)."""
    specs = mask(specs, axis=time_axis, max_mask_size=24, n_mask=6)
    specs = mask(specs, axis=freq_axis, max_mask_size=16)
    return specs, labels


def augment_draw(n_time: int, n_freq: int, rng: Optional[np.random.Generator] = None):
    """The random draws of `augment` for one sample: (t_bands [6, 2], f_bands [1, 2])."""
    return _tr.mask_draw(n_time, 24, 6, rng), _tr.mask_draw(n_freq, 16, 1, rng)


def augment_draw_batch(batch: int, n_time: int, n_freq: int, rng: Optional[np.random.Generator] = None):
    """The draws of `augment` for a whole batch, vectorised: (t_bands [B, 6, 2], f_bands [B, 1, 2])."""
    return _tr.mask_draw_batch(batch, n_time, 24, 6, rng), _tr.mask_draw_batch(batch, n_freq, 16, 1, rng)


class DeviceAugmentDraw:
    """The draws of `augment` (6 time masks up to 23 frames, 1 frequency mask up to 15 bins per sample, data_utils.py:58-61)
    made ON THE DEVICE by one small HIP kernel (`iris_augment_draw`: Philox keyed by `seed`, call counter in device
    memory): no host draw, no upload, replayable from a hipGraph.  Optional fixed `stft_filter` band (bins 1..k) appended
    to the frequency bands.  Returns long-lived int32 device tensors (t_bands [B, 6, 2], f_bands [B, 1 (+1), 2])."""

    def __init__(self, device, seed: int = 0, filter_bins: int = 0):
        from . import _native as N
        self._N, self.device = N, torch.device(device)
        N.lib()
        self.seed, self.filter_bins = int(seed) & 0xFFFFFFFFFFFFFFFF, int(filter_bins)
        self.state = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._bufs = {}

    def __call__(self, batch: int, n_time: int, n_freq: int):
        import ctypes as C
        key = (batch, n_time, n_freq)
        if key not in self._bufs:
            nf = 2 if self.filter_bins else 1
            tb = torch.zeros((batch, 6, 2), dtype=torch.int32, device=self.device)
            fb = torch.zeros((batch, nf, 2), dtype=torch.int32, device=self.device)
            if self.filter_bins:
                fb[:, 1, 0], fb[:, 1, 1] = 1, self.filter_bins
            self._bufs[key] = (tb, fb, torch.empty((batch, 1, 2), dtype=torch.int32, device=self.device))
        tb, fb, f1 = self._bufs[key]
        with torch.cuda.device(self.device):
            rc = self._N.lib().iris_augment_draw(batch, n_time, 6, 24, n_freq, 1, 16, self.seed, self.state.data_ptr(),
                                                 tb.data_ptr(), (f1 if self.filter_bins else fb).data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._N.check(rc, "iris_augment_draw")
        if self.filter_bins:
            fb[:, :1].copy_(f1)
        return tb, fb


def to_frame_labels(x, y):
    """[..., n_voices, n_frames, n_classes] -> [..., n_frames, n_classes] (data_utils.py:64-70)."""
    return x, torch.sum(y, dim=-3)


def mono_chan(x, y=None):
    """data_utils.py:73-76, quirks included: with labels it returns x[..., :1] + x[..., 1:]
    (a broadcast add, a true down-mix only for a 2-entry last axis); without labels it is
    the identity."""
    if y is not None:
        return x[..., :1] + x[..., 1:], y
    return x


def stereo_mono(x, y=None):
    """[re0, re1, re0+re1, im0, im1, im0+im1] (data_utils.py:79-82)."""
    out = torch.cat([x[..., :2], x[..., :1] + x[..., 1:2], x[..., 2:4], x[..., 2:3] + x[..., 3:4]], -1)
    if y is None:
        return out
    return out, y


def avg_pool1d_same(y: torch.Tensor, k: int) -> torch.Tensor:
    """Keras AveragePooling1D(k, k, padding='same') on [B, T, K]: the ragged tail window
    is averaged over its valid entries only."""
    yt = y.transpose(1, 2)
    out = torch.nn.functional.avg_pool1d(yt, k, k, ceil_mode=True, count_include_pad=False)
    return out.transpose(1, 2)


def label_downsample(resolution: int = 32, ref_batch_slice: bool = False):
    """Average-pool labels by `resolution`, threshold at 0.5 (data_utils.py:85-97).
    The reference's trailing `[:resolution]` slices the *batch* axis -- harmless while
    batch <= resolution (its default batch is 12) but it would drop rows at BASELINE's
    batch 64, so it is applied only with ref_batch_slice=True (documented deviation)."""
    def _down(y_):
        y_ = avg_pool1d_same(y_, resolution)
        y_ = (y_ >= 0.5).to(y_.dtype)
        return y_[:resolution] if ref_batch_slice else y_

    def _label_downsample(x, y):
        if isinstance(y, (list, tuple)):
            y = (_down(y[0]),) + tuple(y[1:])
        else:
            y = _down(y)
        return x, y
    return _label_downsample


def random_merge_aug_apply(x, number: int, factor):
    """Deterministic half of random_merge_aug (data_utils.py:106-115): `factor` [1, 1, number - 2] is the
    U(0.1, 0.9) draw.  Works on any device (torch slicing / arithmetic on the tensor's own device)."""
    chan = x.shape[-1] // 2
    if chan != 2:
        raise ValueError("This augment can be used in 2 channel audio")
    real, imag = x[..., :chan], x[..., chan:]
    k = number - chan
    factor = torch.as_tensor(factor, dtype=x.dtype, device=x.device)
    aug_real = factor * real[..., :1].repeat_interleave(k, -1) \
        + torch.sqrt(1 - factor) * real[..., 1:].repeat_interleave(k, -1)
    real = torch.cat([real, aug_real], -1)
    imag = torch.cat([imag, (imag[..., :1] + imag[..., 1:]).repeat_interleave(k, -1)], -1)
    return torch.cat([real, imag], -1)


def random_merge_aug(number: int):
    """Extra mixed channels from a 2-channel spectrogram (data_utils.py:100-117): draw + apply."""
    def _random_merge_aug(x, y=None):
        if x.shape[-1] // 2 != 2:
            raise ValueError("This augment can be used in 2 channel audio")
        factor = _tr.get_rng().uniform(0.1, 0.9, size=(1, 1, number - 2))
        out = random_merge_aug_apply(x, number, factor)
        if y is not None:
            return out, y
        return out
    return _random_merge_aug


def multiply_label(multiply_factor):
    def _multiply_label(x, y):
        return x, y * multiply_factor
    return _multiply_label


def stft_filter(filter_num: int):
    """Zero the bins 1..filter_num of axis 0 (data_utils.py:126-136)."""
    def _stft_filter(x, y=None):
        if x.is_cuda:
            x = _fe.mask_apply(x, 0, [[1, filter_num]])
        else:
            x = x.clone()
            x[1:1 + filter_num] = 0
        if y is None:
            return x
        return x, y
    return _stft_filter


def speech_enhancement_preprocess(x, y=None):
    """data_utils.py:139-148 (speech-enhancement model variant; kept for signature parity)."""
    x = x[1:, ..., :x.shape[-1] // 2]
    if y is None:
        return x
    y = (torch.sum(y[0], dim=-3), y[1][1:, ..., :x.shape[-1] // 2], y[2][1:, ..., :x.shape[-1] // 2])
    return x, y
