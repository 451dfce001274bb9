"""Drop-in counterpart of the reference's sj_train.py for the VAD CNN/CRNN path
(sj_train.py:20-255, :402-529): same flags, `make_dataset`, `custom_scheduler`,
`adaptive_clip_grad`, `CustomModel.train_step`, `define_keras_model`, `get_model`,
`main`.  The model is a torch nn.Module on PyTorch-ROCm (MIOpen / hipBLASLt -- not
hand-written, per the north star); the feature frontend feeding it is the HIP library.
Data parallelism (absent in the reference) is one process per GPU with
torch.distributed over RCCL: DistributedDataParallel all-reduces the gradients in
buckets overlapped with backward; AGC and clipvalue then act on the averaged gradients,
identically on every rank.

Out of scope here: model_type 'eff' / 'se' branches
(sj_train.py:258-401).  The training metrics and the challenge score are challenge_amd.metrics
(`--metrics reference` compiles the reference's list, sj_train.py:454-457)."""
from __future__ import annotations

import argparse
import csv
import functools
import math
import os
import time
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn as nn

from . import data_utils as _du
from . import frontend as _fe
from . import transforms as _tr
from .data_utils import (augment, label_downsample, log_on_mel, minmax, mono_chan, multiply_label,  # noqa: F401
                         random_merge_aug, stereo_mono, stft_filter, to_frame_labels)
from .dataset import AUTOTUNE, Dataset
from .pipeline import make_pipeline
from .transforms import complex_to_magphase, magphase_to_mel
from .utils import label_downsample_model, load_data, sigmoid_focal_crossentropy, unitwise_norm


def _curve_bins(text):
    """--curves: 0 (off) or a bin count the score histogram takes."""
    from .metrics import check_curve_bins
    try:
        bins = int(text)
        return bins if bins == 0 else check_curve_bins(bins)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


def _sed_thresholds(text):
    """--sed_eval: '' (off) or a comma list of strictly increasing thresholds metrics.sed_eval takes."""
    from .metrics import check_sed_params
    if not text.strip():
        return ()
    try:
        return check_sed_params(tuple(float(h) for h in text.split(',')))[0]
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


def output_hop(config) -> int:
    """Samples per OUTPUT frame of the model: the STFT hop of 256 times the label down-sampling of its version (make_dataset)."""
    if config.v in label_downsample_model:
        return 256 * 32
    if config.v == 5:
        return 256 * (config.n_frame // (config.n_frame * 256 // 16000))
    return 256


def row_names(config) -> list:
    """The entries `main`'s `fit` rows hold besides epoch / lr / time for these flags: what --checkpoint_monitor may name."""
    names = ['loss']
    if getattr(config, 'metrics', 'none') == 'reference':
        names += ['cos_sim', 'f1_score'] + (['er'] if config.v != 5 else [])
    val = ['val_' + n for n in names]
    from .metrics import CURVE_NAMES, PSDS_NAMES, SED_NAMES
    for flag, added in (('curves', CURVE_NAMES), ('sed_eval', SED_NAMES), ('psds', PSDS_NAMES)):
        if getattr(config, flag, 0):
            val += ['val_' + n for n in added]
    ema = ['val_ema_' + n[len('val_'):] for n in val] if getattr(config, 'ema', 0) else []
    return names + val + ema


def count_metrics(config) -> list:
    """The compiled count metrics of --curves / --sed_eval / --psds, made anew at every call: the model and its EMA copy each
    compile a list of their own, so the EMA's validation pass never counts into the live model's states."""
    from .metrics import psds, score_curves, sed_eval
    hop = output_hop(config)
    return ([score_curves(config.curves)] if config.curves else []) \
        + ([sed_eval(config.sed_eval, hop=hop)] if config.sed_eval else []) \
        + ([psds(config.psds, hop=hop)] if config.psds else [])


class ARGS:
    """Same flags and defaults as sj_train.py:20-71, plus the knobs the reference has no
    equivalent for (synthetic data, device, distributed launch)."""

    def __init__(self, trainer_flags: bool = True) -> None:
        """trainer_flags=False: without the flags that only `main` here reads (--curves, --sed_eval, --psds, --checkpoint_monitor,
        --recordings*), for a tool that extends this parser with flags of its own (`eval`, whose --curves names a file)."""
        self.args = argparse.ArgumentParser()
        a = self.args.add_argument
        a('--name', type=str, default='')
        a('--gpus', type=str, default='-1')
        a('--model', type=int, default=0)
        a('--model_type', type=str, default='vad', choices=['vad', 'eff', 'se'])
        a('--v', type=int, default=1)
        a('--pretrain', type=bool, default=False)
        a('--n_layers', type=int, default=0)
        a('--n_dim', type=int, default=256)
        a('--n_chan', type=int, default=2)
        a('--n_classes', type=int, default=3)
        a('--patience', type=int, default=10)
        # DATA
        a('--mse_multiplier', type=int, default=1)
        a('--datapath', type=str, default='/root/datasets/Interspeech2020/generate_wavs/codes')
        a('--background_sounds', type=str, default='drone_normed_complex_v4.pickle')
        a('--voices', type=str, default='voice_normed_complex_v3.pickle')
        a('--labels', type=str, default='voice_labels_mfc_v3.npy')
        a('--noises', type=str, default='noises_specs_v2.pickle')
        a('--test_background_sounds', type=str, default='test_drone_normed_complex_v2.pickle')
        a('--test_voices', type=str, default='test_voice_normed_complex.pickle')
        a('--test_labels', type=str, default='test_voice_labels_mfc.npy')
        a('--n_mels', type=int, default=80)
        # TRAINING
        a('--optimizer', type=str, default='adam', choices=['adam', 'sgd', 'rmsprop', 'adabelief'])
        a('--lr', type=float, default=1e-3)
        a('--end_lr', type=float, default=1e-4)
        a('--lr_power', type=float, default=0.5)
        a('--lr_div', type=float, default=2)
        a('--clipvalue', type=float, default=0.01)
        a('--epochs', type=int, default=300)
        a('--batch_size', type=int, default=12)
        a('--n_frame', type=int, default=512)
        a('--steps_per_epoch', type=int, default=100)
        a('--l1', type=float, default=0)
        a('--l2', type=float, default=1e-6)
        a('--loss', type=str, default='BCE')
        # AUGMENTATION
        a('--snr', type=float, default=-20)
        a('--max_voices', type=int, default=7)
        a('--max_noises', type=int, default=2)
        # not in the reference
        a('--synthetic', action='store_true', help='synthetic sources instead of the pickled datasets')
        a('--online_stft', action='store_true',
          help='keep (synthetic) waveform corpora on the device, mix them before the STFT (WaveMixer) and run the '
               'fused HIP frontend on line instead of mixing pre-computed spectra (make_wave_dataset)')
        a('--wave_corpus', type=str, default='synthetic', choices=['synthetic', 'pickles', 'wavs'],
          help="--online_stft only.  'synthetic' (default): synthetic waveform corpora.  'pickles': the pickled SPECTRUM corpora "
               "(or their --synthetic stand-ins) are inverted to waveforms once at start-up (waves_from_specs: one iris_istft "
               "launch per corpus list) and mixed from there.  'wavs': folders of wav files under --corpus_dir "
               "(corpus.load_wav_corpus), the voices passed through the activity gate")
        a('--corpus_dir', type=str, default=None, metavar='ROOT',
          help="--online_stft --wave_corpus wavs only.  ROOT/train and ROOT/test each hold backgrounds/*.wav and voices/<class>/*.wav "
               "(classes 0, 1, 2); ROOT/train/noises/*.wav is optional and serves both.  Resampled to 16 kHz and scaled as load_wav "
               "scales a file.  Not part of the run name")
        a('--gate_range_db', type=float, default=40.0, metavar='DB',
          help='the activity gate of the voices of --corpus_dir (iris_activity_gate): a frame of 256 samples is speech when its '
               'energy is within DB of the loudest frame of its clip; the samples of the other frames become exact zeros, which is '
               'what the mixer labels as silence (default 40; a choice, not a measurement)')
        a('--gate_min_gap', type=int, default=12, metavar='FRAMES', help='pauses of up to FRAMES frames inside speech stay active (default 12)')
        a('--gate_min_event', type=int, default=6, metavar='FRAMES', help='bursts shorter than FRAMES frames are dropped (default 6)')
        a('--gate_hang', type=int, default=1, metavar='FRAMES', help='what is left is widened by FRAMES frames a side (default 1)')
        a('--no_gate', action='store_true', help='--corpus_dir holds voices that are already zeroed outside speech: do not gate them')
        a('--per_sample_pipeline', action='store_true',
          help='build samples one at a time with the tf.data-shaped graph (make_dataset) instead of the '
               'batched on-device synthesis (make_device_dataset), which is the default on a GPU')
        a('--host_draws', action='store_true',
          help='draw the random half of every batch (source choice, offsets, gains, SpecAugment bands) on the host and upload '
               'it, instead of on the device (iris_mix_draw / iris_augment_draw, the default on a GPU: no upload, so the '
               'host is never held behind the previous step)')
        a('--no_clipvalue_after_agc', action='store_true',
          help="skip Adam's element-wise clipvalue (TF < 2.4 behaviour of the custom train_step)")
        a('--validation_steps', type=int, default=16)
        a('--ema', type=float, default=0.0, metavar='DECAY',
          help='keep an exponential moving average of the weights, updated every step (inside the fused AGC + optimiser launch where that '
               'runs), validate it beside the live model (val_ema_* columns) and save the best as <name>_EMA.pt; 0 (default): off. '
               'Not part of the run name')
        a('--reset_bn', type=int, default=0, metavar='N',
          help='recompute the BatchNorm running statistics of the averaged models (<name>_SWA.pt, <name>_EMA.pt) from N training '
               'batches before they are written at the end of the run; 0 (default): off')
        a('--metrics', type=str, default='none', choices=['none', 'reference'],
          help="'reference': compile cos_sim, f1_score() and (v != 5) er_score(smoothing=False) as sj_train.py:454-457 does, "
               "checkpoint on val_er and score the checkpoint every 5 epochs against ./sample_answer.json and ./*.wav "
               "(metrics.eval_callback; the file must exist); 'none': loss only")

        if not trainer_flags:
            return
        a('--curves', type=_curve_bins, default=0, metavar='BINS',
          help='log the threshold-free validation numbers val_auc (macro ROC-AUC), val_map (macro average precision) and '
               'val_best_f1 (best frame F1 over thresholds) from an on-device score histogram with BINS bins (a power of two in '
               '[16, 4096]; metrics.score_curves, one more launch per validation batch); 0 (default): off.  Not part of the run name')
        a('--sed_eval', type=_sed_thresholds, default=(), metavar='THRESHOLDS',
          help='log the detection measures of sed_eval / DCASE on the validation pass - val_seg_f1, val_seg_er (1 s segments), '
               'val_event_f1 (200 ms onset collar, offset collar max(200 ms, 50 %% of the event)) at the FIRST threshold of this comma '
               'list of up to 16 increasing thresholds, e.g. 0.5 - from on-device integer counts (metrics.sed_eval, two more launches '
               'per validation batch); empty (default): off.  Not part of the run name')
        a('--psds', type=int, default=0, choices=[0, 1, 2], metavar='SCENARIO',
          help='log val_psds, the polyphonic sound detection score (Bilen et al. 2020) of the validation pass under DCASE scenario 1 '
               '(DTC / GTC 0.7, no cross-triggers) or 2 (DTC / GTC 0.1, CTTC 0.3, alpha_ct 0.5), alpha_st 1, over 50 thresholds - from '
               'on-device integer counts (metrics.psds, two more launches per validation batch); 0 (default): off.  Not part of the '
               'run name')
        a('--checkpoint_monitor', type=str, default=None, metavar='NAME',
          help="the row entry the checkpoint follows, e.g. val_map or val_event_f1 (auc / map / best_f1 / seg_f1 / event_f1 / psds are "
               "maximised, everything else minimised); default: val_er with --metrics reference, else val_loss")
        a('--recordings', type=str, default=None, metavar='DIR',
          help='--online_stft only.  Cut a share of every training batch from the labelled recordings DIR/*.wav '
               '(recordings.load_recordings: resampled to 16 kHz, scaled as load_wav scales a file) - random windows, drawn and '
               'gathered on the device (iris_crop_draw, iris_crop_windows), labelled from --recordings_answer; the rest of the '
               'batch is synthetic as before.  The validation set is unchanged.  Not part of the run name')
        a('--rirs', type=str, default=None, metavar='DIR',
          help="--online_stft only, with a 'reverb' token in --name.  Reverberate the training voices with the measured room "
               "impulse responses DIR/*.wav (transforms.load_rirs: resampled to 16 kHz, trimmed to the direct sound, cut at "
               "16384 taps = 1.024 s, unit norm) instead of synthetic ones: one drawn per voice and epoch, through the "
               "partitioned FFT convolution (iris_fft_fir_batch).  Refused with 'shoebox'.  Not part of the run name")
        a('--recordings_answer', type=str, default=None, metavar='FILE',
          help="the recordings' events: a JSON in sample_answer.json's schema whose 'task2_answer' has an entry per wav of "
               "--recordings (default: DIR/answer.json)")
        a('--recordings_share', type=float, default=0.5, metavar='S',
          help='the share of a batch cut from --recordings, in (0, 1]: max(1, round(S * batch_size)) windows; 1: no synthetic '
               'corpus is loaded at all (default 0.5)')

    def get(self, argv=None):
        config = self.args.parse_args(argv)
        monitor = getattr(config, 'checkpoint_monitor', None)
        if monitor is not None and monitor not in row_names(config):
            raise ValueError(f"--checkpoint_monitor {monitor!r}: the rows of this run will hold {row_names(config)}")
        if config.wave_corpus == 'wavs' or config.corpus_dir is not None:
            if config.corpus_dir is None:
                raise ValueError("--wave_corpus wavs needs --corpus_dir ROOT (ROOT/train and ROOT/test: backgrounds/*.wav, "
                                 "voices/<class>/*.wav)")
            if config.wave_corpus != 'wavs':
                raise ValueError(f"--corpus_dir {config.corpus_dir!r} is read by --wave_corpus wavs only (got --wave_corpus "
                                 f"{config.wave_corpus})")
            if not config.online_stft:
                raise ValueError("--wave_corpus wavs --corpus_dir mixes waveforms and needs the waveform path: add --online_stft")
            if not config.no_gate:   # (the gate's ranges, before any file is read)
                _fe.check_gate_settings(256, config.gate_range_db, 0.0, config.gate_min_gap, config.gate_min_event, config.gate_hang)
        if getattr(config, 'rirs', None) is not None:
            if not config.online_stft:
                raise ValueError("--rirs reverberates the waveform corpus and needs the waveform path: add --online_stft")
            tokens = _du.run_tokens(config)
            if not tokens.reverb:
                raise ValueError(f"--rirs needs a 'reverb' token in --name (got {tokens.name!r}): the responses feed that augmentation")
            if tokens.shoebox:
                raise ValueError(f"--rirs with 'shoebox' in --name {tokens.name!r}: measured responses replace the room model, name one")
        if getattr(config, 'recordings', None) is not None:
            if not config.online_stft:
                raise ValueError("--recordings cuts waveform windows and needs the waveform path: add --online_stft")
            if not 0.0 < config.recordings_share <= 1.0:
                raise ValueError(f"--recordings_share {config.recordings_share} is outside (0, 1]")
            if config.metrics == 'reference':
                from glob import glob
                scored = {os.path.realpath(p) for p in glob(os.path.join('.', '*.wav'))}
                both = sorted(p for p in glob(os.path.join(config.recordings, '*.wav')) if os.path.realpath(p) in scored)
                if both:
                    raise ValueError(f"--recordings {config.recordings!r} holds {both}, which --metrics reference scores every 5 "
                                     "epochs (./*.wav against ./sample_answer.json): fine-tuning on the scored files flatters val_er "
                                     "and test_er; train on other recordings or drop --metrics reference")
        return config


# ---------------------------------------------------------------------------
# dataset assembly                                            sj_train.py:74-130
# ---------------------------------------------------------------------------
RIR_MAX_TAPS = 16384   # tap buffers of a 'reverb_long' run and of --rirs: 1.024 s at 16 kHz (the longest synthetic response, rt60 = 1 s
                       # followed down to -40 dB, is 10667 taps)
def complex_to_mel(n_mels: int, num_spectrogram_bins: int = 257, sample_rate: float = 16000, **kwargs):
    """complex_to_magphase + magphase_to_mel as ONE kernel (sj_train.py:119-120 maps them
    one after the other; the phase computed by the first is discarded by the second)."""
    to_mel = magphase_to_mel(n_mels, num_spectrogram_bins, sample_rate, **kwargs)
    n_fft = 2 * (num_spectrogram_bins - 1)
    plans = {}

    def _complex_to_mel(x, y=None, t_bands=None, f_bands=None, mel_gain=None):
        """t_bands / f_bands ([B, n, 2] (offset, size), optional): SpecAugment / stft_filter bands
        zeroed in the complex spectrum first (== `augment` / `stft_filter` mapped before this stage).
        mel_gain ([B, n_mels], optional): FilterAugment gains, multiplied into the mel values by the kernel."""
        if not x.is_cuda or n_fft not in (256, 512, 1024, 2048):
            if mel_gain is not None:
                raise ValueError("complex_to_mel: mel_gain (FilterAugment) needs a ROCm tensor and n_fft 256 / 512 / 1024 / 2048")
            if t_bands is not None:
                x = _tr.mask_apply(x, -2, t_bands)
            if f_bands is not None:
                x = _tr.mask_apply(x, -3, f_bands)
            out = to_mel(complex_to_magphase(x))
        else:
            out = _plan(x).magmel(x.float(), is_magphase=False, t_bands=t_bands, f_bands=f_bands, mel_gain=mel_gain)
        return out if y is None else (out, y)

    def _plan(x):
        chan = x.shape[-1] // 2
        key = (x.device.index, chan)
        plan = plans.get(key)
        if plan is None or plan.max_batch < x.shape[0]:
            plan = _fe.FrontendPlan(n_fft, None, n_mels, sample_rate, chan, max(int(x.shape[0]), 1), n_fft,
                                    x.device, mel_matrix=to_mel.mel_matrix)
            plans[key] = plan
        return plan

    def _ipd(x, t_bands=None, f_bands=None):
        """The inter-channel phase channels [B, n_mels, T, 2] of the same stereo spectrum under the same bands and mel
        matrix (`transforms.mel_ipd`; on a ROCm tensor `FrontendPlan.ipd` of this closure's plan)."""
        if not x.is_cuda or n_fft not in (256, 512, 1024, 2048):
            return _tr.mel_ipd(x, to_mel.mel_matrix, t_bands, f_bands)
        return _plan(x).ipd(x.float(), t_bands=t_bands, f_bands=f_bands)

    def _whiten(x, block, t_bands=None, f_bands=None):
        """The whitened energy channel ln(e + 1e-8) [B, n_mels, T] of the same stereo spectrum with the same mel matrix, the
        bands acting on its output (`transforms.mel_whiten`; on a ROCm tensor `FrontendPlan.whiten` of this closure's plan)."""
        if not x.is_cuda or n_fft not in (256, 512, 1024, 2048):
            return _tr.mel_whiten(x, to_mel.mel_matrix, block, t_bands=t_bands, f_bands=f_bands)
        return _plan(x).whiten(x.float(), block, t_bands=t_bands, f_bands=f_bands)

    _complex_to_mel.ipd = _ipd
    _complex_to_mel.whiten = _whiten
    return _complex_to_mel


def synthetic_sources(n_chan: int = 2, n_classes: int = 3, freq: int = 257, n_bg: int = 8, n_voice: int = 24,
                      n_noise: int = 12, seed: int = 0):
    """Random stand-ins for the pickled datasets of sj_train.py:79-89: lists of
    [freq, t_i, 2*chan] float32 spectra and integer class labels."""
    rng = np.random.default_rng(seed)
    backgrounds = [rng.standard_normal((freq, int(rng.integers(300, 900)), 2 * n_chan)).astype(np.float32) * 0.1
                   for _ in range(n_bg)]
    voices = []
    for _ in range(n_voice):
        t = int(rng.integers(40, 200))
        v = np.abs(rng.standard_normal((freq, t, 2 * n_chan))).astype(np.float32)
        v[:, int(t * 0.8):] = 0  # trailing silence, as padded voices have
        voices.append(v)
    labels = rng.integers(0, n_classes, size=n_voice)
    noises = [rng.standard_normal((freq, int(rng.integers(20, 120)), 2 * n_chan)).astype(np.float32) * 0.3
              for _ in range(n_noise)]
    return backgrounds, voices, labels, noises


def _load_sources(config, training, n_classes, sources):
    """The pickled corpora of sj_train.py:79-89 (or `sources` / --synthetic stand-ins) with one-hot labels."""
    if sources is None and getattr(config, 'synthetic', False):
        sources = synthetic_sources(2, n_classes, seed=0 if training else 1)
    if sources is None:
        if not os.path.exists(config.datapath):
            config.datapath = ''
        if training:
            backgrounds = load_data(os.path.join(config.datapath, config.background_sounds))
            voices = load_data(os.path.join(config.datapath, config.voices))
            labels = load_data(os.path.join(config.datapath, config.labels))
        else:
            backgrounds = load_data(os.path.join(config.datapath, config.test_background_sounds))
            voices = load_data(os.path.join(config.datapath, config.test_voices))
            labels = load_data(os.path.join(config.datapath, config.test_labels))
        if labels.max() - 1 != config.n_classes:
            labels //= 10
        noises = load_data(os.path.join(config.datapath, config.noises))
    else:
        backgrounds, voices, labels, noises = sources
    labels = np.eye(n_classes, dtype='float32')[np.asarray(labels)]  # to one-hot vectors
    return backgrounds, voices, labels, noises


_FILTER_BINS = int(round(200 / (16000 / 256)))   # the band of a 'filter' run name: `stft_filter` zeroes the bins 1..3


def _compression_map(config):
    """The compression stage a run name selects, as a `(mel, labels=None)` map (None: 'pcen_learn', no stage - the raw mel
    magnitudes go to the model's trainable PCEN layer)."""
    return {'pcen_learn': None, 'pcen': _du.pcen_on_mel, 'minmax_log': _du.minmax_log_on_mel,   # (min-max + log: :121-123 fused)
            'log': log_on_mel}[_du.run_tokens(config).compression]


def _label_tail(pipeline, config, compressed=False):
    """The stages after the mel features (sj_train.py:121-129): the compression of `_compression_map`, then the labels'.
    `compressed`: a batched builder, whose generator has applied the compression itself."""
    compress = None if compressed else _compression_map(config)
    if compress is not None:
        pipeline = pipeline.map(compress)
    if config.v in label_downsample_model:
        pipeline = pipeline.map(label_downsample(32))
    elif config.v == 5:
        pipeline = pipeline.map(label_downsample(config.n_frame // (config.n_frame * 256 // 16000)))
    if config.loss.upper() in ('MSE', 'MAE'):
        pipeline = pipeline.map(multiply_label(config.mse_multiplier))
    return pipeline.prefetch(AUTOTUNE)


def make_dataset(config, training=True, n_classes=3, sources=None):
    """Stage order of sj_train.py:74-130.  `sources` = (backgrounds, voices, labels, noises)
    overrides the pickle files (used with --synthetic and by the tests)."""
    tokens = _du.run_tokens(config)
    _du.check_builder(tokens, 'make_dataset')
    backgrounds, voices, labels, noises = _load_sources(config, training, n_classes, sources)

    pipeline = make_pipeline(backgrounds, voices, labels, noises, n_frame=config.n_frame,
                             max_voices=config.max_voices, max_noises=config.max_noises, n_classes=n_classes,
                             snr=config.snr, min_ratio=1,
                             seperate_noise_voice=config.model_type == 'se' and config.v == 9)
    if config.model_type == 'se' and config.v == 9:
        raise NotImplementedError("model_type 'se' is outside the accelerated path (SURVEY.md section 2)")
    pipeline = pipeline.map(to_frame_labels)
    if training:
        pipeline = pipeline.map(augment)
    if config.n_chan == 1:
        pipeline = pipeline.map(mono_chan)
    elif config.n_chan == 3:
        pipeline = pipeline.map(stereo_mono)
    elif config.n_chan > 3:
        pipeline = pipeline.map(random_merge_aug(config.n_chan))
    if tokens.filter:
        pipeline = pipeline.map(stft_filter(_FILTER_BINS))
    pipeline = pipeline.batch(config.batch_size, drop_remainder=False)
    n_bins = int(np.asarray(backgrounds[0]).shape[0])
    pipeline = pipeline.map(complex_to_mel(config.n_mels, n_bins))  # :119-120 fused
    return _label_tail(pipeline, config)


class BatchDraws:
    """The per-batch random draws of a batched dataset, and the one place that says which stream each comes from: the mixer
    keeps `seed` for the batch itself, the SpecAugment bands take `seed + 1` and the FilterAugment gains `seed + 2` (seed
    None: unseeded host generators; the device generators, which are keyed by an integer, take 0).  Calling it with a batch
    size (and the batch's frame and mel counts) gives (t_bands, f_bands, mel_gain) for the mel kernels:
    - the bands of SpecAugment (`augment`, data_utils.py:58-61: 6 time masks, 1 frequency mask per sample) on training sets,
      and behind them the `stft_filter` band (data_utils.py:126-136: bins 1..k) of a 'filter' name on every set; None
      where there is nothing to mask.  device_draw: one `iris_augment_draw` launch into long-lived device tensors (the filter
      band included), else NumPy on the host - uploaded here, once for all kernels that read them, on an 'ipd' / 'whiten' run;
    - the gains [B, n_mels] of a 'filtaug' name on training sets (`FilterAugmentDraw`), else None.
    A validation set draws neither SpecAugment bands nor gains."""

    def __init__(self, tokens, training, device, seed, device_draw, n_bins):
        key = 0 if seed is None else seed
        self.training, self.device, self.n_bins = training, device, n_bins
        self.filter_bins = _FILTER_BINS if tokens.filter else 0
        self.upload = tokens.ipd or tokens.whiten
        self.rng = np.random.default_rng(None if seed is None else seed + 1)
        self.band_draw = _du.DeviceAugmentDraw(device, key + 1, self.filter_bins) if device_draw and training else None
        self.gain_draw = None
        if training and tokens.filtaug:
            self.gain_draw = _du.FilterAugmentDraw(device, tokens.filtaug, key + 2, device_draw,
                                                   None if seed is not None else np.random.default_rng())

    def __call__(self, b, n_frame, n_mels):
        if self.band_draw is not None:
            tb, fb = self.band_draw(b, n_frame, self.n_bins)
        else:
            tb, fb = _du.augment_draw_batch(b, n_frame, self.n_bins, self.rng) if self.training else (None, None)
            if self.filter_bins:
                flt = np.tile(np.array([[[1, self.filter_bins]]], np.int32), (b, 1, 1))
                fb = flt if fb is None else np.concatenate([fb, flt], axis=1)
        if self.upload:
            tb, fb = (None if v is None else torch.as_tensor(v).to(self.device, torch.int32) for v in (tb, fb))
        return tb, fb, None if self.gain_draw is None else self.gain_draw(b, n_mels)


def _every_epoch(fn, steps_per_epoch):
    """A function to call before every batch: it calls `fn` (None: nothing) before every `steps_per_epoch`-th batch after the
    first."""
    n_batches = 0

    def tick():
        nonlocal n_batches
        if fn is not None and n_batches and n_batches % max(int(steps_per_epoch), 1) == 0:
            fn()
        n_batches += 1
    return tick


def make_device_dataset(config, training=True, n_classes=3, sources=None, device=None, seed=None, device_draw=False):
    """MI355X-native `make_dataset`: same stages, same outputs (sj_train.py:74-130), but a whole
    batch at a time on the device.  The corpora stay resident in HBM; `DeviceMixer` synthesises the
    batch in two launches (merge_complex_specs, pipeline.py:6-110); SpecAugment and `stft_filter`
    reach the mel kernel as band descriptors instead of being multiplied into the 135 MB complex
    batch (they zero time / frequency ranges, which commutes with the per-bin channel mixes and with
    the magnitude).  Yields (x [B, n_mels, n_frame, C], y) forever, like the repeated reference graph.
    device_draw=True: the random half of a batch (sources, offsets, gains, SpecAugment bands) is drawn by two small HIP
    kernels on the device (`iris_mix_draw`, `iris_augment_draw`) instead of NumPy on the host - no table upload, the
    host only enqueues launches.
    Of the run-name tokens (`data_utils.RunTokens`) this builder honours 'stretch', 'filtaug' and 'ipd' and refuses 'speed'
    and 'reverb' (`data_utils.BUILDER_REFUSALS`).  With 'ipd' x is [B, n_mels, n_frame, 4]: one more launch
    (`FrontendPlan.ipd`) over the same mixed spectrum; the corpora must be stereo.  'whiten' (`check_builder` honours it here)
    appends one channel behind those, ln(e + 1e-8) of the spatially whitened energy of the same spectrum with the clip as one
    block (`FrontendPlan.whiten`, two more launches), the batch's bands acting on its output; stereo corpora as well."""
    from .mixer import DeviceMixer
    tokens = _du.run_tokens(config)
    _du.check_builder(tokens, 'make_device_dataset')
    backgrounds, voices, labels, noises = _load_sources(config, training, n_classes, sources)
    if config.model_type == 'se' and config.v == 9:
        raise NotImplementedError("model_type 'se' is outside the accelerated path (SURVEY.md section 2)")
    if tokens.whiten and int(np.asarray(backgrounds[0]).shape[-1]) != 4:   # (before the device is touched)
        raise ValueError(f"run name {config.name!r} asks for 'whiten' but the corpus has {int(np.asarray(backgrounds[0]).shape[-1]) // 2} "
                         "channel(s): the inter-channel covariance needs stereo corpora")
    mixer = DeviceMixer(backgrounds, voices, labels, noises, n_frame=config.n_frame, max_voices=config.max_voices,
                        max_noises=config.max_noises, n_classes=n_classes, device=device, snr=config.snr,
                        min_ratio=1, seed=seed)
    if device_draw:
        mixer.enable_device_draw(0 if seed is None else seed)
    draws = BatchDraws(tokens, training, mixer.device, seed, device_draw, mixer.n_bins)
    stretch = training and tokens.stretch
    if stretch:   # the voice corpus is re-stretched now and once per epoch (the validation set never is)
        mixer.enable_stretch()
        mixer.restretch()
    to_mel = complex_to_mel(config.n_mels, mixer.n_bins)
    if tokens.ipd and mixer.chan2 != 4:
        raise ValueError(f"run name {config.name!r} asks for 'ipd' but the corpus has {mixer.chan2 // 2} channel(s): the inter-channel "
                         "phase difference needs stereo corpora")
    compress = _compression_map(config)
    chan_map = None
    if config.n_chan == 1:
        chan_map = mono_chan
    elif config.n_chan == 3:
        chan_map = stereo_mono
    elif config.n_chan > 3:
        chan_map = random_merge_aug(config.n_chan)

    def gen():
        reaugment = _every_epoch(mixer.restretch if stretch else None, config.steps_per_epoch)
        while True:
            reaugment()
            x, y = to_frame_labels(*mixer.mix(config.batch_size))
            tb, fb, gain = draws(int(x.shape[0]), config.n_frame, config.n_mels)
            if chan_map is not None:
                x, y = chan_map(x, y)
            mel = to_mel(x, None, t_bands=tb, f_bands=fb, mel_gain=gain)
            if compress is not None:
                mel, y = compress(mel, y)   # (called as `Dataset.map` calls a stage)
            if tokens.ipd:   # the phase channels: neither compressed nor gained
                mel = torch.cat([mel, to_mel.ipd(x, tb, fb)], dim=-1)
            if tokens.whiten:   # the whitened channel, last: the clip is one block; neither compressed nor gained
                mel = torch.cat([mel, to_mel.whiten(x, config.n_frame, tb, fb).unsqueeze(-1)], dim=-1)
            yield mel, y

    dataset = _label_tail(Dataset.from_generator(gen), config, compressed=True)
    dataset.mixer = mixer   # (for inspection: the resident corpus, its draws and - 'stretch' runs - the current voice lengths)
    return dataset


def synthetic_wave_sources(n_chan: int = 2, n_classes: int = 3, hop: int = 256, n_bg: int = 8, n_voice: int = 24,
                           n_noise: int = 12, seed: int = 0):
    """Waveform stand-ins of the same shape statistics as `synthetic_sources` (frame counts x hop samples):
    lists of [chan, L_i] float32 waveforms and integer class labels."""
    rng = np.random.default_rng(seed)
    backgrounds = [rng.standard_normal((n_chan, hop * int(rng.integers(300, 900)))).astype(np.float32) * 0.1
                   for _ in range(n_bg)]
    voices = []
    for _ in range(n_voice):
        t = int(rng.integers(40, 200))
        v = rng.standard_normal((n_chan, hop * t)).astype(np.float32) * 0.3
        v[:, hop * int(t * 0.8):] = 0  # trailing silence, as padded voices have
        voices.append(v)
    labels = rng.integers(0, n_classes, size=n_voice)
    noises = [rng.standard_normal((n_chan, hop * int(rng.integers(20, 120)))).astype(np.float32) * 0.3
              for _ in range(n_noise)]
    return backgrounds, voices, labels, noises


def waves_from_specs(sources, n_fft=512, hop=256, device=None):
    """(background spectra, voice spectra, labels, noise spectra) -> the same tuple with WAVEFORMS: every [F, T_i, 2C] complex
    spectrogram (re block, im block last - what `load_wav` pickles) becomes a [C, (T_i - 1) hop] float32 tensor on `device`
    by the inverse STFT (`frontend.istft_batch`: one `iris_istft` launch per corpus list).  Labels pass through.
    What comes back: a corpus made by `load_wav` is a consistent STFT (of the reflect-padded recording), so its inverse is the
    recording's first (T - 1) hop samples up to rounding, the stretch under the last frames included (in float64 to 1e-12:
    tests/test_istft_host.py); the recording's tail beyond a multiple of `hop` was never in the kept range and is not
    recoverable.  Spectra that are not the STFT of any waveform (mixed, masked or stretched ones) are inverted in the
    least-squares sense (Griffin & Lim 1984)."""
    backgrounds, voices, labels, noises = sources
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("waves_from_specs needs a ROCm device (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("waves_from_specs needs a ROCm device (no CPU fallback)")
    n_bins = n_fft // 2 + 1
    plans = {}

    def convert(items, what):
        if items is None:
            return None
        specs = []
        for i, x in enumerate(items):
            t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32)))
            if t.dim() != 3 or int(t.shape[0]) != n_bins or int(t.shape[2]) < 2 or int(t.shape[2]) % 2:
                raise ValueError(f"waves_from_specs: {what}[{i}] has shape {tuple(t.shape)}; expected [F = n_fft / 2 + 1 = "
                                 f"{n_bins}, T, 2 * chan] at n_fft {n_fft}")
            if int(t.shape[1]) < 2:
                raise ValueError(f"waves_from_specs: {what}[{i}] has {int(t.shape[1])} frame(s); the inverse needs two")
            specs.append(t.to(device, torch.float32))
        if not specs:
            return []
        chan = int(specs[0].shape[2]) // 2
        if chan not in plans:
            plans[chan] = _fe.FrontendPlan(n_fft, hop, 64, 16000, chan, 1, n_fft, device)
        out = []
        for i in range(0, len(specs), 65535):   # (the launch's grid holds 65535 records)
            out += _fe.istft_batch(plans[chan], specs[i:i + 65535])
        return out

    waves = convert(backgrounds, "backgrounds"), convert(voices, "voices"), labels, convert(noises, "noises")
    torch.cuda.current_stream(device).synchronize()   # the spectra above are released here
    for plan in plans.values():
        plan.close()
    return waves


def wave_features(plan, compression, do_minmax, wav, t_bands=None, f_bands=None, mel_gain=None, out=None, ipd=False, whiten=0):
    """The features [B, M, T, C] of the waveforms `wav` [B, C, L] on `plan`, one body for `make_wave_dataset` and
    `WaveFrontend`: compression 'log' is ONE launch of the fused kernel (STFT, bands, mel, gains, min-max if `do_minmax`,
    log); 'mel' the same launch stopping at the (gained) mel magnitudes; 'pcen' that, then `frontend.pcen` in place (a
    second launch).  `out` (optional) receives these channels.  ipd: the batch's spectrum is materialised as well (`iris_stft`)
    and the two phase channels (`FrontendPlan.ipd`) under the same bands, neither compressed nor gained, are appended - two
    more launches and a `torch.cat`: deliberately NOT fused into the hot kernel.  whiten (a block length in frames, 0: off):
    the whitened energy channel ln(e + 1e-8) (`FrontendPlan.whiten`, two launches) of that same materialised spectrum - made
    once when both are asked for - is appended last, the bands acting on its output.  Capturable into a hipGraph in every form."""
    if compression == 'log':
        mel = plan.wav_to_logmel(wav, minmax=do_minmax, log=True, t_bands=t_bands, f_bands=f_bands, out=out, mel_gain=mel_gain)
    else:
        mel = plan.wav_to_logmel(wav, minmax=False, log=False, t_bands=t_bands, f_bands=f_bands, out=out, mel_gain=mel_gain)
        if compression == 'pcen':
            mel = _fe.pcen(mel, out=mel)
    if ipd or whiten:
        spec, extra = plan.stft(wav), []
        if ipd:
            extra.append(plan.ipd(spec, t_bands=t_bands, f_bands=f_bands))
        if whiten:
            extra.append(plan.whiten(spec, whiten, t_bands=t_bands, f_bands=f_bands).unsqueeze(-1))
        return torch.cat([mel, *extra], dim=-1)
    return mel


def make_wave_dataset(config, training=True, n_classes=3, sources=None, device=None, seed=None, n_fft=512, hop=256,
                      sample_rate=16000, device_draw=False, spec_sources=None, recordings=None, recordings_share=0.5,
                      rirs=None):
    """`make_device_dataset` from WAVEFORMS (waveform-domain variant): the corpora
    stay resident in HBM as [chan, L_i] waveforms, `WaveMixer` mixes a batch before the STFT (which is linear), and
    the fused kernel takes it from there - STFT, SpecAugment / `stft_filter` bands, mel, min-max, log in one pass;
    no spectrum is ever materialised.  Same stages as sj_train.py:74-130 otherwise; `sources` =
    (background waveforms, voice waveforms, labels, noise waveforms).  n_fft defaults to the reference's 512 (F = 257).
    INTENTIONAL DIVERGENCE at n_chan == 1 with stereo corpora: here the two channels are summed BEFORE the STFT - a true
    down-mix, features [B, M, T, 1].  The reference's `mono_chan` (data_utils.py:73-76), which `make_device_dataset`
    reproduces quirk and all, is the broadcast `x[..., :1] + x[..., 1:]` on the 4-entry re / im axis: 3 entries, i.e.
    2 magnitude channels [B, M, T, 2].  So `--online_stft` and the default path feed the model different features
    and channel counts for stereo corpora at n_chan == 1; at n_chan == 2 (the reference's default) they agree up to
    the boundary frames of the waveform-domain mix.  The augmenting maps of n_chan > 2 mix spectra with per-bin
    factors and are not available here.  device_draw=True: sources / offsets / gains / SpecAugment bands are drawn on
    the device (`iris_mix_draw`, `iris_augment_draw`), as in `make_device_dataset`.
    Of the run-name tokens (`data_utils.RunTokens`) this builder honours 'speed', 'reverb' (with 'shoebox'), 'filtaug' and
    'ipd' and refuses 'stretch', and 'speed' beside 'reverb' (`data_utils.BUILDER_REFUSALS`).  With 'ipd' x is
    [B, n_mels, n_frame, 4] (`wave_features`); the corpora must be stereo.  'whiten' (`check_builder` honours it here) appends
    the whitened energy channel behind those, the clip as one block; stereo corpora and recordings as well.  'flyby'
    (`check_builder` honours it here alone): the training voices as a moving microphone array hears them, redrawn every epoch
    (`WaveMixer.enable_flyby` / `reflyby`); it touches the synthetic part only, as 'speed' / 'reverb' do, and is refused beside either.
    spec_sources: the same tuple as SPECTRA ([F, T_i, 2C], integer labels), e.g. the pickled corpora - converted once here by
    `waves_from_specs` at this n_fft / hop and used as `sources` (giving both is a ValueError).
    recordings: a `recordings.RecordingSampler` (built for this n_frame and hop), or a (waves, events) pair - what
    `recordings.load_recordings` returns - that is wrapped in one here (seeded `seed`, drawing on the device under
    `device_draw`).  Training sets only (a validation set is what it is without it): with k = max(1, round(recordings_share *
    batch_size)) every batch holds k windows cut from the recordings, labelled from their events, FIRST, then batch_size - k
    synthetic samples of the mixer; the concatenated batch takes the one `BatchDraws` / `wave_features` call, so SpecAugment
    bands, 'filter', 'filtaug', 'pcen', 'pcen_learn', 'ipd' and the n_chan == 1 down-mix apply to all of it, while the
    voice-corpus augmentations 'speed' / 'reverb' ('shoebox') touch the synthetic part only.  At recordings_share == 1.0 no mixer
    is built and no synthetic corpus is loaded (`dataset.mixer` is None).  `dataset.recordings` is the sampler (None without).
    ValueError: a share outside (0, 1], a sampler of another n_frame / hop, recordings whose channel count differs from the
    synthetic corpus's, 'ipd' with mono recordings - each before the device is touched.
    'reverb_long' in the name: the 'reverb' augmentation with rt60 ~ U[0.2, 1.0) s and tap buffers of RIR_MAX_TAPS = 16384 on the
    partitioned FFT convolution (`WaveMixer.enable_reverb(max_taps=16384)`).  rirs: measured room responses, a list of
    [corpus channels, K <= 16384] arrays (`transforms.load_rirs`): a training set's 'reverb' then draws one of them per voice
    and epoch instead of synthesising, on the same long path.  ValueError without a 'reverb' token or with 'shoebox', before
    anything is loaded; validation sets ignore them as they ignore the token."""
    from .mixer import WaveMixer
    if spec_sources is not None and sources is not None:
        raise ValueError("make_wave_dataset: give `sources` (waveforms) or `spec_sources` (spectra), not both")
    tokens = _du.run_tokens(config)
    _du.check_builder(tokens, 'make_wave_dataset')
    if rirs is not None and not tokens.reverb:
        raise ValueError(f"make_wave_dataset: measured room responses (rirs=) need a 'reverb' token in the run name {tokens.name!r}")
    if rirs is not None and tokens.shoebox:
        raise ValueError(f"make_wave_dataset: run name {tokens.name!r} asks for 'shoebox' rooms; measured responses (rirs=) replace "
                         "the room model, name one")
    sampler, n_rec = None, 0
    if recordings is not None:
        from .recordings import RecordingSampler, _channels_of
        if not 0.0 < float(recordings_share) <= 1.0:
            raise ValueError(f"make_wave_dataset: recordings_share = {recordings_share} is outside (0, 1]")
        if isinstance(recordings, RecordingSampler):
            if (recordings.n_frame, recordings.hop) != (config.n_frame, hop):
                raise ValueError(f"make_wave_dataset: the RecordingSampler cuts windows of n_frame {recordings.n_frame} at hop "
                                 f"{recordings.hop}, this dataset is built for n_frame {config.n_frame} at hop {hop}")
            rec_chan = recordings.channels
        else:
            rec_chan = _channels_of(recordings[0])
        if tokens.ipd and rec_chan != 2:
            raise ValueError(f"run name {config.name!r} asks for 'ipd' but the recordings have {rec_chan} channel(s): the "
                             "inter-channel phase difference needs stereo recordings")
        if tokens.whiten and rec_chan != 2:
            raise ValueError(f"run name {config.name!r} asks for 'whiten' but the recordings have {rec_chan} channel(s): the "
                             "inter-channel covariance needs stereo recordings")
        if float(recordings_share) < 1.0:
            corpus_chan = 2 if sources is None else int(sources[0][0].shape[0])
            if spec_sources is not None:
                corpus_chan = int(spec_sources[0][0].shape[2]) // 2
            if rec_chan != corpus_chan:
                raise ValueError(f"make_wave_dataset: the recordings have {rec_chan} channel(s), the synthetic corpus {corpus_chan}: "
                                 "one batch holds both")
        if training:
            n_rec = min(max(1, int(round(float(recordings_share) * config.batch_size))), config.batch_size)
            sampler = recordings
    if config.model_type == 'se' and config.v == 9:
        raise NotImplementedError("model_type 'se' is outside the accelerated path (SURVEY.md section 2)")
    if config.n_chan not in (1, 2):
        raise NotImplementedError("make_wave_dataset: n_chan 1 (mono sum) or 2; the augmenting channel maps mix spectra")
    mixer = None
    if sampler is None or float(recordings_share) < 1.0:
        if tokens.whiten and (sources is not None or spec_sources is not None):   # (before the device is touched)
            corpus_chan = int(spec_sources[0][0].shape[2]) // 2 if spec_sources is not None else int(sources[0][0].shape[0])
            if corpus_chan != 2:
                raise ValueError(f"run name {config.name!r} asks for 'whiten' but the corpus has {corpus_chan} channel(s): the "
                                 "inter-channel covariance needs stereo corpora")
        if spec_sources is not None:
            sources = waves_from_specs(spec_sources, n_fft, hop, device)
        if sources is None:
            sources = synthetic_wave_sources(2, n_classes, hop, seed=0 if training else 1)
        backgrounds, voices, labels, noises = sources
        labels = np.eye(n_classes, dtype='float32')[np.asarray(labels)]
        mixer = WaveMixer(backgrounds, voices, labels, noises, n_frame=config.n_frame, n_fft=n_fft, hop=hop,
                          max_voices=config.max_voices, max_noises=config.max_noises, n_classes=n_classes, device=device,
                          snr=config.snr, min_ratio=1, seed=seed)
    if sampler is not None and not isinstance(sampler, RecordingSampler):
        sampler = RecordingSampler(sampler[0], sampler[1], config.n_frame, hop, n_classes, device if mixer is None else mixer.device, seed)
        if device_draw:
            sampler.enable_device_draw(0 if seed is None else seed)
    dev = sampler.device if mixer is None else mixer.device
    length = (config.n_frame - 1) * hop
    plan = _fe.FrontendPlan(n_fft, hop, config.n_mels, sample_rate, config.n_chan, config.batch_size, length, dev)
    # `wave_features`' words for the compression: the raw mel magnitudes of 'pcen_learn' go to the model's PCEN layer
    compression = {'pcen': 'pcen', 'pcen_learn': 'mel'}.get(tokens.compression, 'log')
    do_minmax = tokens.compression == 'minmax_log'
    if tokens.ipd and mixer is not None and mixer.channels != 2:
        raise ValueError(f"run name {config.name!r} asks for 'ipd' but the corpus has {mixer.channels} channel(s): the inter-channel "
                         "phase difference needs stereo corpora")
    if device_draw and mixer is not None:
        mixer.enable_device_draw(0 if seed is None else seed)
    draws = BatchDraws(tokens, training, dev, seed, device_draw, plan.n_bins)
    # the voice corpus is augmented anew now and once per epoch (the validation set never is)
    respeed = rereverb = reflyby = None
    if training and tokens.flyby and mixer is not None:
        mixer.enable_flyby()
        reflyby = mixer.reflyby
        reflyby()
    if training and tokens.speed and mixer is not None:
        mixer.enable_speed()
        respeed = mixer.respeed
        respeed()
    if training and tokens.reverb and mixer is not None:
        if tokens.reverb_long or rirs is not None:
            # long rooms (rt60 up to 1 s: 10667 taps, none truncated) and measured responses: the partitioned FFT convolution
            ranges = dict(rt60_lo=0.2, rt60_hi=1.0) if tokens.reverb_long else {}
            mixer.enable_reverb(max_taps=RIR_MAX_TAPS, rirs=rirs, **ranges)
        else:
            mixer.enable_reverb(model="shoebox" if tokens.shoebox else "noise")
        rereverb = mixer.rereverb
        rereverb()

    def synthetic(n):
        wav, y = mixer.mix(n)
        _, y = to_frame_labels(None, y)
        return wav, y

    def mixed(n):
        """n_rec windows of the recordings, then the mixer's samples.  The sampler's outputs are long-lived buffers that its next
        call overwrites, and the dataset prefetches: what leaves this function is a copy (`cat`, or `clone` where there is no
        synthetic part; the waveform alone is consumed by the feature launch before the next draw)."""
        wav, y = sampler.sample(n_rec)
        if n == n_rec:
            return wav, y.clone()
        syn_wav, syn_y = synthetic(n - n_rec)
        return torch.cat([wav, syn_wav]), torch.cat([y, syn_y])
    batch = synthetic if sampler is None else mixed

    def gen():
        reaugment = _every_epoch(respeed or rereverb or reflyby, config.steps_per_epoch)
        while True:
            reaugment()
            wav, y = batch(config.batch_size)
            if config.n_chan == 1 and wav.shape[1] == 2:
                wav = wav[:, :1] + wav[:, 1:]            # true down-mix (NOT the reference's broadcast mono_chan: see docstring)
            tb, fb, gain = draws(int(wav.shape[0]), config.n_frame, config.n_mels)
            yield wave_features(plan, compression, do_minmax, wav.contiguous(), tb, fb, gain, None, tokens.ipd,
                                config.n_frame if tokens.whiten else 0), y

    dataset = _label_tail(Dataset.from_generator(gen), config, compressed=True)
    dataset.mixer = mixer   # (for inspection: the resident corpus, its draws and - 'speed' / 'reverb' runs - the current voices)
    dataset.recordings = sampler   # (the RecordingSampler of a training set built with `recordings`, else None)
    return dataset


class WaveFrontend:
    """MI355X-native on-line variant of the chain: waveforms [B, C, L] on the device ->
    SpecAugment bands drawn per sample -> fused HIP kernel (STFT, magnitude, masks, mel,
    min-max, log) -> [B, M, T, C].  Equivalent to load_wav + augment + complex_to_magphase
    + magphase_to_mel + minmax + log_on_mel without materialising the spectrum.
    compression='pcen': the fused kernel stops at the mel magnitudes and `frontend.pcen` follows in place (a second
    launch) instead of min-max + log; compression='mel': the mel magnitudes themselves, for a model whose first layer is the
    trainable `PCEN` (a 'pcen_learn' run name).
    `features(wav, t_bands=None, f_bands=None, out=None)`: the features of `wav` with the given bands (no draws) -
    `wave_features` bound to this plan and compression, with nothing in between."""

    def __init__(self, n_fft=1024, hop=256, n_mels=64, sample_rate=16000, n_chan=1, batch=64, length=130816,
                 device=None, training=True, filter_bins: int = 0, do_minmax: bool = True,
                 device_draw: bool = False, seed: int = 0, compression: str = 'log'):
        if compression not in ('log', 'pcen', 'mel'):
            raise ValueError(f"WaveFrontend: compression must be 'log', 'pcen' or 'mel', got {compression!r}")
        if compression != 'log' and not do_minmax:
            raise ValueError(f"WaveFrontend: compression={compression!r} replaces min-max + log; do_minmax=False does not apply")
        self.compression = compression
        self.plan = _fe.FrontendPlan(n_fft, hop, n_mels, sample_rate, n_chan, batch, length, device)
        self.training, self.filter_bins, self.do_minmax = training, filter_bins, do_minmax
        self.device_draw = device_draw
        self.rng = np.random.default_rng(seed)
        self._seed, self._ddraw = int(seed), None
        self.features = functools.partial(wave_features, self.plan, compression, do_minmax)

    def draw_bands(self, batch: int, n_time: int):
        """Host draw (NumPy Generator): exact integer distributions of transforms.py:25-26."""
        return _du.augment_draw_batch(batch, n_time, self.plan.n_bins, self.rng)

    def draw_bands_device(self, batch: int, n_time: int):
        """Device draw, no host round trip, ONE launch (`iris_augment_draw`: Philox keyed by the seed, call counter in device
        memory; the exact integer distributions of transforms.py:25-26; capturable into a hipGraph).  Returns long-lived int32
        device tensors (t_bands [B, 6, 2], f_bands [B, 1, 2]) that the next draw of the same shape overwrites.  (Until round 6
        this was ~20 small torch launches per call - randint, rand, floor, minimum, stack ... - a tenth of a millisecond in front
        of every training step: scripts/gpu_op_census.py.)"""
        if self._ddraw is None:
            self._ddraw = _du.DeviceAugmentDraw(self.plan.device, seed=self._seed)
        return self._ddraw(batch, n_time, self.plan.n_bins)

    def __call__(self, wav: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        b, n_time = wav.shape[0], self.plan.num_frames(wav.shape[2])
        tb = fb = None
        if self.training:
            tb, fb = self.draw_bands_device(b, n_time) if self.device_draw else self.draw_bands(b, n_time)
        if self.filter_bins:
            if isinstance(fb, torch.Tensor) or (fb is None and self.device_draw):
                flt = torch.tensor([[[1, self.filter_bins]]], dtype=torch.int32, device=self.plan.device).expand(b, 1, 2)
                fb = flt if fb is None else torch.cat([fb, flt], dim=1)
            else:
                flt = np.tile(np.array([[[1, self.filter_bins]]], np.int32), (b, 1, 1))
                fb = flt if fb is None else np.concatenate([fb, flt], axis=1)
        return self.features(wav, tb, fb, out=out)


# ---------------------------------------------------------------------------
# schedule, AGC                                             sj_train.py:133-155
# ---------------------------------------------------------------------------
def custom_scheduler(d_model, warmup_steps=4000, lr_div=2):
    """lr(step) = d_model^-0.5 * min((step+1)^-0.5, (step+1) * warmup^-1.5) / lr_div, with
    `step` the EPOCH index as Keras' LearningRateScheduler passes it (sj_train.py:501-503)."""
    d_model = float(d_model)

    def _scheduler(step):
        step = float(step + 1)
        arg1 = step ** -0.5
        arg2 = step * (warmup_steps ** -1.5)
        return d_model ** -0.5 * min(arg1, arg2) / lr_div
    return _scheduler


# ---------------------------------------------------------------------------
# the rest of the reference's sj_train surface lives in sibling modules (round 6 split) and is re-exported under the
# reference's names: model.py (define_keras_model, get_model, CustomModel, ConvMPBlock, FullyConnectedLayer :191-255, :402-403),
# hip_autograd.py (adaptive_clip_grad :145-155 and the HIP passes), distributed.py (absent upstream), fit.py (:434-519)
# ---------------------------------------------------------------------------
from . import switches as SW  # noqa: E402
from .hip_autograd import (FusedAGC, _BiLSTM128, _FusedBiasBNReLU, _FusedConv0BNReLU, _IN_STEP, _WinoConv3x3, _ZERO_POOL,  # noqa: E402,F401
                           _ZeroPool, _is_first_layer_conv, _is_pool_2x2_same, _lstm_is_bilstm128, _wino_train_conv, _zeros,
                           adaptive_clip_grad, bilstm128)
from .model import (ConvMPBlock, CustomModel, FullyConnectedLayer, InferenceEngine, _Bottleneck, _ConvBNReLU,  # noqa: E402,F401
                    _ConvBiasReLU, _HipBiLSTM, _SmoothPool, _WinoStack, _keras_weight_list, binary_crossentropy,
                    define_keras_model, fold_batchnorm, get_model, keras_weight_shapes, load_keras_weights)
from .distributed import (_gradient_buckets, average_bn_statistics, collectives_on, distributed_env,  # noqa: E402,F401
                          force_process_group, init_distributed, wrap_ddp)
from .fit import (GraphCaptureError, GraphedTrainStep, configure_miopen, fit, graph_step_possible, make_optimizer,  # noqa: E402,F401
                  miopen_db_status, optimizer_capturable, run_name)


class _SjTrainModule(type(os)):
    """`sj_train.<SWITCH>` reads and writes the attribute of switches.py (one table, read at call time by every module), so
    `sj_train.WINO_TRAIN = False` / `monkeypatch.setattr(sj_train, "FUSED_BN_RELU", False)` keep working after the split."""

    def __getattr__(self, name):
        if name in SW.NAMES:
            return getattr(SW, name)
        raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in SW.NAMES:
            setattr(SW, name, value)
        else:
            super().__setattr__(name, value)


import sys as _sys  # noqa: E402
_sys.modules[__name__].__class__ = _SjTrainModule


def main(argv=None):
    config = ARGS().get(argv)
    config.loss = config.loss.upper()
    if config.loss != 'MSE':
        config.mse_multiplier = 1
    configure_miopen()
    rank, world, device = init_distributed()
    if rank == 0:
        print(config)
    NAME = run_name(config)
    model = get_model(config).to(device).to(memory_format=torch.channels_last)
    # a GPU, adam / sgd / rmsprop (and not IRIS_GRAPH_STEP=0): the step as one replayed hipGraph - the optimiser then keeps its rate
    # on the device; with more than one rank the gradient all-reduce over RCCL is part of the graph (GraphedTrainStep)
    opt = make_optimizer(config, model.parameters(),
                         capturable=SW.GRAPH_STEP and device.type == 'cuda' and config.optimizer in ('adam', 'sgd', 'rmsprop'))
    loss = binary_crossentropy if config.loss == 'BCE' else \
        (lambda yt, yp: sigmoid_focal_crossentropy(yt, yp).mean())
    metrics, callbacks, monitor = None, [], None
    if config.metrics == 'reference':   # sj_train.py:454-457, :475-495
        from .metrics import cos_sim, er_score, eval_callback, f1_score
        if not os.path.exists('sample_answer.json'):
            # eval_callback scores against ./sample_answer.json and ./*.wav from epoch 2 on, on rank 0 only: checked here, on
            # every rank alike, instead of one rank failing mid-run while the others wait in fit's collectives
            raise FileNotFoundError("--metrics reference: sample_answer.json is missing from the working directory (the "
                                    "checkpoint is scored against it and the *.wav files beside it every 5 epochs)")
        metrics = [cos_sim, f1_score()]
        if config.v != 5:
            metrics.append(er_score(smoothing=False))
        monitor = 'val_er'
        if rank == 0:
            callbacks.append(eval_callback(config, NAME.replace('.h5', '.pt')))
    metrics = ((metrics or []) + count_metrics(config)) or None   # (with --metrics none the only metrics)
    if config.checkpoint_monitor is not None:
        monitor = config.checkpoint_monitor
    ema = None
    if config.ema:   # after the metrics are known, before DDP wraps the model: a second CustomModel, not a submodule
        from .ema import WeightEMA
        ema = WeightEMA(model, config.ema)
        own = None
        if config.metrics == 'reference':   # fresh metric objects: the F1 counts of the EMA pass must not land in the live model's
            from .metrics import cos_sim, er_score, f1_score
            own = [cos_sim, f1_score()] + ([er_score(smoothing=False)] if config.v != 5 else [])
        ema.compile(loss, metrics=((own or []) + count_metrics(config)) or None)   # (and counts of its own)
    model.compile(opt, loss, clipvalue=None if config.no_clipvalue_after_agc else config.clipvalue,
                  ddp=wrap_ddp(model, device, world), metrics=metrics, ema=ema)
    if rank == 0:
        print(NAME, sum(p.numel() for p in model.parameters()), 'parameters')
    if config.pretrain:
        # `model.load_weights(NAME)` (sj_train.py:467-469): this module's own .pt checkpoint, or - a model trained with the
        # reference - its Keras weights as an .npz next to it (scripts/dump_keras_weights.py writes one from the .h5)
        if os.path.exists(NAME.replace('.h5', '.pt')):
            model.load_state_dict(torch.load(NAME.replace('.h5', '.pt'), map_location=device))
            if ema is not None:
                ema.load_state_dict(model.state_dict())
            if rank == 0:
                print('loaded pretrained model', NAME.replace('.h5', '.pt'))
        elif os.path.exists(NAME.replace('.h5', '.npz')):
            load_keras_weights(model, NAME.replace('.h5', '.npz'))
            if ema is not None:
                ema.load_state_dict(model.state_dict())
            if rank == 0:
                print('loaded pretrained Keras weights', NAME.replace('.h5', '.npz'))
    if device.type == 'cuda' and config.online_stft:
        # corpora resident in HBM as WAVEFORMS, mixed before the STFT, fused frontend on line.  Synthetic sources by default;
        # --wave_corpus pickles: the reference's pickles hold spectra, inverted to waveforms once (waves_from_specs)
        dd = not config.host_draws

        def spec_sources(training):
            if config.wave_corpus != 'pickles':
                return None
            backgrounds, voices, onehot, noises = _load_sources(config, training, 3, None)
            return backgrounds, voices, onehot.argmax(-1), noises
        recordings = None
        if config.recordings is not None:   # loaded once per rank; each rank draws its own windows
            from .recordings import RecordingSampler, load_recordings
            recordings = RecordingSampler(*load_recordings(config.recordings, config.recordings_answer, device), config.n_frame, 256,
                                          device=device, seed=3000 + rank)
            if dd:
                recordings.enable_device_draw(3000 + rank)
        synthetic_part = recordings is None or config.recordings_share < 1.0
        rirs = None
        if config.rirs is not None:   # loaded once per rank (the corpora are stereo); files up to 1.024 s are kept whole
            from .transforms import load_rirs
            rirs = load_rirs(config.rirs, 2, max_taps=RIR_MAX_TAPS)
        def wav_sources(split, wanted=True):
            """--wave_corpus wavs: ROOT/<split> as waveforms, the voices gated (each rank loads for itself)."""
            if config.wave_corpus != 'wavs' or not wanted:
                return None
            from .corpus import GateSettings, load_wav_corpus
            gate = None if config.no_gate else GateSettings(range_db=config.gate_range_db, min_gap=config.gate_min_gap,
                                                            min_event=config.gate_min_event, hang=config.gate_hang)
            *sources, report = load_wav_corpus(config.corpus_dir, split, device, 3, gate)
            if rank == 0:
                print('corpus', report)
            return tuple(sources)
        train_set = make_wave_dataset(config, training=True, device=device, seed=1000 + rank, device_draw=dd,
                                      sources=wav_sources('train', synthetic_part),
                                      spec_sources=spec_sources(True) if synthetic_part else None, recordings=recordings,
                                      recordings_share=config.recordings_share, rirs=rirs)
        test_set = make_wave_dataset(config, training=False, device=device, seed=2000 + rank, device_draw=dd,
                                     sources=wav_sources('test'), spec_sources=spec_sources(False))
    elif device.type == 'cuda' and not config.per_sample_pipeline:
        # corpora resident in HBM, whole batches synthesised on the device (each rank draws its own stream)
        dd = not config.host_draws
        train_set = make_device_dataset(config, training=True, device=device, seed=1000 + rank, device_draw=dd)
        test_set = make_device_dataset(config, training=False, device=device, seed=2000 + rank, device_draw=dd)
    else:
        train_set = make_dataset(config, training=True)
        test_set = make_dataset(config, training=False)
    from .swa import NO_SWA_ERROR, SWA
    swa = SWA(start_epoch=config.epochs // 4, swa_freq=2)  # sj_train.py:491
    fit(model, train_set, config.epochs, config.steps_per_epoch, test_set, config.validation_steps,
        scheduler=custom_scheduler(4096, config.epochs / 12, config.lr_div),
        csv_path=NAME.replace('.h5', '.csv'), checkpoint_path=NAME.replace('.h5', '.pt'),
        patience=config.patience, rank=rank, world=world, swa=swa, checkpoint_monitor=monitor, callbacks=callbacks,
        **({} if ema is None else {'ema': ema, 'ema_checkpoint_path': NAME.replace('.h5', '_EMA.pt')}))

    def bn_batches():   # --reset_bn N: the next N training batches
        it = iter(train_set)
        for _ in range(config.reset_bn):
            yield next(it)
    if ema is not None and config.reset_bn > 0:
        # the best EMA checkpoint of the run (else the EMA as training left it) with statistics of its own instead of the live
        # model's: every rank recalibrates (the ranks' statistics are averaged), rank 0 writes
        path = NAME.replace('.h5', '_EMA.pt')
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()
        if os.path.exists(path):
            ema.load_state_dict(torch.load(path, map_location=device))
        from .ema import recalibrate_bn
        recalibrate_bn(ema.module, bn_batches(), world)
        if rank == 0:
            torch.save(ema.state_dict(), path)
    try:
        swa.finalize(model, reset_bn=bn_batches() if config.reset_bn > 0 else None, world=world)
        if rank == 0:
            torch.save(model.state_dict(), NAME.replace('.h5', '_SWA.pt'))
            print('best model:', NAME.replace('.h5', '_SWA.pt'))
    except NO_SWA_ERROR:
        pass
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    if rank == 0:
        print(NAME.split('.h5')[0])


if __name__ == "__main__":
    main()