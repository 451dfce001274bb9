"""Time the recordings sampler on one MI355X at the training shape (batch 64, 2 channels, n_frame 512, hop 256: 67 MB
written and as much read per launch).

  (a) `iris_crop_windows` alone, draws fixed per call but different from call to call, from a corpus larger than the
      Infinity Cache (48 stereo recordings of 60 - 120 s: ~550 MB), the outputs rotating over 6 buffer sets (400 MB), so
      neither side is served from cache;
  (b) the yardstick: a contiguous `Tensor.copy_` of the same 67 MB, sources and destinations rotating likewise;
  (c) `iris_crop_draw` for the batch;
  (d) what a training batch pays: `RecordingSampler.sample(32)` under the device draw plus the `torch.cat` with 32 synthetic
      samples (stand-ins of the mixer's shapes), beside `WaveMixer.mix(64)` and `mix(32)`.

Device events around groups of calls, warm.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from challenge_amd import frontend as FE  # noqa: E402
from challenge_amd import sj_train as S  # noqa: E402
from challenge_amd.mixer import WaveMixer  # noqa: E402
from challenge_amd.recordings import RecordingSampler  # noqa: E402


def timed(fns, warmup=2, runs=12):
    """Median / min / max microseconds per call of the functions `fns`, called round robin: one event pair around every round."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for fn in fns:
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / len(fns))
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "calls": runs * len(fns)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crop needs a GPU"
    dev = torch.device("cuda", 0)
    batch, chan, n_frame, hop, k = 64, 2, 512, 256, 3
    length = (n_frame - 1) * hop
    gen = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    waves = [torch.randn((chan, int(16000 * rng.uniform(60, 120))), device=dev, generator=gen) * 0.1 for _ in range(48)]
    events = []
    for w in waves:   # a dozen events per recording, up to 3 s long
        start = rng.integers(0, w.shape[1] // hop, 12)
        events.append(np.stack([rng.integers(0, k, 12), start, start + rng.integers(1, 200, 12)], axis=1))
    sampler = RecordingSampler(waves, events, n_frame, hop, k, device=dev, seed=0)
    nbytes = batch * chan * length * 4
    result = {"device": torch.cuda.get_device_name(0), "corpus_MB": round(sampler.storage.numel() * 4 / 1e6, 1),
              "batch_MB": round(nbytes / 1e6, 1), "windows": sampler.n_windows}

    sets = 6
    draws = [torch.from_numpy(sampler.draw(batch)).to(dev) for _ in range(sets)]
    outs = [(torch.empty((batch, chan, length), device=dev), torch.empty((batch, n_frame, k), device=dev)) for _ in range(sets)]
    crop = [lambda d=d, o=o: FE.crop_windows(sampler._recs_dev, sampler.events, d, chan, hop, n_frame, k, out=o) for d, o in zip(draws, outs)]
    srcs = [torch.randn((batch, chan, length), device=dev, generator=gen) for _ in range(sets)]
    copy = [lambda s=s, o=o: o[0].copy_(s) for s, o in zip(srcs, outs)]
    for name, fns in (("crop_windows", crop), ("copy_", copy), ("crop_windows_again", crop), ("copy_again", copy)):
        result[name] = timed(fns)
        result[name]["GBps_read_plus_write"] = round(2 * nbytes / result[name]["median_us"] / 1e3, 1)
    result["crop_over_copy"] = round(result["crop_windows"]["median_us"] / result["copy_"]["median_us"], 3)
    del srcs, copy

    state = torch.zeros(1, dtype=torch.int64, device=dev)
    buf = FE.crop_draw(sampler.prefix, batch, 0, state)
    result["crop_draw"] = timed([lambda: FE.crop_draw(sampler.prefix, batch, 0, state, out=buf)] * sets)

    sampler.enable_device_draw(0)
    half = batch // 2
    syn_wav, syn_y = torch.randn((half, chan, length), device=dev, generator=gen), torch.zeros((half, n_frame, k), device=dev)

    def sample_and_cat():
        wav, y = sampler.sample(half)
        return torch.cat([wav, syn_wav]), torch.cat([y, syn_y])
    result["sample32_plus_cat"] = timed([sample_and_cat] * sets)
    result["sample32"] = timed([lambda: sampler.sample(half)] * sets)
    backgrounds, voices, labels, noises = S.synthetic_wave_sources(chan, k, hop)
    mixer = WaveMixer(backgrounds, voices, np.eye(k, dtype="float32")[np.asarray(labels)], noises, n_frame=n_frame, n_fft=512, hop=hop,
                      max_voices=7, max_noises=2, n_classes=k, device=dev, snr=-20, min_ratio=1, seed=0)
    mixer.enable_device_draw(0)
    result["mixer_mix64"] = timed([lambda: mixer.mix(batch)] * sets)
    result["mixer_mix32"] = timed([lambda: mixer.mix(half)] * sets)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
