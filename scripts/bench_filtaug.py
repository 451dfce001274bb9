"""Time FilterAugment on one MI355X: the fused kernel without and with per-sample mel-band gains, and the device draw.

  (a) `FrontendPlan.wav_to_logmel` at c2 (batch 32 x 10 s mono, n_fft 1024, hop 256, 64 mel, min-max + log) and at the
      waveform dataset's default shape (batch 64 x 511 hops stereo, n_fft 512, 80 mel), with SpecAugment bands as a training
      step has them: the kernel's own start / stop timestamps (`timing_enable`), median of the sampled launches, ungained
      entry (`iris_wav_to_logmel`) beside the gained sibling (`iris_wav_to_logmel_gain`);
  (b) `iris_magmel` / `iris_magmel_gain` on the spectra of the second shape (device events around the call);
  (c) one `iris_filter_draw` for the batch (device events around the call).

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from challenge_amd import data_utils as DU  # noqa: E402
from challenge_amd import frontend as FE  # noqa: E402


def timed(fn, warmup=5, runs=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_us": round(1e3 * statistics.median(ms), 2), "min_us": round(1e3 * min(ms), 2), "max_us": round(1e3 * max(ms), 2)}


def kernel_us(plan, fn, runs=60):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    plan.timing_enable(True)
    for _ in range(runs + 8):
        fn()
    torch.cuda.synchronize()
    us = 1e3 * plan.timing_samples(0)
    plan.timing_enable(False)
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(us.min()), 2), "max_us": round(float(us.max()), 2),
            "launches": int(us.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filtaug needs a GPU"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for tag, (n_fft, hop, m, c, b, length) in {"c2": (1024, 256, 64, 1, 32, 160000), "wave_default": (512, 256, 80, 2, 64, 130816)}.items():
        plan = FE.FrontendPlan(n_fft, hop, m, 16000, c, b, length, dev)
        wav = torch.from_numpy((rng.standard_normal((b, c, length)) * 0.1).astype(np.float32)).to(dev)
        out = torch.empty((b, m, plan.num_frames(length), c), device=dev)
        gain = FE.filter_draw(b, m, device=dev)[2]
        tb, fb = DU.augment_draw_batch(b, plan.num_frames(length), plan.n_bins, rng)
        entry = {"kernel": plan.fused_kernel_name(True)}
        for name, kw in (("no_bands", {}), ("bands", {"t_bands": torch.from_numpy(tb).to(dev), "f_bands": torch.from_numpy(fb).to(dev)})):
            plain = plan.prepare(wav, out=out, **kw)
            gained = plan.prepare(wav, out=out, mel_gain=gain, **kw)
            entry[name] = {"ungained": kernel_us(plan, plain.launch), "gained": kernel_us(plan, gained.launch),
                           "ungained_again": kernel_us(plan, plain.launch), "epilogue": plan.last_epilogue()}
        if tag == "wave_default":
            spec = plan.stft(wav)
            entry["magmel"] = {"ungained": timed(lambda: plan.magmel(spec)), "gained": timed(lambda: plan.magmel(spec, mel_gain=gain))}
            state = torch.zeros(1, dtype=torch.int64, device=dev)
            bufs = FE.filter_draw(b, m, state=state)
            entry["filter_draw"] = timed(lambda: FE.filter_draw(b, m, state=state, out=bufs))
        result[tag] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
