"""Time the reverberation kernels (iris_fir_batch, iris_fft_fir_batch) on one MI355X: device events around the call, 3 warm-ups, the median of 20.

  (a) one `WaveMixer.rereverb()` over the corpus of `sj_train.synthetic_wave_sources` (host side included: 24 impulse
      responses drawn and uploaded, one launch);
  (b) one `iris_fir_batch` over 2048 voices x 2 s x 2 channels at 4096 taps;
  (c) the same table through torch.fft.rfft / irfft per voice on the device (the only baseline here);
  (d) with --step_ms (the training step of bench.py's line): (a) and (b) as a share of steps_per_epoch x step_ms;
  (e) the table of (b) through `iris_fft_fir_batch` (the partitioned FFT convolution; groups of at most --budget_mb of spectra,
      one launch pair each), compared with (b) on the first voices before it is timed;
  (f) the same at --long_taps (16384) taps, where the direct form does not run;
  (g) one `rereverb()` of a 'reverb_long' mixer (rt60 ~ U[0.2, 1.0) s, max_taps 16384) over the corpus of (a).

Prints one JSON line; --out also writes it to a file.  (b) and (c) are compared on the first voices before they are timed."""
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


def timed(fn, warmup=3, runs=20):
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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--taps", type=int, default=4096)
    ap.add_argument("--long_taps", type=int, default=16384)
    ap.add_argument("--budget_mb", type=int, default=256)
    ap.add_argument("--step_ms", type=float, default=None, help="ms per training step (bench.py's train_step_ms)")
    ap.add_argument("--steps_per_epoch", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reverb needs a GPU"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0)}

    # (a) the synthetic corpus through the mixer
    backgrounds, voices, labels, noises = S.synthetic_wave_sources(2, 3)
    mixer = WaveMixer(backgrounds, voices, np.eye(3, dtype=np.float32)[labels], noises, n_frame=512, n_fft=512, hop=256, device=dev,
                      seed=0)
    mixer.enable_reverb()
    result["a_rereverb_synthetic"] = dict(timed(mixer.rereverb), voices=len(voices), samples=int(sum(v.shape[1] for v in voices)))

    # (b) the larger table
    n, chan, length, k = args.voices, 2, int(args.seconds * 16000), args.taps
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn((n, chan, length), device=dev, generator=gen) * 0.3
    taps = torch.randn((n, chan, k), device=dev, generator=gen) * (1.0 / k ** 0.5)
    dst = torch.empty_like(src)
    table = np.zeros(n, FE.FIR_SRC)
    table["src"], table["dst"] = [src[i].data_ptr() for i in range(n)], [dst[i].data_ptr() for i in range(n)]
    table["taps"], table["len"], table["n_taps"] = [taps[i].data_ptr() for i in range(n)], length, k
    table_dev = torch.empty(table.nbytes, dtype=torch.uint8, device=dev)
    fmas = n * chan * sum(min(m + 1, k) for m in range(length))
    b = timed(lambda: FE.fir_launch(table, chan, length, k, dev, table_dev))
    result["b_fir_batch"] = dict(b, voices=n, channels=chan, samples=length, taps=k, fma=fmas,
                                 tflops=round(2 * fmas / (b["median_ms"] * 1e-3) / 1e12, 2))

    # (c) torch.fft per voice on the device
    n_fft = 1 << (length + k - 1).bit_length()

    def fft_conv(i):
        return torch.fft.irfft(torch.fft.rfft(src[i], n_fft) * torch.fft.rfft(taps[i], n_fft), n_fft)[:, :length]

    def fft_all():
        for i in range(n):
            dst_fft[i] = fft_conv(i)
    dst_fft = torch.empty_like(src)
    diff = max(float((fft_conv(i) - dst[i]).abs().max()) for i in range(4))
    result["c_torch_fft_per_voice"] = dict(timed(fft_all, warmup=1, runs=5), n_fft=n_fft, max_abs_diff_to_b_first_4_voices=diff)

    # (e), (f) the partitioned FFT convolution on the same voices
    def fft_leg(tap_tensor, n_taps):
        ftable = np.zeros(n, FE.FFT_FIR_SRC)
        ftable["src"], ftable["dst"] = table["src"], [dst_long[i].data_ptr() for i in range(n)]
        ftable["taps"], ftable["len"], ftable["n_taps"] = [tap_tensor[i].data_ptr() for i in range(n)], length, n_taps
        groups, largest = FE.fft_fir_groups(ftable, chan, args.budget_mb << 20)
        ws = torch.empty(largest, dtype=torch.uint8, device=dev)
        ftable_dev = torch.empty(ftable.nbytes, dtype=torch.uint8, device=dev)

        def run():
            for lo, hi in groups:
                FE.fft_fir_launch(ftable[lo:hi], chan, length, n_taps, 0, ws, dev, ftable_dev[lo * 40:hi * 40])
        t = timed(run)
        return dict(t, voices=n, channels=chan, samples=length, taps=n_taps, groups=len(groups), workspace_mb=round(largest / 2 ** 20, 1))
    dst_long = torch.empty_like(src)
    e = fft_leg(taps, k)
    e["max_abs_diff_to_b_first_4_voices"] = max(float((dst_long[i] - dst[i]).abs().max()) for i in range(4))
    e["max_abs_diff_to_b_all_voices"] = float((dst_long - dst).abs().max())     # (every group of the workspace budget)
    e["speedup_over_b"] = round(b["median_ms"] / e["median_ms"], 3)
    result["e_fft_fir_batch"] = e
    long_taps = torch.randn((n, chan, args.long_taps), device=dev, generator=gen) * (1.0 / args.long_taps ** 0.5)
    result["f_fft_fir_batch_long"] = fft_leg(long_taps, args.long_taps)
    del long_taps, dst_long

    # (g) the 'reverb_long' mixer
    long_mixer = WaveMixer(backgrounds, voices, np.eye(3, dtype=np.float32)[labels], noises, n_frame=512, n_fft=512, hop=256,
                           device=dev, seed=0)
    long_mixer.enable_reverb(rt60_lo=0.2, rt60_hi=1.0, max_taps=S.RIR_MAX_TAPS)
    result["g_rereverb_long_synthetic"] = dict(timed(long_mixer.rereverb), voices=len(voices), groups=len(long_mixer._aug.groups),
                                               workspace_mb=round(long_mixer._aug.workspace.numel() / 2 ** 20, 1))

    if args.step_ms:
        epoch_ms = args.steps_per_epoch * args.step_ms
        result["d_share_of_epoch"] = {"step_ms": args.step_ms, "steps_per_epoch": args.steps_per_epoch,
                                      "a_percent": round(100 * result["a_rereverb_synthetic"]["median_ms"] / epoch_ms, 4),
                                      "b_percent": round(100 * b["median_ms"] / epoch_ms, 4)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
