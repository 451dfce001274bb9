"""Timings of the shoebox room simulation at a realistic corpus: 1000 voices x 2 channels, rt60 ~ U[0.1, 0.4).

    python scripts/bench_shoebox.py [--voices 1000] [--seconds 2.0] [--reps 5]

prints one JSON line: the wall time of `WaveMixer.rereverb()` (host draw + launches + device time, synchronised) in the "noise"
and the "shoebox" model on the same corpus, and the device-event time of the `iris_ism_rir` launch alone.  For the kernel time
run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_shoebox.py --reps 1` and read `k_ism_rir`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from challenge_amd import frontend as FE
    from challenge_amd.mixer import WaveMixer
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    n = int(args.seconds * 16000)
    voices = [rng.standard_normal((2, n)).astype(np.float32) * 0.1 for _ in range(args.voices)]
    backgrounds = [rng.standard_normal((2, 4 * 16000)).astype(np.float32) * 0.1 for _ in range(2)]
    labels = np.eye(3, dtype=np.float32)[rng.integers(0, 3, args.voices)]
    out = {"voices": args.voices, "channels": 2, "seconds": args.seconds, "reps": args.reps}
    for model in ("noise", "shoebox"):
        mixer = WaveMixer(backgrounds, voices, labels, backgrounds, n_frame=64, n_fft=1024, hop=256, max_voices=4, max_noises=1,
                          n_classes=3, device=dev, seed=1)
        mixer.enable_reverb(model=model)
        mixer.rereverb()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mixer.rereverb()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[f"rereverb_{model}_ms"] = round(1e3 * float(np.median(times)), 3)
        if model == "shoebox":
            aug = mixer._aug
            out["images_per_voice_channel_mean"] = round(float(np.mean(
                [8 * np.prod(2 * (np.floor(343.0 * (g["n_taps"] + 100) / 16000 / (2 * g["room"])) + 1) + 1) for g in aug.geometry])))
            out["n_taps_mean"] = round(float(np.mean(aug.ism_table["n_taps"])), 1)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ks = []
            for _ in range(args.reps):
                ev[0].record()
                FE.shoebox_rir_launch(aug.ism_table, 2, FE.FIR_MAX_TAPS, dev, aug.ism_table_dev)
                ev[1].record()
                torch.cuda.synchronize()
                ks.append(ev[0].elapsed_time(ev[1]))
            out["iris_ism_rir_event_ms"] = round(float(np.median(ks)), 3)
        del mixer
    print(json.dumps(out))


if __name__ == "__main__":
    main()
