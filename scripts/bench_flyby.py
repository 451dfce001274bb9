"""Fly-by augmentation on one MI355X: one `WaveMixer.reflyby()` over a voice corpus - host draws and record packing, one table
upload, one `iris_flyby` launch and one `iris_mix_wave_frame_active_batch` launch - and, beside it in the same process and over
the same corpus, the nearest existing kernel: one `iris_speed_perturb` launch at rates ~ U[0.9, 1.1).  The launches are timed
with device events (table resident, the two kernels alternating, medians); `reflyby` with a host clock around a synchronise.
For stereo with the ground path k_flyby evaluates four times the taps of k_speed_perturb (two paths, and no tap shared by the
channel pair), so about 4 x its time is expected.  Bytes are what a launch reads and writes once (every source, every output).
Prints one JSON line and writes it under the output directory.

usage: python3 scripts/bench_flyby.py [--out DIR] [--voices 2048] [--seconds 2.0] [--reps 20]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7
FS = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="flyby_bench_out")
    ap.add_argument("--voices", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    from challenge_amd.mixer import WaveMixer
    if not torch.cuda.is_available():
        raise SystemExit("bench_flyby needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    n_voice, length, chan = args.voices, int(round(args.seconds * FS)), 2
    gen = torch.Generator(device=dev).manual_seed(SEED)
    voices = [torch.randn((chan, length), device=dev, generator=gen) * 0.3 for _ in range(n_voice)]
    for v in voices:
        v[:, length - length // 5:] = 0            # trailing silence, as padded voices have
    rng = np.random.default_rng(SEED)
    backgrounds = [rng.standard_normal((chan, 256 * 600)).astype(np.float32) * 0.1 for _ in range(2)]
    labels = np.eye(3, dtype=np.float32)[rng.integers(0, 3, n_voice)]
    mixer = WaveMixer(backgrounds, voices, labels, None, n_frame=512, n_fft=512, hop=256, max_voices=7, max_noises=0, n_classes=3,
                      device=dev, min_ratio=1, seed=0)
    mixer.enable_flyby()
    aug = mixer._aug

    def clock(fn, reps):
        ts = []
        for i in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts)), [1e3 * t for t in ts]

    # (a) the whole call, draws and packing included, and the same with the flights given
    reflyby_ms, reflyby_runs = clock(mixer.reflyby, args.reps)
    geoms = [T.draw_flyby(rng, chan, args.seconds) for _ in range(n_voice)]
    given_ms, _ = clock(lambda: mixer.reflyby(geoms), args.reps)
    paths = int((aug.table["n_paths"] == 2).sum())

    # (b) the two kernels alone, tables resident, alternating
    rates = rng.uniform(0.9, 1.1, size=n_voice)
    speed = np.zeros(n_voice, FE.SPEED_SRC)
    outs = [torch.empty((chan, FE.speed_len(length, r)), device=dev) for r in rates]
    speed["src"], speed["dst"] = [v.data_ptr() for v in voices], [o.data_ptr() for o in outs]
    speed["len_in"], speed["len_out"], speed["rate"] = length, [o.shape[1] for o in outs], rates
    speed_dev = torch.from_numpy(speed.view(np.uint8).reshape(-1).copy()).to(dev)
    from challenge_amd import _native as N
    lib, stream = N.lib(), FE._stream_ptr(dev)
    max_out = int(speed["len_out"].max())
    launches = {"flyby": lambda: lib.iris_flyby(aug.table_dev.data_ptr(), n_voice, chan, length, stream),
                "speed": lambda: lib.iris_speed_perturb(speed_dev.data_ptr(), n_voice, chan, max_out, stream)}
    times = {k: [] for k in launches}
    for i in range(args.reps + 3):
        for name, fn in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            N.check(fn(), name)
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b))
    flyby_ms, speed_ms = float(np.median(times["flyby"])), float(np.median(times["speed"]))
    row = chan * 4
    res = {"n_voice": n_voice, "channels": chan, "samples": length, "voices_with_ground_path": paths,
           "reflyby_ms": reflyby_ms, "reflyby_ms_min_max": [min(reflyby_runs), max(reflyby_runs)], "reflyby_given_flights_ms": given_ms,
           "flyby_launch_ms": flyby_ms, "flyby_launch_ms_min_max": [min(times["flyby"]), max(times["flyby"])],
           "speed_launch_ms": speed_ms, "speed_launch_ms_min_max": [min(times["speed"]), max(times["speed"])],
           "flyby_over_speed": flyby_ms / speed_ms,
           "flyby_bytes": 2 * row * length * n_voice, "flyby_gb_per_s": 2 * row * length * n_voice / (flyby_ms * 1e6),
           "flyby_ns_per_output_sample": flyby_ms * 1e6 / (chan * length * n_voice),
           "speed_ns_per_output_sample": speed_ms * 1e6 / (chan * int(speed["len_out"].sum()))}
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_flyby.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
