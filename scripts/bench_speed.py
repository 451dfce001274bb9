"""Speed-perturbation augmentation on one MI355X: (a) k_speed_perturb and k_mix_wave_frame_active_batch under
`rocprofv3 --kernel-trace --stats`, each corpus in a run of its own (a child process), median launch time with the bytes the
launch reads + writes (every source once, every output once) and the resulting GB/s; (b) wall time of `WaveMixer.respeed()` -
one resampling launch and one activity launch over the voice corpus - against the form that exists without the kernel: per
voice, the same formula as batched torch ops on the device (gather of the tap window, elementwise taps, sum).
Corpora are `sj_train.synthetic_wave_sources` (stereo voices of 40-200 frames of 256 samples), rates ~ U[0.9, 1.1).
Prints one JSON line and writes it, with rocprofv3's CSVs, under the output directory.

usage: python3 scripts/bench_speed.py [--out DIR] [--voices 24,512] [--reps 20]
       python3 scripts/bench_speed.py --child N_VOICE LAUNCHES        (what runs under rocprofv3)"""
import argparse, csv, glob, json, math, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

RATE_SEED = 7


def make_mixer(n_voice):
    import torch
    from challenge_amd import sj_train as S
    from challenge_amd.mixer import WaveMixer
    backgrounds, voices, labels, noises = S.synthetic_wave_sources(2, 3, 256, n_bg=2, n_voice=n_voice, n_noise=2, seed=0)
    mixer = WaveMixer(backgrounds, voices, np.eye(3, dtype=np.float32)[np.asarray(labels)], noises, n_frame=512, n_fft=512, hop=256,
                      max_voices=7, max_noises=2, n_classes=3, device=torch.device("cuda", 0), min_ratio=1, seed=0)
    mixer.enable_speed()
    return mixer


def launch_bytes(mixer, rates):
    """Bytes one k_speed_perturb launch over the corpus reads (every source once) and writes (every output once)."""
    row = mixer.channels * 4
    l_in = mixer._aug.orig_n
    n_out = np.ceil(l_in / rates).astype(np.int64)
    return int(row * l_in.sum()), int(row * n_out.sum())


def child(n_voice, launches):
    import torch
    mixer = make_mixer(n_voice)
    rates = np.random.default_rng(RATE_SEED).uniform(0.9, 1.1, size=n_voice)
    for _ in range(launches + 1):
        mixer.respeed(rates)   # one k_speed_perturb and one k_mix_wave_frame_active_batch per call
    torch.cuda.synchronize()
    rd, wr = launch_bytes(mixer, rates)
    print(json.dumps({"n_voice": n_voice, "respeed_calls": launches + 2, "bytes_read": rd, "bytes_written": wr,
                      "samples_out": wr // 4}))


def profile(n_voice, launches, out):
    d = os.path.join(out, f"rocprof_v{n_voice}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "speed", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(n_voice), str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if p.returncode:
        raise RuntimeError(f"rocprofv3 run failed ({p.returncode}): {p.stderr[-2000:]}")
    info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(trace)))
    for key, name in (("kernel", "k_speed_perturb"), ("activity", "k_mix_wave_frame_active_batch")):
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
        info[f"{key}_launches"] = len(ns)      # == respeed_calls: one launch per call, whatever the corpus size
        ns = ns[2:]   # enable_speed's rate-1 copy, and the first launch with real rates
        info.update({f"{key}_launches_timed": len(ns), f"{key}_median_us": float(np.median(ns)) / 1e3,
                     f"{key}_min_us": min(ns) / 1e3, f"{key}_max_us": max(ns) / 1e3})
    info["gb_per_s"] = (info["bytes_read"] + info["bytes_written"]) / (info["kernel_median_us"] * 1e3)
    info["ns_per_output_sample"] = info["kernel_median_us"] * 1e3 / info["samples_out"]
    return info


def torch_speed(x, rate):
    """The definition of iris_speed_perturb for one [C, L] device tensor as torch ops: fp64 positions, fp32 taps."""
    import torch
    length = int(x.shape[1])
    n = int(math.ceil(length / rate))
    cut = 0.99 * min(1.0, 1.0 / rate)
    h = int(math.ceil(6 / cut))
    pos = torch.arange(n, dtype=torch.float64, device=x.device) * rate
    i0 = torch.floor(pos)
    frac = (pos - i0).to(torch.float32)
    k = torch.arange(-h, h + 2, device=x.device)
    idx = i0.to(torch.int64)[:, None] + k[None, :]
    t = cut * (k[None, :].to(torch.float32) - frac[:, None])
    pt = math.pi * t
    taps = torch.where(t.abs() < 6, cut * torch.special.sinc(t) * torch.cos(pt / 12) ** 2, torch.zeros_like(t))
    taps = taps * ((idx >= 0) & (idx < length))
    return (x[:, idx.clamp(0, length - 1)] * taps[None]).sum(-1)


def wall(n_voice, reps):
    import torch
    mixer = make_mixer(n_voice)
    rng = np.random.default_rng(RATE_SEED)
    originals = mixer._aug.orig

    def torch_loop(rates):
        return [torch_speed(v, float(r)) for v, r in zip(originals, rates)]

    def timed(fn):
        ts = []
        for i in range(reps + 3):
            rates = rng.uniform(0.9, 1.1, size=n_voice)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(rates)
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    # alternate the two forms so that both see the same machine state
    a, b = [], []
    for _ in range(3):
        a.append(timed(mixer.respeed))
        b.append(timed(torch_loop))
    t_new, t_old = float(np.median(a)), float(np.median(b))
    # the two forms compute the same thing
    rates = rng.uniform(0.9, 1.1, size=n_voice)
    mixer.respeed(rates)
    worst = max(float((torch_speed(v, float(r)) - o).abs().max()) for v, r, o in list(zip(originals, rates, mixer.voices))[:8])
    return {"n_voice": n_voice, "respeed_ms": 1e3 * t_new, "respeed_ms_runs": [1e3 * t for t in a], "torch_loop_ms": 1e3 * t_old,
            "torch_loop_ms_runs": [1e3 * t for t in b], "torch_loop_over_respeed": t_old / t_new, "max_abs_difference_8_voices": worst}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="speed_bench_out")
    ap.add_argument("--voices", default="24,512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=45)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    counts = [int(v) for v in args.voices.split(",")]
    res = {"kernel": [], "wall": []}
    for n_voice in counts:     # profiled runs first: each is a fresh child, and this process has not touched the GPU yet
        res["kernel"].append(profile(n_voice, args.launches, args.out))
    for n_voice in counts:
        res["wall"].append(wall(n_voice, args.reps))
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_speed.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
