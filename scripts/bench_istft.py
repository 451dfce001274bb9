"""Inverse STFT of a spectrum corpus on one MI355X: (a) k_istft under `rocprofv3 --kernel-trace --stats`, each corpus in a run
of its own (a child process), median launch time with the bytes the launch reads + writes (every spectrum once, every waveform
once) and the resulting GB/s; (b) wall time of `frontend.istft_batch` over the voice corpus - one launch - against the form
that exists without the kernel: `torch.istft` on the device tensors, looped over the voices.
Corpora are `sj_train.synthetic_sources`-like stereo voices at F = 257 (40-200 frames; n_fft 512, hop 256).
Prints one JSON line and writes it, with rocprofv3's CSVs, under the output directory.

usage: python3 scripts/bench_istft.py [--out DIR] [--voices 24,512] [--reps 20]
       python3 scripts/bench_istft.py --child N_VOICE LAUNCHES        (what runs under rocprofv3)"""
import argparse, csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

N_FFT, HOP, CHAN = 512, 256, 2


def make_corpus(n_voice):
    import torch
    from challenge_amd import sj_train as S
    from challenge_amd.frontend import FrontendPlan
    dev = torch.device("cuda", 0)
    _, voices, _, _ = S.synthetic_sources(CHAN, 3, N_FFT // 2 + 1, n_bg=1, n_voice=n_voice, n_noise=1, seed=0)
    specs = [torch.from_numpy(v).to(dev) for v in voices]
    return FrontendPlan(N_FFT, HOP, 64, 16000, CHAN, 1, N_FFT, dev), specs


def launch_bytes(specs):
    rd = sum(int(s.numel()) * 4 for s in specs)
    wr = sum(CHAN * (int(s.shape[1]) - 1) * HOP * 4 for s in specs)
    return rd, wr


def child(n_voice, launches):
    import torch
    from challenge_amd import frontend as FE
    plan, specs = make_corpus(n_voice)
    for _ in range(launches + 2):
        FE.istft_batch(plan, specs)
    torch.cuda.synchronize()
    rd, wr = launch_bytes(specs)
    print(json.dumps({"n_voice": n_voice, "calls": launches + 2, "bytes_read": rd, "bytes_written": wr, "samples_out": wr // 4}))


def profile(n_voice, launches, out):
    d = os.path.join(out, f"rocprof_v{n_voice}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "istft", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(n_voice), str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if p.returncode:
        raise RuntimeError(f"rocprofv3 run failed ({p.returncode}): {p.stderr[-2000:]}")
    info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(trace)))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "k_istft" in r["Kernel_Name"]]
    info["kernel_launches"] = len(ns)      # == calls: one launch per call, whatever the corpus size
    ns = ns[2:]
    info.update({"kernel_launches_timed": len(ns), "kernel_median_us": float(np.median(ns)) / 1e3, "kernel_min_us": min(ns) / 1e3,
                 "kernel_max_us": max(ns) / 1e3})
    info["gb_per_s"] = (info["bytes_read"] + info["bytes_written"]) / (info["kernel_median_us"] * 1e3)
    info["ns_per_output_sample"] = info["kernel_median_us"] * 1e3 / info["samples_out"]
    return info


def wall(n_voice, reps):
    import torch
    from challenge_amd import frontend as FE
    plan, specs = make_corpus(n_voice)
    window = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64).to(torch.float32).to(specs[0].device)

    def torch_loop():
        out = []
        for s in specs:   # [F, T, 2C] -> complex [C, F, T]
            z = torch.complex(s[..., :CHAN], s[..., CHAN:]).permute(2, 0, 1)
            out.append(torch.istft(z, N_FFT, hop_length=HOP, window=window, center=True))
        return out

    def timed(fn):
        ts = []
        for i in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    # alternate the two forms so that both see the same machine state
    a, b = [], []
    for _ in range(3):
        a.append(timed(lambda: FE.istft_batch(plan, specs)))
        b.append(timed(torch_loop))
    t_new, t_old = float(np.median(a)), float(np.median(b))
    worst = max(float((x - y).abs().max()) for x, y in list(zip(FE.istft_batch(plan, specs), torch_loop()))[:8])
    return {"n_voice": n_voice, "istft_batch_ms": 1e3 * t_new, "istft_batch_ms_runs": [1e3 * t for t in a], "torch_loop_ms": 1e3 * t_old,
            "torch_loop_ms_runs": [1e3 * t for t in b], "torch_loop_over_istft_batch": t_old / t_new,
            "max_abs_difference_8_voices": worst}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="istft_bench_out")
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
    with open(os.path.join(args.out, "bench_istft.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
