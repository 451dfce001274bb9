"""Time-stretch augmentation on one MI355X: (a) k_phase_vocoder under `rocprofv3 --kernel-trace --stats`, each corpus shape in a
run of its own (a child process), median launch time with the bytes the launch reads + writes and the resulting GB/s;
(b) wall time of `DeviceMixer.restretch()` - one launch over the voice corpus plus the per-voice frame-activity launches -
against what there was before it: `transforms.phase_vocoder` (torch ops) on fp32 device tensors, looped over the voices.
Corpora are `sj_train.synthetic_sources`-like (voices of 40-200 frames, stereo) at F = 257 and F = 513.
Prints one JSON line and writes it, with rocprofv3's CSVs, under the output directory.

usage: python3 scripts/bench_stretch.py [--out DIR] [--voices 24,512] [--reps 20]
       python3 scripts/bench_stretch.py --child F N_VOICE LAUNCHES        (what runs under rocprofv3)"""
import argparse, csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

RATE_SEED = 7


def corpus(freq, n_voice):
    from challenge_amd import sj_train as S
    backgrounds, voices, labels, noises = S.synthetic_sources(2, 3, freq=freq, n_bg=2, n_voice=n_voice, n_noise=2, seed=0)
    return backgrounds, voices, np.eye(3, dtype=np.float32)[np.asarray(labels)], noises


def make_mixer(freq, n_voice):
    import torch
    from challenge_amd.mixer import DeviceMixer
    backgrounds, voices, labels, noises = corpus(freq, n_voice)
    mixer = DeviceMixer(backgrounds, voices, labels, noises, n_frame=512, max_voices=7, max_noises=2, n_classes=3,
                        device=torch.device("cuda", 0), min_ratio=1, seed=0)
    mixer.enable_stretch()
    return mixer


def launch_bytes(mixer, rates):
    """Bytes one k_phase_vocoder launch over the corpus reads (every source once) and writes (every stretched voice once)."""
    row = mixer.n_bins * mixer.chan2 * 4
    t_in = mixer._aug.orig_n
    n_out = np.ceil(t_in / rates).astype(np.int64)
    return int(row * t_in.sum()), int(row * n_out.sum())


def child(freq, n_voice, launches):
    import torch
    from challenge_amd import frontend as FE
    mixer = make_mixer(freq, n_voice)
    rates = np.random.default_rng(RATE_SEED).uniform(0.8, 1.2, size=n_voice)
    mixer.restretch(rates)   # fills the table; the launches below repeat the kernel alone
    st = mixer._aug
    for _ in range(launches):
        FE.phase_vocoder_launch(st.table, mixer.n_bins, mixer.chan2, int(st.cap.max()), mixer.device, st.table_dev)
    torch.cuda.synchronize()
    rd, wr = launch_bytes(mixer, rates)
    print(json.dumps({"freq": freq, "n_voice": n_voice, "launches": launches + 1, "bytes_read": rd, "bytes_written": wr}))


def profile(freq, n_voice, launches, out):
    d = os.path.join(out, f"rocprof_f{freq}_v{n_voice}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "stretch", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(freq), str(n_voice), str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if p.returncode:
        raise RuntimeError(f"rocprofv3 run failed ({p.returncode}): {p.stderr[-2000:]}")
    info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(trace)) if "k_phase_vocoder" in r["Kernel_Name"]]
    ns = ns[1:]   # the first launch loads the code object
    med = float(np.median(ns))
    info.update(kernel_launches_timed=len(ns), kernel_median_us=med / 1e3, kernel_min_us=min(ns) / 1e3, kernel_max_us=max(ns) / 1e3,
                gb_per_s=(info["bytes_read"] + info["bytes_written"]) / med)
    return info


def wall(freq, n_voice, reps):
    import torch
    from challenge_amd import transforms as T
    mixer = make_mixer(freq, n_voice)
    rng = np.random.default_rng(RATE_SEED)
    originals = mixer._aug.orig

    def torch_loop(rates):
        return [T.phase_vocoder(v, float(r)) for v, r in zip(originals, rates)]

    def timed(fn):
        ts = []
        for i in range(reps + 3):
            rates = rng.uniform(0.8, 1.2, size=n_voice)
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
        a.append(timed(mixer.restretch))
        b.append(timed(torch_loop))
    t_new, t_old = float(np.median(a)), float(np.median(b))
    # the share of restretch() that is the per-voice iris_mix_frame_active loop: time the vocoder launch alone
    from challenge_amd import frontend as FE
    st = mixer._aug
    t_voc = timed(lambda rates: FE.phase_vocoder_launch(st.table, mixer.n_bins, mixer.chan2, int(st.cap.max()), mixer.device,
                                                        st.table_dev))
    return {"freq": freq, "n_voice": n_voice, "restretch_ms": 1e3 * t_new, "vocoder_launch_alone_ms": 1e3 * t_voc,
            "torch_loop_ms": 1e3 * t_old, "torch_loop_over_restretch": t_old / t_new}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="stretch_bench_out")
    ap.add_argument("--voices", default="24,512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=45)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    counts = [int(v) for v in args.voices.split(",")]
    res = {"kernel": [], "wall": []}
    for freq in (257, 513):     # profiled runs first: each is a fresh child, and this process has not touched the GPU yet
        for n_voice in counts:
            res["kernel"].append(profile(freq, n_voice, args.launches, args.out))
    for freq in (257, 513):
        for n_voice in counts:
            res["wall"].append(wall(freq, n_voice, args.reps))
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_stretch.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
