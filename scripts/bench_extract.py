"""Event extraction on one MI355X: one `FrontendPlan.beamform` call (the table and delay uploads, one output allocation,
`k_beamform`) over 64 events of 64 frames in a 4 x 257 x 2048 stereo spectrum (load_wav's n_fft 512) with the whitening factors
of blocks of 512 frames - and, beside it in the same process and on the same spectrum, (a) a torch complex64 restatement of the
same definition on the device (gather the event frames, form g0 and g1, multiply: what one would write without the kernel)
and (b) the `iris_istft` launch that follows it in `transforms.extract_events` (`clips_from_slabs`), timed separately.  The
calls alternate and are timed with device events (medians; min and max beside them); the slabs of the kernel and of the
restatement are compared.  The kernel moves 24 bytes per (bin, frame) - a 16-byte record in, 8 bytes out.  Its rate is taken
from the launch alone (the C entry point on buffers made once, 50 launches between two device events: launch to launch, so
the gaps between launches are inside it) and stated as a share of the 8.0 TB/s HBM peak; at this size (25 MB moved, a 34 MB
spectrum) everything stays in the Infinity Cache between launches, so it is a rate of the kernel, not of the HBM.  Prints one
JSON line and writes it under the output directory.

usage: python3 scripts/bench_extract.py [--out DIR] [--events 64] [--frames 64] [--reps 20]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7
B, F, T, BLOCK = 4, 257, 2048, 512
HBM_PEAK = 8.0e12   # bytes / s, the MI355X's specified peak


def torch_beamform(x, fac, events, tdoa, block):
    """The definition in torch complex64 on the device, events of equal length inside one block each: [E, F, n, 2]."""
    import torch
    ev = torch.as_tensor(events, device=x.device, dtype=torch.int64)
    n = int(ev[0, 2] - ev[0, 1]) + 1
    frames = ev[:, 1:2] + torch.arange(n, device=x.device)[None, :]                                  # [E, n]
    seg = x[ev[:, 0, None, None], torch.arange(x.shape[1], device=x.device)[None, :, None], frames[:, None, :]]   # [E, F, n, 4]
    g = fac[ev[:, 0], :, ev[:, 1] // block]                                                          # [E, F, 4]
    a, b, c = g[..., 0:1], g[..., 1:2], torch.complex(g[..., 2:3], g[..., 3:4])
    x0, x1 = torch.complex(seg[..., 0], seg[..., 2]), torch.complex(seg[..., 1], seg[..., 3])
    k = torch.arange(x.shape[1], device=x.device, dtype=torch.float64)[None, :]
    r = k * torch.as_tensor(tdoa, device=x.device, dtype=torch.float64)[:, None] / (2 * (x.shape[1] - 1))
    r = r - torch.round(r)
    e = torch.polar(torch.ones_like(r), -2.0 * np.pi * r).to(torch.complex64)[..., None]             # [E, F, 1]
    s1 = b * (e - c)
    den = a ** 2 + s1.abs() ** 2
    g1 = b * s1.conj() / den
    g0 = a ** 2 / den - g1 * c
    y = torch.where(a != 0, g0 * x0 + g1 * x1, torch.zeros_like(x0))
    return torch.view_as_real(y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="extract_bench_out")
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("bench_extract needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    x = torch.randn((B, F, T, 4), device=dev, generator=gen)
    x[..., 1] = 0.9 * x[..., 0] + 0.1 * x[..., 1]        # a coherent pair, as a dominant interferer makes it
    x[..., 3] = 0.9 * x[..., 2] + 0.1 * x[..., 3]
    rng = np.random.default_rng(SEED)
    n = args.frames
    events = np.array([[rng.integers(B), BLOCK * j + s, BLOCK * j + s + n - 1]
                       for j, s in zip(rng.integers(T // BLOCK, size=args.events), rng.integers(BLOCK - n + 1, size=args.events))],
                      np.int32)
    tdoa = rng.uniform(-4.0, 4.0, size=args.events)
    plan = FE.FrontendPlan(512, 256, 64, 16000, 2, B, 512, dev)
    fac = plan.whiten_factors(x, BLOCK)
    slabs = plan.beamform(x, events, tdoa, fac, BLOCK)
    calls = {"beamform": lambda: plan.beamform(x, events, tdoa, fac, BLOCK),
             "torch_complex64": lambda: torch_beamform(x, fac, events, tdoa, BLOCK),
             "istft": lambda: TR.clips_from_slabs(slabs)}
    times = {k: [] for k in calls}
    for i in range(args.reps + 3):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b))
    # the launch alone: the C entry point on buffers made once, `burst` launches between two device events
    from challenge_amd import _native as N
    table = FE.beamform_table(events, T, B)
    table_dev, tdoa_dev = torch.from_numpy(table).to(dev), torch.from_numpy(np.ascontiguousarray(tdoa, np.float64)).to(dev)
    flat = torch.empty((2 * F * n * args.events,), dtype=torch.float32, device=dev)
    stream, burst, launch = FE._stream_ptr(dev), 50, []

    def launches():
        for _ in range(burst):
            N.check(N.lib().iris_beamform_events(plan._handle, x.data_ptr(), fac.data_ptr(), T // BLOCK, table_dev.data_ptr(),
                                                 table.ctypes.data, tdoa_dev.data_ptr(), args.events, B, T, BLOCK, 0, F,
                                                 flat.data_ptr(), flat.numel(), stream), "iris_beamform_events")
    for i in range(args.reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            launch.append(a.elapsed_time(b) / burst)
    got = torch.stack(plan.beamform(x, events, tdoa, fac, BLOCK))
    want = torch_beamform(x, fac, events, tdoa, BLOCK)
    med = {k: float(np.median(v)) for k, v in times.items()}
    moved = 24 * F * n * args.events
    res = {"batch": B, "bins": F, "frames": T, "block": BLOCK, "events": args.events, "event_frames": n,
           "beamform_ms": med["beamform"], "beamform_ms_min_max": [min(times["beamform"]), max(times["beamform"])],
           "torch_complex64_ms": med["torch_complex64"],
           "torch_complex64_ms_min_max": [min(times["torch_complex64"]), max(times["torch_complex64"])],
           "istft_ms": med["istft"], "istft_ms_min_max": [min(times["istft"]), max(times["istft"])],
           "torch_over_beamform": med["torch_complex64"] / med["beamform"],
           "bytes_moved": moved, "spectrum_bytes": 16 * B * F * T,
           "launch_ms": float(np.median(launch)), "launch_ms_min_max": [min(launch), max(launch)],
           "launch_bytes_per_s": moved / (float(np.median(launch)) * 1e-3),
           "launch_share_of_hbm_peak": moved / (float(np.median(launch)) * 1e-3) / HBM_PEAK,
           "call_share_of_hbm_peak": moved / (med["beamform"] * 1e-3) / HBM_PEAK,
           "max_rel_diff_vs_torch_complex64": float(((got - want).abs().max() / want.abs().max()))}
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_extract.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
