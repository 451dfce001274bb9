"""The Wiener post-filter of event extraction on one MI355X: one `FrontendPlan.postfilter` call (the table, delay and floor
uploads, one output allocation, `k_postfilter`) over bench_extract.py's scene - 64 events of 64 frames in a 4 x 257 x 2048 stereo
spectrum (load_wav's n_fft 512), blocks of 512 frames, here with the factors of noise="quiet" - beside the two launches it sits
between in `transforms.extract_events`: `FrontendPlan.beamform` before it and `iris_istft` (`clips_from_slabs`) after it.  The
calls alternate and are timed with device events (medians; min and max beside them).  The launch alone is the C entry point on
buffers made once, 50 launches between two device events (launch to launch, the gaps between launches inside it), with one
delay per event and with one per frame.  The kernel reads 8 bytes per (bin, frame) twice - the second time out of cache - and
writes 8; with 64-frame events a workgroup's chain is one chunk long, so the launch is bound by the double-precision phase
and gain arithmetic per cell, not by memory.  As checks, the floor 1 returns the input slabs bit for bit and the floor -20 dB
leaves less energy than it found.  Prints one JSON line and writes it under the output directory.

usage: python3 scripts/bench_postfilter.py [--out DIR] [--events 64] [--frames 64] [--reps 20]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7
B, F, T, BLOCK = 4, 257, 2048, 512
LOADING, ALPHA, FLOOR_DB = 1e-2, 0.98, -20.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="postfilter_bench_out")
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("bench_postfilter needs a ROCm device: nothing is measured without one")
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
    fac, quiet = TR._quiet_factors(plan, x, events, BLOCK, LOADING, 0, 32, 1)
    floor = 10.0 ** (FLOOR_DB / 20.0)
    slabs = plan.beamform(x, events, tdoa, fac, BLOCK)
    post = lambda g=floor: plan.postfilter(slabs, events, tdoa, fac, BLOCK, LOADING, 0, F, ALPHA, g)
    filtered = post()
    calls = {"beamform": lambda: plan.beamform(x, events, tdoa, fac, BLOCK), "postfilter": post,
             "istft": lambda: TR.clips_from_slabs(filtered)}
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
    floors = np.full(args.events, floor)
    per_event = np.ascontiguousarray(tdoa, np.float64)
    per_frame = np.repeat(per_event, n)
    table_dev, floors_dev = torch.from_numpy(table).to(dev), torch.from_numpy(floors).to(dev)
    src = slabs[0].data_ptr()                             # `beamform`'s flat buffer
    flat = torch.empty((2 * F * n * args.events,), dtype=torch.float32, device=dev)
    stream, burst, launch = FE._stream_ptr(dev), 50, {}
    for name, delays in (("launch", per_event), ("launch_per_frame", per_frame)):
        delays_dev = torch.from_numpy(delays).to(dev)

        def launches():
            for _ in range(burst):
                N.check(N.lib().iris_postfilter_events(plan._handle, src, fac.data_ptr(), T // BLOCK, table_dev.data_ptr(),
                                                       table.ctypes.data, delays_dev.data_ptr(), len(delays), int(name != "launch"),
                                                       floors_dev.data_ptr(), floors.ctypes.data, args.events, B, T, BLOCK, LOADING,
                                                       ALPHA, 0, F, flat.data_ptr(), flat.numel(), stream), "iris_postfilter_events")
        launch[name] = []
        for i in range(args.reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launches()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                launch[name].append(a.elapsed_time(b) / burst)
        assert torch.equal(flat, torch.cat([s.reshape(-1) for s in filtered]))      # both forms: the bits of the call
    bypass = post(1.0)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bypass, slabs))
    before, after = (float(sum(s.double().square().sum() for s in v)) for v in (slabs, filtered))
    assert after < before
    res = {"batch": B, "bins": F, "frames": T, "block": BLOCK, "events": args.events, "event_frames": n,
           "quiet_frames_min": int(TR.quiet_frames(events, quiet, BLOCK).min()), "alpha": ALPHA, "floor_db": FLOOR_DB}
    for name, v in list(times.items()) + list(launch.items()):
        res[name + "_ms"] = float(np.median(v))
        res[name + "_ms_min_max"] = [min(v), max(v)]
    res["postfilter_over_beamform"] = res["postfilter_ms"] / res["beamform_ms"]
    res["launch_ns_per_cell"] = res["launch_ms"] * 1e6 / (F * n * args.events)
    res["energy_after_over_before_db"] = 10.0 * float(np.log10(after / before))
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_postfilter.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
