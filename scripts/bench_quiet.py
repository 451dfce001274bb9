"""The noise-covariance launches on one MI355X: `iris_spec_whiten_factors` (the block covariance, k_whiten_factors<false>) and
`iris_spec_whiten_factors_ranges` (k_whiten_factors<true>) over the same 4 x 513 x 2048 stereo spectrum with blocks of 512
frames, in one process, alternating:
  (a) the unmasked kernel;
  (b) the ranges kernel with an empty mask and every range its own block - the same bytes plus the mask;
  (c) the ranges kernel with 64 events of 64 frames masked (guard 6), min_quiet 32, at reach 0 and at reach 1 - and, so that
      reach 1 has something to borrow for, (d) the same with one recording's block filled by an event.
The C entries are called directly on resident inputs (no allocation, no table upload inside the timed window); a timed sample
is `--inner` launches between two device events, divided by `--inner`; medians over `--reps` samples after a warm-up, min and
max beside them.  (b) must equal (a) bit for bit; that is checked.  Last, `FrontendPlan.whiten_factors` and
`FrontendPlan.whiten_factors_ranges` as a user calls them, one call per sample (allocation, table checks and upload inside).
Prints one JSON line and writes it under the output directory.

usage: python3 scripts/bench_quiet.py [--out DIR] [--reps 30] [--inner 20]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7
B, F, T, BLOCK, EVENTS, EVENT_FRAMES, GUARD, MIN_QUIET = 4, 513, 2048, 512, 64, 64, 6, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="quiet_bench_out")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("bench_quiet needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    x = torch.randn((B, F, T, 4), device=dev, generator=gen)
    x[..., 1] = 0.9 * x[..., 0] + 0.1 * x[..., 1]        # a coherent pair, as a dominant interferer makes it
    x[..., 3] = 0.9 * x[..., 2] + 0.1 * x[..., 3]
    rng = np.random.default_rng(SEED)
    n = EVENT_FRAMES
    events = np.array([[rng.integers(B), BLOCK * j + s, BLOCK * j + s + n - 1]
                       for j, s in zip(rng.integers(T // BLOCK, size=EVENTS), rng.integers(BLOCK - n + 1, size=EVENTS))], np.int64)
    filled = np.concatenate([events, [[0, BLOCK, 2 * BLOCK - 1]]])      # ... and block 1 of recording 0 filled
    plan = FE.FrontendPlan(1024, 256, 64, 16000, 2, B, 1024, dev)
    lib, stream = N.lib(), FE._stream_ptr(dev)
    n_blocks = T // BLOCK
    out = {k: torch.empty((B, F, n_blocks, 4), device=dev) for k in ("block", "empty", "reach0", "reach1", "filled0", "filled1")}

    def tables(ev, reach):
        mask = TR.quiet_mask(ev, [T] * B, GUARD)
        ranges, quiet = TR.quiet_ranges(mask, [T] * B, BLOCK, MIN_QUIET, reach)
        return torch.from_numpy(mask).to(dev), torch.from_numpy(ranges).to(dev), ranges, quiet
    inputs = {"empty": tables(np.zeros((0, 3), np.int64), 0), "reach0": tables(events, 0), "reach1": tables(events, 1),
              "filled0": tables(filled, 0), "filled1": tables(filled, 1)}

    def ranges_call(name):
        mask, table_dev, table, _ = inputs[name]
        return lambda: N.check(lib.iris_spec_whiten_factors_ranges(plan._handle, x.data_ptr(), mask.data_ptr(), table_dev.data_ptr(),
                                                                   table.ctypes.data, out[name].data_ptr(), B, T, BLOCK, 1e-2, stream),
                               "iris_spec_whiten_factors_ranges")
    calls = {"block": lambda: N.check(lib.iris_spec_whiten_factors(plan._handle, x.data_ptr(), out["block"].data_ptr(), B, T, 0, BLOCK,
                                                                   1e-2, stream), "iris_spec_whiten_factors")}
    calls.update({name: ranges_call(name) for name in inputs})
    times = {k: [] for k in calls}
    with torch.cuda.device(dev):
        for i in range(args.reps + 5):
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                torch.cuda.synchronize()
                if i >= 5:
                    times[name].append(a.elapsed_time(b) / args.inner)
    # the two Python calls as a user makes them (one call between the events: the allocation, and for the ranges call the
    # table's checks and upload, are inside), for comparison with the call times README quotes
    wrappers = {"call_block": lambda: plan.whiten_factors(x, BLOCK),
                "call_ranges": lambda: plan.whiten_factors_ranges(x, inputs["reach1"][0], inputs["reach1"][2], BLOCK)}
    times.update({k: [] for k in wrappers})
    for i in range(args.reps + 5):
        for name, fn in wrappers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 5:
                times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"batch": B, "bins": F, "frames": T, "block": BLOCK, "events": EVENTS, "event_frames": n, "guard": GUARD,
           "min_quiet": MIN_QUIET, "reps": args.reps, "inner": args.inner, "spectrum_bytes": 16 * B * F * T, "mask_bytes": B * T}
    for k in times:
        res[k + "_ms"] = med[k]
        res[k + "_ms_min_max"] = [min(times[k]), max(times[k])]
    for k in inputs:
        _, _, ranges, quiet = inputs[k]
        masked = int(inputs[k][0].sum().item())
        res[k + "_over_block"] = med[k] / med["block"]
        res[k + "_masked_frames"] = masked
        res[k + "_range_frames"] = int((ranges[..., 1] - ranges[..., 0]).sum())
        res[k + "_fallback_blocks"] = int((ranges[..., 2] == 0).sum())
    res["empty_equals_block_bitwise"] = bool(torch.equal(out["empty"], out["block"]))
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_quiet.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    if not res["empty_equals_block_bitwise"]:
        raise SystemExit("the ranges kernel with an empty mask differs from the unmasked kernel")


if __name__ == "__main__":
    main()
