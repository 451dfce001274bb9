"""Time the spatially whitened energy channel on one MI355X: `FrontendPlan.whiten_factors`, the apply launch alone
(`iris_spec_whiten` on factors made once) and `FrontendPlan.ipd` beside them on the same spectrum, B = 64, F = 257, T = 512,
M = 80, block = T and block = 64 (device events around each call, interleaved rounds, median / min).  --kernels-only runs the
launches in a loop and nothing else, for `rocprofv3 --kernel-trace --stats` in a run of its own.  The byte floor of a launch
is the spectrum read once, 16 B F T, plus what it writes (16 B F J for the factors, 4 B M T for the output; the apply launch
also reads the factors), over the 6.0 TB/s a streaming read reaches on this chip.

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from challenge_amd import _native as N  # noqa: E402
from challenge_amd import frontend as FE  # noqa: E402

B, F, T, M = 64, 257, 512, 80
HBM_BPS = 6.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_whiten needs a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    plan = FE.FrontendPlan(512, 256, M, 16000, 2, B, 512, dev)
    spec = torch.from_numpy((0.1 * rng.standard_normal((B, F, T, 4))).astype(np.float32)).to(dev)
    out = torch.empty((B, M, T), device=dev)
    out_ipd = torch.empty((B, M, T, 2), device=dev)
    stream = FE._stream_ptr(dev)
    calls, floors = {}, {}
    for block in (T, 64):
        fac = plan.whiten_factors(spec, block)
        j = int(fac.shape[2])

        def apply(block=block, fac=fac):
            N.check(N.lib().iris_spec_whiten(plan._handle, spec.data_ptr(), fac.data_ptr(), out.data_ptr(), B, T, 0, block, 1,
                                             None, 0, None, 0, stream), "iris_spec_whiten")
        calls[f"factors_block{block}"] = lambda block=block: plan.whiten_factors(spec, block)
        calls[f"apply_block{block}"] = apply
        floors[f"factors_block{block}"] = 16 * B * F * T + 16 * B * F * j
        floors[f"apply_block{block}"] = 16 * B * F * T + 16 * B * F * j + 4 * B * M * T
    calls["ipd"] = lambda: plan.ipd(spec, out=out_ipd)
    floors["ipd"] = 16 * B * F * T + 8 * B * M * T
    if args.kernels_only:
        for _ in range(50):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"launches_each": 50, "floor_bytes": floors}))
        return
    for _ in range(5):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(30):   # interleaved rounds
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    result = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "F": F, "T": T, "M": M}, "calls": {}}
    for k, v in ms.items():
        med = 1e3 * statistics.median(v)
        floor_us = 1e6 * floors[k] / HBM_BPS
        result["calls"][k] = {"median_us": round(med, 2), "min_us": round(1e3 * min(v), 2), "max_us": round(1e3 * max(v), 2),
                              "floor_bytes": floors[k], "floor_us": round(floor_us, 2), "times_floor": round(med / floor_us, 2)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
