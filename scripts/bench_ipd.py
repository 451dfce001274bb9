"""Time the inter-channel phase features on one MI355X.

  (a) `FrontendPlan.ipd` beside `FrontendPlan.magmel` on the same spectrum, B = 64, F = 257, T = 512, M = 80 (device events
      around the call; --kernels-only runs just these two in a loop, for `rocprofv3 --kernel-trace --stats` in a run of its own);
      the bytes either kernel needs, 16 B F T read + 8 B M T written, over the time give the GB/s printed beside it;
  (b) one batch of `make_device_dataset` and of `make_wave_dataset` (batch 64, n_frame 512, 80 mel, stereo, training set)
      without and with the 'ipd' token: host clock around `next()` + a device synchronise, median;
  (c) one eager training step of the CRNN (v 9, batch 64, n_frame 512, 80 mel) on 2 and on 4 input channels: device events.

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from challenge_amd import frontend as FE  # noqa: E402
from challenge_amd import sj_train as S  # noqa: E402

B, F, T, M = 64, 257, 512, 80


def timed(fn, warmup=5, runs=30):
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
    return {"median_us": round(1e3 * statistics.median(ms), 2), "min_us": round(1e3 * min(ms), 2), "max_us": round(1e3 * max(ms), 2)}


def batches_ms(ds, warmup=3, runs=15):
    it = iter(ds)
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        next(it)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def cfg(name, batch=B, n_frame=T):
    return S.ARGS().get(['--v', '9', '--n_mels', str(M), '--n_frame', str(n_frame), '--n_chan', '2', '--batch_size', str(batch),
                         '--name', name])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ipd needs a GPU"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "F": F, "T": T, "M": M}}
    rng = np.random.default_rng(0)
    plan = FE.FrontendPlan(512, 256, M, 16000, 2, B, 512, dev)
    spec = torch.from_numpy((0.1 * rng.standard_normal((B, F, T, 4))).astype(np.float32)).to(dev)
    out = torch.empty((B, M, T, 2), device=dev)
    n_bytes = 16 * B * F * T + 8 * B * M * T
    if args.kernels_only:
        for _ in range(50):
            plan.ipd(spec, out=out)
            plan.magmel(spec)
        torch.cuda.synchronize()
        print(json.dumps({"launches_each": 50, "bytes_per_launch": n_bytes}))
        return
    kern = {"ipd": timed(lambda: plan.ipd(spec, out=out)), "magmel": timed(lambda: plan.magmel(spec)),
            "ipd_again": timed(lambda: plan.ipd(spec, out=out)), "bytes": n_bytes}
    for k in ("ipd", "magmel", "ipd_again"):
        kern[k]["GBps"] = round(n_bytes / (kern[k]["median_us"] * 1e-6) / 1e9, 1)
    result["kernels"] = kern
    data = {}
    for which, make, sources in (("device", S.make_device_dataset, S.synthetic_sources(2, 3, seed=0)),
                                 ("wave", S.make_wave_dataset, S.synthetic_wave_sources(2, 3, seed=0))):
        data[which] = {}
        for name in ("run", "run_ipd", "run"):
            ds = make(cfg(name), training=True, sources=sources, device=dev, seed=1, device_draw=True)
            key = name if name not in data[which] else name + "_again"
            data[which][key] = batches_ms(ds)
            del ds
    result["datasets"] = data
    steps = {}
    for name, chans in (("run", 2), ("run_ipd", 4), ("run", 2)):
        c = cfg(name)
        torch.manual_seed(0)
        model = S.get_model(c).to(dev).to(memory_format=torch.channels_last)
        model.compile(S.make_optimizer(c, model.parameters()), S.binary_crossentropy, clipvalue=c.clipvalue)
        x = torch.randn(B, M, T, chans, device=dev)
        y = (torch.rand(B, T // 32, 3, device=dev) > 0.7).float()
        key = f"chan{chans}" if f"chan{chans}" not in steps else f"chan{chans}_again"
        steps[key] = timed(lambda: model.train_step((x, y)), warmup=8, runs=20)
        del model
    result["train_step"] = steps
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
