"""Event localisation on one MI355X: one `FrontendPlan.locate` call (the table upload, `k_locate_moments`, `k_locate_scan`) over
64 events of 64 frames in a 4 x 513 x 2048 stereo spectrum with 81 lags (max_lag 40, q 8) and the whitening factors of blocks of
512 frames - and, beside it in the same process and on the same spectrum, (a) a torch float64 restatement of the same
definition on the device (gather the event frames, whiten, moments, steer, sum: what one would write without the kernels) and
(b) `iris_spec_whiten_factors`, the nearest existing kernel, which reads the whole spectrum once.  The calls alternate and are
timed with device events (medians; min and max beside them); the curves of the kernel and of the restatement are compared.
Prints one JSON line and writes it under the output directory.

usage: python3 scripts/bench_locate.py [--out DIR] [--events 64] [--frames 64] [--reps 20]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7
B, F, T, BLOCK, MAX_LAG, Q = 4, 513, 2048, 512, 40, 8


def torch_locate(x, fac, events, block, max_lag, q):
    """The definition in torch float64 on the device, events of equal length inside one block each: [E, 2 max_lag + 1]."""
    import torch
    ev = torch.as_tensor(events, device=x.device, dtype=torch.int64)
    n = int(ev[0, 2] - ev[0, 1]) + 1
    frames = ev[:, 1:2] + torch.arange(n, device=x.device)[None, :]                                  # [E, n]
    seg = x[ev[:, 0, None, None], torch.arange(x.shape[1], device=x.device)[None, :, None], frames[:, None, :]].double()   # [E, F, n, 4]
    g = fac[ev[:, 0], :, ev[:, 1] // block].double()                                                 # [E, F, 4]
    a, b, c = g[..., 0:1], g[..., 1:2], torch.complex(g[..., 2:3], g[..., 3:4])
    x0, x1 = torch.complex(seg[..., 0], seg[..., 2]), torch.complex(seg[..., 1], seg[..., 3])
    z0, z1 = a * x0, b * (x1 - c * x0)
    p00, p11 = (z0.abs() ** 2).sum(-1, keepdim=True), (z1.abs() ** 2).sum(-1, keepdim=True)
    p10 = (z1 * z0.conj()).sum(-1, keepdim=True)
    k = torch.arange(x.shape[1], device=x.device)[:, None]
    lag = torch.arange(-max_lag, max_lag + 1, device=x.device)[None, :]
    period = 2 * (x.shape[1] - 1) * q
    phase = ((k * lag) % period).double() * (-2.0 * np.pi / period)
    s1 = b * (torch.polar(torch.ones_like(phase), phase)[None] - c)
    term = (a ** 2 * p00 + s1.abs() ** 2 * p11 + 2 * a * (s1.conj() * p10).real) / (a ** 2 + s1.abs() ** 2)
    return torch.where(a != 0, term, torch.zeros_like(term)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="locate_bench_out")
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import frontend as FE
    if not torch.cuda.is_available():
        raise SystemExit("bench_locate needs a ROCm device: nothing is measured without one")
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
    plan = FE.FrontendPlan(1024, 256, 64, 16000, 2, B, 1024, dev)
    fac = plan.whiten_factors(x, BLOCK)
    calls = {"locate": lambda: plan.locate(x, events, fac, BLOCK, 0, F, MAX_LAG, Q),
             "torch_float64": lambda: torch_locate(x, fac, events, BLOCK, MAX_LAG, Q),
             "whiten_factors": lambda: plan.whiten_factors(x, BLOCK)}
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
    curve = plan.locate(x, events, fac, BLOCK, 0, F, MAX_LAG, Q)[0]
    want = torch_locate(x, fac, events, BLOCK, MAX_LAG, Q)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"batch": B, "bins": F, "frames": T, "block": BLOCK, "events": args.events, "event_frames": n, "lags": 2 * MAX_LAG + 1,
           "locate_ms": med["locate"], "locate_ms_min_max": [min(times["locate"]), max(times["locate"])],
           "torch_float64_ms": med["torch_float64"], "torch_float64_ms_min_max": [min(times["torch_float64"]), max(times["torch_float64"])],
           "whiten_factors_ms": med["whiten_factors"],
           "whiten_factors_ms_min_max": [min(times["whiten_factors"]), max(times["whiten_factors"])],
           "torch_over_locate": med["torch_float64"] / med["locate"], "locate_over_whiten_factors": med["locate"] / med["whiten_factors"],
           "event_bytes_read": 16 * F * n * args.events, "spectrum_bytes": 16 * B * F * T,
           "max_rel_diff_vs_torch_float64": float(((curve - want).abs() / want.abs().max()).max())}
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_locate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
