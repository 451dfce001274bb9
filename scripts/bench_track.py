"""Delay tracking on one MI355X: the three new launches of K19 - `FrontendPlan.locate_steps` (the table upload,
`k_locate_moments<steps>`, `k_track_scan`), `FrontendPlan.track` (`k_track_viterbi`) and `FrontendPlan.beamform_frames`
(`k_beamform_frames`) - over 64 events of 64 frames in a 4 x 257 x 2048 stereo spectrum with 81 lags (max_lag 40, q 8), steps of
16 frames and the whitening factors of blocks of 512 frames; and, beside each in the same process and on the same data, a torch
float64 restatement of the same definition on the device (what one would write without the kernels).  For comparison also the
per-event launches they stand beside: `FrontendPlan.locate` and `FrontendPlan.beamform`.  The calls alternate and are timed
with device events (medians; min and max beside them); the results of kernel and restatement are compared.  Prints one JSON
line and writes it under the output directory.

usage: python3 scripts/bench_track.py [--out DIR] [--events 64] [--frames 64] [--reps 20]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np

from bench_locate import torch_locate

SEED = 7
B, F, T, BLOCK, STEP, MAX_LAG, Q = 4, 257, 2048, 512, 16, 40, 8
PENALTY, MAX_JUMP = 0.03, 41


def torch_viterbi(resp, pen, jump):
    """resp [E, U, L] float64 on the device -> path [E, U]: the recurrence with a dense [E, L, L] candidate table per step."""
    import torch
    e, u_n, lags = resp.shape
    idx = torch.arange(lags, device=resp.device)
    dist = (idx[:, None] - idx[None, :]).abs()                                  # [n, n']
    cost = torch.where(dist <= jump, dist.double() * pen, torch.full_like(dist, float("inf"), dtype=torch.float64))
    d, back = resp[:, 0], []
    for u in range(1, u_n):
        best, arg = (d[:, None, :] - cost[None]).max(-1)
        d = best + resp[:, u]
        back.append(arg)
    path = [d.argmax(-1)]
    for arg in reversed(back):
        path.append(arg.gather(1, path[-1][:, None])[:, 0])
    return torch.stack(path[::-1], 1)


def torch_beamform_frames(x, fac, events, tdoa, block):
    """Events of equal length inside one block each, tdoa [E, n] float64 on the device -> Y [E, F, n] complex128."""
    import torch
    ev = torch.as_tensor(events, device=x.device, dtype=torch.int64)
    n, f = int(ev[0, 2] - ev[0, 1]) + 1, x.shape[1]
    frames = ev[:, 1:2] + torch.arange(n, device=x.device)[None, :]
    seg = x[ev[:, 0, None, None], torch.arange(f, device=x.device)[None, :, None], frames[:, None, :]].double()      # [E, F, n, 4]
    g = fac[ev[:, 0], :, ev[:, 1] // block].double()
    a, b, c = g[..., 0:1], g[..., 1:2], torch.complex(g[..., 2:3], g[..., 3:4])
    x0, x1 = torch.complex(seg[..., 0], seg[..., 2]), torch.complex(seg[..., 1], seg[..., 3])
    r = torch.arange(f, device=x.device, dtype=torch.float64)[None, :, None] * tdoa[:, None, :] / (2.0 * (f - 1))
    r = r - torch.round(r)
    e = torch.polar(torch.ones_like(r), -2.0 * np.pi * r)
    s1 = b * (e - c)
    den = a ** 2 + s1.abs() ** 2
    g1 = b * s1.conj() / den
    return (a ** 2 / den - g1 * c) * x0 + g1 * x1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="track_bench_out")
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from challenge_amd import frontend as FE
    if not torch.cuda.is_available():
        raise SystemExit("bench_track needs a ROCm device: nothing is measured without one")
    if args.frames % STEP or args.frames > BLOCK:
        raise SystemExit(f"--frames must be a multiple of {STEP} up to {BLOCK}: the restatement takes steps of equal length")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    x = torch.randn((B, F, T, 4), device=dev, generator=gen)
    x[..., 1] = 0.9 * x[..., 0] + 0.1 * x[..., 1]        # a coherent pair, as a dominant interferer makes it
    x[..., 3] = 0.9 * x[..., 2] + 0.1 * x[..., 3]
    rng = np.random.default_rng(SEED)
    n, e, steps = args.frames, args.events, args.frames // STEP
    starts = STEP * rng.integers((BLOCK - n) // STEP + 1, size=e)               # on a step boundary, inside one block
    events = np.array([[rng.integers(B), BLOCK * j + s, BLOCK * j + s + n - 1] for j, s in zip(rng.integers(T // BLOCK, size=e), starts)],
                      np.int32)
    step_events = np.array([[b, first + STEP * u, first + STEP * (u + 1) - 1] for b, first, _ in events for u in range(steps)], np.int32)
    plan = FE.FrontendPlan(512, 256, 64, 16000, 2, B, 512, dev)
    fac = plan.whiten_factors(x, BLOCK)
    lags, pen = 2 * MAX_LAG + 1, PENALTY * F * STEP / Q
    resp, _, offsets = plan.locate_steps(x, events, fac, BLOCK, STEP, 0, F, MAX_LAG, Q)
    delays = torch.from_numpy(np.linspace(rng.uniform(-4, 4, e), rng.uniform(-4, 4, e), n, axis=1)).to(dev)       # [E, n]
    flat_delays, static = delays.reshape(-1).cpu().numpy(), delays[:, 0].cpu().numpy()
    calls = {"locate_steps": lambda: plan.locate_steps(x, events, fac, BLOCK, STEP, 0, F, MAX_LAG, Q),
             "locate_steps_torch_float64": lambda: torch_locate(x, fac, step_events, BLOCK, MAX_LAG, Q),
             "locate": lambda: plan.locate(x, events, fac, BLOCK, 0, F, MAX_LAG, Q),
             "track": lambda: plan.track(resp, offsets, pen, MAX_JUMP),
             "track_torch_float64": lambda: torch_viterbi(resp.view(e, steps, lags), pen, MAX_JUMP),
             "beamform_frames": lambda: plan.beamform_frames(x, events, flat_delays, fac, BLOCK),
             "beamform_frames_torch_float64": lambda: torch_beamform_frames(x, fac, events, delays, BLOCK),
             "beamform": lambda: plan.beamform(x, events, static, fac, BLOCK)}
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
    want = torch_locate(x, fac, step_events, BLOCK, MAX_LAG, Q)
    path, path_t = plan.track(resp, offsets, pen, MAX_JUMP).long(), torch_viterbi(resp.view(e, steps, lags), pen, MAX_JUMP).reshape(-1)
    slabs = torch.stack(plan.beamform_frames(x, events, flat_delays, fac, BLOCK)).double()                          # [E, F, n, 2]
    y = torch_beamform_frames(x, fac, events, delays, BLOCK)
    res = {"batch": B, "bins": F, "frames": T, "block": BLOCK, "step": STEP, "events": e, "event_frames": n, "rows": e * steps,
           "lags": lags, "max_jump": MAX_JUMP}
    for name, v in times.items():
        res[name + "_ms"], res[name + "_ms_min_max"] = float(np.median(v)), [min(v), max(v)]
    for name in ("locate_steps", "track", "beamform_frames"):
        res[f"torch_over_{name}"] = res[name + "_torch_float64_ms"] / res[name + "_ms"]
    res["locate_steps_over_locate"] = res["locate_steps_ms"] / res["locate_ms"]
    res["beamform_frames_over_beamform"] = res["beamform_frames_ms"] / res["beamform_ms"]
    res["response_max_rel_diff_vs_torch_float64"] = float(((resp - want).abs() / want.abs().max()).max())
    res["path_rows_equal_to_torch"] = int((path == path_t).sum())
    res["slab_max_rel_diff_vs_torch_float64"] = float((torch.complex(slabs[..., 0], slabs[..., 1]) - y).abs().max() / y.abs().max())
    line = json.dumps(res)
    with open(os.path.join(args.out, "bench_track.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
