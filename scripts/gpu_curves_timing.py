"""What the validation score histogram costs.

    rocprofv3 --kernel-trace --stats -f csv -d prof_curves -- python scripts/gpu_curves_timing.py --kernel
    python scripts/gpu_curves_timing.py --report prof_curves
    python scripts/gpu_curves_timing.py --torch
    python scripts/gpu_curves_timing.py --val

--kernel   at (B, T, K, bins) = (64, 512, 3, 1024): 60 launches of iris_score_hist on uniform scores, 60 with every score at 1.0
           (all of a class in one slot), 60 on sigmoid-like scores piled up at both ends, then the uniform ones again: the second
           uniform run gives the run-to-run spread of the session.  Run it under rocprofv3 --kernel-trace, in a run of its own.
--report   the median over launches 11-60 of each run from rocprofv3's kernel trace in DIR.
--torch    the same inputs through the torch form of `ScoreHistogram.update` (metrics.score_hist_host on GPU tensors: floor,
           clamp, where, bincount ...) and through the launch, device time per update from events: median of 5 x 40 updates.
--val      `fit`'s validation pass on the v9 CRNN (64 mel x 512 frames, batch 64): device time per `test_step` without metrics
           and with score_curves(1024) compiled in, median of 5 x 16 steps, two models each."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (64, 512, 3, 1024)


def inputs(dev):
    import numpy as np
    import torch
    b, t, k, _ = SHAPE
    rng = np.random.default_rng(0)
    yt = torch.from_numpy((rng.random((b, t, k)) < 0.3).astype(np.float32)).to(dev)
    uniform = torch.from_numpy(rng.random((b, t, k)).astype(np.float32)).to(dev)
    ones = torch.ones(b, t, k, device=dev)
    z = rng.standard_normal((b, t, k)) * 6 + (yt.cpu().numpy() * 2 - 1) * 2
    sharp = torch.from_numpy((1 / (1 + np.exp(-z))).astype(np.float32)).to(dev)
    return yt, [("uniform", uniform), ("all 1.0", ones), ("sigmoid-like", sharp), ("uniform again", uniform)]


def kernel_runs():
    import torch
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    yt, cases = inputs(dev)
    for name, yp in cases:
        h = M.ScoreHistogram(SHAPE[2], SHAPE[3])
        for _ in range(60):
            h.update(yt, yp)
        torch.cuda.synchronize(dev)
        c = h.counts()
        print(f"{name}: 60 launches, {int(c.sum())} counts, {int((c > 0).sum())} occupied slots")


def report(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "k_score_hist" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    for i, name in enumerate(("uniform", "all 1.0", "sigmoid-like", "uniform again")):
        tail = us[60 * i + 10:60 * i + 60]
        if tail:
            print(f"k_score_hist, {name}: median of launches 11-60 {statistics.median(tail):.2f} us (min {min(tail):.2f}, max {max(tail):.2f})")
    print(len(us), "launches in all")


def _median_ms(fn, dev, reps, inner):
    import torch
    meds = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        meds.append(a.elapsed_time(b) / inner)
    return statistics.median(meds), meds


def torch_form():
    import torch
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    yt, cases = inputs(dev)
    k, bins = SHAPE[2], SHAPE[3]
    for name, yp in cases[:3]:
        state = torch.zeros(k, 2, bins + 1, dtype=torch.int64, device=dev)
        h = M.ScoreHistogram(k, bins)

        def torch_update():
            state.add_(M.score_hist_host(yt, yp, bins))
        torch_update(), h.update(yt, yp)
        torch.cuda.synchronize(dev)
        assert torch.equal(state, h.state(dev))
        t_ms, _ = _median_ms(torch_update, dev, 5, 40)
        h_ms, _ = _median_ms(lambda: h.update(yt, yp), dev, 5, 40)
        print(f"{name}: torch form {1e3 * t_ms:.1f} us per update, iris_score_hist {1e3 * h_ms:.1f} us per update (events around 40 "
              f"back-to-back updates, host launch cost included)")


def val_pass():
    import torch
    from challenge_amd import metrics as M
    from challenge_amd import sj_train as S
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_frame', '512', '--n_chan', '1', '--batch_size', '64'])
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2)
    x = torch.rand(64, 64, 512, 1, generator=gen, device=dev)
    y = (torch.rand(64, 16, 3, generator=gen, device=dev) < 0.2).float()
    for bins in (0, 1024, 0, 1024):
        torch.manual_seed(0)
        model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
        model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                      metrics=[M.score_curves(bins)] if bins else None)
        for _ in range(3):
            model.test_step((x, y))
        torch.cuda.synchronize(dev)
        med, meds = _median_ms(lambda: model.test_step((x, y)), dev, 5, 16)
        print(f"--curves {bins:4d}: {med:.3f} ms per validation step (5 x 16 steps: {', '.join(f'{m:.3f}' for m in meds)})")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--report", type=str, default=None)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--val", action="store_true")
    args = ap.parse_args()
    if args.kernel:
        kernel_runs()
    if args.report:
        report(args.report)
    if args.torch:
        torch_form()
    if args.val:
        val_pass()
