"""What the PSDS validation counts cost.

    rocprofv3 --kernel-trace --stats -f csv -d prof_psds -- python scripts/gpu_psds_timing.py --kernel
    python scripts/gpu_psds_timing.py --report prof_psds
    python scripts/gpu_psds_timing.py --torch
    python scripts/gpu_psds_timing.py --val

--kernel   60 updates of Psds (iris_psds_counts: k_psds_prep + k_psds_score, scenario 2, the 50 default thresholds) at each of
           (B, T, K) = (64, 512, 3), (64, 16, 3) - a validation batch - and (1, 40000, 3) - one recording of `evaluate` - then the
           first again (the run-to-run spread of the session).  Run it under rocprofv3 --kernel-trace, in a run of its own.
--report   the median over updates 11-60 of each run and kernel from rocprofv3's kernel trace in DIR, with min and max.
--torch    the same inputs through `metrics.psds_counts_host` on the GPU tensors (torch ops, threshold after threshold, one copy
           to the host) and through the launches: device time per update from events around back-to-back updates, host launch
           cost included; the torch form's wall time beside it (it synchronises); iris_sed_counts at 9 thresholds on the same
           shape beside both; and the workspace of each shape.
--val      `fit`'s validation pass on the v9 CRNN (64 mel x 512 frames, batch 64): device time per `test_step` without metrics
           and with psds(2) compiled in, median of 5 x 16 steps, two models each."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((64, 512, 3), (64, 16, 3), (1, 40000, 3))
NINE = tuple(i / 10 for i in range(1, 10))
SCENARIO = 2


def inputs(dev):
    import numpy as np
    import torch
    out = []
    for b, t, k in SHAPES:
        rng = np.random.default_rng(t)
        unit = 16 if t >= 512 else 4
        yt = np.repeat(rng.random((b, t // unit, k)) < 0.3, unit, axis=1).astype(np.float32)   # block labels
        z = (yt * 2 - 1) * 2 + np.roll(yt, 1, axis=2) + np.repeat(rng.standard_normal((b, t // 4, k)), 4, axis=1) * 2
        yp = (1 / (1 + np.exp(-z))).astype(np.float32)
        out.append((f"{b} x {t} x {k}", torch.from_numpy(yt).to(dev), torch.from_numpy(yp).to(dev)))
    return out + [(out[0][0] + " again",) + out[0][1:]]


def kernel_runs():
    import torch
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    for name, yt, yp in inputs(dev):
        p = M.Psds(yt.shape[2], SCENARIO)
        for _ in range(60):
            p.update(yt, yp)
        torch.cuda.synchronize(dev)
        c = p.counts()
        print(f"{name}: 60 updates, {int(c[50, :, 0].sum()) // 60} ground-truth events and {int(c[:50, :, -1].sum()) // 60} detections "
              f"(over 50 thresholds) per update")


def report(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "k_psds_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [f"{b} x {t} x {k}" for b, t, k in SHAPES] + ["%d x %d x %d again" % SHAPES[0]]
    for kernel in ("k_psds_prep", "k_psds_score"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        for i, name in enumerate(names):
            tail = us[60 * i + 10:60 * i + 60]
            if tail:
                print(f"{kernel}, {name}: median of launches 11-60 {statistics.median(tail):.2f} us (min {min(tail):.2f}, max {max(tail):.2f})")
        print(kernel, len(us), "launches in all")


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
    from challenge_amd import _native as N
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    for name, yt, yp in inputs(dev)[:3]:
        p = M.Psds(yt.shape[2], SCENARIO)
        sed = M.SedEval(yt.shape[2], NINE)
        state = torch.zeros_like(p.state(dev), device='cpu')

        def torch_update():
            state.add_(M.psds_counts_host(yt, yp, p.thresholds, p.dtc_pct, p.gtc_pct, p.cttc_pct))
        torch_update(), p.update(yt, yp), sed.update(yt, yp)
        torch.cuda.synchronize(dev)
        assert torch.equal(state, p.counts())
        h_ms, h_all = _median_ms(lambda: p.update(yt, yp), dev, 5, 40)
        s_ms, _ = _median_ms(lambda: sed.update(yt, yp), dev, 5, 40)
        walls = []
        for _ in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            torch_update()
            walls.append(1e3 * (time.perf_counter() - t0))
        b, t, k = yt.shape
        print(f"{name}: iris_psds_counts {1e3 * h_ms:.1f} us per update (events around 40 back-to-back updates, host launch cost "
              f"included; 5 runs: {', '.join(f'{1e3 * m:.1f}' for m in h_all)}); psds_counts_host on the same GPU tensors "
              f"{statistics.median(walls):.2f} ms wall per update (min {min(walls):.2f}; it ends in a copy to the host); iris_sed_counts at 9 "
              f"thresholds {1e3 * s_ms:.1f} us; workspace {int(N.lib().iris_psds_workspace_bytes(b, t, k, 50))} bytes")


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
    for on in (False, True, False, True):
        torch.manual_seed(0)
        model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
        model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                      metrics=[M.psds(SCENARIO, hop=S.output_hop(cfg))] if on else None)
        for _ in range(3):
            model.test_step((x, y))
        torch.cuda.synchronize(dev)
        med, meds = _median_ms(lambda: model.test_step((x, y)), dev, 5, 16)
        print(f"psds {'on ' if on else 'off'}: {med:.3f} ms per validation step (5 x 16 steps: {', '.join(f'{m:.3f}' for m in meds)})")
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
