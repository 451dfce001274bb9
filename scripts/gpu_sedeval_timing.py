"""What the segment- / event-based validation counts cost.

    rocprofv3 --kernel-trace --stats -f csv -d prof_sed -- python scripts/gpu_sedeval_timing.py --kernel
    python scripts/gpu_sedeval_timing.py --report prof_sed
    python scripts/gpu_sedeval_timing.py --torch
    python scripts/gpu_sedeval_timing.py --val

--kernel   at (B, T, K) = (64, 512, 3): 60 updates of SedEval (iris_sed_counts: k_sed_extract + k_sed_score) with 1 threshold,
           60 with 9, 60 with 1 on the alternating row (T / 2 events per list: the matching walk's worst case), then the first
           again (the run-to-run spread of the session).  Run it under rocprofv3 --kernel-trace, in a run of its own.
--report   the median over updates 11-60 of each run and kernel from rocprofv3's kernel trace in DIR.
--torch    the same inputs through `metrics.sed_counts_host` on the GPU tensors (torch ops for activities, segments and run
           ends, one copy to the host, the matching there) and through the launches: device time per update from events around
           back-to-back updates, host launch cost included; the torch form's wall time beside it (it synchronises).
--val      `fit`'s validation pass on the v9 CRNN (64 mel x 512 frames, batch 64): device time per `test_step` without metrics
           and with sed_eval((0.5,)) compiled in, median of 5 x 16 steps, two models each."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (64, 512, 3)
NINE = tuple(i / 10 for i in range(1, 10))


def inputs(dev):
    import numpy as np
    import torch
    b, t, k = SHAPE
    rng = np.random.default_rng(0)
    yt = np.repeat(rng.random((b, t // 16, k)) < 0.3, 16, axis=1).astype(np.float32)     # block labels: 16-frame units
    z = (yt * 2 - 1) * 2 + np.repeat(rng.standard_normal((b, t // 4, k)), 4, axis=1) * 2
    yp = (1 / (1 + np.exp(-z))).astype(np.float32)
    alt = np.broadcast_to((np.arange(t) % 2 == 0).astype(np.float32)[None, :, None], (b, t, k)).copy()
    g = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    return [("sigmoid-like, 1 threshold", g(yt), g(yp), (0.5,)), ("sigmoid-like, 9 thresholds", g(yt), g(yp), NINE),
            ("alternating rows, 1 threshold", g(alt), g(alt), (0.5,)), ("sigmoid-like, 1 threshold again", g(yt), g(yp), (0.5,))]


def kernel_runs():
    import torch
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    for name, yt, yp, thr in inputs(dev):
        sed = M.SedEval(SHAPE[2], thr)
        for _ in range(60):
            sed.update(yt, yp)
        torch.cuda.synchronize(dev)
        c = sed.counts()
        print(f"{name}: 60 updates, {int(c[0, :3, 3:5].sum()) // 60} predicted and {int(c[0, :3, [3, 5]].sum()) // 60} reference events per update")


def report(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "k_sed_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("k_sed_extract", "k_sed_score"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        for i, name in enumerate(("1 threshold", "9 thresholds", "alternating rows", "1 threshold again")):
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
    from challenge_amd import metrics as M
    dev = torch.device("cuda", 0)
    for name, yt, yp, thr in inputs(dev)[:3]:
        sed = M.SedEval(SHAPE[2], thr)
        state = torch.zeros_like(sed.state(dev), device='cpu')

        def torch_update():
            state.add_(M.sed_counts_host(yt, yp, thr))
        torch_update(), sed.update(yt, yp)
        torch.cuda.synchronize(dev)
        assert torch.equal(state, sed.counts())
        h_ms, _ = _median_ms(lambda: sed.update(yt, yp), dev, 5, 40)
        walls = []
        for _ in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            torch_update()
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: iris_sed_counts {1e3 * h_ms:.1f} us per update (events around 40 back-to-back updates, host launch cost "
              f"included); sed_counts_host on the same GPU tensors {statistics.median(walls):.2f} ms wall per update (it ends in a copy "
              f"to the host and a host loop over the events)")


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
                      metrics=[M.sed_eval((0.5,), hop=S.output_hop(cfg))] if on else None)
        for _ in range(3):
            model.test_step((x, y))
        torch.cuda.synchronize(dev)
        med, meds = _median_ms(lambda: model.test_step((x, y)), dev, 5, 16)
        print(f"sed_eval {'on ' if on else 'off'}: {med:.3f} ms per validation step (5 x 16 steps: {', '.join(f'{m:.3f}' for m in meds)})")
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
