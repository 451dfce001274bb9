"""What the weight EMA costs ("Weight EMA in the optimiser's launch").

    rocprofv3 --kernel-trace --stats -f csv -d prof_ema -- python scripts/gpu_ema_timing.py --kernel
    python scripts/gpu_ema_timing.py --report prof_ema
    python scripts/gpu_ema_timing.py --step

--kernel   60 launches of iris_agc_clip_adam on the CRNN's table (v9, 64 mel x 512 frames, mono), 60 of iris_agc_clip_adam_ema on the
           same table with a shadow column, then 60 of iris_agc_clip_adam again: the second run of the parent gives the run-to-run
           spread of the session.  Run it under rocprofv3 --kernel-trace, in a run of its own.
--report   the median over launches 11-60 of each of the three runs from rocprofv3's kernel trace in DIR.
--step     the c4 training step as a replayed hipGraph (batch 64), with and without an EMA compiled in: median of 5 x 40 replays."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = ['--v', '9', '--n_mels', '64', '--n_frame', '512', '--n_chan', '1', '--batch_size', '64']


def model_on_device(ema_decay=None, capturable=False):
    import torch
    from challenge_amd import sj_train as S
    from challenge_amd.ema import WeightEMA
    S.configure_miopen()
    cfg = S.ARGS().get(CFG)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    ema = WeightEMA(model, ema_decay) if ema_decay else None
    model.compile(S.make_optimizer(cfg, model.parameters(), capturable=capturable), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=ema)
    return model, ema, cfg, dev


def kernel_runs():
    import torch
    from challenge_amd.hip_autograd import FusedAGC
    model, ema, cfg, dev = model_on_device(0.999)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in model.parameters():
        p.grad = torch.empty_like(p, memory_format=torch.preserve_format).copy_(torch.randn(p.shape, generator=gen, device=dev) * 1e-3)
    agc = FusedAGC(list(model.parameters()))
    print(sum(p.numel() for p in model.parameters()), "parameters")
    for shadow in (None, ema.shadow, None):
        agc.attach_ema(shadow, ema.decay) if shadow is not None else agc.attach_ema(None)
        assert agc.attach_adam(model.optimizer)
        for _ in range(60):
            assert agc.adam_step(0.01, 1e-3, cfg.clipvalue)
        torch.cuda.synchronize(dev)
        print("60 launches,", agc._table.shape[1], "columns")


def report(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "k_agc_clip_adam" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    runs, last = [], None
    for r in rows:   # consecutive launches of one kernel form a run
        name = r["Kernel_Name"].split("(")[0]
        if name != last:
            runs.append((name, []))
            last = name
        runs[-1][1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in runs:
        tail = us[10:60]
        print(f"{name}: {len(us)} launches; median of launches 11-60 {statistics.median(tail):.2f} us (min {min(tail):.2f}, max {max(tail):.2f})")


def step_times():
    import torch
    from challenge_amd import sj_train as S
    out = {}
    for decay in (None, 0.999, None, 0.999):
        model, ema, cfg, dev = model_on_device(decay, capturable=True)
        gen = torch.Generator(device=dev).manual_seed(2)
        x = torch.rand(64, 64, 512, 1, generator=gen, device=dev)
        y = (torch.rand(64, 16, 3, generator=gen, device=dev) < 0.2).float()
        step = S.GraphedTrainStep(model, (x, y))
        meds = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(40):
                step((x, y))
            b.record()
            torch.cuda.synchronize(dev)
            meds.append(a.elapsed_time(b) / 40)
        out.setdefault("ema" if decay else "plain", []).append(statistics.median(meds))
        six = step._agc._table.shape[1]
        print(f"{'--ema 0.999' if decay else 'no EMA    '}: {statistics.median(meds):.3f} ms per replayed step (5 x 40 replays: "
              f"{', '.join(f'{m:.3f}' for m in meds)}); table columns {six}")
        del step, model, ema
        torch.cuda.empty_cache()
    print("plain", out["plain"], "ema", out["ema"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--report", type=str, default=None)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.kernel:
        kernel_runs()
    if args.report:
        report(args.report)
    if args.step:
        step_times()
