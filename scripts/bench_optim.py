"""What `--optimizer sgd` / `--optimizer rmsprop` cost with the one-launch tail and the captured step ("sgd and rmsprop in
the optimiser's launch").

    rocprofv3 --kernel-trace --stats -f csv -d prof_optim -- python scripts/bench_optim.py --kernel
    python scripts/bench_optim.py --report prof_optim
    python scripts/bench_optim.py --step

--kernel   for sgd and rmsprop, without and with a weight EMA, on the CRNN's table (v9, 64 mel x 512 frames, mono): 60 launches of
           the one-launch tail (iris_agc_clip_sgd / _rmsprop / their _ema siblings), 60 tails of the path before it (iris_agc_clip,
           torch's multi-tensor step, one lerp per parameter with the EMA), then the 60 launches again: the second run gives the
           run-to-run spread of the session.  Run it under rocprofv3 --kernel-trace, in a run of its own.
--report   from rocprofv3's kernel trace in DIR: per configuration the median device time of tails 11-59 of each of the three runs
           (the AGC kernel alone, and the sum over the tail's kernels: torch's launches and the lerps of the path before, the counter
           increments beside a one-launch tail), and the launch's bytes per parameter and bandwidth (--params N).
--step     the c4 training step (batch 64) by device events and by host time, per configuration: eager with IRIS_FUSED_OPTIM_AGC=0
           and the optimiser `make_optimizer(capturable=False)` builds - the step as it ran before the one-launch tail - against
           the replayed hipGraph with the capturable optimiser; each twice, median of 5 x 40 steps."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = ['--v', '9', '--n_mels', '64', '--n_frame', '512', '--n_chan', '1', '--batch_size', '64']
CONFIGS = [(kind, ema) for kind in ("sgd", "rmsprop") for ema in (False, True)]
BYTES = {"sgd": 24, "rmsprop": 32}   # p, g, b read and written (+ s); + 8 with the shadow


def model_on_device(kind, ema_decay=None, capturable=False):
    import torch
    from challenge_amd import sj_train as S
    from challenge_amd.ema import WeightEMA
    S.configure_miopen()
    cfg = S.ARGS().get(CFG + ['--optimizer', kind])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    ema = WeightEMA(model, ema_decay) if ema_decay else None
    model.compile(S.make_optimizer(cfg, model.parameters(), capturable=capturable), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=ema)
    return model, ema, cfg, dev


def kernel_runs():
    import torch
    from challenge_amd.hip_autograd import FusedAGC
    for kind, with_ema in CONFIGS:
        model, ema, cfg, dev = model_on_device(kind, 0.999 if with_ema else None)
        gen = torch.Generator(device=dev).manual_seed(1)
        for p in model.parameters():
            p.grad = torch.empty_like(p, memory_format=torch.preserve_format).copy_(torch.randn(p.shape, generator=gen, device=dev) * 1e-3)
        fused, plain = FusedAGC(list(model.parameters())), FusedAGC(list(model.parameters()))
        if with_ema:
            assert ema.attach(fused)
        assert fused.attach_optimizer(model.optimizer)
        torch.cuda.synchronize(dev)
        print(kind, "ema" if with_ema else "plain", sum(p.numel() for p in model.parameters()), "parameters")
        for run in ("launch", "before", "launch"):
            for _ in range(60):
                if run == "launch":
                    assert fused.optimizer_step(0.01, 1e-3, cfg.clipvalue)
                else:
                    plain(0.01, 1e-3, cfg.clipvalue)
                    model.optimizer.step()
                    if with_ema:
                        ema.update(model.optimizer)
            torch.cuda.synchronize(dev)
        del model, ema, fused, plain
        torch.cuda.empty_cache()


def report(directory, n_params=None):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0].split()[-1] for r in rows]
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    # a run = the launches of one AGC kernel in a row; whatever else runs between two of them belongs to the tail of the first
    # (torch's multi-tensor step and the lerps behind iris_agc_clip; the counter increments beside a one-launch tail).  The last
    # tail of a run also collects the next configuration's set-up kernels, so the medians stop at tail 59.
    runs = []
    for name, t in zip(names, us):
        if name.startswith("k_agc_clip"):
            if not runs or runs[-1]["name"] != name:
                runs.append({"name": name, "own": [], "rest": [], "kernels": []})
            runs[-1]["own"].append(t)
            runs[-1]["rest"].append(0.0)
            runs[-1]["kernels"].append(1)
        elif runs:
            runs[-1]["rest"][-1] += t
            runs[-1]["kernels"][-1] += 1
    for run in runs:
        own = run["own"][10:59]
        whole = [a + b for a, b in zip(run["own"], run["rest"])][10:59]
        if not own:
            continue
        name = run["name"]
        line = (f"{name}: {len(run['own'])} tails of {statistics.median(run['kernels'][10:59]):g} kernels; median of tails 11-59: the kernel "
                f"{statistics.median(own):.2f} us (min {min(own):.2f}, max {max(own):.2f}), the tail {statistics.median(whole):.2f} us "
                f"(min {min(whole):.2f}, max {max(whole):.2f})")
        if n_params and name != "k_agc_clip":
            per = BYTES["sgd" if "sgd" in name else "rmsprop"] + (8 if name.endswith("_ema") else 0)
            line += f"; {per} bytes per parameter, {per * n_params / statistics.median(own) / 1e6:.2f} TB/s"
        print(line)
    if n_params is None:
        print("(bandwidth: pass --params N to --report, the parameter count --kernel printed)")


def step_times():
    import torch
    from challenge_amd import sj_train as S

    def timed(call, dev):
        meds, host = [], []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            t0 = time.perf_counter()
            for _ in range(40):
                call()
            host.append((time.perf_counter() - t0) / 40 * 1e3)
            b.record()
            torch.cuda.synchronize(dev)
            meds.append(a.elapsed_time(b) / 40)
        return meds, host

    for kind, with_ema in CONFIGS:
        for how in ("eager-before", "graph", "eager-before", "graph"):
            graph = how == "graph"
            S.FUSED_OPTIM = graph
            try:
                model, ema, cfg, dev = model_on_device(kind, 0.999 if with_ema else None, capturable=graph)
                gen = torch.Generator(device=dev).manual_seed(2)
                x = torch.rand(64, 64, 512, 1, generator=gen, device=dev)
                y = (torch.rand(64, 16, 3, generator=gen, device=dev) < 0.2).float()
                if graph:
                    assert S.graph_step_possible(model)
                    step = S.GraphedTrainStep(model, (x, y))
                    assert step._agc._kind == kind
                else:
                    assert not S.graph_step_possible(model)
                    step = model.train_step
                    for _ in range(5):
                        step((x, y))
                meds, host = timed(lambda: step((x, y)), dev)
            finally:
                S.FUSED_OPTIM = True
            print(f"{kind:7s} {'ema  ' if with_ema else 'plain'} {how:12s}: {statistics.median(meds):.3f} ms per step by device events "
                  f"(5 x 40: {', '.join(f'{m:.3f}' for m in meds)}); host {statistics.median(host):.3f} ms per step "
                  f"({', '.join(f'{h:.3f}' for h in host)})", flush=True)
            del step, model, ema
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--report", type=str, default=None)
    ap.add_argument("--params", type=int, default=None)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.kernel:
        kernel_runs()
    if args.report:
        report(args.report, args.params)
    if args.step:
        step_times()
