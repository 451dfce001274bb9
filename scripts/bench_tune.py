"""sweep_decoder (one iris_decode_sweep call) against the form it replaces - one decode_events call per grid point plus the
host get_er per file - on the same device tensors: the default grid (511 points), K = 3, files of about 1,900 frames
(n_frame 512, overlap_hop 512, 16 model outputs per window), 16 and 64 files.  Wall time around the call plus a device
synchronise, the two forms alternated, median over the repeats after a warm-up.  Checks first that the two forms agree on the
counts.  Prints one JSON line per size.
    usage: python3 scripts/bench_tune.py [reps] [loop_reps] [--sweep-only]
(--sweep-only: a few sweep calls per size and nothing else, for a kernel-trace run of the two kernels.)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from challenge_amd import detect as DT, metrics as M

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if len(args) > 0 else 20
loop_reps = int(args[1]) if len(args) > 1 else 20
sweep_only = "--sweep-only" in sys.argv
dev = torch.device("cuda", 0)
HOP, SR, N_FRAME, N_OUT = 256, 16000, 512, 16
grid = DT.decoder_grid()


def make(n_files, seed):
    """Window outputs whose frames follow random on / off runs (levels 0.12 / 0.88 plus noise per window), and as ground truth
    the seconds of those runs."""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1800, 2000, n_files)]
    chunks, win_off, gt = [], [0], []
    for t_len in lens:
        n_win = -(-t_len // N_FRAME)
        span = n_win * N_FRAME
        flips = rng.random((span, 3)) < 1.0 / 150.0
        on = np.cumsum(flips, 0) % 2 == 1
        idx = np.arange(n_win)[:, None] * N_FRAME + np.arange(N_OUT)[None, :] * (N_FRAME // N_OUT)
        chunks.append(np.where(on, 0.88, 0.12)[idx] + 0.25 * rng.standard_normal((n_win, N_OUT, 3)))
        win_off.append(win_off[-1] + n_win)
        rows = []
        for c in range(3):
            e = np.diff(np.concatenate([[0], on[:t_len, c].astype(np.int8), [0]]))
            for s, t in zip(np.flatnonzero(e == 1), np.flatnonzero(e == -1) - 1):
                rows.append([c, int(s * HOP / SR), int(np.ceil(t * HOP / SR))])
        gt.append(rows or [[0, 0, 1]])
    return torch.from_numpy(np.concatenate(chunks).astype(np.float32)).to(dev), np.asarray(win_off), lens, gt


def loop_form(preds, win_off, lens, gt):
    """What the parent commit offers: per grid point the decoder's launches and copy back, then get_er per file."""
    er = np.empty((len(grid), len(lens)))
    for g, (thr, avg, mx) in enumerate(grid):
        for f, ev in enumerate(DT.decode_events(preds, win_off, lens, N_FRAME, N_FRAME, avg, mx, thr)):
            er[g, f] = M.get_er(gt[f], M.output_to_metric(HOP, SR)(*ev))
    return er


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for n_files in (16, 64):
    preds, win_off, lens, gt = make(n_files, n_files)
    sweep = lambda: DT.sweep_decoder(preds, win_off, lens, gt, grid, N_FRAME, N_FRAME)
    if sweep_only:          # 5 calls over the whole grid and 5 over its first 40 points: two kernels per call either way
        for _ in range(5):
            wall(sweep)
            wall(lambda: DT.sweep_decoder(preds, win_off, lens, gt, grid[:40], N_FRAME, N_FRAME))
        continue
    _, (n_pred, matched, n_gt) = wall(sweep)          # warm-up of both forms, and the check that they agree
    _, er = wall(lambda: loop_form(preds, win_off, lens, gt))
    mine = (n_pred + n_gt[None] - 2 * matched).sum(2) / n_gt.sum(1)[None]
    assert np.array_equal(mine, er), "the sweep's counts do not give the loop's get_er"
    t_sweep, t_loop = [], []
    for r in range(reps):
        t_sweep.append(wall(sweep)[0])
        if r < loop_reps:
            t_loop.append(wall(lambda: loop_form(preds, win_off, lens, gt))[0])
    lay = DT.SweepLayout(win_off, lens, 3, gt, grid)
    meta, p_ws, out = lay.buffers(dev)
    DT.launch_sweep(preds, lay, meta, p_ws, out, N_FRAME, N_FRAME)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        DT.launch_sweep(preds, lay, meta, p_ws, out, N_FRAME, N_FRAME)
    torch.cuda.synchronize()
    t_launch = (time.perf_counter() - t0) / 50
    print(json.dumps({"files": n_files, "frames": int(sum(lens)), "grid_points": len(grid), "classes": 3,
                      "sweep_decoder_ms_median": 1e3 * float(np.median(t_sweep)), "sweep_decoder_ms_min_max":
                      [1e3 * min(t_sweep), 1e3 * max(t_sweep)], "sweep_reps": reps,
                      "loop_ms_median": 1e3 * float(np.median(t_loop)), "loop_ms_all": [1e3 * t for t in t_loop],
                      "loop_reps": loop_reps, "launches_back_to_back_ms": 1e3 * t_launch,
                      "forms_agree": True}), flush=True)
