"""detect() against the per-file loop it replaces: inference.predict_frames + the host decode (get_start_end_frame,
output_to_metric, get_start_end_time) on 6 synthetic stereo recordings of 186-231 s, v9 defaults (80 mel, 2 channels,
n_frame 512, overlap_hop 512).  Also times the decode step alone: iris_decode_events on the stacked window outputs against
the torch chain behind the forward (repeat_interleave, two overlap_and_add, divide, pools, threshold, copy, run search).
Prints one JSON line.      usage: python3 scripts/bench_detect.py [reps]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from challenge_amd import data_utils as D, detect as DT, inference as I, metrics as M, sj_train as S

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda", 0)
S.configure_miopen()
cfg = S.ARGS().get(['--v', '9'])
torch.manual_seed(0)
model = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last).eval()
rng = np.random.default_rng(0)
items = [(f"f{i}", (rng.standard_normal((2, int(16000 * s))) * 0.1).astype(np.float32))
         for i, s in enumerate([186.0, 193.5, 201.2, 212.8, 224.4, 231.0])]


def loop():
    out = []
    for name, wav in items:
        feats = I.features_for_eval(D.load_wav_array(wav, 16000, dev), cfg)
        d = I.predict_frames(model, feats, cfg, 512)
        ev = M.Challenge_Metric().get_start_end_frame(d.cpu().numpy())
        out.append((M.output_to_metric(256, 16000)(*ev), DT._FromEvents(ev).get_start_end_time(None)))
    return out


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


t_loop, _ = timed(loop)
t_det, _ = timed(lambda: DT.detect(model, items, cfg))

# decode alone, on the same window outputs
wins, lens = [], []
for _, wav in items:
    feats = I.features_for_eval(D.load_wav_array(wav, 16000, dev), cfg)
    lens.append(int(feats.shape[-2]))
    wins.append(I.frame(feats, 512, 512, pad_end=True, axis=-2).permute(1, 0, 2, 3)[..., :cfg.n_chan].contiguous())
preds = [model.predict(w, batch_size=32) for w in wins]
stacked = torch.cat(preds).contiguous()
win_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in preds])])


def torch_chain():
    for p, t in zip(preds, lens):
        x = p.repeat_interleave(512 // p.shape[-2], dim=-2).permute(2, 0, 1)
        cnt = I.overlap_and_add(torch.ones_like(x), 512)[..., :t]
        d = (I.smooth((I.overlap_and_add(x, 512)[..., :t] / cnt).t()) >= 0.5).to(torch.float32)
        M.Challenge_Metric().get_start_end_frame(d.cpu().numpy())


t_chain, _ = timed(torch_chain)
t_dec, _ = timed(lambda: DT.decode_events(stacked, win_off, lens, 512, 512))
lay = DT.DecodeLayout(win_off, lens, 3)
meta, bits, out = lay.buffers(dev)
DT.launch_decode(stacked, lay, meta, bits, out, 512, 512)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(100):
    DT.launch_decode(stacked, lay, meta, bits, out, 512, 512)
torch.cuda.synchronize()
t_launch = (time.perf_counter() - t0) / 100
same = all(np.array_equal(a, b) for x, y in zip(DT.decode_events(stacked, win_off, lens, 512, 512),
                                                 DT.decode_events(stacked.cpu(), win_off, lens, 512, 512)) for a, b in zip(x, y))
res = {"files": len(items), "frames": lens, "reps": reps,
       "loop_ms_per_file": 1e3 * t_loop / len(items), "detect_ms_per_file": 1e3 * t_det / len(items),
       "torch_decode_chain_ms_all_files": 1e3 * t_chain, "decode_events_ms_all_files": 1e3 * t_dec,
       "decode_launches_back_to_back_us": 1e6 * t_launch, "kernel_equals_host_restatement": bool(same)}
print(json.dumps(res))
