"""iris_decode_events_hmm beside iris_decode_events on the same window predictions: 64 files x 3750 frames x 3 classes,
n_frame 512, overlap_hop 512, 16 model outputs per window; the pooling decoder at the reference constants (0.5, 31, 124), the
HMM decoder at its defaults (0.5, 8 nats).  Both are two launches into caller-owned buffers.  After a warm-up of each, the two
are alternated in rounds: each round times `launches` back-to-back calls of one decoder between two device events, then the same
for the other; the figure is the median over the rounds of the time per call (both launches).  Checks first that the HMM launches
equal the CPU restatement on these inputs.  Prints one JSON line.
    usage: python3 scripts/bench_hmm.py [rounds] [launches]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from challenge_amd import detect as DT

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
dev = torch.device("cuda", 0)
N_FILES, T_LEN, K, N_FRAME, HOP, N_OUT = 64, 3750, 3, 512, 512, 16

rng = np.random.default_rng(0)
n_win = -(-T_LEN // HOP)
chunks = []
for _ in range(N_FILES):       # frames follow random on / off runs (levels 0.12 / 0.88 plus noise per model output)
    on = np.cumsum(rng.random((n_win * N_FRAME, K)) < 1.0 / 150.0, 0) % 2 == 1
    idx = np.arange(n_win)[:, None] * HOP + np.arange(N_OUT)[None, :] * (N_FRAME // N_OUT)
    chunks.append(np.where(on, 0.88, 0.12)[idx] + 0.25 * rng.standard_normal((n_win, N_OUT, K)))
preds_host = torch.from_numpy(np.concatenate(chunks).astype(np.float32))
preds = preds_host.to(dev)
win_off = np.arange(N_FILES + 1) * n_win
lens = [T_LEN] * N_FILES

settings = DT.HmmSettings.default(K)
lay = DT.DecodeLayout(win_off, lens, K)
meta, bits, out = lay.buffers(dev)
work = torch.empty(2 * lay.n_words, dtype=torch.int64, device=dev)
lut = torch.from_numpy(DT.hmm_lut()).to(dev)
pool = lambda: DT.launch_decode(preds, lay, meta, bits, out, N_FRAME, HOP)
hmm = lambda: DT.launch_decode_hmm(preds, lay, meta, lut, work, bits, out, N_FRAME, HOP, settings)

hmm()
got = lay.parse(out.cpu().numpy())
want = DT.decode_events_hmm(preds_host, win_off, lens, N_FRAME, HOP, settings)
same = all(np.array_equal(a, b) for x, y in zip(got, want) for a, b in zip(x, y))
assert same, "the HMM launches do not equal the CPU restatement"
n_hmm = sum(len(c) for f in got for c in f)
pool()
n_pool = sum(len(c) for f in lay.parse(out.cpu().numpy()) for c in f)


def per_call_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


for fn in (pool, hmm):         # warm-up of both at the timed shape
    per_call_us(fn)
t_pool, t_hmm = [], []
for _ in range(rounds):
    t_pool.append(per_call_us(pool))
    t_hmm.append(per_call_us(hmm))
print(json.dumps({"files": N_FILES, "frames_per_file": T_LEN, "classes": K, "overlap_hop": HOP, "rounds": rounds,
                  "launches_per_round": launches, "pool_decoder_us_per_call_median": float(np.median(t_pool)),
                  "pool_decoder_us_min_max": [min(t_pool), max(t_pool)],
                  "hmm_decoder_us_per_call_median": float(np.median(t_hmm)), "hmm_decoder_us_min_max": [min(t_hmm), max(t_hmm)],
                  "hmm_over_pool": float(np.median(t_hmm) / np.median(t_pool)), "events_pool": n_pool, "events_hmm": n_hmm,
                  "hmm_equals_host_restatement": bool(same)}))
