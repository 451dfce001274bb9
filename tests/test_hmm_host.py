"""CPU tests of the HMM event decoder: detect.decode_events_hmm's sequential restatement against hmm_ref (an independent
restatement in Python integers) and against brute force over all paths, NaN and tie rules, the pinned table values, the
settings files of both kinds, the argument checks (in Python and at the C ABI) and the command line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import hmm_ref as R
from challenge_amd import _native as N
from challenge_amd import detect as DT
from test_detect_host import assert_same_events, run_preds

CENTRE = lambda b: (np.asarray(b, np.float64) + 0.5) / 1024       # bucket centres: exact in fp32, far from a bucket edge


def frames_to_preds(sig):
    """Frame values sig [T, K] -> (preds [W, 64, K], win_off, [T]) with n_frame = hop = n_out = 64: p[t] is sig[t] itself (one
    window covers each frame: the fp32 sum from 0 of one value, divided by 1)."""
    sig = np.asarray(sig, np.float32)
    t_len, k = sig.shape
    n_win = max(-(-t_len // 64), 1)
    buf = np.zeros((n_win * 64, k), np.float32)
    buf[:t_len] = sig
    return torch.from_numpy(buf.reshape(n_win, 64, k)), [0, n_win], [t_len]


def small_lut(seed=None):
    """An integer table with entries in [-2, 2]: bucket i scores (i % 5) - 2 (or random ones)."""
    if seed is None:
        return (np.arange(1024) % 5 - 2).astype(np.int32)
    return np.random.default_rng(seed).integers(-2, 3, 1024).astype(np.int32)


def ref_events(preds, win_off, frame_lens, n_frame, hop, settings, lut):
    """hmm_ref on the overlap-add average of each file (step 1 is decode_core.h's, taken from detect._overlap_add_host)."""
    out = []
    for f, t_len in enumerate(frame_lens):
        k = preds.shape[2]
        if t_len == 0:
            out.append(tuple(np.zeros((0, 2), np.int64) for _ in range(k)))
            continue
        p = DT._overlap_add_host(preds, int(win_off[f]), int(win_off[f + 1] - win_off[f]), t_len, n_frame, hop).numpy()
        out.append(tuple(np.asarray(R.decode([float(x) for x in p[:, c]], lut, settings.threshold[c], settings.cost[c]),
                                    np.int64).reshape(-1, 2) for c in range(k)))
    return out


def units(c):
    """An event cost of c score units, in nats."""
    return c / 256.0


def test_pinned_values():
    lut = DT.hmm_lut()
    assert lut.dtype == np.int32 and lut.shape == (1024,)
    assert lut[511] == -1 and lut[512] == 1 and lut[0] == -1952 and lut[1023] == 1952
    assert np.array_equal(lut, -lut[::-1]) and (np.diff(lut) >= 0).all()
    assert lut.tolist() == R.default_lut()
    s = DT.HmmSettings.default(3)
    assert s.points() == [(0.5, 8.0)] * 3 and s.bias().tolist() == [0, 0, 0] and s.cost_units().tolist() == [2048] * 3
    t = DT.HmmSettings([0.3, 0.7, 0.999], [0.0, 2048.0, 1.0])
    assert t.bias().tolist() == [R.bias_of(x) for x in (0.3, 0.7, 0.999)] and t.cost_units().tolist() == [0, 1 << 19, 256]
    grid = DT.hmm_grid()
    assert grid[0] == (0.5, 8.0) and len(grid) == 41 and grid[1] == (DT._f32(0.3), 0.0) and grid[-1] == (DT._f32(0.7), 128.0)


def test_definition_against_brute_force():
    """The recurrence is a maximiser: on 300 short sequences under a small-integer table, the path decode_events_hmm returns
    (and hmm_ref's) reaches the best objective over all 2^T paths."""
    rng = np.random.default_rng(0)
    for case in range(300):
        t_len = int(rng.integers(1, 11))
        lut = small_lut(case)
        buckets = rng.integers(0, 1024, (t_len, 1))
        c = int(rng.integers(0, 7))
        e = [int(lut[b]) for b in buckets[:, 0]]
        best = R.brute_force_best(e, c)
        s_ref = R.viterbi(e, c)
        assert R.objective(e, s_ref, c) == best
        preds, win_off, lens = frames_to_preds(CENTRE(buckets))
        ev = DT.decode_events_hmm(preds, win_off, lens, 64, 64, DT.HmmSettings([0.5], [units(c)]), lut=lut)[0][0]
        assert ev.tolist() == R.runs(s_ref)
        s = np.zeros(t_len, np.int64)
        for a, b in ev:
            s[a:b + 1] = 1
        assert R.objective(e, s.tolist(), c) == best


@pytest.mark.parametrize("hop", [128, 256, 512])
@pytest.mark.parametrize("n_out", [512, 16])
def test_decode_matches_hmm_ref(hop, n_out):
    rng = np.random.default_rng(hop + n_out)
    frame_lens = [1000, 300, 0, 2049, 513, 1]       # T < n_frame, T not a multiple of 64 or of the hop, empty, one frame
    preds, win_off = run_preds(rng, frame_lens, 512, hop, n_out, noise=0.3, mean_run=40.0)
    preds = torch.from_numpy(preds)
    total = 0
    for settings in (DT.HmmSettings.default(3), DT.HmmSettings([0.3, 0.5, 0.7], [0.0, 2.0, 64.0])):
        got = DT.decode_events_hmm(preds, win_off, frame_lens, 512, hop, settings)
        assert_same_events(got, ref_events(preds, win_off, frame_lens, 512, hop, settings, R.default_lut()))
        total += sum(len(c) for f in got for c in f)
    assert total > 20


def test_values_outside_the_unit_interval_clamp():
    sig = np.array([[-0.5], [2.0], [np.inf], [-np.inf], [0.0], [1.0], [3e38], [1e-45]], np.float32)
    preds, win_off, lens = frames_to_preds(sig)
    lut = np.zeros(1024, np.int32)
    lut[0], lut[1023] = -7, 9
    got = DT.decode_events_hmm(preds, win_off, lens, 64, 64, DT.HmmSettings([0.5], [0.0]), lut=lut)
    assert got[0][0].tolist() == [[1, 2], [5, 6]]
    assert [R.score(float(x), lut, 0) for x in sig[:, 0]] == [-7, 9, 9, -7, -7, 9, 9, -7]


def test_nan_frame_is_off_and_splits_an_event():
    sig = np.full((300, 2), 0.9, np.float32)
    sig[117, 1] = np.nan
    preds, win_off, lens = frames_to_preds(sig)
    for cost in (0.0, 8.0, 300.0):
        s = DT.HmmSettings([0.5, 0.5], [cost, cost])
        got = DT.decode_events_hmm(preds, win_off, lens, 64, 64, s)
        assert got[0][0].tolist() == [[0, 299]]
        # a frame at 0.9 scores 562 (256 ln 9): the 182 frames after the NaN pay 300 nats, the 117 before it do not
        assert got[0][1].tolist() == ([[0, 116], [118, 299]] if cost < 300.0 else [[118, 299]])
        assert_same_events(got, ref_events(preds, win_off, lens, 64, 64, s, R.default_lut()))
    assert 117 * 562 < 300 * 256 < 182 * 562 and R.default_lut()[921] == 562
    # a NaN from one window reaches every frame that window covers with an overlap
    nan = np.full((3, 16, 1), 0.9, np.float32)
    nan[1, 3, 0] = np.nan                        # window 1 covers 256 .. 767; output 3 is its frames 96 .. 127
    got = DT.decode_events_hmm(torch.from_numpy(nan), [0, 3], [1024], 512, 256, DT.HmmSettings.default(1))
    assert got[0][0].tolist() == [[0, 351], [384, 1023]]


def test_zero_cost_follows_the_sign():
    """At C = 0 a frame with a positive score is on and one with a negative score is off; a zero score joins a neighbour."""
    rng = np.random.default_rng(5)
    lut = small_lut()
    buckets = rng.integers(0, 1024, (700, 3))
    preds, win_off, lens = frames_to_preds(CENTRE(buckets))
    got = DT.decode_events_hmm(preds, win_off, lens, 64, 64, DT.HmmSettings([0.5] * 3, [0.0] * 3), lut=lut)
    e = lut[buckets]
    assert (e == 0).sum() > 100
    for c in range(3):
        s = np.zeros(700, bool)
        for a, b in got[0][c]:
            s[a:b + 1] = True
        assert s[e[:, c] > 0].all() and not s[e[:, c] < 0].any()


TIE_CASES = [      # (scores, cost in units, the events the tie rules give)
    ([-1, 2, 2, -1], 4, []),                          # a run worth exactly C: stay off
    ([-1, 2, 3, -1], 4, [[1, 2]]),                    # ... worth C + 1: taken
    ([3, 3, -2, -2, 3, 3], 4, [[0, 5]]),              # a gap worth exactly -C: stay on
    ([3, 3, -2, -3, 3, 3], 4, [[0, 1], [4, 5]]),      # ... worth -C - 1: two events
    ([0, 0, 0, 0, 0], 0, []),                         # all zero: stay off, end off
    ([0, 0, 0, 0, 0], 3, []),
    ([2, 0, 0, 2], 0, [[0, 3]]),                      # zeros inside an event stay on
    ([0, 0, 2, 0, 0], 0, [[0, 2]]),                   # "end off" drops the zeros after an event; traced back, "stay on" keeps
    ([0, 2, 0, -1, 0], 0, [[0, 1]]),                  # the zeros before it
    ([5], 5, []), ([6], 5, [[0, 0]]), ([-1], 0, []),
]


def test_known_answer_ties():
    lut = (np.arange(1024) % 16 - 8).astype(np.int32)       # bucket b scores (b % 16) - 8: -8 .. 7
    for e, c, want in TIE_CASES:
        assert R.runs(R.viterbi(e, c)) == want, (e, c)
        assert R.objective(e, R.viterbi(e, c), c) == R.brute_force_best(e, c)
        preds, win_off, lens = frames_to_preds(CENTRE([[x + 8 + 16 * 7] for x in e]))
        got = DT.decode_events_hmm(preds, win_off, lens, 64, 64, DT.HmmSettings([0.5], [units(c)]), lut=lut)
        assert got[0][0].tolist() == want, (e, c)


def test_tie_heavy_long_sequences_match_hmm_ref():
    rng = np.random.default_rng(8)
    lut = small_lut()
    buckets = rng.integers(0, 5, (1500, 7))                  # scores -2 .. 2: almost every comparison is a tie
    preds, win_off, lens = frames_to_preds(CENTRE(buckets))
    s = DT.HmmSettings([0.5] * 7, [units(c) for c in range(7)])
    got = DT.decode_events_hmm(preds, win_off, lens, 64, 64, s, lut=lut)
    assert_same_events(got, ref_events(preds, win_off, lens, 64, 64, s, lut))
    assert all(len(c) > 3 for c in got[0])


def test_settings_round_trip_and_kinds(tmp_path):
    s = DT.HmmSettings([0.3, 0.5, 0.61], [0.0, 8.0, 17.5], grid=DT.hmm_grid(), score=[[1.0, 2.0, 3.0]] * 41)
    s.save(str(tmp_path / "hmm.json"))
    with open(tmp_path / "hmm.json") as f:
        assert json.load(f)["kind"] == "hmm"
    back = DT.HmmSettings.load(str(tmp_path / "hmm.json"))
    assert back == s and back.grid == s.grid and back.score == s.score and back.threshold == s.threshold
    pool = DT.DecoderSettings([0.3, 0.5, 0.75], [15, 31, 47], [62, 124, 31])
    pool.save(str(tmp_path / "pool.json"))
    with open(tmp_path / "pool.json") as f:
        assert "kind" not in json.load(f)
    a, b = DT.load_settings(str(tmp_path / "hmm.json")), DT.load_settings(str(tmp_path / "pool.json"))
    assert isinstance(a, DT.HmmSettings) and a == s
    assert isinstance(b, DT.DecoderSettings) and b == pool
    with pytest.raises(ValueError, match="hmm"):
        DT.HmmSettings.load(str(tmp_path / "pool.json"))
    with open(tmp_path / "other.json", "w") as f:
        json.dump({"kind": "crf"}, f)
    with pytest.raises(ValueError, match="unknown decoder kind"):
        DT.load_settings(str(tmp_path / "other.json"))


def test_python_rejects():
    for thr, cost in (([0.0], [1.0]), ([1.0], [1.0]), ([float("nan")], [1.0]), ([0.5], [-0.1]), ([0.5], [2048.5]),
                      ([0.5, 0.5], [1.0])):
        with pytest.raises(ValueError):
            DT.HmmSettings(thr, cost)
    preds = torch.zeros(2, 16, 3)
    ok = DT.HmmSettings.default(3)
    with pytest.raises(ValueError, match="3"):
        DT.decode_events_hmm(preds, [0, 2], [900], 512, 512, DT.HmmSettings.default(2))
    with pytest.raises(ValueError, match="HmmSettings"):
        DT.decode_events_hmm(preds, [0, 2], [900], 512, 512, DT.DecoderSettings.default(3))
    with pytest.raises(ValueError, match="no window covers"):
        DT.decode_events_hmm(preds, [0, 2], [1100], 512, 512, ok)
    with pytest.raises(ValueError, match="overlap_hop"):
        DT.decode_events_hmm(preds, [0, 2], [900], 512, 600, ok)
    with pytest.raises(ValueError, match="classes"):
        DT.decode_events_hmm(torch.zeros(2, 16, 17), [0, 2], [900], 512, 512, DT.HmmSettings.default(17))
    for lut in (np.zeros(1023, np.int32), np.full(1024, (1 << 15) + 1), np.full(1024, 0.5)):
        with pytest.raises(ValueError, match="lut"):
            DT.decode_events_hmm(preds, [0, 2], [900], 512, 512, ok, lut=lut)
    assert DT.decode_events_hmm(preds, [0, 2], [900], 512, 512, ok, lut=np.full(1024, -(1 << 15)))[0][0].shape == (0, 2)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(lut=None), -1, b"lut"),
    (dict(work=None), -1, b"work"),
    (dict(cost=[(1 << 19) + 1, 0, 0]), -1, b"cost"),
    (dict(cost=[0, 0, -1]), -1, b"cost"),
    (dict(k=17), -2, b"K 17"),
    (dict(overlap_hop=600), -1, b"overlap_hop"),
    (dict(n_frame=520), -1, b"multiple"),
    (dict(frame_len=1100), -1, b"no window covers"),
])
def test_c_abi_rejects(kw, code, msg):
    """The checks at the C ABI fail before any device work: host memory stands in for the device buffers and stays untouched."""
    lib = N.lib()
    k = kw.get("k", 3)
    buf = (C.c_int * 64)(*([-7] * 64))
    p = C.cast(buf, C.c_void_p)
    vp = lambda x: C.cast(x, C.c_void_p)
    win_off = (C.c_int * 2)(0, 2)
    frame_len = (C.c_int * 1)(kw.get("frame_len", 900))
    bias = (C.c_int * 17)()
    cost = (C.c_int * 17)(*kw.get("cost", [0, 0, 0]))
    st = lib.iris_decode_events_hmm(p, p, p, vp(win_off), vp(frame_len), 1, kw.get("n_frame", 512), kw.get("overlap_hop", 512),
                                    16, k, kw.get("lut", p), vp(bias), vp(cost), kw.get("work", p), p, p, p, None)
    assert st == code
    err = lib.iris_last_error()
    assert err.startswith(b"iris_decode_events_hmm") and msg in err, err
    assert list(buf) == [-7] * 64
    assert lib.iris_decode_hmm_workspace_len(vp((C.c_int * 3)(0, 1, 130)), 3, 2) == 2 * 2 * (0 + 1 + 3)
    assert lib.iris_abi_version() == 1


def test_cli_hmm_decoder(tmp_path, monkeypatch, capsys):
    """--decoder_kind hmm with and without --tune, and --decoder loading either kind, through detect.main with test_tune_host's
    CPU stand-ins for the model and the front end (a 'recording' is a text file of on / off flags per block of 32 frames)."""
    from challenge_amd import eval as E
    from test_tune_host import HOP, SR, _Stub
    rng = np.random.default_rng(4)
    answer = {}
    for i in range(3):
        n_blocks = 40 + 16 * i
        flags = np.zeros(n_blocks, np.int64)
        rows, b = [], 3
        while b + 12 < n_blocks:
            n = int(rng.integers(6, 10))
            flags[b:b + n] = 1
            rows += [[c, int(b * 32 * HOP / SR), int(np.ceil((b + n) * 32 * HOP / SR))] for c in range(3)]
            b += n + int(rng.integers(8, 12))
        np.savetxt(tmp_path / f"rec{i}.wav", flags, fmt="%d")
        answer[f"rec{i}"] = rows
    with open(tmp_path / "answer_gt.json", "w") as f:
        json.dump({"task2_answer": answer}, f)
    monkeypatch.setattr(E, "load_model", lambda config, path='', device=None: _Stub())
    monkeypatch.setattr(DT.D, "load_wav", lambda path, device=None: torch.from_numpy(np.loadtxt(path)).float())
    monkeypatch.setattr(DT, "features_for_eval",
                        lambda spec, config: spec.repeat_interleave(32)[None, :, None].expand(4, -1, 1).contiguous())
    base = ["--name", "run", "--v", "9", "--n_mels", "64", "--n_frame", "512", "--n_chan", "1", "--wav_dir", str(tmp_path),
            "--out", str(tmp_path / "answer.json"), "--score", str(tmp_path / "answer_gt.json")]
    def written():
        with open(tmp_path / "answer.json") as f:
            return json.load(f)["task2_answer"]

    pool = DT.main(base)
    pool_ans = written()
    plain = DT.main(base + ["--decoder_kind", "hmm"])                   # HmmSettings.default
    ans = written()
    # the stub's class 0 is 0.3 where the recording is on: under 0.5, so missed by both decoders; the HMM does not widen what
    # it finds, so its events are shorter than the pooling rule's
    assert all({r[0] for r in rows} == {1, 2} for rows in ans.values()) and all(er > 0 for er in plain)
    assert all(len(ans[n]) == len(pool_ans[n]) for n in ans)
    assert sum(r[2] - r[1] for rows in ans.values() for r in rows) < sum(r[2] - r[1] for rows in pool_ans.values() for r in rows)
    from challenge_amd.sj_train import ARGS
    cfg = ARGS().get(["--v", "9", "--n_mels", "64", "--n_frame", "512", "--n_chan", "1"])
    want = DT.detect(_Stub(), sorted(str(p) for p in tmp_path.glob("*.wav")), cfg, settings=DT.HmmSettings.default(3))
    assert {d.name: DT.answer_rows(d) for d in want} == ans
    capsys.readouterr()
    tuned = DT.main(base + ["--decoder_kind", "hmm", "--tune", str(tmp_path / "answer_gt.json"),
                            "--decoder_out", str(tmp_path / "decoder.json")])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("MEAN ER")][0].split()
    assert line[2] == "default" and float(line[3]) == float(np.mean(plain))
    assert float(line[5]) == float(np.mean(tuned)) <= float(np.mean(plain))
    s = DT.load_settings(str(tmp_path / "decoder.json"))
    assert isinstance(s, DT.HmmSettings) and s.n_classes == 3 and len(s.grid) == 41 and np.asarray(s.score).shape == (41, 3)
    assert DT.main(base + ["--decoder", str(tmp_path / "decoder.json")]) == tuned           # the file names its own kind
    DT.DecoderSettings.default(3).save(str(tmp_path / "pool.json"))
    assert DT.main(base + ["--decoder_kind", "hmm", "--decoder", str(tmp_path / "pool.json")]) == pool
    with pytest.raises(ValueError, match="one of the two"):
        DT.main(base + ["--decoder_kind", "hmm", "--tune", "x.json", "--decoder", "y.json"])
