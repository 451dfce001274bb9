"""Delay tracking on the GPU: the step response of k_track.h against the float64 reference (tests/track_ref.py) fed the device's
own fp32 factors, within the bound derived from its summation order; the device's path against the NumPy recurrence on the
device's own doubles (integers: equal); the per-frame beamformer against extract_ref per frame and, with a constant delay,
against the per-event kernel bit for bit; repeatability and independence; `detect(..., locate=LocateSettings(track=))` and its
CLI.

The smallest shapes at which the kernels can still go wrong: F 33 (n_fft 64), T 96, B 2, blocks of 32 frames, steps of 8, q 4, bins
[2, 33); 25 lags (under a wave), 81, and 321 (past one workgroup's 256 threads)."""
import itertools
import json

import numpy as np
import pytest
import torch

import extract_ref as X
import locate_ref as R
import track_ref as K
import whiten_ref as W

pytestmark = pytest.mark.gpu

F, T_LEN, BLOCK, STEP, Q, K_LO, K_HI = 33, 96, 32, 8, 4, 2, 33
MAX_LAGS = (12, 40, 160)
# one frame; inside one step; from mid-step to mid-step across the block boundary at 32; the whole file (sample 1: its last block
# is all zero); inside that all-zero block; the whole of sample 0
EVENTS = np.array([[0, 5, 5], [0, 9, 14], [0, 27, 37], [1, 0, 95], [1, 70, 85], [0, 0, 95]], np.int32)
ROWS = [1, 1, 2, 12, 3, 12]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


_STATE = {}


def _scene(dev):
    """The spectrum (computed once, never written to), the plan and the three kinds of factors: block, quiet (the covariance
    outside the short events) and None."""
    if not _STATE:
        from challenge_amd import transforms as T
        x = W.mixed_spec(11, 2, F, T_LEN)
        x[1, :, 64:] = 0
        xd = torch.from_numpy(x).to(dev)
        plan = T._locate_plan(xd)
        block = plan.whiten_factors(xd, BLOCK, 1e-2)
        quiet, _ = T._quiet_factors(plan, xd, EVENTS[[0, 1, 2, 4]], BLOCK, 1e-2, 1, 8, 1)
        assert not block.cpu().numpy()[1, :, 2].any() and not quiet.cpu().numpy()[1, :, 2].any()   # the silent block: zero factors
        assert not torch.equal(block, quiet)
        _STATE.update(x=x, xd=xd, plan=plan, facs={"block": block, "quiet": quiet, "none": None})
    return _STATE["x"], _STATE["xd"], _STATE["plan"], _STATE["facs"]


def _steps(plan, xd, fac, max_lag, events=EVENTS):
    return plan.locate_steps(xd, events, fac, BLOCK, STEP, K_LO, K_HI, max_lag, Q)


@pytest.mark.parametrize("max_lag", MAX_LAGS)
def test_step_response_within_the_derived_bound(dev, max_lag):
    """R within (n_l + n_s + 72) 2^-53 sum A per step - n_l = ceil(step frames / 64) = 1, n_s = ceil(31 / 64) = 1 - of
    track_ref.step_response (its share doubled, as locate_ref does), n_terms and the row offsets equal; rows in the all-zero block
    are exactly 0 with n_terms 0."""
    x, xd, plan, facs = _scene(dev)
    for kind, fac in facs.items():
        resp, n_terms, offsets = _steps(plan, xd, fac, max_lag)
        assert resp.dtype == torch.float64 and resp.is_cuda and n_terms.dtype == torch.int64 and offsets.dtype == np.int32
        abc = None if fac is None else R.factors_of(fac.cpu().numpy())
        ref, ref_n, ref_off, bound = K.step_response(x, EVENTS, abc, BLOCK, STEP, K_LO, K_HI, max_lag, Q, with_bound=True)
        got = resp.cpu().numpy()
        assert got.shape == ref.shape == (sum(ROWS), 2 * max_lag + 1) and np.diff(offsets).tolist() == ROWS
        assert np.array_equal(offsets, ref_off) and np.array_equal(n_terms.cpu().numpy(), ref_n)
        frac = R.worst_fraction(got, ref, bound)
        print(f"lags {2 * max_lag + 1} factors {kind}: worst fraction of the bound {frac:.3e}")
        assert frac <= 1.0, (kind, frac)
        if fac is not None:
            silent = list(range(offsets[3] + 8, offsets[4])) + list(range(offsets[4], offsets[5]))
            assert not got[silent].any() and not ref_n[silent].any() and ref_n[offsets[3]] == 8 * 31
        assert got[offsets[0]].any() and ref_n[0] == 31 and ref_n[offsets[2]] == 5 * 31 and ref_n[offsets[2] + 1] == 6 * 31
    empty = plan.locate_steps(xd, np.zeros((0, 3), np.int32), facs["block"], BLOCK, STEP, K_LO, K_HI, max_lag, Q)
    assert tuple(empty[0].shape) == (0, 2 * max_lag + 1) and empty[2].tolist() == [0]


@pytest.mark.parametrize("max_lag", MAX_LAGS)
def test_path_equals_the_numpy_recurrence_on_the_device_response(dev, max_lag):
    """The device's path from the device's own R equals the NumPy loop with the same two operations per candidate on those same
    doubles: integer equality, for pen 0 / moderate / huge and a jump limit of 0, 3 and more than L."""
    x, xd, plan, facs = _scene(dev)
    lags = 2 * max_lag + 1
    for kind in ("block", "none"):
        resp, n_terms, offsets = _steps(plan, xd, facs[kind], max_lag)
        host = resp.cpu().numpy()
        moderate = 0.03 * (K_HI - K_LO) * STEP / Q
        for pen, jump in itertools.product((0.0, moderate, 1e12), (0, 3, lags + 5)):
            path = plan.track(resp, offsets, pen, jump)
            assert path.dtype == torch.int32 and path.is_cuda and tuple(path.shape) == (sum(ROWS),)
            want = K.paths(host, offsets, pen, jump)
            assert np.array_equal(path.cpu().numpy(), want), (kind, pen, jump)
            if jump == 0 or pen == 1e12:
                assert all(len(set(want[a:z].tolist())) == 1 for a, z in zip(offsets[:-1], offsets[1:]))   # one lag per event
        free = plan.track(resp, offsets, 0.0, lags - 1).cpu().numpy()
        assert np.array_equal(free, host.argmax(1))                          # no penalty, any jump: each step's first argmax
    flat = torch.ones((7, lags), dtype=torch.float64, device=dev)           # all equal: the smallest lag everywhere
    assert not plan.track(flat, [0, 1, 7], 0.0, 3).any() and not plan.track(flat, [0, 1, 7], 0.5, lags).any()
    assert tuple(plan.track(flat[:0], [0], 0.0, 3).shape) == (0,)
    with pytest.raises(ValueError):
        plan.track(flat, [0, 3], 0.0, 3)                                    # offsets that do not end at the rows
    with pytest.raises(ValueError):
        plan.track(torch.ones((2, 2051), dtype=torch.float64, device=dev), [0, 2], 0.0, 3)      # more than 2049 lags
    with pytest.raises(ValueError):
        plan.track(flat.float(), [0, 1, 7], 0.0, 3)
    with pytest.raises(ValueError):
        plan.locate_steps(xd, EVENTS, facs["block"], BLOCK, 12, K_LO, K_HI, max_lag, Q)         # block % step != 0


def _moving_delays(events, seed=3):
    """One delay per frame of every event: a line from a random start to a random end, with a NaN frame in the longer events."""
    rng = np.random.default_rng(seed)
    parts = []
    for _, first, last in events:
        n = last - first + 1
        d = np.linspace(rng.uniform(-4, 4), rng.uniform(-4, 4), n)
        if n > 20:
            d[7] = np.nan
        parts.append(d)
    return parts


def test_per_frame_beamformer(dev):
    """Within 6 u A (u = 2^-24) of extract_ref evaluated frame by frame, with block factors, quiet factors and none; exactly 0
    outside the bins, in the silent block and at a NaN frame; with a constant delay per event the bits of `beamform`."""
    x, xd, plan, facs = _scene(dev)
    parts = _moving_delays(EVENTS)
    flat = np.concatenate(parts)
    for kind, fac in facs.items():
        abc = None if fac is None else R.factors_of(fac.cpu().numpy())
        for k_lo, k_hi in ((K_LO, K_HI), (0, F - 3)):
            slabs = plan.beamform_frames(xd, EVENTS, flat, fac, BLOCK, k_lo, k_hi)
            refs, mags = K.beamform_frames_ref(x, EVENTS, flat, abc, BLOCK, k_lo, k_hi)
            worst = 0.0
            for i, (s, ref, mag) in enumerate(zip(slabs, refs, mags)):
                got = s.cpu().numpy()
                assert got.shape == (F, EVENTS[i, 2] - EVENTS[i, 1] + 1, 2) and got.dtype == np.float32
                frac = X.worst_fraction(got, ref, mag)
                assert frac <= 1.0, (kind, k_lo, i, frac)
                worst = max(worst, frac)
                assert not got[:k_lo].any() and not got[k_hi:].any()
                if len(parts[i]) > 20:
                    assert not got[:, 7].any() and got[k_lo:k_hi, 8].any()  # the NaN frame, and its neighbour
            if fac is not None:
                assert not slabs[4].any() and not slabs[3][:, 64:].any()   # the all-zero block
            print(f"factors {kind} bins [{k_lo}, {k_hi}): worst fraction of the bound {worst:.3e}")
        const = np.array([-3.0, 2.5, 0.125, -7.3, 1e-3, np.nan])
        per_event = plan.beamform(xd, EVENTS, const, fac, BLOCK, K_LO, K_HI)
        per_frame = plan.beamform_frames(xd, EVENTS, np.concatenate([np.full(len(p), c) for p, c in zip(parts, const)]), fac, BLOCK,
                                         K_LO, K_HI)
        assert all(torch.equal(a, b) for a, b in zip(per_event, per_frame)) and bool(per_event[0].any())
    inner, whole = plan.beamform_frames(xd, [[0, 27, 37], [0, 0, 95]], np.concatenate([parts[5][27:38], parts[5]]), facs["block"], BLOCK)
    assert torch.equal(inner, whole[:, 27:38])                             # a frame does not know its event
    with pytest.raises(ValueError):
        plan.beamform_frames(xd, EVENTS, flat[:-1], facs["block"], BLOCK)   # a delay per output frame
    assert plan.beamform_frames(xd, np.zeros((0, 3), np.int32), [], facs["block"], BLOCK) == []


def test_repeatable_and_independent(dev):
    """Two runs give the same bits; an event's rows do not change when other events and samples join the call; and
    `transforms.track_events` is the three launches plus the host refinement."""
    from challenge_amd import transforms as T
    x, xd, plan, facs = _scene(dev)
    max_lag, pen, jump = 40, 0.03 * 31 * STEP / Q, 3
    for kind, fac in facs.items():
        resp, n_terms, offsets = _steps(plan, xd, fac, max_lag)
        path = plan.track(resp, offsets, pen, jump)
        again = _steps(plan, xd, fac, max_lag)
        assert torch.equal(resp, again[0]) and torch.equal(n_terms, again[1]) and torch.equal(path, plan.track(again[0], offsets, pen, jump))
        order = np.array([5, 0, 3, 1, 4, 2])
        r2, n2, o2 = _steps(plan, xd, fac, max_lag, EVENTS[order])
        p2 = plan.track(r2, o2, pen, jump)
        for i, o in enumerate(order):                                      # reordered
            mine, theirs = slice(o2[i], o2[i + 1]), slice(offsets[o], offsets[o + 1])
            assert torch.equal(r2[mine], resp[theirs]) and torch.equal(n2[mine], n_terms[theirs]) and torch.equal(p2[mine], path[theirs])
        mine = np.flatnonzero(EVENTS[:, 0] == 1)                           # sample 1 alone, the other events left out
        alone_ev = EVENTS[mine].copy()
        alone_ev[:, 0] = 0
        r1, n1, o1 = _steps(plan, xd[1:2].contiguous(), None if fac is None else fac[1:2].contiguous(), max_lag, alone_ev)
        p1 = plan.track(r1, o1, pen, jump)
        for i, m in enumerate(mine):
            theirs = slice(offsets[m], offsets[m + 1])
            assert torch.equal(r1[o1[i]:o1[i + 1]], resp[theirs]) and torch.equal(p1[o1[i]:o1[i + 1]], path[theirs])
    tracks = T.track_events(xd, EVENTS, BLOCK, 1e-2, "block", K_LO, K_HI, max_lag, Q, STEP, pen, jump)
    resp, n_terms, offsets = _steps(plan, xd, facs["block"], max_lag)
    host = resp.cpu().numpy()
    peak = K.peaks(host, n_terms.cpu().numpy(), K.paths(host, offsets, pen, jump), Q)
    assert [len(t) for t in tracks] == ROWS
    for i, (tr, (_, first, last)) in enumerate(zip(tracks, EVENTS)):
        assert tr[:, :2].tolist() == [[t0, t1] for _, t0, t1 in K.steps_of(int(first), int(last), STEP)]
        assert np.array_equal(tr[:, 2:], peak[offsets[i]:offsets[i + 1]], equal_nan=True)
    assert np.isnan(tracks[4][:, 2]).all() and not tracks[4][:, 3].any() and np.isfinite(tracks[5]).all()
    assert np.isnan(T.track_delays(tracks[4], 70, 85)).all()
    plain = T.track_events(xd, EVENTS, None, 1e-2, "identity", K_LO, K_HI, max_lag, Q, STEP, pen, jump)
    assert [len(t) for t in plain] == ROWS and np.isfinite(plain[5]).all()
    assert T.track_events(xd, np.zeros((0, 3), np.int32), BLOCK, step=STEP) == []


def _rows(det):
    return [(int(a), int(b)) for cls in det.events for a, b in np.asarray(cls).reshape(-1, 2)]


def test_detect_fills_tracks_and_steers_along_them(dev):
    """A two-file group with `track`: each file's tracks and clips equal `detect` on the file alone and the transforms on the
    file's own spectrum, bit for bit; the rest of `Detection` is what it is without `track`, where `track` is None."""
    from challenge_amd import data_utils as D
    from challenge_amd import detect as DT
    from challenge_amd import transforms as T
    from test_detect_gpu import StubModel, _cfg, _wavs
    cfg, model = _cfg(), StubModel().to(dev)
    items = _wavs([9.3, 6.1], seed=5)
    for noise in ("block", "quiet"):
        plain = DT.LocateSettings(noise=noise)
        loc = DT.LocateSettings(noise=noise, track=DT.TrackSettings(step_s=0.128))
        ext = DT.ExtractSettings(context_s=0.1)
        base = DT.detect(model, items, cfg, locate=plain, extract=ext)
        res = DT.detect(model, items, cfg, locate=loc, extract=ext)
        assert sum(len(_rows(r)) for r in res) >= 2
        for r, b, item in zip(res, base, items):
            alone = DT.detect(model, [item], cfg, locate=loc, extract=ext)[0]
            assert b.track is None and all(np.array_equal(x, y) for x, y in zip(r.events, b.events))
            assert np.array_equal(r.metric, b.metric) and all(np.array_equal(x, y) for x, y in zip(r.answer, b.answer))
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(r.location, b.location))       # still the static estimate
            assert all(np.array_equal(x, y) for x, y in zip(r.audio_span, b.audio_span))
            assert [len(c) for c in r.track] == [len(c) for c in r.events] == [len(c) for c in alone.track]
            got = [t for cls in r.track for t in cls]
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, [t for cls in alone.track for t in cls]))
            clips = [c for cls in r.audio for c in cls]
            assert all(np.array_equal(x, y) for x, y in zip(clips, [c for cls in alone.audio for c in cls]))
            spec = D.load_wav_array(item[1], 16000, dev)
            f = int(spec.shape[0])
            k_lo, k_hi = loc.bins(f)
            step = loc.track.step_frames(f - 1)
            assert step == 8
            events = [(0, a, z) for a, z in _rows(r)]
            guard = loc.guard_frames(f - 1)
            want = T.track_events(spec, events, cfg.n_frame, loc.loading, noise, k_lo, k_hi, loc.max_lag, loc.q, step,
                                  loc.track.pen(k_hi - k_lo, loc.q, f - 1), loc.track.max_jump(loc.q, f - 1), guard, loc.min_quiet, loc.reach)
            assert len(want) == len(got) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, want))
            assert all(t.shape == (z // step - a // step + 1, 4) and t[0, 0] == a and t[-1, 1] == z for t, (_, a, z) in zip(got, events))
            wide = T.widen_events(np.asarray(events, np.int64), ext.frames(f - 1), int(spec.shape[1]))
            along = [T.track_delays(t, a, z) for t, (_, a, z) in zip(got, wide)]
            own, _ = T.extract_events(spec, events, along, cfg.n_frame, loc.loading, noise, k_lo, k_hi, ext.frames(f - 1), None, guard,
                                      loc.min_quiet, loc.reach)
            assert all(np.array_equal(c, w.cpu().numpy()) for c, w in zip(clips, own))
            moved = [np.ptp(t[:, 2]) > 0 for t in got if len(t) > 1]
            if any(moved):                                                 # steering along a track that moves changes the clip
                assert any(not np.array_equal(x, y) for x, y in zip(clips, [c for cls in b.audio for c in cls]))
    with pytest.raises(ValueError):
        DT.detect(model, items, cfg, locate=DT.LocateSettings(block=100, track=DT.TrackSettings()))   # 100 % 16 != 0


def test_cli_lists_tracks_only_when_asked(dev, tmp_path, monkeypatch):
    from challenge_amd import detect as DT
    from test_detect_gpu import _cfg, _v9_model, _write_named_wavs
    cfg = _cfg()
    torch.save(_v9_model(cfg, dev).state_dict(), tmp_path / "run.pt")
    names = _write_named_wavs(tmp_path, [6.0], seed=8)
    monkeypatch.chdir(tmp_path)
    common = ["--name", "run", "--path", str(tmp_path), "--v", "9", "--n_mels", "64", "--n_frame", "512", "--n_chan", "1",
              "--wav_dir", str(tmp_path), "--locate"]
    DT.main(common + ["--out", str(tmp_path / "plain.json"), "--locate_out", str(tmp_path / "plain_where.json")])
    DT.main(common + ["--out", str(tmp_path / "answer.json"), "--locate_out", str(tmp_path / "where.json"), "--locate_track",
                      "--track_step", "0.512", "--track_max_rate", "10", "--track_penalty", "0.1"])
    with open(tmp_path / "plain.json", "rb") as fa, open(tmp_path / "answer.json", "rb") as fb:
        assert fa.read() == fb.read()
    with open(tmp_path / "plain_where.json") as f:
        plain = json.load(f)
    with open(tmp_path / "where.json") as f:
        where = json.load(f)
    assert list(plain) == ["task2_location"] and list(where) == ["task2_location", "track"]
    assert where["task2_location"] == plain["task2_location"]
    for name in names:
        rows, tracks = where["task2_location"][name], where["track"][name]
        assert len(tracks) == len(rows) == 1                                # the head: class 0 on over the whole file
        first, last = rows[0][1:3]
        assert len(tracks[0]) == last // 32 - first // 32 + 1 and tracks[0][0][0] == first and tracks[0][-1][1] == last
        assert all(len(r) == 4 and r[2] is not None and abs(r[2]) <= 38 / 8 + 1e-9 for r in tracks[0])
