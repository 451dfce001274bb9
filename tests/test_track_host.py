"""Delay tracking without a GPU: the float64 reference (tests/track_ref.py) does what the feature is for - on a source whose
delay moves under a louder interferer the tracked delay follows it where the static one is off by samples, and steering along it
returns the source where static steering returns something else; the path's properties on random responses;
`transforms.track_peak` / `track_delays`; the refusals of `TrackSettings`, `LocateSettings`, the host helpers and the C ABI
before any launch."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import extract_ref as X
import locate_ref as R
import track_ref as K
import whiten_ref as W


def T():
    from challenge_amd import transforms
    return transforms


def _steered(parts, abc, tdoa, ev, k_lo):
    """(SINR gain, source distortion) in dB of steering every frame of the event at tdoa [n]."""
    source, noise = parts
    ys, _ = K.beamform_frames_ref(source, [ev], tdoa, abc, None, k_lo, None)
    yn, _ = K.beamform_frames_ref(noise, [ev], tdoa, abc, None, k_lo, None)
    return X.gains(source, noise, ys[0], yn[0], ev[1:], k_lo)


@pytest.mark.parametrize("source_db", [-10.0, -15.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_track_follows_a_moving_source(seed, source_db):
    """F 257, one block of 512 frames, a white interferer at +2.5 samples, sensor noise 20 dB under it, a white source in frames
    100 .. 355 whose delay moves linearly from -3.0 to +1.0 samples; penalty 0.03, steps of 16, max_rate 20, q 8, bins from 250 Hz
    (k >= 8), the aperture's 38 lag steps either way.  The issue's bounds."""
    from challenge_amd.detect import LocateSettings, TrackSettings
    loc = LocateSettings(track=TrackSettings())
    f, q, ev = 257, loc.q, (0, 100, 355)
    k_lo, k_hi = loc.bins(f)
    step, jump, pen = loc.track.step_frames(f - 1), loc.track.max_jump(q, f - 1), loc.track.pen(k_hi - k_lo, q, f - 1)
    assert (k_lo, k_hi, loc.max_lag, step, jump) == (8, 257, 38, 16, 41) and abs(pen - 0.03 * 249 * 16 / 8) < 1e-12
    source, noise, truth = K.moving_scene(seed, source_db=source_db)
    x = source + noise
    abc = W.factors_ref(x, None, loc.loading)
    resp, n_terms, offsets = K.step_response(x, [ev], abc, None, step, k_lo, k_hi, loc.max_lag, q)
    assert resp.shape == (17, 77) and (n_terms == 16 * 249).sum() == 15 and n_terms[0] == 12 * 249 and n_terms[-1] == 4 * 249
    path = K.paths(resp, offsets, pen, jump)
    peak = T().track_peak(resp, n_terms, path, q)
    assert np.array_equal(peak, K.peaks(resp, n_terms, path, q))
    track = T().track_rows([ev], offsets, step, peak)[0]
    assert track.shape == (17, 4) and track[0, :2].tolist() == [100, 111] and track[-1, :2].tolist() == [352, 355]
    tracked = T().track_delays(track, ev[1], ev[2])
    assert np.array_equal(tracked, K.delays(K.steps_of(ev[1], ev[2], step), peak[:, 0], ev[1], ev[2]))
    curve, n_all = R.locate_ref(x, [ev], abc, None, k_lo, k_hi, loc.max_lag, q)
    static = np.full(truth.shape, T().locate_peak(curve, n_all, q)[0, 0])
    rms = lambda d: float(np.sqrt(np.mean((d - truth) ** 2)))
    abc0 = tuple(v[:1] for v in abc)
    g_track, d_track = _steered((source, noise), abc0, tracked, ev, k_lo)
    g_static, d_static = _steered((source, noise), abc0, static, ev, k_lo)
    g_true, d_true = _steered((source, noise), abc0, truth, ev, k_lo)
    print(f"seed {seed} source {source_db} dB: delay rms tracked {rms(tracked):.3f} static {rms(static):.3f} (static peak {static[0]:+.2f}); "
          f"distortion tracked {d_track:.1f} static {d_static:.1f} true {d_true:.1f} dB; SINR gain tracked {g_track:.2f} true {g_true:.2f} dB")
    assert rms(tracked) <= 0.2
    assert rms(static) >= 2.0
    assert d_track <= -10.0
    assert d_static >= -2.0
    assert abs(g_track - g_true) <= 0.2


def test_path_properties_on_random_responses():
    rng = np.random.default_rng(7)
    resp = rng.standard_normal((9, 25))
    lags = resp.shape[1]
    free = K.viterbi(resp, 0.0, lags - 1)                                   # no penalty, every jump allowed: each step's own peak
    assert np.array_equal(free, resp.argmax(1)) and np.array_equal(K.viterbi(resp, 0.0, 10 * lags), free)
    held = K.viterbi(resp, 0.3, 0)                                          # no jump: one lag, the peak of the running sum
    total = resp[0].copy()
    for row in resp[1:]:
        total = total + row
    assert np.array_equal(held, np.full(9, int(np.argmax(total))))
    stiff = K.viterbi(resp, 1e6, lags - 1)                                  # a huge penalty holds the lag as well
    assert len(set(stiff.tolist())) == 1
    some = K.viterbi(resp, 0.5, 3)
    assert np.abs(np.diff(some)).max() <= 3
    score = lambda p: resp[np.arange(9), p].sum() - 0.5 * np.abs(np.diff(p)).sum()
    assert score(some) >= score(held) - 1e-12                               # (a constant path is allowed under any limit)
    flat = np.ones((5, 11))                                                 # all equal: the smallest lag everywhere
    for pen, jump in ((0.0, 0), (0.0, 3), (0.0, 20), (0.25, 3)):
        assert not K.viterbi(flat, pen, jump).any()
    two = np.zeros((3, 11))
    two[:, 4] = two[:, 7] = 1.0                                             # a tie between two constant paths: the smaller lag
    assert K.viterbi(two, 0.1, 5).tolist() == [4, 4, 4]
    one = K.viterbi(resp[:1], 0.3, 2)                                       # an event of one step: its first argmax
    assert one.tolist() == [int(np.argmax(resp[0]))]
    both = K.paths(np.concatenate([resp, resp[:1]]), np.array([0, 9, 10]), 0.5, 3)
    assert np.array_equal(both, np.concatenate([some, one]))


def test_track_peak_and_delays():
    n, q = 10, 4
    grid = np.arange(-n, n + 1, dtype=np.float64)
    y = np.stack([5.0 - 0.125 * (grid - x0) ** 2 for x0 in (-3.3, 2.45)] + [grid, np.zeros(2 * n + 1)])
    peak = T().track_peak(y, [3, 3, 1, 0], [7, 12, 2 * n, 5], q)
    assert abs(peak[0, 0] + 3.3 / q) <= 1e-12 and abs(peak[1, 0] - 2.45 / q) <= 1e-12 and peak[0, 1] == y[0, 7] / 3
    assert peak[2, 0] == n / q and peak[2, 1] == n                          # the last lag: no parabola
    assert np.isnan(peak[3, 0]) and peak[3, 1] == 0                         # nothing contributed
    off = T().track_peak(y[:1], [3], [9], q)[0, 0]                          # a path lag that is no local maximum: the clip holds
    assert off == (9 - n - 0.5) / q
    for bad in (dict(resp=np.zeros((1, 4)), n_terms=[1], path=[0]), dict(resp=np.zeros((2, 5)), n_terms=[1], path=[0, 0]),
                dict(resp=np.zeros((1, 5)), n_terms=[1], path=[5]), dict(resp=np.zeros((1, 5)), n_terms=[1], path=[0], q=0)):
        with pytest.raises(ValueError):
            T().track_peak(**bad)
    assert T().track_peak(np.zeros((0, 5)), [], []).shape == (0, 2)
    track = np.array([[20, 23, 1.0, 2.0], [24, 31, np.nan, 0.0], [32, 39, 3.0, 2.0], [40, 41, 3.5, 1.0]])
    d = T().track_delays(track, 20, 41)
    assert d.shape == (22,) and d[0] == d[1] == 1.0 and d[-1] == 3.5        # held before the first and after the last centre
    assert abs(d[28 - 20] - (1.0 + 2.0 * (28 - 21.5) / (35.5 - 21.5))) <= 1e-15     # across the NaN step: the finite ones only
    wide = T().track_delays(track, 10, 60)                                  # context frames: the nearest end value
    assert (wide[:12] == 1.0).all() and (wide[-20:] == 3.5).all() and np.array_equal(wide[10:32], d)
    assert np.array_equal(T().track_delays(track[:1], 18, 30), np.full(13, 1.0))    # a single step: constant
    assert np.isnan(T().track_delays(track[1:2], 24, 31)).all()             # no finite step: NaN for the whole event
    rows = T().track_rows([[0, 20, 41], [1, 7, 7]], [0, 4, 5], 8, np.arange(10.0).reshape(5, 2))
    assert rows[0][:, :2].tolist() == [[20, 23], [24, 31], [32, 39], [40, 41]] and rows[1].tolist() == [[7, 7, 8, 9]]
    flat, per = T().frame_delays([1.0, 2.0], [[0, 3, 5], [0, 9, 9]])
    assert not per and flat.tolist() == [1.0, 2.0]
    flat, per = T().frame_delays([np.array([1.0, 2.0, 3.0]), [4.0]], [[0, 3, 5], [0, 9, 9]])
    assert per and flat.tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        T().frame_delays([np.array([1.0, 2.0]), [4.0]], [[0, 3, 5], [0, 9, 9]])


def test_settings_refusals_and_defaults():
    from challenge_amd.detect import Detection, LocateSettings, TrackSettings
    s = TrackSettings()
    assert (s.step_s, s.max_rate, s.penalty) == (0.25, 20.0, 0.03)
    assert s.step_frames() == 16 and s.step_frames(512) == 8 and TrackSettings(step_s=0.001).step_frames() == 1
    assert s.max_jump(8) == int(np.ceil(20.0 * 16 * 256 / 16000 * 8)) == 41 and s.max_jump(4, 512) == int(np.ceil(20.0 * 8 * 512 / 16000 * 4))
    assert s.pen(249, 8) == 0.03 * 249 * 16 / 8 and TrackSettings(penalty=0).pen(249, 8) == 0.0
    for bad in (dict(step_s=0.0), dict(step_s=float("nan")), dict(step_s="1"), dict(step_s=True), dict(max_rate=0.0),
                dict(max_rate=float("inf")), dict(penalty=-0.1), dict(penalty=float("nan")), dict(penalty=None)):
        with pytest.raises(ValueError):
            TrackSettings(**bad)
    assert LocateSettings().track is None and LocateSettings(track=s, noise="quiet").track is s
    with pytest.raises(ValueError, match="whitened"):
        LocateSettings(track=s, noise="identity")
    with pytest.raises(ValueError):
        LocateSettings(track=dict(step_s=0.25))
    assert LocateSettings(track=s, max_lag=1024).max_lag == 1024
    with pytest.raises(ValueError, match="2049"):
        LocateSettings(track=s, max_lag=1025)
    assert LocateSettings(max_lag=1025).max_lag == 1025                     # (untracked: locate's own limit)
    det = Detection("a", 50, (), np.zeros((0, 2), np.int32), ())
    assert det.track is None


def test_host_helpers_refuse():
    from challenge_amd import frontend as FE
    assert FE.TRACK_MAX_LAGS == 2049
    assert FE.track_step(8, 32) == 8 and FE.track_step(16) == 16 and FE.track_step(np.int64(4), 512) == 4
    for bad in ((0, None), (-1, None), (2.0, None), (True, None), (12, 32), (64, 32)):
        with pytest.raises(ValueError):
            FE.track_step(*bad)
    assert FE.track_penalties(0.5, 3, 25).tolist() == [0.0, 0.5, 1.0, 1.5] and len(FE.track_penalties(0.5, 99, 25)) == 25
    assert FE.track_penalties(0, 0, 1).tolist() == [0.0]
    for bad in ((-1.0, 3, 25), (float("nan"), 3, 25), ("1", 3, 25), (0.5, -1, 25), (0.5, 1.5, 25), (0.5, 3, 24), (0.5, 3, 2051)):
        with pytest.raises(ValueError):
            FE.track_penalties(*bad)
    assert FE.track_offsets([0, 4, 5], 5).dtype == np.int32 and FE.track_offsets([0], 0).tolist() == [0]
    for bad in (([1, 4, 5], 5), ([0, 4, 4], 4), ([0, 4, 5], 6), ([0.0, 5.0], 5), ([[0, 5]], 5), ([], 0)):
        with pytest.raises(ValueError):
            FE.track_offsets(*bad)
    x = torch.zeros(1, 33, 96, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T().track_events(x, [[0, 0, 5]], 32, step=8)
    for bad in (dict(step=12), dict(step=0), dict(pen=-1.0), dict(max_jump=-1), dict(max_lag=1025), dict(noise="frame")):
        with pytest.raises(ValueError):
            T().track_events(x, [[0, 0, 5]], 32, **{**dict(step=8), **bad})
    with pytest.raises(ValueError):
        T().track_events(torch.zeros(1, 33, 96, 2), [[0, 0, 5]], 32, step=8)


def test_write_locations_lists_tracks_only_when_tracking(tmp_path):
    from challenge_amd import detect as DT
    ev = (np.array([[3, 9], [20, 40]], np.int64), np.zeros((0, 2), np.int64))
    loc = (np.array([[-3.0, 40.0, 1.5, 0.2], [np.nan, np.nan, 0.0, 0.0]]), np.zeros((0, 4)))
    tracks = ([np.array([[3.0, 7.0, -3.0, 1.5], [8.0, 9.0, -2.5, 1.25]]), np.array([[20.0, 23.0, np.nan, 0.0]])], [])
    none2 = (np.zeros((0, 2), np.int32),) * 2
    det = DT.Detection("a", 50, ev, np.zeros((0, 2), np.int32), none2, loc, track=tracks)
    out = DT.write_locations([det], str(tmp_path / "where.json"))
    with open(tmp_path / "where.json") as f:
        assert json.load(f) == out
    assert out["track"] == {"a": [[[3, 7, -3.0, 1.5], [8, 9, -2.5, 1.25]], [[20, 23, None, 0.0]]]}
    plain = DT.write_locations([DT.Detection("a", 50, ev, np.zeros((0, 2), np.int32), none2, loc)], str(tmp_path / "plain.json"))
    assert list(plain) == ["task2_location"] and plain["task2_location"] == out["task2_location"]


def test_c_abi_refuses_before_any_launch():
    """As test_locate_host.py: every check that does not read the plan happens before the plan is touched, so a made-up plan
    pointer reaches it."""
    from challenge_amd import _native as N
    lib = N.lib()
    p16, p8, p4 = C.c_void_p(16), C.c_void_p(8), C.c_void_p(4)
    INVALID, UNSUPPORTED = -1, -2

    def steps(plan=p16, spec=p16, fac=p16, j=3, ev_dev=p16, ev=((0, 10, 120, 0),), n_ev=None, batch=2, t=150, block=50, step=10,
              k_lo=0, k_hi=129, max_lag=40, q=8, ws=p16, ws_bytes=1 << 30, resp=p16, n_terms=p16):
        host = (C.c_int32 * (4 * max(len(ev), 1)))(*[v for r in ev for v in r]) if ev is not None else None
        return lib.iris_locate_steps(plan, spec, fac, j, ev_dev, host, len(ev) if n_ev is None else n_ev, batch, t, block, step,
                                     k_lo, k_hi, max_lag, q, ws, ws_bytes, resp, n_terms, None)
    assert steps(plan=None) == INVALID and steps(spec=None) == INVALID and steps(spec=p8) == INVALID
    assert steps(step=0) == INVALID and steps(step=-3) == INVALID
    assert steps(step=20) == INVALID and steps(step=100) == INVALID           # block % step != 0 with three blocks
    assert b"iris_locate_steps" in lib.iris_last_error()
    assert steps(k_lo=5, k_hi=5) == INVALID and steps(q=0) == INVALID and steps(max_lag=2049) == UNSUPPORTED
    assert steps(j=2) == INVALID and steps(block=0) == INVALID
    assert steps(ev=((0, 10, 150, 0),)) == INVALID and steps(ev=((0, 6, 5, 0),)) == INVALID and steps(ev=((2, 0, 5, 0),)) == INVALID
    assert steps(ev=((0, 10, 120, 0), (1, 0, 5, 3))) == INVALID              # the first event has twelve steps, not three
    assert steps(ev=((0, 10, 120, 1),)) == INVALID
    assert steps(ws=None) == INVALID and steps(resp=None) == INVALID and steps(n_terms=C.c_void_p(12)) == INVALID

    def lags(plan=p16, resp=p16, off_dev=p16, off=(0, 4, 5), n_ev=None, rows=5, max_lag=12, pen=p16, n_pen=4, jump=3, ws=p16,
             ws_bytes=1 << 30, path=p16):
        host = (C.c_int32 * max(len(off), 1))(*off) if off is not None else None
        return lib.iris_track_lags(plan, resp, off_dev, host, len(off) - 1 if n_ev is None else n_ev, rows, max_lag, pen, n_pen,
                                   jump, ws, ws_bytes, path, None)
    assert lags(plan=None) == INVALID and lags(n_ev=-1) == INVALID and lags(rows=-1) == INVALID
    assert lags(max_lag=-1) == INVALID and lags(jump=-1) == INVALID
    assert lags(max_lag=1025, n_pen=4) == UNSUPPORTED                        # 2051 lags
    assert b"iris_track_lags" in lib.iris_last_error() and b"2049" in lib.iris_last_error()
    assert lags(n_pen=3) == INVALID and lags(jump=99, n_pen=100) == INVALID and lags(n_pen=0) == INVALID
    assert lags(resp=None) == INVALID and lags(off_dev=None) == INVALID and lags(off=None, n_ev=2) == INVALID
    assert lags(pen=None) == INVALID and lags(ws=None) == INVALID and lags(path=None) == INVALID
    assert lags(resp=C.c_void_p(12)) == INVALID and lags(pen=C.c_void_p(12)) == INVALID and lags(path=C.c_void_p(6)) == INVALID
    assert lags(off=(1, 4, 5)) == INVALID and lags(off=(0, 4, 4), rows=4) == INVALID and lags(off=(0, 4, 5), rows=6) == INVALID
    assert lags(off=(0,), rows=3) == INVALID

    def frames(plan=p16, spec=p16, fac=p16, j=3, ev_dev=p16, ev=((0, 10, 29, 0), (1, 0, 4, 20)), tdoa=p16, n_tdoa=25, batch=2,
               t=150, block=50, k_lo=0, k_hi=129, out=p16, out_floats=1 << 40):
        host = (C.c_int32 * (4 * len(ev)))(*[v for r in ev for v in r])
        return lib.iris_beamform_frames(plan, spec, fac, j, ev_dev, host, tdoa, n_tdoa, len(ev), batch, t, block, k_lo, k_hi, out,
                                        out_floats, None)
    assert frames(plan=None) == INVALID and frames(spec=p8) == INVALID and frames(k_lo=9, k_hi=3) == INVALID
    assert frames(n_tdoa=2) == INVALID and frames(n_tdoa=26) == INVALID       # one delay per output frame: 25
    assert b"iris_beamform_frames" in lib.iris_last_error()
    assert frames(n_tdoa=1 << 31) == UNSUPPORTED
    assert frames(tdoa=None) == INVALID and frames(tdoa=p4) == INVALID and frames(out=None) == INVALID
    assert frames(ev=((0, 10, 29, 0), (1, 0, 4, 19))) == INVALID and frames(ev=((0, 10, 150, 0),), n_tdoa=141) == INVALID
