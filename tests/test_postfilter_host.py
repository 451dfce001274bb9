"""The Wiener post-filter without a GPU: the float64 reference (tests/postfilter_ref.py) - the closed-form noise power against
the measured one, the demonstration figures against the constants the reference itself measured, the bypass - and every
refusal of the settings, `extract_events`, `FrontendPlan.postfilter`'s helpers and the C ABI that happens before device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import extract_ref as X      # noqa: E402
import postfilter_ref as P   # noqa: E402


@pytest.mark.parametrize("which", ["large", "small"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_phi_is_the_measured_output_noise_power(which, seed):
    """phi = 1/den - d |w|^2 within 10 % of mean |Y_noise|^2 (median over bins); the loaded form 1/den alone reads more than
    1.5 times too much - at loading 1e-2 the loading is as large as the sensor noise - so the correction term is tested."""
    phi, loaded = P.phi_identity(which, seed)
    print(f"{which} seed {seed}: phi / measured {phi:.4f}, (1/den) / measured {loaded:.4f}")
    assert 0.9 <= phi <= 1.1
    assert loaded > 1.5


@pytest.mark.parametrize("which", ["large", "small"])
@pytest.mark.parametrize("source_db", [-10.0, 0.0])
def test_demonstration_matches_its_constants(which, source_db):
    want = np.asarray(P.MEASURED[which, source_db])
    floor = 10.0 ** (P.FLOOR_DB / 20.0)
    for seed in (0, 1, 2):
        fig, g = P.demonstration(which, seed, source_db)
        print(f"{which} {source_db:+.0f} dB seed {seed}: SINR {fig[0]:.2f} -> {fig[1]:.2f}, error {fig[2]:.2f} -> {fig[3]:.2f}, "
              f"context {fig[4]:.2f} dB; worst distance from the constants {np.abs(np.asarray(fig) - want).max():.2f} dB")
        assert np.abs(np.asarray(fig) - want).max() <= P.MARGIN_DB
        assert floor <= g.min() and g.max() < 1.0                 # every gain in [g_min, 1)
        assert P.FLOOR_DB < fig[4] < 0.0                          # the context goes down, by less than the floor
        if source_db == -10.0:
            assert fig[1] > fig[0]


def test_floor_one_is_the_bypass_and_the_exact_zeros():
    f, t, _, frames, context, k_lo = P.SCENES["small"][:6]
    source, noise = P.sparse_scene("small", 0, -10.0)
    abc, block = P.quiet_abc(source + noise, "small")
    ev, d = [[0, frames[0] - context, frames[1] + context]], [P.TRUE_DELAY]
    (y,) = X.beamform_ref(source + noise, ev, d, abc, block, k_lo)
    (z,), (g,) = P.postfilter_ref([y], ev, d, abc, block, P.LOADING, k_lo, None, P.ALPHA, 1.0)
    assert (g == 1.0).all() and np.array_equal(z, y)
    (z,), (g,) = P.postfilter_ref([y], ev, d, abc, block, P.LOADING, k_lo, f - 3, P.ALPHA, 0.1)
    assert (z[:k_lo] == 0).all() and (z[f - 3:] == 0).all() and (np.abs(z[k_lo:f - 3]) > 0).all()
    (z,), (g,) = P.postfilter_ref([y], ev, [np.nan], abc, block, P.LOADING, k_lo, None, 0.5, 0.1)
    assert (g[:, 0] == 1 / 3).all() and (g[:, -1] == 0.1).all()   # gamma = 0 throughout: xi = alpha p only, down to the floor
    per_frame = np.full(ev[0][2] - ev[0][1] + 1, P.TRUE_DELAY)
    (z2,), _ = P.postfilter_ref([y], ev, per_frame, abc, block, P.LOADING, k_lo, None, P.ALPHA, 0.1, per_frame=True)
    (z1,), _ = P.postfilter_ref([y], ev, d, abc, block, P.LOADING, k_lo, None, P.ALPHA, 0.1)
    assert np.array_equal(z1, z2)


def test_postfilter_settings_refusals_and_defaults():
    from challenge_amd.detect import ExtractSettings, PostFilterSettings
    assert PostFilterSettings().smoothing == 0.98 and PostFilterSettings().floor_db == -20.0
    assert PostFilterSettings(smoothing=0, floor_db=0).pair() == (0.0, 0.0)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.98", True, None):
        with pytest.raises(ValueError):
            PostFilterSettings(smoothing=bad)
    for bad in (0.1, float("nan"), float("-inf"), float("inf"), -1e5, "-20", True, None):
        with pytest.raises(ValueError):
            PostFilterSettings(floor_db=bad)
    assert ExtractSettings().postfilter is None
    assert ExtractSettings(postfilter=PostFilterSettings()).postfilter.pair() == (0.98, -20.0)
    for bad in (True, (0.98, -20.0), "on"):
        with pytest.raises(ValueError):
            ExtractSettings(postfilter=bad)


def test_detect_refuses_postfilter_without_a_quiet_covariance():
    """Raised before anything is loaded: neither the model nor the recordings are touched."""
    from challenge_amd import detect as DT
    extract = DT.ExtractSettings(postfilter=DT.PostFilterSettings())
    for noise in ("block", "identity"):
        with pytest.raises(ValueError, match="quiet"):
            DT.detect(None, ["/nowhere/at/all.wav"], None, locate=DT.LocateSettings(noise=noise), extract=extract)


def test_cli_refuses_postfilter_without_its_companions(tmp_path, capsys):
    from challenge_amd import detect as DT
    base = ["--name", "run", "--path", str(tmp_path), "--wav_dir", str(tmp_path), "--locate"]
    with pytest.raises(SystemExit) as exc:
        DT.main(base + ["--extract_postfilter"])
    assert exc.value.code == 2 and "--extract" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        DT.main(base + ["--extract", str(tmp_path / "clips"), "--extract_postfilter"])
    assert exc.value.code == 2 and "quiet" in capsys.readouterr().err
    assert not (tmp_path / "clips").exists()


def test_extract_events_refusals():
    from challenge_amd import transforms as T
    spec = torch.zeros(1, 129, 20, 4)
    for noise in ("block", "identity"):
        with pytest.raises(ValueError, match="quiet"):
            T.extract_events(spec, [[0, 0, 5]], [0.0], noise=noise, postfilter=(0.98, -20.0))
    for bad in ((1.0, -20.0), (-0.1, -20.0), (0.98, 1.0), (0.98, float("nan")), (0.98,), 0.98, (0.98, -20.0, 1), ("a", -20.0),
                (True, -20.0), (0.98, -1e5)):
        with pytest.raises(ValueError):
            T.extract_events(spec, [[0, 0, 5]], [0.0], noise="quiet", postfilter=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.extract_events(spec, [[0, 0, 5]], [0.0], noise="quiet", postfilter=(0.98, -20.0))


def test_floors_follow_the_quiet_frames():
    from challenge_amd import transforms as T
    alpha, floors = T.postfilter_floors((0.9, -20.0), [40, 0, 16])
    assert alpha == 0.9 and floors.dtype == np.float64 and floors.tolist() == [10.0 ** -1.0, 1.0, 10.0 ** -1.0]
    assert T.postfilter_floors((0, 0), [3])[1].tolist() == [1.0] and T.postfilter_floors((0, -6.0), [])[1].shape == (0,)


def test_write_extracts_lists_the_postfilter(tmp_path):
    from challenge_amd import detect as DT
    ev = (np.array([[3, 9], [20, 30]], np.int64),)
    loc = (np.array([[0.5, 1.0, 2.0, 3.0], [np.nan, np.nan, 0.0, 0.0]]),)
    clips = ([np.zeros(8, np.float32), np.ones(4, np.float32)],)
    spans = (np.array([[0, 8], [16, 20]], np.int64),)
    args = ("a.wav", 50, ev, np.zeros((0, 2), np.int32), (np.zeros((0, 2), np.int32),), loc, clips, spans)
    plain = DT.Detection(*args)
    assert plain.postfiltered is None
    before = DT.write_extracts([plain], str(tmp_path / "plain"))
    assert list(before) == ["task2_extract"]                                         # nothing new without the settings
    with pytest.raises(ValueError, match="postfiltered"):
        DT.write_extracts([plain], str(tmp_path / "bad"), DT.PostFilterSettings())
    done = DT.Detection(*args, None, None, (np.array([True, False]),))
    index = DT.write_extracts([done], str(tmp_path / "post"), DT.PostFilterSettings(floor_db=-12.0))
    assert index["task2_extract"] == before["task2_extract"]
    assert index["postfilter"] == {"smoothing": 0.98, "floor_db": -12.0, "applied": {"a.wav": [True, False]}}
    import json
    with open(tmp_path / "post" / "extract.json") as f:
        assert json.load(f) == index


def test_c_abi_refuses_before_any_launch():
    """As test_extract_host.py reaches iris_beamform_events' checks: a made-up plan pointer for the checks that do not read the
    plan, a zeroed block whose sixth and seventh int are n_bins and channels for those that do."""
    from challenge_amd import _native as N
    lib = N.lib()
    p16 = C.c_void_p(16)
    OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -3

    def call(plan=p16, slabs=p16, fac=p16, j=3, ev_dev=p16, ev=((0, 10, 120, 0),), tdoa=p16, n_tdoa=None, per_frame=0, g_dev=p16,
             floors=None, n_ev=None, batch=2, t=150, block=50, loading=1e-2, alpha=0.98, k_lo=0, k_hi=129, out=p16,
             out_floats=1 << 40):
        n = len(ev) if ev is not None else 1
        host = (C.c_int32 * (4 * max(n, 1)))(*[v for r in ev for v in r]) if ev is not None else None
        floors = [0.1] * n if floors is None else floors
        g_host = (C.c_double * max(len(floors), 1))(*floors) if floors != "null" else None
        frames = sum(r[2] - r[1] + 1 for r in ev) if ev else 0
        n_tdoa = (frames if per_frame else n) if n_tdoa is None else n_tdoa
        return lib.iris_postfilter_events(plan, slabs, fac, j, ev_dev, host, tdoa, n_tdoa, per_frame, g_dev, g_host,
                                          n if n_ev is None else n_ev, batch, t, block, loading, alpha, k_lo, k_hi, out, out_floats, None)
    assert call(plan=None) == INVALID and call(fac=None) == INVALID and call(slabs=None) == INVALID
    assert call(batch=0) == INVALID and call(t=0) == INVALID and call(n_ev=-1) == INVALID
    assert call(k_lo=5, k_hi=5) == INVALID and call(k_lo=-1) == INVALID
    for alpha in (-0.01, 1.0, 2.0, float("nan")):
        assert call(alpha=alpha) == INVALID
    for loading in (0.0, -1e-2, float("nan"), float("inf")):
        assert call(loading=loading) == INVALID
    for floor in (0.0, -0.1, 1.0000001, float("nan")):
        assert call(floors=[floor]) == INVALID
    assert call(block=0) == INVALID and call(fac=C.c_void_p(8)) == INVALID and call(j=2) == INVALID
    assert call(ev=((0, 10, 150, 0),)) == INVALID and call(ev=((0, 6, 5, 0),)) == INVALID and call(ev=((2, 0, 5, 0),)) == INVALID
    assert call(ev=((0, 10, 120, 0), (1, 0, 5, 110))) == INVALID            # the first event has 111 frames, not 110
    assert call(n_tdoa=2) == INVALID and call(per_frame=1, n_tdoa=110) == INVALID
    assert call(ev=None, n_ev=1) == INVALID and call(ev_dev=None) == INVALID and call(tdoa=None) == INVALID
    assert call(g_dev=None) == INVALID and call(floors="null") == INVALID and call(out=None) == INVALID
    for odd in ("tdoa", "out", "slabs", "g_dev"):
        assert call(**{odd: C.c_void_p(12)}) == INVALID
    assert b"iris_postfilter_events" in lib.iris_last_error()

    def plan_of(n_bins, channels):
        head = (C.c_int32 * 1024)()
        head[5], head[6] = n_bins, channels
        return head
    stereo = plan_of(129, 2)
    for channels in (1, 3):
        assert call(plan=plan_of(129, channels)) == UNSUPPORTED            # C != 2
    assert call(plan=stereo, k_hi=130) == INVALID
    two = ((0, 10, 120, 0), (1, 0, 5, 111))
    assert call(plan=stereo, ev=two, out_floats=2 * 129 * 117 - 1) == CAPACITY
    assert call(plan=stereo, ev=two, per_frame=1, out_floats=0) == CAPACITY
    assert call(plan=stereo, ev=(), n_ev=0) == OK                           # nothing to do: no launch
