"""The noise covariance from the frames outside events, without a GPU: `transforms.quiet_mask` and `transforms.quiet_ranges`
against the frame-by-frame restatement (tests/quiet_ref.py) on hand cases; what the feature is for - a dominant event steered
1/8 sample off no longer nulls itself - through the float64 references; the refusals of `LocateSettings`, of the CLI, of the C
ABI before any launch and of CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import quiet_ref as Q
import whiten_ref as W


def _both(events, lens, guard, block, min_quiet, reach):
    """(mask, ranges, quiet) of the host code, checked against the restatement."""
    from challenge_amd import transforms as T
    mask = T.quiet_mask(np.asarray(events, np.int64).reshape(-1, 3), lens, guard)
    want = Q.mask_ref(events, lens, guard)
    assert mask.dtype == np.uint8 and mask.shape == want.shape and np.array_equal(mask, want)
    ranges, quiet = T.quiet_ranges(mask, lens, block, min_quiet, reach)
    r_ref, q_ref = Q.ranges_ref(want, lens, block, min_quiet, reach)
    assert ranges.dtype == np.int32 and quiet.dtype == np.int64
    assert ranges.tolist() == r_ref.tolist() and quiet.tolist() == q_ref.tolist()
    return mask, ranges, quiet


def test_guard_is_clipped_at_both_ends():
    mask, _, _ = _both([[0, 1, 3], [0, 95, 97]], [100], 4, 25, 4, 1)
    assert mask[0].tolist() == [1] * 8 + [0] * 83 + [1] * 9
    mask, _, _ = _both([[0, 0, 0], [0, 99, 99]], [100], 0, 25, 4, 1)
    assert mask[0].sum() == 2 and mask[0, 0] == 1 and mask[0, 99] == 1


def test_overlapping_events_of_different_classes():
    """The table does not know classes: any event masks its frames, overlapping ones once."""
    mask, ranges, quiet = _both([[0, 10, 30], [0, 25, 45], [0, 27, 28]], [100], 2, 50, 8, 0)
    assert mask[0].tolist() == [0] * 8 + [1] * 40 + [0] * 52
    assert ranges[0].tolist() == [[0, 50, 1], [50, 100, 1]] and quiet[0].tolist() == [10, 50]


def test_a_short_last_block_and_every_reach():
    events, lens = [[0, 64, 127]], [150]               # block 1 of [0, 64), [64, 128), [128, 150) is filled exactly
    _, ranges, quiet = _both(events, lens, 0, 64, 16, 0)
    assert ranges[0].tolist() == [[0, 64, 1], [64, 128, 0], [128, 150, 1]] and quiet[0].tolist() == [64, 0, 22]
    _, ranges, quiet = _both(events, lens, 0, 64, 16, 1)
    assert ranges[0].tolist() == [[0, 64, 1], [0, 150, 1], [128, 150, 1]] and quiet[0].tolist() == [64, 86, 22]
    _, ranges, quiet = _both(events, lens, 0, 64, 30, 1)                   # the short block's neighbour has nothing to lend
    assert ranges[0].tolist() == [[0, 64, 1], [0, 150, 1], [128, 150, 0]] and quiet[0].tolist() == [64, 86, 0]
    _, ranges, quiet = _both(events, lens, 0, 64, 80, 2)                   # reach 2: blocks 0 and 2 need the whole recording
    assert ranges[0].tolist() == [[0, 150, 1], [0, 150, 1], [0, 150, 1]] and quiet[0].tolist() == [86, 86, 86]
    _, ranges, quiet = _both(events, lens, 0, 64, 80, 1)                   # ... which reach 1 gives only block 1
    assert ranges[0].tolist() == [[0, 64, 0], [0, 150, 1], [128, 150, 0]] and quiet[0].tolist() == [0, 86, 0]
    _both(events, lens, 3, 50, 1, 2)
    _both(events, lens, 3, 1, 2, 1)
    _both(events, lens, 3, None, 2, 1)
    _both(events, lens, 0, 1000, 2, 1)                 # a block longer than the recording counts as the recording


def test_the_edge_of_the_recording_is_reached_before_min_quiet():
    """Block 0 of four 25-frame blocks, all but 5 frames of blocks 0 and 1 masked: reach 1 stops at the recording's left edge
    and finds 5 < 8 quiet frames, reach 2 finds them in block 2."""
    events, lens = [[0, 0, 44]], [100]
    _, ranges, quiet = _both(events, lens, 0, 25, 8, 1)
    assert ranges[0, 0].tolist() == [0, 25, 0] and quiet[0, 0] == 0
    assert ranges[0, 1].tolist() == [0, 75, 1] and quiet[0, 1] == 30
    _, ranges, quiet = _both(events, lens, 0, 25, 8, 2)
    assert ranges[0, 0].tolist() == [0, 75, 1] and quiet[0, 0] == 30


def test_a_fully_masked_recording_falls_back_everywhere():
    for reach in (0, 1, 2):
        mask, ranges, quiet = _both([[0, 0, 99]], [100], 0, 30, 1, reach)
        assert mask.all() and not quiet.any()
        assert ranges[0].tolist() == [[0, 30, 0], [30, 60, 0], [60, 90, 0], [90, 100, 0]]


def test_ragged_lengths_in_one_table():
    """Every range is clipped to its sample's own length; a block past a sample's end gets its padding frames, use_mask = 0."""
    events, lens = [[0, 40, 60], [1, 0, 29], [2, 5, 6], [1, 31, 31]], [100, 33, 61]
    mask, ranges, quiet = _both(events, lens, 1, 30, 4, 1)
    assert mask.shape == (3, 100) and not mask[1, 33:].any() and not mask[2, 61:].any()
    assert ranges[1].tolist() == [[0, 30, 0], [30, 33, 0], [60, 90, 0], [90, 100, 0]] and not quiet[1].any()
    assert ranges[2].tolist() == [[0, 30, 1], [30, 60, 1], [30, 61, 1], [90, 100, 0]] and quiet[2].tolist() == [26, 30, 31, 0]
    from challenge_amd import transforms as T
    alone = T.quiet_ranges(T.quiet_mask([[0, 5, 6]], [61], 1), [61], 30, 4, 1)    # sample 2 alone: the same rows
    assert alone[0][0].tolist() == ranges[2, :3].tolist() and alone[1][0].tolist() == quiet[2, :3].tolist()
    got = T.quiet_frames(events, quiet, 30)
    assert got.dtype == np.int64 and got.tolist() == Q.quiet_frames_ref(events, quiet, 30).tolist()
    assert T.quiet_mask([], [5, 7], 3).shape == (2, 7) and T.quiet_mask([[1, 2, 3]], 10, 0, batch=2).sum() == 2


def test_mask_and_range_refusals():
    from challenge_amd import transforms as T
    for bad in ([[0, 5, 100]], [[0, -1, 5]], [[0, 6, 5]], [[1, 0, 5]], [[-1, 0, 5]], [[0.0, 1.0, 2.0]], [[0, 1]]):
        with pytest.raises(ValueError):
            T.quiet_mask(bad, [100], 0)
    for kw in (dict(guard=-1), dict(guard=1.5), dict(guard=True)):
        with pytest.raises(ValueError):
            T.quiet_mask([[0, 1, 2]], [100], **kw)
    with pytest.raises(ValueError):
        T.quiet_mask([[0, 1, 2]], [0])
    mask = np.zeros((2, 50), np.uint8)
    for kw in (dict(min_quiet=0), dict(reach=-1), dict(block=0), dict(min_quiet=2.0)):
        with pytest.raises(ValueError):
            T.quiet_ranges(mask, [50, 40], **{"block": 10, "min_quiet": 4, "reach": 1, **kw})
    with pytest.raises(ValueError):
        T.quiet_ranges(mask, [50, 51], 10)
    with pytest.raises(ValueError):
        T.quiet_ranges(mask, [50], 10)
    with pytest.raises(ValueError):
        T.quiet_ranges(mask.astype(np.int32), [50, 40], 10)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_dominant_event_no_longer_nulls_itself(seed):
    """extract_ref's scene with the source 10 dB ABOVE the interferer in frames 56 .. 455 of one 512-frame block, steered 1/8
    sample off: the block covariance gives <= 0 dB (NumPy: -1.01 .. -1.06), the covariance of the 108 frames outside the
    event widened by 2 gives >= 11 dB (12.35 .. 12.46).  10 dB under the interferer the two agree within 0.5 dB."""
    for source_db in (10.0, -10.0):
        source, noise, block, frames, k_lo = Q.scene("large", seed, source_db)
        mix = source + noise
        mask, ranges = Q.quiet_inputs(mix.shape[2], block, frames, 32, 1)
        assert ranges.tolist() == [[[0, 512, 1]]] and int((mask == 0).sum()) == 108
        g_block = Q.gain_of(source, noise, W.factors_ref(mix, block, 1e-2), block, frames, k_lo)
        g_quiet = Q.gain_of(source, noise, Q.factors_ref(mix, mask, ranges, 1e-2), block, frames, k_lo)
        print(f"large scene, seed {seed}, source {source_db:+.0f} dB: SINR gain block {g_block:+.2f} dB, quiet {g_quiet:+.2f} dB")
        if source_db > 0:
            assert g_block <= 0.0 and g_quiet >= 11.0
        else:
            assert abs(g_quiet - g_block) <= 0.5


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_filled_block_borrows_from_its_neighbours(seed):
    """F 33, T 96, blocks of 32, the event in frames 20 .. 75 fills block 1, min_quiet 16: its own block holds no quiet frame
    and falls back at reach 0 (<= 1.5 dB; NumPy: -0.16 .. 0.62), borrows 36 at reach 1 (>= 10.5 dB; 11.34 .. 11.86).  10 dB
    under the interferer quiet and block agree within 0.5 dB."""
    for source_db in (10.0, -10.0):
        source, noise, block, frames, k_lo = Q.scene("small", seed, source_db)
        mix = source + noise
        gains = {}
        for reach in (0, 1):
            mask, ranges = Q.quiet_inputs(mix.shape[2], block, frames, 16, reach)
            assert ranges[0, 1].tolist() == ([32, 64, 0] if reach == 0 else [0, 96, 1])
            gains[reach] = Q.gain_of(source, noise, Q.factors_ref(mix, mask, ranges, 1e-2), block, frames, k_lo)
        g_block = Q.gain_of(source, noise, W.factors_ref(mix, block, 1e-2), block, frames, k_lo)
        print(f"small scene, seed {seed}, source {source_db:+.0f} dB: SINR gain block {g_block:+.2f} dB, quiet at reach 0 "
              f"{gains[0]:+.2f} dB, at reach 1 {gains[1]:+.2f} dB")
        if source_db > 0:
            assert gains[0] <= 1.5 and gains[1] >= 10.5
        else:
            assert abs(gains[1] - g_block) <= 0.5


def test_the_reference_reduces_to_the_block_factors():
    """Own-block ranges without a mask are whiten_ref.factors_ref; a masked range without a quiet frame is zero."""
    x = W.mixed_spec(7, 2, 17, 50).astype(np.float64)
    mask = np.zeros((2, 50), np.uint8)
    ranges = np.array([[[0, 20, 0], [20, 40, 1], [40, 50, 0]]] * 2, np.int32)
    got, want = Q.factors_ref(x, mask, ranges, 1e-2), W.factors_ref(x, 20, 1e-2)
    assert all(np.allclose(g, w, rtol=1e-13, atol=0) for g, w in zip(got, want))     # (the means sum in another order)
    mask[1, 20:40] = 1
    got = Q.factors_ref(x, mask, ranges, 1e-2)
    assert not got[0][1, :, 1].any() and not got[1][1, :, 1].any() and not got[2][1, :, 1].any()
    assert np.allclose(got[0][0], want[0][0], rtol=1e-13, atol=0) and np.allclose(got[0][1, :, 0], want[0][1, :, 0], rtol=1e-13, atol=0)


def test_locate_settings_refusals_and_defaults():
    from challenge_amd.detect import LocateSettings
    s = LocateSettings(noise="quiet")
    assert (s.guard_s, s.min_quiet, s.reach) == (0.1, 32, 1) and LocateSettings().noise == "block"
    assert s.guard_frames() == 6 and s.guard_frames(512) == 3 and LocateSettings(guard_s=0).guard_frames() == 0
    assert LocateSettings(noise="quiet", guard_s=0.5, min_quiet=1, reach=0).guard_frames(256) == 31
    for kw in (dict(guard_s=-0.1), dict(guard_s=float("nan")), dict(guard_s=float("inf")), dict(guard_s="0.1"), dict(guard_s=True),
               dict(guard_s=None), dict(min_quiet=0), dict(min_quiet=-3), dict(min_quiet=1.5), dict(min_quiet=True),
               dict(min_quiet=None), dict(reach=-1), dict(reach=0.5), dict(reach=True), dict(reach=None)):
        with pytest.raises(ValueError, match="LocateSettings"):
            LocateSettings(noise="quiet", **kw)
    with pytest.raises(ValueError, match="noise"):
        LocateSettings(noise="bogus")


def test_cli_parsing(tmp_path, capsys):
    from challenge_amd import detect as DT
    common = ["--name", "run", "--path", str(tmp_path), "--wav_dir", str(tmp_path), "--locate"]
    with pytest.raises(SystemExit) as exc:
        DT.main(common + ["--locate_noise", "bogus"])
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "--locate_noise" in err and "quiet" in err
    for flag, bad in (("--locate_guard", "soon"), ("--locate_min_quiet", "1.5"), ("--locate_reach", "far")):
        with pytest.raises(SystemExit) as exc:
            DT.main(common + ["--locate_noise", "quiet", flag, bad])
        assert exc.value.code == 2 and flag in capsys.readouterr().err
    with pytest.raises(ValueError, match="min_quiet"):                      # parsed, then refused by LocateSettings' wording
        DT.main(common + ["--locate_noise", "quiet", "--locate_min_quiet", "0"])


def test_noise_frames_is_none_without_quiet(tmp_path):
    from challenge_amd import detect as DT
    ev = (np.array([[3, 9]], np.int64),)
    plain = DT.Detection("a", 50, ev, np.zeros((0, 2), np.int32), (np.zeros((0, 2), np.int32),))
    assert plain.noise_frames is None
    loc = (np.array([[0.5, -10.0, 2.0, 1.0]]),)
    located = DT.Detection("a", 50, ev, np.zeros((0, 2), np.int32), (np.zeros((0, 2), np.int32),), loc)
    assert located.noise_frames is None
    assert list(DT.write_locations([located], str(tmp_path / "where.json"))) == ["task2_location"]
    quiet = DT.Detection("a", 50, ev, np.zeros((0, 2), np.int32), (np.zeros((0, 2), np.int32),), loc,
                         noise_frames=(np.array([41], np.int64),))
    where = DT.write_locations([quiet], str(tmp_path / "quiet.json"))
    assert list(where) == ["task2_location", "noise_frames"] and where["noise_frames"] == {"a": [41]}


def test_c_abi_refuses_before_any_launch():
    """As test_extract_host's: a made-up plan pointer reaches every check that does not read the plan; the channel count is
    read from a zeroed block of memory whose seventh int is `channels`, the head of `struct iris_plan`."""
    from challenge_amd import _native as N
    lib = N.lib()
    p16, p8 = C.c_void_p(16), C.c_void_p(8)
    INVALID, UNSUPPORTED = -1, -2
    own = ((0, 50, 0), (50, 100, 1), (100, 150, 1))

    def call(plan=p16, spec=p16, mask=p16, dev=p16, rows=(own, own), fac=p16, batch=2, t=150, block=50, loading=1e-2):
        host = None
        if rows is not None:
            flat = [v for sample in rows for r in sample for v in r]
            host = (C.c_int32 * max(len(flat), 1))(*flat)
        return lib.iris_spec_whiten_factors_ranges(plan, spec, mask, dev, host, fac, batch, t, block, loading, None)
    for null in ("plan", "spec", "mask", "dev", "rows", "fac"):
        assert call(**{null: None}) == INVALID
    assert call(batch=0) == INVALID and call(t=0) == INVALID and call(batch=-1) == INVALID
    assert call(block=0) == INVALID and call(block=-5) == INVALID
    for loading in (0.0, -1e-2, float("nan"), float("inf")):
        assert call(loading=loading) == INVALID
    assert call(spec=p8) == INVALID and call(fac=p8) == INVALID            # not 16-byte aligned
    assert call(dev=C.c_void_p(18)) == INVALID
    for bad in ((-1, 50, 0), (50, 50, 1), (60, 50, 1), (100, 151, 0), (0, 50, 2), (0, 50, -1)):
        assert call(rows=(own, (own[0], bad, own[2]))) == INVALID
    assert b"iris_spec_whiten_factors_ranges" in lib.iris_last_error()

    def plan_of(channels):
        head = (C.c_int32 * 1024)()
        head[5], head[6] = 129, channels
        return head
    for channels in (1, 3):
        assert call(plan=plan_of(channels)) == UNSUPPORTED                 # the covariance is that of a stereo pair
    assert b"iris_spec_whiten_factors_ranges" in lib.iris_last_error()
    assert call(plan=plan_of(1), rows=(own, (own[0], (0, 151, 0), own[2]))) == INVALID   # the table is checked first


def test_cpu_tensors_are_refused():
    from challenge_amd import frontend as FE
    from challenge_amd import transforms as T
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        object.__new__(FE.FrontendPlan).whiten_factors_ranges(torch.zeros(1, 129, 20, 4), np.zeros((1, 20), np.uint8),
                                              np.array([[[0, 20, 0]]], np.int32), 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.locate_events(torch.zeros(1, 129, 20, 4), [[0, 0, 5]], noise="quiet")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.extract_events(torch.zeros(1, 129, 20, 4), [[0, 0, 5]], [0.0], noise="quiet")
    for fn, args in ((T.locate_events, ()), (T.extract_events, ([0.0],))):
        with pytest.raises(ValueError, match="quiet"):
            fn(torch.zeros(1, 129, 20, 4), [[0, 0, 5]], *args, noise="bogus")
