"""Host tests of tests/stft_ref.py (no GPU): the float64 definition against torch.stft in float64, K and the normalised K derived
from the float32 yardstick (CPU torch.stft with the rounded-once window) over the case table, the restated launch geometry
against the tile sizes read off host_ops.h by hand, every declared reach of the case table at several CU counts, and the
presence of silent frames in the inputs."""
import numpy as np
import pytest

import stft_ref as S

CU_COUNTS = (256, 64, 304)


@pytest.mark.parametrize("n_fft,hop,c,length", [(256, 64, 2, 1500), (512, 77, 1, 3001), (1024, 256, 3, 4097), (2048, 512, 1, 9000),
                                                (256, 256, 1, 129), (256, 400, 1, 300)])
def test_definition_equals_torch_stft_in_float64(n_fft, hop, c, length):
    wav = S.gen_noise(1, c, length, n_fft, 3)[0]
    x, s = S.stft_ref(wav, n_fft, hop)
    t64 = S.torch_stft(wav, n_fft, hop, __import__("torch").float64)
    assert x.shape == t64.shape == (c, n_fft // 2 + 1, 1 + length // hop) and s.shape == (c, 1 + length // hop)
    assert np.abs(x - t64).max() <= 1e-12 * np.abs(x).max()
    # the window is the float64 form rounded to float32 once, and the oracle's own
    from oracle import frontend_ref as R
    assert np.array_equal(S.hann(n_fft), R.hann_periodic(n_fft)) and S.hann(n_fft).dtype == np.float32
    # the normalised reference is linear in the float64 scale
    xn, sn = S.stft_ref_normalized(wav, n_fft, hop)
    g = 1.0 / (np.sqrt(np.mean(wav.astype(np.float64) ** 2)) * 10.0)
    assert np.abs(xn - g * x).max() <= 1e-12 * np.abs(xn).max() and np.abs(sn - g * s).max() <= 1e-12 * sn.max()


def _yardstick_worst(normalized):
    worst, where = 0.0, None
    for case in S.CASES:
        if case["kind"] == "impulse":
            continue
        cc = S.concrete(case, 256)
        wav = S.make_input(case, cc["length"])
        for b in range(case["B"]):
            if normalized:
                x, s = S.stft_ref_normalized(wav[b], case["n_fft"], case["hop"])
                y = S.yardstick32_normalized(wav[b], case["n_fft"], case["hop"])
            else:
                x, s = S.stft_ref(wav[b], case["n_fft"], case["hop"])
                y = S.yardstick32(wav[b], case["n_fft"], case["hop"])
            r, at = S.rule_ratio(y, x, s)
            if r > worst:
                worst, where = r, (case["name"], b, at)
    return worst, where


def test_k_is_derived_from_the_float32_yardstick():
    worst, where = _yardstick_worst(False)
    print(f"yardstick (torch.stft float32): worst |dX| / (u S) = {worst:.3f} at {where} -> K = {S.k_from(worst)}")
    assert S.k_from(worst) == S.K, (worst, where)
    assert abs(worst - S.YARDSTICK_WORST) <= 0.05 * S.YARDSTICK_WORST, (worst, S.YARDSTICK_WORST)   # the recorded figure is this one


def test_normalized_k_is_derived_from_the_float32_yardstick():
    worst, where = _yardstick_worst(True)
    print(f"yardstick (float32 normalise + torch.stft float32): worst ratio {worst:.3f} at {where} -> K = {S.k_from(worst)}")
    assert S.k_from(worst) == S.K_NORMALIZED, (worst, where)
    assert abs(worst - S.YARDSTICK_WORST_NORMALIZED) <= 0.05 * S.YARDSTICK_WORST_NORMALIZED, (worst, S.YARDSTICK_WORST_NORMALIZED)


def test_geometry_reproduces_the_hand_derived_tile_table():
    for n_fft, row in S.TILE_FRAMES.items():
        for c, tf in row.items():
            g = S.geometry(n_fft, n_fft // 4, c, 2, 8 * n_fft, 256)
            assert g["tile_frames"] == tf and g["waves"] == S.WAVES[n_fft], (n_fft, c, g)
    assert S.WAVES == {256: 16, 512: 16, 1024: 12, 2048: 4}
    # the fused kernel's balanced chunks: one chunk per CU when the problem is large enough, never across clips
    g = S.geometry(1024, 256, 1, 40, 25600, 256)
    assert (g["T"], g["chunks_per_clip"], g["n_chunks"], g["grid"]) == (101, 6, 240, 240)
    g = S.geometry(1024, 256, 1, 40, 25600, 256, 8)
    assert (g["chunks_per_clip"], g["n_chunks"], g["grid"], g["chunk_base"], g["chunk_rem"]) == (13, 520, 256, 7, 10)


@pytest.mark.parametrize("num_cu", CU_COUNTS)
def test_every_declared_reach_holds(num_cu):
    reached, sizes, chans = set(), {}, set()
    for case in S.CASES:
        cc = S.concrete(case, num_cu)
        got = S.reach(cc["geom"])
        assert case["reach"] <= got, (case["name"], num_cu, sorted(case["reach"] - got), cc["geom"])
        reached |= case["reach"]
        sizes[case["n_fft"]] = sizes.get(case["n_fft"], 0) + 1
        chans.add(case["C"])
        assert cc["T"] * case["B"] <= 6000, (case["name"], cc["T"])          # the reference stays a few thousand frames
        if case["shape"] == "many":
            lv = S.many_levels(case["B"])
            assert lv.max() / lv.min() >= 1e3 and np.all(lv[1:] / lv[:-1] >= 2)
    assert reached >= {"forward_3_tiles_short_last", "backward_3_tiles_short_first", "idle_wave_prefetch", "chunk_rem", "one_chunk_many_tiles",
                       "third_chunk_of_another_clip", "round_straddles_frames", "more_channels_than_waves", "one_frame"}
    assert all(sizes.get(n, 0) >= 2 for n in (256, 512, 1024, 2048)), sizes
    assert chans >= {1, 2, 3, 5}
    by = S.CASE_BY_NAME
    assert by["shortest256"]["length"] == 256 // 2 + 1 and by["oddhop512"]["hop"] % 2 and by["oddlen1024"]["length"] % 2
    assert by["hop_is_nfft256"]["hop"] == 256 and by["one_frame256"]["hop"] > by["one_frame256"]["length"]
    assert any(c["B"] == c["max_batch"] for c in S.CASES) and any(c["B"] < c["max_batch"] and c["max_len_extra"] for c in S.CASES)


def test_inputs_contain_silent_frames():
    for name in ("walk256_c1", "walk2048_c2", "one1024_c1", "oddhop512"):
        case = S.CASE_BY_NAME[name]
        cc = S.concrete(case, 256)
        wav = S.make_input(case, cc["length"])
        n = sum(int((S.stft_ref(wav[b], case["n_fft"], case["hop"])[1] == 0).sum()) for b in range(case["B"]))
        assert n > 0, name
    imp = S.CASE_BY_NAME["impulse512"]
    wav = S.make_input(imp, imp["length"])
    assert (S.stft_ref(wav[0], 512, 256)[1] == 0).any()
