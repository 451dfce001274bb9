"""The standalone STFT kernel (iris_stft, k_stft<LOG2N> in csrc/k_stft.h) against the float64 definition of tests/stft_ref.py,
frame by frame: |X - X_ref| <= K u S[c, t] on the re and im part of every bin, S = ||w x_t||_2 + max_k |X_ref[c, k, t]| per frame and
channel, exact zeros where S == 0 (stft_ref's docstring states the rule; tests/test_stft_host.py derives K = 16, and 16 for
normalize=True, from CPU torch.stft in float32, whose own worst ratios are 2.73 and 3.42).

Cases are chosen by the launch geometry, not by workload (stft_ref.CASES): every case declares what the kernel's control flow
must reach - a forward walk of 3 tiles with a short last tile, a backward walk whose short first tile leaves waves without a
frame (the `wv >= nwf` prefetch), chunks that differ by one frame, one chunk of many tiles, workgroups that take a second and a
third chunk of OTHER clips (plain and with the per-clip normalize scale, clip levels 1e-3 ... 3e1), rounds that straddle
frames (C = 3), more channels than waves (C = 5 at n_fft 2048) - and the declaration is asserted from `iris_stft_geometry` before a
single number is compared; the Python restatement of the geometry must equal that query.  Every call goes through the C ABI
on buffers the test owns: the spectrum between two bands of 4096 words of the NaN pattern 0x7FE5A5A5 (both bands keep it, no output
word does), the waveform inside such a buffer too, so a read before the first or after the last sample of the batch is a NaN in
the output.

Measured on one MI355X (256 CUs; profiles/stft/rule_ratios.log has the cases): the kernel's worst ratio is 2.83 plain (case
walk512_c3: n_fft 512, C 3, noise, clip 1, bin 131, frame 45) and 3.64 with normalize=True (case many256_c2_norm: n_fft 256, C 2,
clip 2, bin 50, frame 568) - 0.18 and 0.23 of the bound, beside the float32 yardstick's 2.73 and 3.42.

What the module found: test_one_nan_stays_in_the_frames_that_cover_it[0-1-514] failed on the kernel as it was.  With the NaN at
window index i = 0 or 1 mod n_fft / 4 of a frame, ONE word of that frame stayed finite: bin n_fft / 4, its imaginary part for even
i, its real part for odd i (at all four sizes; nothing leaked into another frame).  The definition's coefficient there is an
exact zero (sin or cos of pi i / 2) that the transform never multiplied by: sample i sits in lane 0's points of the packed
half-size FFT, whose path to Z[n_fft / 4] is additions and +-j swaps only, and X[n_fft / 4] = conj(Z[n_fft / 4]) copied the parts.
k_stft now adds 0 * the other part to each part of that bin (no finite value changes); p = 10 hop - n_fft / 2, the window's
zero, is such an index, p = 5 is not."""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_ref as S
from test_conv_gpu import GUARD, PATTERN, Guarded

pytestmark = pytest.mark.gpu

WORST = {}          # case name -> (ratio, where): printed by the last test of the module


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def num_cu(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _N():
    from challenge_amd import _native
    return _native


def make_plan(cc, dev, monkeypatch, chunk):
    """A plan of the case's capacity whose chunk target is `chunk` frames (0: the automatic geometry)."""
    from challenge_amd import frontend as FE
    if chunk:
        monkeypatch.setenv("IRIS_CHUNK_FRAMES", str(chunk))
    else:
        monkeypatch.delenv("IRIS_CHUNK_FRAMES", raising=False)
    try:
        return FE.FrontendPlan(cc["n_fft"], cc["hop"], 8, 16000, cc["C"], cc["max_batch"], cc["max_len"], dev)
    finally:
        monkeypatch.delenv("IRIS_CHUNK_FRAMES", raising=False)


def query(plan, batch, length):
    out = (C.c_int * 5)()
    N = _N()
    N.check(N.lib().iris_stft_geometry(plan._handle, batch, length, out), "iris_stft_geometry")
    return tuple(out)


def run_stft(plan, dev, wav, normalize=False, what="iris_stft"):
    """wav [B, C, L] NumPy -> (spectrum [B, F, T, 2C] as a device tensor inside its guarded buffer, checked).  Both buffers are
    the test's own; the call is the C ABI's."""
    N = _N()
    b, c, length = wav.shape
    f, t = plan.n_fft // 2 + 1, 1 + length // plan.hop
    src = Guarded(dev, wav.size)
    src.t.copy_(torch.from_numpy(np.ascontiguousarray(wav).reshape(-1)))
    dst = Guarded(dev, b * f * t * 2 * c)
    with torch.cuda.device(dev):
        rc = N.lib().iris_stft(plan._handle, src.ptr(), dst.ptr(), b, length, N.IRIS_F_NORMALIZE if normalize else 0,
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    N.check(rc, "iris_stft")
    dst.check(what)                                      # both bands keep the pattern, no output word does
    assert bool((src.buf[:GUARD] == PATTERN).all()) and bool((src.buf[GUARD + src.n:] == PATTERN).all())
    return dst.t.view(b, f, t, 2 * c)


_REF = {}


def reference(case, cc):
    """(wav, [X_ref per clip], [S per clip]) of a case, computed once and shared."""
    key = (case["name"], cc["length"])
    if key not in _REF:
        wav = S.make_input(case, cc["length"])
        fn = S.stft_ref_normalized if case["normalize"] else S.stft_ref
        refs = [fn(wav[b], case["n_fft"], case["hop"]) for b in range(case["B"])]
        _REF[key] = (wav, [r[0] for r in refs], [r[1] for r in refs])
    return _REF[key]


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_case_meets_the_rule_at_its_geometry(dev, num_cu, monkeypatch, name):
    case = S.CASE_BY_NAME[name]
    cc = S.concrete(case, num_cu)
    b, length, norm = case["B"], cc["length"], case["normalize"]
    plan = make_plan(cc, dev, monkeypatch, cc["chunk_target"])
    # 1. the geometry: the query equals the restatement, and the launch reaches what the case declares
    q = query(plan, b, length)
    assert q == S.query_tuple(cc["geom"]), (name, q, cc["geom"])
    assert q[0] == S.TILE_FRAMES[case["n_fft"]][case["C"]]
    got = S.reach(S.with_query(cc["geom"], q))
    assert case["reach"] <= got, (name, sorted(case["reach"] - got), q)
    # 2. the rule, on every element
    wav, xs, ss = reference(case, cc)
    spec_dev = run_stft(plan, dev, wav, norm, name)
    spec = spec_dev.cpu().numpy()
    k = S.K_NORMALIZED if norm else S.K
    worst, where = 0.0, None
    for i in range(b):
        r, at = S.rule_ratio(spec[i], xs[i], ss[i])
        if r >= worst:
            worst, where = r, (i,) + at
    n_silent = sum(int((s == 0).sum()) for s in ss)
    print(f"stft {name}: n_fft {case['n_fft']} C {case['C']} B {b} T {cc['T']} hop {case['hop']} {case['kind']}{' normalize' if norm else ''} "
          f"tile {q[0]} chunks/clip {q[1]} chunks {q[2]} grid {q[3]} waves {q[4]}: worst |dX| / (u S) = {worst:.3f} at (b, k, t, j) = {where} "
          f"(K = {k}; {n_silent} silent frames)")
    WORST[name] = (worst, where, norm)
    assert worst <= k, (name, worst, where)
    # 3. bit equality across geometries: the per-frame arithmetic does not depend on the walk, nor on the batch around a clip
    for chunk in (0, 8, 1 << 20):
        if chunk == cc["chunk_target"]:
            continue
        other = make_plan(cc, dev, monkeypatch, chunk)
        assert torch.equal(run_stft(other, dev, wav, norm, f"{name} chunk target {chunk}"), spec_dev), (name, chunk, query(other, b, length))
    if b > 1:
        for i in (0, b - 1):
            alone = run_stft(plan, dev, wav[i:i + 1], norm, f"{name} clip {i} alone")
            assert torch.equal(alone[0], spec_dev[i]), (name, i)


def test_orientation_of_the_spectrum(dev, num_cu, monkeypatch):
    """Conjugation and channel blocks, by name: the imaginary part at the line's peak bin has the sign the definition gives it,
    and channel c's re / im sit in blocks c and C + c (channel 0 holds a line, the last channel DC)."""
    case = S.CASE_BY_NAME["walk1024_c2"]
    cc = S.concrete(case, num_cu)
    wav, xs, _ = reference(case, cc)
    spec = run_stft(make_plan(cc, dev, monkeypatch, cc["chunk_target"]), dev, wav).cpu().numpy()[0]   # [F, T, 2C]
    x, c = xs[0], case["C"]
    kp = int(round(S.tone_bin(case["n_fft"])))
    frames = np.arange(4, cc["T"] - 4)                      # away from the reflected edges
    peak = np.abs(x[0, kp, frames])
    assert np.all(peak > 100) and np.all(np.abs(x[c - 1, kp, frames]) < 1e-2 * peak)        # the line is channel 0's alone
    strong = frames[np.abs(x[0, kp, frames].imag) > 0.2 * peak]
    assert strong.size > 10
    assert np.array_equal(np.sign(spec[kp, strong, c + 0]), np.sign(x[0, kp, strong].imag)), "conjugated spectrum"
    assert np.all(np.abs(spec[kp, frames, 0] - x[0, kp, frames].real) < 1e-3 * peak), "channel 0's re is not in block 0"
    assert np.all(np.abs(spec[kp, frames, c] - x[0, kp, frames].imag) < 1e-3 * peak), "channel 0's im is not in block C"
    dc = x[c - 1, 0, frames].real
    assert np.all(dc > 100)
    assert np.all(np.abs(spec[0, frames, c - 1] - dc) < 1e-3 * dc), "the last channel's re is not in block C - 1"
    assert np.all(np.abs(spec[0, frames, 2 * c - 1]) < 1e-3 * dc), "the last channel's im is not in block 2C - 1"
    assert np.all(np.abs(spec[0, frames, 0]) < 1e-1 * dc)


@pytest.mark.parametrize("clip,chan,p", [(1, 2, 5), (0, 1, 10 * 77 - 256)])
def test_one_nan_stays_in_the_frames_that_cover_it(dev, num_cu, monkeypatch, clip, chan, p):
    """One NaN at sample p of (clip, chan): exactly the frames whose window covers p - through the reflection too (p = 5), and
    where it meets the window's zero at index 0 (p = 10 hop - n_fft / 2) - are NaN in all bins of re and im of that (clip, chan);
    every other frame, channel and clip is bitwise what the run without the NaN gave."""
    case = S.CASE_BY_NAME["walk512_c3"]
    cc = S.concrete(case, num_cu)
    n_fft, hop, c, length = case["n_fft"], case["hop"], case["C"], cc["length"]
    assert S.reach(cc["geom"]) >= {"forward_3_tiles_short_last", "backward_3_tiles_short_first"} and c == 3
    wav = reference(case, cc)[0]
    plan = make_plan(cc, dev, monkeypatch, cc["chunk_target"])
    clean = run_stft(plan, dev, wav)
    bad = wav.copy()
    bad[clip, chan, p] = np.nan
    out = run_stft(plan, dev, bad)
    origin = np.pad(np.arange(length), (n_fft // 2, n_fft // 2), mode="reflect")
    idx = np.arange(cc["T"])[:, None] * hop + np.arange(n_fft)[None, :]
    covers = (origin[idx] == p).any(axis=1)                                      # [T]
    assert 2 <= covers.sum() < cc["T"]
    if p == 5:
        assert covers[0] and (origin[:n_fft // 2] == p).any()                     # reached through the reflection as well
    else:
        assert (origin[idx][:, 0] == p).any()                                     # one frame holds it at the window's zero
    expect = torch.zeros(clean.shape, dtype=torch.bool)
    expect[clip, :, torch.from_numpy(covers), chan] = True
    expect[clip, :, torch.from_numpy(covers), c + chan] = True
    expect = expect.to(dev)
    assert bool(torch.isnan(out)[expect].all()), "a frame that covers the NaN has a finite bin"
    same = out.view(torch.int32) == clean.view(torch.int32)
    assert bool(same[~expect].all()), "the NaN leaked into another frame, channel or clip"


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048])
def test_the_plan_uploads_the_window_rounded_once(dev, n_fft):
    """hop 1 and one unit impulse: frame t holds it at window index i = p + n_fft / 2 - t, every other term of every sum is an
    exact zero, so the DC bin IS w[i] - equal bit for bit to the float64 Hann window rounded to float32 once (stft_ref.hann),
    for all n_fft indices."""
    from challenge_amd import frontend as FE
    length = n_fft + 44
    p = length // 2
    wav = np.zeros((1, 1, length), np.float32)
    wav[0, 0, p] = 1.0
    plan = FE.FrontendPlan(n_fft, 1, 8, 16000, 1, 1, length, dev)
    spec = run_stft(plan, dev, wav).cpu().numpy()[0]
    t = p + n_fft // 2 - np.arange(n_fft)
    assert t.min() >= 0 and t.max() < spec.shape[1]
    assert np.array_equal(spec[0, t, 0], S.hann(n_fft))
    assert np.all(spec[0, t, 1] == 0)


def test_report_the_worst_ratios():
    """Prints what the module docstring and DESIGN.md record (run with -s); needs the cases above to have run."""
    if not WORST:
        return
    for norm in (False, True):
        rows = [(r, n, w) for n, (r, w, nm) in WORST.items() if nm == norm]
        r, n, w = max(rows)
        case = S.CASE_BY_NAME[n]
        print(f"stft worst ratio{' (normalize)' if norm else ''}: {r:.3f} at case {n} (n_fft {case['n_fft']}, C {case['C']}, {case['kind']}), "
              f"(b, k, t, j) = {w}; yardstick {S.YARDSTICK_WORST_NORMALIZED if norm else S.YARDSTICK_WORST}, K = {S.K_NORMALIZED if norm else S.K}")
