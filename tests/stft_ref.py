"""Reference form, error rule, launch geometry and case table of the standalone STFT (iris_stft, csrc/k_stft.h), a helper
beside the tests.  No GPU dependency.

Definition (load_wav's Spectrogram(n_fft, power=None)): wav [C, L] float32, N = n_fft, h = hop, F = N / 2 + 1, T = 1 + L // h

    w[i]       = 0.5 - 0.5 cos(2 pi i / N)        formed in float64 and rounded to float32 ONCE
    x_t[i]     = pad(wav)[t h + i],  0 <= i < N,   pad = reflect by N / 2 on both sides (no edge sample repeated)
    X[c, k, t] = sum_i w[i] x_t[i] exp(-2 pi j i k / N)

`stft_ref` evaluates it with numpy.fft.rfft on float64 copies of the float32 input and of that float32 window.  The window is
what the plan uploads: host_plan.h (`build_tables`) forms 0.5 - 0.5 cos(two_pi n / N) in double and casts it to float once, with
the same double two_pi, the same product / quotient order and libm's cos - `hann` below restates it.  The GPU module checks the
identity on the device: the DC bin of a unit impulse at window index i is w[i] with no rounding at all (every other term of
every sum is an exact zero), and it equals `hann(N)[i]` bit for bit for all N indices of all four sizes.

The rule.  For the re and the im part of every bin of frame (c, t)

    |X - X_ref| <= K u S[c, t],    u = 2^-24,    S[c, t] = ||w x_t||_2 + max_k |X_ref[c, k, t]|

and where S == 0 the output is exactly 0.  The scale is per frame and per channel - never per clip: a frame 1e4 times
quieter than its clip's loudest is held to its own level.  ||w x||_2 alone is not uniform (7 - 9 on noise, 30 - 90 on a tone:
a line's error is that of the line's peak, sqrt(N) above the norm), the per-bin |X_ref| does not help (leakage bins next to a
strong line inherit its error), the frame's peak bin does (measured by tests/test_stft_host.py on the table below).

K is not chosen here: tests/test_stft_host.py derives it with the repository's recipe (`istft_ref.k_from`: the smallest power
of two at or above four times the yardstick's worst ratio) from CPU torch.stft in float32 with the rounded-once window over
the case table, and asserts that the values recorded below are what it derives.  With normalize=True the reference is
R.normalize's definition in float64 (wav / (10 rms), rms over all channels of the clip jointly) followed by the fp64 STFT,
S comes from that normalised clip, and the yardstick is float32 normalise followed by float32 torch.stft - its own K.

`geometry` restates host_ops.h's `stft_geometry` (tile frames, per-round rounding, the fused kernel's balanced chunks, grid);
`iris_stft_geometry` is the query the GPU module holds it to.  `CASES` names, per case, what the launch must REACH (`reach`
computes it from a geometry); the GPU module asserts the declaration from the queried geometry before it compares a number."""
import numpy as np
import torch

from istft_ref import F32, U, hann, k_from, to_layout  # noqa: F401  (re-exported: one window, one recipe)

# ---- K, and the yardstick's worst ratio it comes from (tests/test_stft_host.py derives both and asserts these) ----
YARDSTICK_WORST = 2.73           # CPU torch.stft float32, rounded-once window, worst |dX| / (u S) over CASES at 256 CUs
K = 16
YARDSTICK_WORST_NORMALIZED = 3.42   # float32 normalise, then float32 torch.stft, against normalise + STFT in float64
K_NORMALIZED = 16

WAVES = {256: 16, 512: 16, 1024: 12, 2048: 4}
PMMAX = {256: 8, 512: 4, 1024: 2, 2048: 1}      # iris_fft.h FftCfg: padding of a wave's exchange buffer
LDS_BYTES = 160 * 1024
MAX_CHUNK_FRAMES = 16384
# host_ops.h by hand: n_fft -> {channels: tile_frames}
TILE_FRAMES = {256: {1: 128, 2: 64}, 512: {1: 48, 2: 24, 3: 15, 4: 12}, 1024: {1: 24, 2: 12}, 2048: {1: 12, 2: 6, 3: 5, 5: 3}}


def n_frames(length, hop):
    return 1 + int(length) // int(hop)


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
def frames64(wav, n_fft, hop):
    """wav [C, L] -> float64 [C, T, N]: the windowed frames w * x_t of the reflect-padded clip."""
    wav = np.asarray(wav)
    assert wav.dtype == F32 and wav.ndim == 2 and wav.shape[1] > n_fft // 2
    x = np.pad(wav.astype(np.float64), ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    t = n_frames(wav.shape[1], hop)
    idx = np.arange(t)[:, None] * hop + np.arange(n_fft)[None, :]
    return x[:, idx] * hann(n_fft).astype(np.float64)


def stft_ref(wav, n_fft, hop):
    """(X complex128 [C, F, T], S float64 [C, T]) by the definition, in float64."""
    fr = frames64(wav, n_fft, hop)
    x = np.fft.rfft(fr, n=n_fft, axis=-1).transpose(0, 2, 1)            # [C, F, T]
    s = np.sqrt((fr * fr).sum(axis=-1)) + np.abs(x).max(axis=1)          # [C, T]
    return x, s


def normalize64(clip):
    """R.normalize's definition in float64: clip [C, L] / (10 rms), rms over all channels jointly."""
    clip = np.asarray(clip, np.float64)
    return clip / (np.sqrt(np.mean(clip * clip)) * 10.0)


def stft_ref_normalized(wav, n_fft, hop):
    """normalize=True: (X, S) of the clip normalised in float64 (never rounded to float32 in between)."""
    wav = np.asarray(wav)
    assert wav.dtype == F32
    z = normalize64(wav)
    x = np.pad(z, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    t = n_frames(wav.shape[1], hop)
    idx = np.arange(t)[:, None] * hop + np.arange(n_fft)[None, :]
    fr = x[:, idx] * hann(n_fft).astype(np.float64)
    spec = np.fft.rfft(fr, n=n_fft, axis=-1).transpose(0, 2, 1)
    return spec, np.sqrt((fr * fr).sum(axis=-1)) + np.abs(spec).max(axis=1)


def layout_scale(s, n_bins):
    """S [C, T] -> the scale of every element of the [F, T, 2C] layout."""
    return np.broadcast_to(np.concatenate([s, s], axis=0).T[None], (n_bins,) + s.T.shape[:1] + (2 * s.shape[0],))


def rule_ratio(out, x_ref, s):
    """out [F, T, 2C] float32 against (X_ref [C, F, T], S [C, T]): (worst |d| / (u S), its (k, t, j) index).  Elements of a
    frame with S == 0 must be exactly 0 (asserted)."""
    out = np.asarray(out)
    ref = to_layout(x_ref)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    sc = layout_scale(s, out.shape[0])
    ok = sc > 0
    assert np.all(out[~ok] == 0), "a frame whose windowed samples are all zero must be exactly 0"
    assert not np.isnan(out).any(), "NaN in the spectrum of a finite input"
    ratio = np.zeros(out.shape)
    ratio[ok] = np.abs(out.astype(np.float64) - ref)[ok] / (U * sc[ok])
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def torch_stft(wav, n_fft, hop, dtype):
    """torch.stft on the CPU in `dtype` with the rounded-once window -> complex [C, F, T]."""
    w = torch.from_numpy(hann(n_fft)).to(dtype)
    return torch.stft(torch.from_numpy(np.asarray(wav)).to(dtype), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True).numpy()


def yardstick32(wav, n_fft, hop):
    return to_layout(torch_stft(wav, n_fft, hop, torch.float32))


def yardstick32_normalized(wav, n_fft, hop):
    """float32 normalise (oracle.frontend_ref.normalize's operations), then float32 torch.stft."""
    wav = np.asarray(wav, F32)
    rms = np.sqrt(np.mean(np.square(wav), dtype=F32), dtype=F32) * F32(10)
    return yardstick32((wav / rms).astype(F32), n_fft, hop)


# ---------------------------------------------------------------------------------------------------------------------
# inputs: [B, C, L] float32
# ---------------------------------------------------------------------------------------------------------------------
def gen_noise(b, c, length, n_fft, seed, levels=None):
    """Gaussian noise, per-clip level 10^U(-3, 1.5) (or `levels`)."""
    rng = np.random.default_rng(seed)
    lv = 10.0 ** rng.uniform(-3, 1.5, size=b) if levels is None else np.asarray(levels, np.float64)
    return (rng.standard_normal((b, c, length)) * lv[:, None, None]).astype(F32)


def gen_burst(b, c, length, n_fft, seed, levels=None):
    """Per-n_fft block levels 10^U(-4, 2), and a stretch of 2.5 n_fft exact zeros (some frames have S == 0) where the clip is
    long enough to hold one."""
    rng = np.random.default_rng(seed)
    nb = (length + n_fft - 1) // n_fft
    lv = np.repeat(10.0 ** rng.uniform(-4, 2, size=(b, 1, nb)), n_fft, axis=2)[:, :, :length]
    x = rng.standard_normal((b, c, length)) * lv
    z = (5 * n_fft) // 2
    if length >= z + n_fft:
        for i in range(b):
            at = int(rng.integers(0, length - z + 1))
            x[i, :, at:at + z] = 0
    return x.astype(F32)


def gen_tone(b, c, length, n_fft, seed, levels=None):
    """Channel 0: a sine at a non-bin frequency (bin 10.37 of n_fft) + 1e-3 noise; last channel: DC 0.5 + 1e-4 noise; channels in
    between: noise at 0.1."""
    rng = np.random.default_rng(seed)
    n = np.arange(length)
    x = rng.standard_normal((b, c, length)) * 0.1
    x[:, c - 1] = 0.5 + 1e-4 * rng.standard_normal((b, length))
    x[:, 0] = np.sin(2 * np.pi * tone_bin(n_fft) / n_fft * n + 0.3)[None] + 1e-3 * rng.standard_normal((b, length))
    return x.astype(F32)


def tone_bin(n_fft):
    return 10.37 if n_fft <= 512 else 40.37


def gen_impulse(b, c, length, n_fft, seed, levels=None):
    """As the indexing test: one unit impulse per clip and channel - first sample, mid-clip, last sample in turn."""
    ps = [0, min(n_fft + 3, length - 1), length - 1]
    x = np.zeros((b, c, length), F32)
    for i in range(b):
        for j in range(c):
            x[i, j, ps[(i + j) % 3]] = 1.0
    return x


GENERATORS = {"noise": gen_noise, "burst": gen_burst, "tone": gen_tone, "impulse": gen_impulse}


# ---------------------------------------------------------------------------------------------------------------------
# geometry: host_ops.h stft_geometry / fused_geometry restated
# ---------------------------------------------------------------------------------------------------------------------
def tile_frames_of(n_fft, c):
    nc, waves = n_fft // 2, WAVES[n_fft]
    f = nc + 1
    wave_buf = ((nc + PMMAX[n_fft] * (nc >> 4) + 1) * 8 + 15) & ~15
    room = (LDS_BYTES - 1024) - waves * wave_buf          # one workgroup per CU

    def tile_bytes(t):
        return f * (t * 2 * c + 1) * 4
    tf = 1
    while tf < 256 and tile_bytes(tf + 1) <= room:
        tf += 1
    assert tile_bytes(tf) <= room
    per_round = max(1, waves // max(1, c))
    if tf > per_round:
        tf -= tf % per_round
    return tf


def geometry(n_fft, hop, c, b, length, num_cu, chunk_target=0):
    """The launch of iris_stft: dict(tile_frames, chunks_per_clip, n_chunks, grid, waves) + T, chunk_base, chunk_rem."""
    t = n_frames(length, hop)
    slots, total = num_cu, b * t
    target = chunk_target if chunk_target > 0 else (total + slots - 1) // slots
    target = max(target, min(8, t))
    cpc = (t + target - 1) // target
    if chunk_target == 0 and b * cpc > slots and b <= slots:
        cpc = max(1, slots // b)
    cpc = max(cpc, (t + MAX_CHUNK_FRAMES - 1) // MAX_CHUNK_FRAMES)
    return dict(tile_frames=tile_frames_of(n_fft, c), chunks_per_clip=cpc, n_chunks=b * cpc, grid=min(b * cpc, num_cu), waves=WAVES[n_fft],
                T=t, chunk_base=t // cpc, chunk_rem=t % cpc, C=c, B=b)


def query_tuple(g):
    return (g["tile_frames"], g["chunks_per_clip"], g["n_chunks"], g["grid"], g["waves"])


def with_query(g, q):
    """The geometry dict with the five queried numbers in place of the restated ones."""
    g = dict(g)
    g["tile_frames"], g["chunks_per_clip"], g["n_chunks"], g["grid"], g["waves"] = (int(v) for v in q)
    g["chunk_base"], g["chunk_rem"] = g["T"] // g["chunks_per_clip"], g["T"] % g["chunks_per_clip"]
    return g


def reach(g):
    """What the kernel's control flow reaches under geometry g (k_stft.h: chunk i of a clip has chunk_base + (i < chunk_rem)
    frames, walks ceil(nt / tile_frames) tiles, backwards when i is odd)."""
    tf, cpc, c, waves = g["tile_frames"], g["chunks_per_clip"], g["C"], g["waves"]
    out = set()
    for i in range(cpc):
        nt = g["chunk_base"] + (1 if i < g["chunk_rem"] else 0)
        tiles, short = (nt + tf - 1) // tf, nt % tf
        if tiles >= 3 and short and i % 2 == 0:
            out.add("forward_3_tiles_short_last")
        if tiles >= 3 and short and i % 2 == 1:
            out.add("backward_3_tiles_short_first")
            if short * c < waves:
                out.add("idle_wave_prefetch")            # wv >= nwf in the first tile
        if tiles >= 2 and min(nt, tf) * c > waves:
            out.add("several_rounds")
            if waves % c:
                out.add("round_straddles_frames")        # wave-frames of one round belong to different frames, unevenly
    if g["chunk_rem"]:
        out.add("chunk_rem")
    if cpc == 1 and (g["T"] + tf - 1) // tf >= 4:
        out.add("one_chunk_many_tiles")
    if g["n_chunks"] > 2 * g["grid"]:
        clips = [[(w + r * g["grid"]) // cpc for r in range(3)] for w in range(g["grid"]) if w + 2 * g["grid"] < g["n_chunks"]]
        if any(a != b2 and b2 != c2 for a, b2, c2 in clips):
            out.add("third_chunk_of_another_clip")
    if c > waves:
        out.add("more_channels_than_waves")
    if g["T"] == 1:
        out.add("one_frame")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case table.  A shape is DERIVED from tile_frames (tf) and the CU count, never hard-coded:
#   walk   T = 4 tf + 3 in two chunks (IRIS_CHUNK_FRAMES = 2 tf + 2): chunk 0 = 2 tf + 2 frames walked forwards (3 tiles, the last of
#          2 frames), chunk 1 = 2 tf + 1 frames walked BACKWARDS (3 tiles, the first of 1 frame), chunk_rem = 1
#   one    one chunk per clip (a huge IRIS_CHUNK_FRAMES), T = 4 tf + 1: 5 tiles
#   many   IRIS_CHUNK_FRAMES = 8 and more than 2 grids of chunks: workgroups take a second and a third chunk of other clips
#   fixed  T from `length` under the automatic geometry (the edge shapes)
# ---------------------------------------------------------------------------------------------------------------------
def _case(name, n_fft, c, b, hop, shape, kind, reach_=(), normalize=False, length=None, max_batch=None, max_len_extra=0, rem=0):
    return dict(name=name, n_fft=n_fft, C=c, B=b, hop=hop, shape=shape, kind=kind, reach=frozenset(reach_), normalize=normalize,
                length=length, max_batch=max_batch or b, max_len_extra=max_len_extra, rem=rem)


_WALK = ("forward_3_tiles_short_last", "backward_3_tiles_short_first", "chunk_rem")
CASES = [
    _case("walk256_c1", 256, 1, 2, 32, "walk", "burst", _WALK + ("idle_wave_prefetch", "several_rounds")),
    _case("walk512_c3", 512, 3, 2, 77, "walk", "noise", _WALK + ("idle_wave_prefetch", "several_rounds", "round_straddles_frames"), rem=5),
    _case("walk1024_c2", 1024, 2, 1, 256, "walk", "tone", _WALK + ("idle_wave_prefetch", "several_rounds"), max_batch=3, max_len_extra=513),
    _case("walk2048_c2", 2048, 2, 2, 512, "walk", "burst", _WALK + ("idle_wave_prefetch", "several_rounds")),
    _case("walk2048_c5", 2048, 5, 1, 300, "walk", "noise", _WALK + ("more_channels_than_waves", "several_rounds")),
    _case("walk2048_c3", 2048, 3, 1, 1024, "walk", "tone", _WALK + ("idle_wave_prefetch", "several_rounds", "round_straddles_frames")),
    _case("one512_c2", 512, 2, 2, 128, "one", "tone", ("one_chunk_many_tiles", "forward_3_tiles_short_last", "several_rounds")),
    _case("one1024_c1", 1024, 1, 3, 255, "one", "burst", ("one_chunk_many_tiles", "forward_3_tiles_short_last", "several_rounds"), rem=7),
    _case("many256_c1", 256, 1, 5, 32, "many", "noise", ("third_chunk_of_another_clip", "chunk_rem")),
    _case("many256_c1_norm", 256, 1, 5, 32, "many", "noise", ("third_chunk_of_another_clip", "chunk_rem"), normalize=True),
    _case("many256_c2_norm", 256, 2, 4, 48, "many", "noise", ("third_chunk_of_another_clip", "chunk_rem"), normalize=True, rem=11),
    _case("shortest256", 256, 1, 2, 64, "fixed", "noise", length=129),
    _case("oddhop512", 512, 1, 3, 77, "fixed", "burst", length=3001),
    _case("oddlen1024", 1024, 1, 1, 255, "fixed", "noise", length=4097, max_batch=2, max_len_extra=100),
    _case("hop_is_nfft256", 256, 2, 4, 256, "fixed", "noise", length=1300),
    _case("one_frame256", 256, 1, 3, 400, "fixed", "noise", ("one_frame",), length=300),
    _case("impulse512", 512, 1, 3, 256, "fixed", "impulse", length=5 * 512 + 37),
    _case("norm_walk512_c2", 512, 2, 3, 200, "walk", "tone", _WALK + ("idle_wave_prefetch",), normalize=True),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def many_levels(b):
    """Clip levels of the `many` cases: 1e-3 ... 3e1 geometrically, neighbours 10^(4.5 / (b - 1)) apart (>= 1e3 end to end)."""
    return 10.0 ** (-3.0 + 4.5 * np.arange(b) / (b - 1))


def concrete(case, num_cu):
    """The case on a device of `num_cu` CUs: length, IRIS_CHUNK_FRAMES (0 = unset), plan capacity and the restated geometry."""
    n_fft, c, b, hop = case["n_fft"], case["C"], case["B"], case["hop"]
    tf = tile_frames_of(n_fft, c)
    if case["shape"] == "walk":
        t, chunk = 4 * tf + 3, 2 * tf + 2
    elif case["shape"] == "one":
        t, chunk = 4 * tf + 1, 1 << 20
    elif case["shape"] == "many":
        cpc = (2 * num_cu + 8 + b - 1) // b + 1
        t, chunk = 8 * cpc - 3, 8
    else:
        t, chunk = n_frames(case["length"], hop), 0
    length = case["length"] if case["shape"] == "fixed" else (t - 1) * hop + case["rem"] % hop
    assert n_frames(length, hop) == t and length > n_fft // 2
    g = geometry(n_fft, hop, c, b, length, num_cu, chunk)
    return dict(case, length=length, T=t, chunk_target=chunk, max_len=length + case["max_len_extra"], geom=g)


def make_input(case, length):
    levels = many_levels(case["B"]) if case["shape"] == "many" else None
    seed = 1000 + sum(ord(ch) for ch in case["name"])
    return GENERATORS[case["kind"]](case["B"], case["C"], length, case["n_fft"], seed, levels)
