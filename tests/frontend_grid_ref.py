"""Host-side reference of the fused-frontend variant grid (tests/test_frontend_grid_gpu.py) -- TEST INFRASTRUCTURE.

The fused waveform -> mel kernel is a family of template instantiations k_wav_to_mel<LOG2N, mel_mode, HI, BANDS, 1, FUSE>; the
plan picks one from n_fft, n_mel and the filterbank's band geometry.  This module holds
  * the CASE TABLE: one shape per (LOG2N, mel_mode, HI) triple the plan can pick, each DECLARING the variant it must reach
    (the GPU test asserts the declaration against `plan.fused_kernel_name` before it looks at a value), plus the edge shapes
    that belong with the grid;
  * the input recipe (three clips at different levels, odd length, 25 frames) and the band draws;
  * `mel_tolerance_w`: the ONE stated mel rule of oracle.frontend_ref.mel_tolerance,
        |mel - ref| <= 1e-5 |ref| + 4 eps_fp32 xrms[b, t, c] sum_k W[k, m],
    restated with the weight matrix W GIVEN (a caller-supplied `mel_matrix` has no (n_mel, edges) to rebuild it from);
    tests/test_frontend_grid_host.py holds it equal to the oracle's on a standard bank;
  * `ordinary_share`: the fraction of elements on which the rule's relative term decides (north_star's literal 1e-5), over the
    columns that carry a weight - the condition that keeps the noise-floor term from hiding a failure.
Nothing here restates the plan's heuristic: the table is a test input, the device's answer is the kernel name."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from oracle import frontend_ref as R

BATCH = 3


class Case(NamedTuple):
    name: str
    n_fft: int
    variant: Tuple[int, int, bool]      # (LOG2N, mel_mode, HI) the plan must pick
    n_mel: int
    channels: int
    sample_rate: float = 16000.0
    lower: float = 125.0
    upper: float = 3800.0
    dense: bool = False                 # a dense random non-negative mel_matrix [n_fft / 2 + 1, n_mel] instead of a standard bank
    ledger: bool = True                 # counts towards the 22-triple ledger (False: an edge shape on an already listed variant)

    @property
    def hop(self) -> int:
        return self.n_fft // 4

    @property
    def length(self) -> int:
        return 6 * self.n_fft + 37      # odd; 1 + length // hop = 25 frames

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    @property
    def n_frames(self) -> int:
        return 1 + self.length // self.hop


# Channel counts 1, 2, 3 are spread so that every mel_mode sees each of them at least once.
GRID = [
    Case("256-40mel", 256, (8, 0, False), 40, 1),
    Case("256-8mel", 256, (8, 1, False), 8, 1),
    Case("256-20mel-full", 256, (8, 1, True), 20, 2, lower=20.0, upper=8000.0),
    Case("256-1mel", 256, (8, 2, False), 1, 1, lower=0.0, upper=4000.0),        # one band of 63 bins
    Case("256-65mel", 256, (8, 3, False), 65, 1),                               # 3 empty columns; 65 = one band past the lanes
    Case("256-dense80", 256, (8, 2, True), 80, 2, dense=True),
    Case("512-40mel", 512, (9, 0, False), 40, 2),
    Case("512-8mel", 512, (9, 1, False), 8, 3),
    Case("512-64mel-full", 512, (9, 1, True), 64, 1, lower=20.0, upper=8000.0),
    Case("512-1mel", 512, (9, 2, False), 1, 3, lower=0.0, upper=4000.0),
    Case("512-128mel", 512, (9, 3, False), 128, 2),                             # 5 empty columns
    Case("512-dense48", 512, (9, 2, True), 48, 3, dense=True),
    Case("1024-64mel", 1024, (10, 0, False), 64, 3),
    Case("1024-150mel", 1024, (10, 1, False), 150, 2),
    Case("1024-40mel-full", 1024, (10, 1, True), 40, 3, lower=20.0, upper=8000.0),
    Case("1024-1mel", 1024, (10, 2, False), 1, 2, lower=0.0, upper=4000.0),
    Case("1024-96mel-low", 1024, (10, 3, False), 96, 3, upper=1500.0),
    Case("1024-dense24", 1024, (10, 2, True), 24, 1, dense=True),
    Case("2048-128mel-22k", 2048, (11, 1, False), 128, 2, sample_rate=22050.0),
    Case("2048-80mel-full", 2048, (11, 1, True), 80, 1, lower=20.0, upper=8000.0),
    Case("2048-1mel", 2048, (11, 2, False), 1, 1, lower=0.0, upper=4000.0),
    Case("2048-800mel-full", 2048, (11, 2, True), 800, 1, lower=20.0, upper=8000.0),   # 41 empty columns
    Case("2048-dense12", 2048, (11, 2, True), 12, 2, dense=True),
]
# Edge shapes on variants the grid already lists:
#   * lower edge 0 Hz: the lowest band starts at bin 1 (bin 0 carries no weight in the recipe), and at n_fft 256 / 40 mel the
#     top bands' 20-bin register windows are clamped to the 64 bins the half-spectrum variant writes;
#   * 129 mel at n_fft 512: one band more than two per lane hold, so the plan leaves mode 3 for the LDS table.
EDGES = [
    Case("256-40mel-from0", 256, (8, 0, False), 40, 2, lower=0.0, ledger=False),
    Case("512-129mel", 512, (9, 1, False), 129, 1, ledger=False),
]
CASES = GRID + EDGES
BY_NAME = {c.name: c for c in CASES}

# the 22 (LOG2N, mel_mode, HI) triples the plan's dispatch can return
TRIPLES = [(l, m, h) for l in (8, 9, 10) for (m, h) in ((0, False), (3, False), (1, False), (1, True), (2, False), (2, True))] + \
          [(11, m, h) for (m, h) in ((1, False), (1, True), (2, False), (2, True))]


def kernel_name(variant, bands: bool, fuse: int = 1) -> str:
    """What `FrontendPlan.fused_kernel_name(bands)` prints for `variant` (one frame stream; fuse 1 = the default epilogue)."""
    log2n, mode, hi = variant
    return f"k_wav_to_mel<{log2n},{mode},{'true' if hi else 'false'},{'true' if bands else 'false'},1,{fuse}>"


def _seed(case: Case) -> int:
    return 1000 * case.n_fft + 10 * case.n_mel + case.channels + (5 if case.dense else 0)


def weights(case: Case) -> np.ndarray:
    """W [n_bins, n_mel] float32: the standard bank of the case (the oracle's recipe, which test_host_mel_matrix_used_by_plan
    holds equal to the plan's own), or the dense random non-negative matrix handed to the plan as `mel_matrix`."""
    if case.dense:
        rng = np.random.default_rng(_seed(case) + 1)
        return rng.uniform(0.0, 1.0, (case.n_bins, case.n_mel)).astype(np.float32)
    return R.linear_to_mel_weight_matrix(case.n_mel, case.n_bins, case.sample_rate, lower_edge_hertz=case.lower,
                                         upper_edge_hertz=case.upper)


def plan_kwargs(case: Case) -> dict:
    """Filterbank arguments of `FrontendPlan` for the case."""
    if case.dense:
        return {"mel_matrix": weights(case)}
    return {"lower_edge_hertz": case.lower, "upper_edge_hertz": case.upper}


def make_wav(case: Case) -> np.ndarray:
    """[3, C, 6 n_fft + 37] float32: white noise, every clip at its own level."""
    rng = np.random.default_rng(_seed(case))
    level = rng.uniform(0.02, 0.5, (BATCH, 1, 1))
    return (rng.standard_normal((BATCH, case.channels, case.length)) * level).astype(np.float32)


def make_bands(case: Case):
    """(t_bands [3, 3, 2], f_bands [3, 2, 2]) int32 of (offset, size), drawn as test_bands_all_fft_sizes draws them."""
    rng = np.random.default_rng(_seed(case) + 2)
    tb = np.stack([np.stack(R.mask_draw(rng, case.n_frames, 6, 3), 1) for _ in range(BATCH)]).astype(np.int32)
    fb = np.stack([np.stack(R.mask_draw(rng, case.n_bins, 16, 2), 1) for _ in range(BATCH)]).astype(np.int32)
    return tb, fb


def band_support(w: np.ndarray):
    """(first [M], length [M]) of every column's non-zero bin range; length 0 for an all-zero column."""
    nz = w != 0
    any_ = nz.any(axis=0)
    first = np.where(any_, nz.argmax(axis=0), 0)
    last = np.where(any_, w.shape[0] - 1 - nz[::-1].argmax(axis=0), -1)
    return first.astype(np.int64), (last - first + 1).astype(np.int64) * any_


def covering_bands(case: Case, w: np.ndarray) -> np.ndarray:
    """f_bands [3, 2, 2]: per clip one band that covers the WHOLE support of a (different, non-empty) mel column, and one that
    runs to the last bin n_fft / 2 inclusive."""
    first, length = band_support(w)
    cols = np.flatnonzero(length > 0)
    picks = cols[np.linspace(0, len(cols) - 1, BATCH + 2).astype(int)[1:-1]] if len(cols) > 2 else np.repeat(cols[:1], BATCH)
    fb = np.zeros((BATCH, 2, 2), np.int32)
    for i, m in enumerate(picks):
        fb[i, 0] = (first[m], length[m])
        fb[i, 1] = (case.n_bins - 6 - i, 6 + i)
    return fb


def covered_columns(w: np.ndarray, f_bands_clip: np.ndarray) -> np.ndarray:
    """Non-empty columns of W whose every non-zero bin lies inside one of the clip's frequency bands: their mel rows are 0."""
    masked = np.zeros(w.shape[0], bool)
    for off, size in f_bands_clip:
        masked[off:off + size] = True
    nz = w != 0
    return np.flatnonzero(~(nz & ~masked[:, None]).any(axis=0) & nz.any(axis=0))


def mel_tolerance_w(wav, n_fft: int, hop: int, w: np.ndarray, t_bands=None, f_bands=None, rel: float = R.MEL_REL_TOL,
                    ulps: float = R.MEL_NOISE_ULPS):
    """(ref, tol) of oracle.frontend_ref.mel_tolerance - the fp64 mel [B, M, T, C] of wav [B, C, L] and the element-wise bound
        |mel - ref| <= rel |ref| + ulps eps_fp32 xrms[b, t, c] sum_k W[k, m]
    - with the float32 weight matrix W [n_fft / 2 + 1, M] given.  xrms: rms of the frame's unmasked fp64 magnitude spectrum; a
    frame inside a time band has tol = 0 (exact zeros), and so has every element of an all-zero column of W."""
    wav64 = np.asarray(wav, np.float64)
    frames = R.frame_signal(wav64, n_fft, hop) * R.hann_periodic(n_fft, np.float64)
    mag = np.abs(np.fft.rfft(frames, n=n_fft, axis=-1))                      # [B, C, T, F]
    xrms = np.sqrt(np.mean(mag * mag, axis=-1))                              # [B, C, T]
    for i in range(wav64.shape[0]):
        if t_bands is not None:
            for off, size in np.asarray(t_bands[i]):
                mag[i, :, off:off + size, :] = 0
                xrms[i, :, off:off + size] = 0
        if f_bands is not None:
            for off, size in np.asarray(f_bands[i]):
                mag[i, :, :, off:off + size] = 0
    w64 = np.asarray(w, np.float32).astype(np.float64)
    ref = np.einsum("bctf,fm->bmtc", mag, w64, optimize=True)
    eps = float(np.finfo(np.float32).eps)
    tol = rel * np.abs(ref) + ulps * eps * w64.sum(axis=0)[None, :, None, None] * np.moveaxis(xrms, 1, -1)[:, None, :, :]
    return ref, tol


def ordinary_share(ref: np.ndarray, tol: np.ndarray, w: np.ndarray, rel: float = R.MEL_REL_TOL) -> float:
    """Fraction of the elements of the columns that carry a weight on which the rule's relative term is at least its
    noise-floor term (`R.mel_strict_rel_err`'s ordinary elements): there the literal 1e-5 relative error is asserted."""
    cols = np.flatnonzero((np.asarray(w) != 0).any(axis=0))
    r, t = np.abs(ref[:, cols]), tol[:, cols]
    ordinary = (rel * r >= t - rel * r) & (r != 0)
    return float(ordinary.mean())


def logmel_ref(ref64: np.ndarray) -> np.ndarray:
    """The oracle's min-max + log (per clip) on the fp64 mel rounded once to float32."""
    return R.log_on_mel(R.minmax(ref64.astype(np.float32)))
