"""Host tests of tests/frontend_grid_ref.py (no GPU): the helper's mel rule equals the oracle's on standard banks, and the case
table - a test input, not a copy of the plan's heuristic - is well formed and leaves the rule's relative term in charge."""
import numpy as np
import pytest

import frontend_grid_ref as G
from oracle import frontend_ref as R


@pytest.mark.parametrize("name", ["512-40mel", "256-65mel", "2048-80mel-full", "256-40mel-from0"])
@pytest.mark.parametrize("with_bands", [False, True])
def test_helper_rule_equals_oracle_rule(name, with_bands):
    """`mel_tolerance_w` with the standard bank's W == `R.mel_tolerance` of the same (n_mel, edges): reference and bound, bit
    for bit - default and full-band edges, empty columns, with and without SpecAugment bands."""
    case = G.BY_NAME[name]
    wav = G.make_wav(case)
    tb, fb = G.make_bands(case) if with_bands else (None, None)
    ref, tol = G.mel_tolerance_w(wav, case.n_fft, case.hop, G.weights(case), tb, fb)
    want_ref, want_tol = R.mel_tolerance(wav, case.n_fft, case.hop, case.n_mel, case.sample_rate, t_bands=tb, f_bands=fb,
                                         lower_edge_hertz=case.lower, upper_edge_hertz=case.upper)
    assert ref.shape == want_ref.shape == (G.BATCH, case.n_mel, 25, case.channels)
    assert np.array_equal(ref, want_ref) and np.array_equal(tol, want_tol)
    if with_bands:
        for i in range(G.BATCH):
            for off, size in tb[i]:
                assert np.all(tol[i, :, off:off + size] == 0) and np.all(ref[i, :, off:off + size] == 0)


def test_case_table_is_complete_and_well_formed():
    """Every one of the 22 (LOG2N, mel_mode, HI) triples is declared by a ledger case, every mel_mode sees 1, 2 and 3
    channels, and every shape has the stated sizes (batch 3, odd length, hop n_fft / 4, 25 frames)."""
    assert len(G.TRIPLES) == 22 and len(set(G.TRIPLES)) == 22
    assert {c.variant for c in G.GRID} == set(G.TRIPLES)
    assert all(c.variant in G.TRIPLES for c in G.EDGES)
    assert len({c.name for c in G.CASES}) == len(G.CASES)
    for mode in (0, 1, 2, 3):
        assert {c.channels for c in G.GRID if c.variant[1] == mode} == {1, 2, 3}, mode
    for c in G.CASES:
        assert c.n_fft == 1 << c.variant[0] and c.length % 2 == 1 and c.hop * 4 == c.n_fft and c.n_frames == 25
        wav = G.make_wav(c)
        assert wav.shape == (G.BATCH, c.channels, c.length) and wav.dtype == np.float32
        rms = np.sqrt((wav.astype(np.float64) ** 2).mean(axis=(1, 2)))
        assert len(set(np.round(rms, 3))) == G.BATCH, "the clips must sit at different levels"
        w = G.weights(c)
        assert w.shape == (c.n_bins, c.n_mel) and w.dtype == np.float32 and w.min() >= 0
    names = {G.kernel_name(v, b) for v in G.TRIPLES for b in (False, True)}
    assert len(names) == 44 and "k_wav_to_mel<10,0,false,true,1,1>" in names


def test_empty_columns_and_band_edges_of_the_table():
    """The properties the table is chosen for, from W alone: the stated numbers of all-zero columns, one band of 63 bins, the
    lowest band at bin 1 with the lower edge at 0 Hz, and bands that reach the upper half of the spectrum exactly where HI is
    declared."""
    empty = {c.name: int((G.band_support(G.weights(c))[1] == 0).sum()) for c in G.CASES}
    assert empty["256-65mel"] == 3 and empty["512-128mel"] == 5 and empty["2048-800mel-full"] == 41 and empty["512-129mel"] == 5
    assert all(n == 0 for name, n in empty.items() if name not in ("256-65mel", "512-128mel", "2048-800mel-full", "512-129mel"))
    first, length = G.band_support(G.weights(G.BY_NAME["256-1mel"]))
    assert (int(first[0]), int(length[0])) == (1, 63)
    first, length = G.band_support(G.weights(G.BY_NAME["256-40mel-from0"]))
    assert int(first[0]) == 1
    # (the 20-bin register windows of the half-spectrum variant end at bin 64: bands whose 4-aligned start lies beyond 44 are clamped)
    assert int(((first & ~3) > 64 - 20).sum()) >= 1
    for c in G.CASES:
        first, length = G.band_support(G.weights(c))
        assert bool((first + length).max() > c.n_fft // 4) == c.variant[2], c.name


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_rule_is_decided_by_its_relative_term(case):
    """On the columns that carry a weight, at least 99 % of the reference's elements are ORDINARY - the 1e-5 relative term of
    the rule is at least its noise-floor term - for the input recipe of the grid (measured: >= 99.78 %).  The GPU test asserts
    the same share, so the noise floor cannot hide a wrong kernel."""
    w = G.weights(case)
    ref, tol = G.mel_tolerance_w(G.make_wav(case), case.n_fft, case.hop, w)
    share = G.ordinary_share(ref, tol, w)
    assert share >= 0.99, f"{case.name}: ordinary share {share:.4f}"
    empty = np.flatnonzero(G.band_support(w)[1] == 0)
    assert np.all(ref[:, empty] == 0) and np.all(tol[:, empty] == 0)


def test_covering_bands_cover_a_column_and_reach_the_last_bin():
    for name in ("512-40mel", "512-128mel", "2048-800mel-full"):
        case = G.BY_NAME[name]
        w = G.weights(case)
        fb = G.covering_bands(case, w)
        assert fb.shape == (G.BATCH, 2, 2)
        picked = set()
        for i in range(G.BATCH):
            cols = G.covered_columns(w, fb[i])
            assert len(cols) >= 1
            picked.update(cols.tolist())
            assert fb[i, 1, 0] + fb[i, 1, 1] == case.n_bins                 # runs to bin n_fft / 2 inclusive
            ref, _ = G.mel_tolerance_w(G.make_wav(case)[i:i + 1], case.n_fft, case.hop, w, f_bands=fb[i:i + 1])
            assert np.all(ref[0, cols] == 0) and np.any(ref[0] != 0)
        assert len(picked) >= G.BATCH                                       # a different column per clip
