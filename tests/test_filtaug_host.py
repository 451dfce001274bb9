"""FilterAugment without a GPU: the float64 definition of the gain curve, the host draw, the run-name token, and the argument
checks of the three new entry points (all of which happen before any HIP call)."""
import ctypes as C

import numpy as np
import pytest

from challenge_amd import _native as N
from challenge_amd import data_utils as DU
from challenge_amd import transforms as T


def test_gains_step_by_hand():
    g = T.filter_augment_gains([0, 6, 13, 20], [-6.0, 0.0, 3.0], 20, "step")
    assert g.dtype == np.float32 and g.shape == (20,)
    want = np.concatenate([np.full(6, 10 ** (-6 / 20)), np.full(7, 1.0), np.full(7, 10 ** (3 / 20))]).astype(np.float32)
    assert np.array_equal(g, want)
    assert g[0] == np.float32(0.5011872336272722) and g[19] == np.float32(1.4125375446227544)   # magnitudes: 10^(dB / 20)


def test_gains_linear_by_hand():
    g = T.filter_augment_gains([0, 6, 13, 20], [-6.0, 0.0, 3.0, -3.0], 20, "linear")
    db = np.empty(20)
    for m in range(6):
        db[m] = -6.0 + 6.0 * m / 6
    for m in range(6, 13):
        db[m] = 0.0 + 3.0 * (m - 6) / 7
    for m in range(13, 20):
        db[m] = 3.0 - 6.0 * (m - 13) / 7
    assert np.array_equal(g, (10.0 ** (db / 20.0)).astype(np.float32))
    assert g[0] == np.float32(10 ** -0.3) and g[6] == 1.0 and g[3] == np.float32(10 ** (-3 / 20))   # row 3: half way up band 0
    assert g[13] == np.float32(10 ** (3 / 20))


@pytest.mark.parametrize("kind", ["step", "linear"])
def test_constant_and_zero_db(kind):
    n = 3 if kind == "step" else 4
    g = T.filter_augment_gains([0, 7, 12, 20], [2.5] * n, 20, kind)
    assert np.all(g == g[0]) and g[0] == np.float32(10 ** (2.5 / 20))
    assert np.all(T.filter_augment_gains([0, 7, 12, 20], [0.0] * n, 20, kind) == 1.0)


@pytest.mark.parametrize("bounds", [[0, 6, 6, 20], [0, 9, 6, 20], [0, 6, 13, 19], [1, 6, 13, 20], [0, 6, 13, 21], [20]])
def test_bad_bounds_raise(bounds):
    with pytest.raises(ValueError):
        T.filter_augment_gains(bounds, [0.0] * max(len(bounds) - 1, 1), 20, "step")


def test_bad_db_count_and_kind_raise():
    with pytest.raises(ValueError):
        T.filter_augment_gains([0, 6, 13, 20], [0.0] * 4, 20, "step")
    with pytest.raises(ValueError):
        T.filter_augment_gains([0, 6, 13, 20], [0.0] * 3, 20, "linear")
    with pytest.raises(ValueError):
        T.filter_augment_gains([0, 6, 13, 20], [0.0] * 3, 20, "cubic")


@pytest.mark.parametrize("kind", ["step", "linear"])
def test_host_draw_ranges_and_reproducibility(kind):
    bounds, db, n = T.filter_augment_draw(np.random.default_rng(5), 500, 64, kind)
    assert bounds.shape == db.shape == (500, 7) and bounds.dtype == np.int32 and db.dtype == np.float32 and n.shape == (500,)
    assert n.min() >= 3 and n.max() <= 6 and set(n.tolist()) == {3, 4, 5, 6}
    for b in range(500):
        k = int(n[b])
        assert bounds[b, 0] == 0 and bounds[b, k] == 64 and np.all(bounds[b, k:] == 64)
        assert np.all(np.diff(bounds[b, :k + 1]) >= 6)
        n_db = k if kind == "step" else k + 1
        assert np.all(db[b, :n_db] >= -6.0) and np.all(db[b, :n_db] < 6.0) and np.all(db[b, n_db:] == 0)
    again = T.filter_augment_draw(np.random.default_rng(5), 500, 64, kind)
    assert all(np.array_equal(a, b) for a, b in zip((bounds, db, n), again))
    other = T.filter_augment_draw(np.random.default_rng(6), 500, 64, kind)
    assert not np.array_equal(bounds, other[0])
    g = T.filter_augment_gain_batch(bounds, db, n, 64, kind)
    assert g.shape == (500, 64) and g.min() >= np.float32(10 ** -0.3) and g.max() < np.float32(10 ** 0.3) * (1 + 1e-6)


def test_host_draw_covers_every_cut_position_and_band_count():
    bounds, _, n = T.filter_augment_draw(np.random.default_rng(11), 20000, 64)
    seen = set()
    for b in range(20000):
        seen.update(bounds[b, 1:int(n[b])].tolist())
    # an interior boundary sits at least min_bw rows from either end: 6 .. 58
    assert seen == set(range(6, 59)), sorted(set(range(6, 59)) - seen)
    se = np.sqrt((4 ** 2 - 1) / 12.0 / 20000)          # U{3..6}: variance (k^2 - 1) / 12, k = 4
    assert abs(n.mean() - 4.5) <= 4 * se, (n.mean(), se)


def test_host_draw_refuses_too_few_mel_rows():
    with pytest.raises(ValueError):
        T.filter_augment_draw(np.random.default_rng(0), 4, 35)
    T.filter_augment_draw(np.random.default_rng(0), 4, 36)


def test_token_parsing():
    assert DU.run_tokens("run_filtaug").filtaug == "step"
    assert DU.run_tokens("run_filter").filtaug is None and DU.run_tokens("run_filter").filter is True
    assert DU.run_tokens("").filtaug is None
    assert DU.run_tokens("run_filtaug_linear_pcen").filtaug == "linear"
    assert DU.run_tokens("run_filtaug_linear").filtaug == "linear" and DU.run_tokens("run_filtaug_linear").filter is False
    assert "filter" not in "run_filtaug_linear"      # the reference's stft_filter token is not triggered by it


def test_make_dataset_refuses_the_token():
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get(['--name', 'run_filtaug', '--synthetic'])
    with pytest.raises(ValueError, match="filtaug"):
        S.make_dataset(cfg, training=True)


def _draw(batch=4, n_mel=64, kind=0, lo=3, hi=6, bw=6, db_lo=-6.0, db_hi=6.0, ptr=0x1000):
    return N.lib().iris_filter_draw(batch, n_mel, kind, lo, hi, bw, db_lo, db_hi, 1, ptr, ptr, ptr, ptr, None)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """No GPU here: a call that got as far as a HIP call would not return IRIS_E_INVALID (-1)."""
    lib = N.lib()
    assert _draw(batch=-1) == -1
    assert _draw(n_mel=35) == -1                       # n_mel < n_band_hi * min_bw
    assert _draw(lo=5, hi=4) == -1
    assert _draw(db_lo=1.0, db_hi=-1.0) == -1
    assert _draw(ptr=None) == -1                       # NULL outputs with batch > 0
    assert _draw(kind=2) == -1 and _draw(lo=0) == -1 and _draw(hi=33, n_mel=400) == -1
    assert b"iris_filter_draw" in lib.iris_last_error()
    assert _draw(batch=0, ptr=None) == 0               # nothing to do, nothing launched
    fake = C.c_void_p(0x1000)                          # never dereferenced: the checks come first
    assert lib.iris_wav_to_logmel_gain(fake, fake, fake, 2, 4000, 0, None, 0, None, 0, None, None) == -1
    assert b"mel_gain" in lib.iris_last_error()
    assert lib.iris_magmel_gain(fake, fake, fake, 2, 10, 0, None, 0, None, 0, None, None) == -1
    assert b"mel_gain" in lib.iris_last_error()
    assert lib.iris_wav_to_logmel_gain(None, fake, fake, 2, 4000, 0, None, 0, None, 0, fake, None) == -1
    assert lib.iris_magmel_gain(None, fake, fake, 2, 10, 0, None, 0, None, 0, fake, None) == -1
    assert lib.iris_magmel_gain(fake, fake, fake, -2, 10, 0, None, 0, None, 0, fake, None) == -1
