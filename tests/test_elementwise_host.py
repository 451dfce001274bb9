"""Host tests of tests/elementwise_ref.py (no GPU): every K of the elementwise rules is derived from a float32 NumPy yardstick
against the float64 reference, by the repository's recipe, over the inputs the GPU module uses (smaller where only the size
differs), and equals the value recorded in the helper."""
import numpy as np

import elementwise_ref as E
from oracle import frontend_ref as R


def _recorded(worst, yard, k, what):
    print(f"{what}: yardstick worst ratio {worst:.3f} -> K = {E.k_from(worst)}")
    assert E.k_from(worst) == k, (what, worst)
    assert abs(worst - yard) <= 0.1 * yard, (what, worst, yard)


def test_normalize_k_and_definition():
    worst = 0.0
    for n in E.NORMALIZE_ROW_LENS:
        x = E.normalize_rows(n)
        worst = max(worst, E.rel_ratio(E.normalize_yardstick(x), E.normalize_ref(x)))
        for i in range(x.shape[0]):     # the yardstick is the oracle's normalize, row by row
            assert np.array_equal(E.normalize_yardstick(x)[i], R.normalize(x[i]))
    _recorded(worst, E.YARD_NORMALIZE, E.K_NORMALIZE, "normalize")
    with np.errstate(all="ignore"):
        assert np.isnan(R.normalize(np.zeros(5, np.float32))).all()     # 0 / 0


def test_minmax_k_and_definition():
    worst = 0.0
    for n in (4096 * 3, 4096 * 3 + 5):
        x = E.minmax_rows(n)
        ref, y = E.minmax_ref(x), E.minmax_yardstick(x)
        worst = max(worst, float(np.abs(y - ref).max() / E.U))
        assert ref.min() == 0 and ref.max() == 1
    _recorded(worst, E.YARD_MINMAX, E.K_MINMAX, "min-max")
    assert np.all(E.minmax_ref(np.full((1, 9), 7.0, np.float32)) == 0)
    assert E.LOG_ABS == 2.4e-6


def test_magphase_and_phasor_k():
    wm = wp = ws = 0.0
    for c in (1, 2, 3):
        z = E.complex_rows(20000, c)
        (mag, ph), (ym, yp) = E.magphase_ref(z), E.magphase_yardstick(z)
        wm = max(wm, float((np.abs(ym - mag) / (E.U * mag)).max()))
        wp = max(wp, float(np.abs(yp - ph).max() / (E.U * np.pi)))
        mp = E.magphase_rows(20000, c)
        (re, im), (yr, yi) = E.phasor_ref(mp), E.phasor_yardstick(mp)
        m = np.abs(mp[:, :c].astype(np.float64))
        ws = max(ws, float((np.maximum(np.abs(yr - re), np.abs(yi - im))[m > 0] / (E.U * m[m > 0])).max()))
    _recorded(wm, E.YARD_MAG, E.K_MAG, "magnitude")
    _recorded(wp, E.YARD_PHASE, E.K_PHASE, "phase")
    _recorded(ws, E.YARD_PHASOR, E.K_PHASOR, "phasor")


def test_phase_edges_in_numpy():
    e = E.phase_edges()
    ph = np.arctan2(e[:, 1], e[:, 0])
    assert ph[0] == 0 and not np.signbit(ph[0]) and np.signbit(ph[2]) and ph[2] == 0          # atan2(+-0, +0) = +-0
    assert ph[1] == np.float32(np.pi) and ph[3] == -np.float32(np.pi)                          # atan2(+-0, -0) = +-pi
    assert ph[4] == np.float32(np.pi) and ph[5] == -np.float32(np.pi) and ph[6] == 0 and np.signbit(ph[7])
    assert E.n_outer_above_cap(3) * 3 > E.GRID_CAP
