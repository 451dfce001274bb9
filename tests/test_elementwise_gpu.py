"""iris_normalize, iris_minmax_log and iris_complex_to_magphase / iris_magphase_to_complex (csrc/k_elementwise.h) against the float64
references and the rules of tests/elementwise_ref.py, through the C ABI on guarded buffers (two bands of 4096 words of the NaN
pattern 0x7FE5A5A5 around every tensor the kernels write).

Shapes are the ones at which the kernels change path: normalize rows of 1, 4095, 4096, 4097 and 3 * 4096 + 5 elements (one partial, the
chunk boundary, a ragged tail); min-max rows of 256 * 4096 and 256 * 4096 + 5 (256 and 257 partials: the per-wave fold and the block
fold), aligned, ragged and with the base pointer 4 bytes off a 16-byte boundary (the scalar path with row_len % 4 == 0), every
flag pair, a constant row, a row with one NaN; magnitude / phase with n_outer * C just above the capped grid's 8192 * 256 threads
(the grid-stride loop takes a second trip), C in {1, 2, 3}, the signed-zero and +-pi edges of atan2, phases up to 4e5 rad.

Pinned behaviour: an all-zero row normalises to NaN (0 / 0), as oracle.frontend_ref.normalize; a NaN in a min-max row is dropped
by fminf / fmaxf (NumPy's min would return NaN): every other element is bit for bit what it is without the NaN and the NaN
stays NaN, in iris_minmax_log and in the fused epilogue of wav_to_logmel alike."""
import ctypes as C

import numpy as np
import pytest
import torch

import elementwise_ref as E
from test_conv_gpu import Guarded

pytestmark = pytest.mark.gpu
F64 = np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _N():
    from challenge_amd import _native
    return _native


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _filled(dev, a, offset=0):
    """A guarded buffer holding `a` from word `offset` on (the words before it zeroed); returns (guard, data pointer)."""
    g = Guarded(dev, a.size + offset)
    if offset:
        g.t[:offset] = 0
    g.t[offset:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return g, g.ptr() + 4 * offset


def run_normalize(dev, x):
    N = _N()
    n_rows, row_len = x.shape
    src, sp = _filled(dev, x)
    dst = Guarded(dev, x.size)
    n_ws = int(N.lib().iris_normalize_workspace(n_rows, row_len))
    ws = Guarded(dev, n_ws)
    with torch.cuda.device(dev):
        N.check(N.lib().iris_normalize(sp, dst.ptr(), n_rows, row_len, ws.ptr(), n_ws, _stream(dev)), "iris_normalize")
    ws.check("normalize workspace")
    assert torch.equal(src.t.cpu(), torch.from_numpy(x.reshape(-1)))          # the input is read, never written
    return dst.check(f"iris_normalize {x.shape}").reshape(x.shape)


@pytest.mark.parametrize("row_len", E.NORMALIZE_ROW_LENS)
def test_normalize_meets_the_rule(dev, row_len):
    x = E.normalize_rows(row_len)
    out = run_normalize(dev, x)
    ratio = E.rel_ratio(out, E.normalize_ref(x))
    print(f"normalize row_len {row_len}: worst |d| / (u |ref|) = {ratio:.3f} (K = {E.K_NORMALIZE}, yardstick {E.YARD_NORMALIZE})")
    assert ratio <= E.K_NORMALIZE


def test_normalize_per_clip_over_all_channels_and_zero_row(dev):
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 2, 4097)) * np.array([1e-3, 1.0, 30.0])[:, None, None] * np.array([1.0, 5.0])[None, :, None]).astype(np.float32)
    out = FE.normalize(torch.from_numpy(x).to(dev)).cpu().numpy()
    ref = E.normalize_ref(x.reshape(3, -1)).reshape(x.shape)       # one rms per clip, both channels jointly
    assert E.rel_ratio(out, ref) <= E.K_NORMALIZE
    per_channel = E.normalize_ref(x.reshape(6, -1)).reshape(x.shape)
    assert E.rel_ratio(out, per_channel) > 1e3                       # (and not per channel)
    z = np.zeros((2, 4097), np.float32)
    z[1] = x[1, 0]
    got = run_normalize(dev, z)
    assert np.isnan(got[0]).all(), "an all-zero row is 0 / 0: NaN, as the oracle's normalize"
    assert E.rel_ratio(got[1:], E.normalize_ref(z[1:])) <= E.K_NORMALIZE


def run_minmax_log(dev, x, do_minmax, do_log, offset=0):
    """In place on a guarded copy of x [R, n] whose first element sits `offset` words behind a 16-byte boundary."""
    N = _N()
    n_rows, row_len = x.shape
    g, ptr = _filled(dev, x, offset)
    assert ptr % 16 == 4 * offset
    n_ws = int(N.lib().iris_minmax_log_workspace(n_rows, row_len))
    ws = Guarded(dev, n_ws)
    with torch.cuda.device(dev):
        N.check(N.lib().iris_minmax_log(ptr, n_rows, row_len, int(do_minmax), int(do_log), E.EPS, E.EPS, ws.ptr(), n_ws, _stream(dev)),
                "iris_minmax_log")
    ws.check("min-max workspace", all_written=bool(do_minmax))
    out = g.check(f"iris_minmax_log {x.shape} +{offset}", all_written=False)
    assert np.all(out[:offset] == 0)
    return out[offset:].reshape(x.shape)


_MM = {}


def _minmax_case(row_len):
    if row_len not in _MM:
        x = E.minmax_rows(row_len)
        _MM[row_len] = (x, E.minmax_ref(x))
    return _MM[row_len]


@pytest.mark.parametrize("row_len,offset", [(E.MINMAX_ROW_LENS[0], 0), (E.MINMAX_ROW_LENS[1], 0), (E.MINMAX_ROW_LENS[0], 1), (4096 * 3 + 2, 0)])
def test_minmax_log_every_flag_pair(dev, row_len, offset):
    N = _N()
    x, ref = _minmax_case(row_len)
    n_part = int(N.lib().iris_minmax_log_workspace(1, row_len)) // 2
    assert n_part == (row_len + 4095) // 4096
    # (0, 0): untouched
    assert np.array_equal(run_minmax_log(dev, x, 0, 0, offset), x)
    # (1, 0): the [0, 1] value
    v = run_minmax_log(dev, x, 1, 0, offset)
    worst = float(np.abs(v.astype(F64) - ref).max() / E.U)
    print(f"min-max row_len {row_len} (+{offset} words, {n_part} partials): worst |d| / u = {worst:.3f} (K = {E.K_MINMAX})")
    assert worst <= E.K_MINMAX
    for r in range(x.shape[0]):
        assert np.all(v[r][x[r] == x[r].min()] == 0), "the row's minimum must map to exactly 0"
        top = v[r][x[r] == x[r].max()]
        assert np.all(np.abs(top.astype(F64) - 1.0) <= 2.0 ** -23), "the row's maximum must be within one ulp of 1"
    # (0, 1): ln(x + eps) of values in [0, 1] at the stated bound of the hardware log
    unit = np.ascontiguousarray(v)
    lg = run_minmax_log(dev, unit, 0, 1, offset)
    d = float(np.abs(lg.astype(F64) - E.log_ref(unit)).max())
    print(f"log row_len {row_len}: worst |d ln| = {d:.3e} (bound {E.LOG_ABS})")
    assert d <= E.LOG_ABS
    # (1, 1): both
    both = run_minmax_log(dev, x, 1, 1, offset)
    bound = E.K_MINMAX * E.U + E.LOG_ABS * (1 + E.LOG_ABS) * (ref + E.EPS)
    assert np.all(np.abs(np.exp(both.astype(F64)) - (ref + E.EPS)) <= bound)


def test_minmax_constant_row_and_one_nan(dev):
    """A constant row takes the eps_div path: (v - mn) / 1e-8 = 0 everywhere.  A row with one NaN: fminf / fmaxf drop it, the other
    elements are bitwise what they are when the NaN is replaced by a value inside the row's range, and the NaN stays NaN."""
    n = 4096 * 2 + 3
    const = np.full((2, n), 7.0, np.float32)
    assert np.all(run_minmax_log(dev, const, 1, 0) == 0)
    assert np.all(run_minmax_log(dev, const, 1, 1) == run_minmax_log(dev, np.zeros((2, n), np.float32), 0, 1))
    x = E.minmax_rows(n)
    inside = x.copy()
    inside[1, 4100] = np.float32(0.5) * (x[1].min() + x[1].max())
    bad = x.copy()
    bad[1, 4100] = np.nan
    for flags in ((1, 0), (1, 1)):
        want, got = run_minmax_log(dev, inside, *flags), run_minmax_log(dev, bad, *flags)
        assert np.isnan(got[1, 4100]) and np.isnan(got).sum() == 1
        keep = np.ones(x.shape, bool)
        keep[1, 4100] = False
        assert np.array_equal(got[keep].view(np.int32), want[keep].view(np.int32))


def test_nan_in_a_clip_fused_epilogue_and_entry_point_agree(dev):
    """The same values through both forms of the step: the fused epilogue of wav_to_logmel and iris_minmax_log on the raw mel of
    the same call.  A NaN sample makes whole frames of the mel NaN; both forms drop them from the clip's min / max, leave them
    NaN and agree bit for bit on every other element."""
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(9)
    wav = (rng.standard_normal((3, 1, 8000)) * 0.1).astype(np.float32)
    wav[1, 0, 3000] = np.nan
    plan = FE.FrontendPlan(512, 128, 40, 16000, 1, 3, 8000, dev)
    x = torch.from_numpy(wav).to(dev)
    raw = plan.wav_to_logmel(x, minmax=False, log=False)
    fused = plan.wav_to_logmel(x)
    unfused = FE.minmax_log(raw)
    nan = torch.isnan(raw)
    assert bool(nan[1].any()) and not bool(nan[0].any()) and not bool(nan[2].any()) and not bool(nan[1].all())
    assert torch.equal(torch.isnan(fused), nan) and torch.equal(torch.isnan(unfused), nan)
    assert torch.equal(fused[~nan].view(torch.int32), unfused[~nan].view(torch.int32))
    finite = raw[1][~nan[1]]
    ref = torch.log((raw[1].double() - finite.min().double()) / (finite.max().double() - finite.min().double()) + 1e-8)
    assert float((torch.exp(fused[1].double()) - torch.exp(ref))[~nan[1]].abs().max()) <= 5e-6     # min / max over the finite values


def run_pair(dev, fn_name, a, c):
    """iris_complex_to_magphase / iris_magphase_to_complex on a [n_outer, 2C] -> NumPy [n_outer, 2C]."""
    N = _N()
    src, sp = _filled(dev, a)
    dst = Guarded(dev, a.size)
    with torch.cuda.device(dev):
        N.check(getattr(N.lib(), fn_name)(sp, dst.ptr(), a.shape[0], c, _stream(dev)), fn_name)
    return dst.check(f"{fn_name} {a.shape}").reshape(a.shape)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_magphase_and_phasor_above_the_grid_cap(dev, c):
    n = E.n_outer_above_cap(c)
    assert n * c > E.GRID_CAP
    z = E.complex_rows(n, c)
    out = run_pair(dev, "iris_complex_to_magphase", z, c)
    mag, ph = E.magphase_ref(z)
    wm = float((np.abs(out[:, :c] - mag) / (E.U * mag)).max())
    wp = float(np.abs(out[:, c:] - ph).max() / (E.U * np.pi))
    mp = E.magphase_rows(n, c)
    pc = run_pair(dev, "iris_magphase_to_complex", mp, c)
    re, im = E.phasor_ref(mp)
    m = np.abs(mp[:, :c].astype(F64))
    err = np.maximum(np.abs(pc[:, :c] - re), np.abs(pc[:, c:] - im))
    assert np.all(err[m == 0] == 0)
    ws = float((err[m > 0] / (E.U * m[m > 0])).max())
    # the round trip of z
    rt = run_pair(dev, "iris_magphase_to_complex", out, c)
    zz = np.hypot(z[:, :c].astype(F64), z[:, c:].astype(F64))
    e2 = np.maximum(np.abs(rt[:, :c].astype(F64) - z[:, :c]), np.abs(rt[:, c:].astype(F64) - z[:, c:]))
    wr = float((e2 / (E.U * zz)).max())
    print(f"C {c} n_outer {n}: magnitude {wm:.3f} (K {E.K_MAG}), phase {wp:.3f} (K {E.K_PHASE}), phasor {ws:.3f} (K {E.K_PHASOR}), "
          f"round trip {wr:.3f} (bound {E.K_MAG + np.pi * E.K_PHASE + E.K_PHASOR:.1f})")
    assert wm <= E.K_MAG and wp <= E.K_PHASE and ws <= E.K_PHASOR
    assert wr <= E.K_MAG + np.pi * E.K_PHASE + E.K_PHASOR


def test_phase_edges_as_numpy(dev):
    e = E.phase_edges()
    out = run_pair(dev, "iris_complex_to_magphase", e, 1)
    mag, ph = np.abs(e).max(axis=1), np.arctan2(e[:, 1], e[:, 0])
    assert np.array_equal(out[:, 0], mag)
    assert np.array_equal(np.signbit(out[:, 1]), np.signbit(ph)), (out[:, 1], ph)
    zero = ph == 0
    assert np.all(out[zero, 1] == 0)                                              # signed zeros, exactly
    assert np.all(np.abs(out[~zero, 1].astype(F64) - ph[~zero]) <= 2.0 ** -22 + 1e-12), (out[:, 1], ph)   # +-pi, +-pi/2 within one ulp
