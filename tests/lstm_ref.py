"""Reference forms of the BiLSTM recurrence kernels (k_bilstm128_fwd / k_bilstm128_bwd, csrc/k_lstm.h), a helper beside the tests.

The kernel's boundary is the recurrent half of Bidirectional(LSTM(128)) with the input GEMM already done:

    forward : gx [B, T, 2, 512] (= x_t W_ih^T + b_ih + b_hh per direction, gate rows i, f, g, o), w_hh [2, 512, 128]
              -> out [B, T, 256] = (h of direction 0, h of direction 1), act [B, T, 2, 5, 128] = (i, f, g, o, c)
                 pre = gx[b, t, d] + W_hh[d] h_prev;  i, f, o = sigmoid, g = tanh;  c = f c_prev + i g;  h = o tanh(c)
                 h_0 = c_0 = 0; direction 0 walks t = 0 .. T-1, direction 1 walks t = T-1 .. 0.
    backward: dout [B, T, 256], act, w_hh -> dgx [B, T, 2, 512], the gradient of the pre-activations.

`bilstm_ref` / `bilstm_bwd_ref` : the definition in float64.  The backward takes `act` as DATA, so it can be fed the kernel's own
                                  float32 activations - that isolates the backward arithmetic from the forward's rounding.
`dw_hh_ref`                     : dW_hh[d] = sum_{b, t} dgx[b, t, d, :]^T h_prev[b, t, :], h_prev = out shifted by one step of d.
`yardstick32` / `yardstick32_bwd`: the same recurrences stepped in NumPy float32 with the library exp / tanh and a plain dot
                                  product (products rounded, then added in ascending k).  Neither the kernel's exp2 / rcp gate
                                  formulas nor its two-accumulator order appear here: the constants of the error rules come from
                                  this yardstick's distance to float64, never from the kernel's.

Error rules (u = 2^-24), asserted for the kernels in tests/test_lstm_gpu.py:

    gates   : |sigmoid32(x) - sigmoid(x)| <= K_G u,  |tanh32(x) - tanh(x)| <= K_G u            (values in [0, 1] / [-1, 1])
    forward : |out - ref| <= K_F u;  the same for the planes i, f, g, o;  |c - c_ref| <= K_F u max(1, |c_ref|)
              (no growth term in T: the yardstick shows none at contractive weights, see tests/test_lstm_host.py)
    backward: |dgx - ref| <= K_B u P[b, d],  P = the peak of |ref| over batch row b and direction d
              (a row's gradient never mixes with another row's or with the other direction's)

Each K = the smallest power of two at or above four times the yardstick's worst ratio over SWEEP (`derive_k`); the host test
re-runs the sweep and asserts that the committed values are what this recipe yields.

The contractive regime.  All parity inputs keep |w_hh| <= 0.3 (torch's default init for 128 units is U(-0.088, 0.088); the older
tests use 0.25 and 0.3).  At w_hh ~ U(-1, 1) the recurrence is chaotic: two correct float32 LSTMs - this yardstick and an
emulation of the kernel's formulas - both sit 700-800 u from float64 there, so no bound separates an error from conditioning."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
H = 128

# the committed constants (derived in tests/test_lstm_host.py; see YARDSTICK_WORST there)
K_G = 8
K_F = 128
K_B = 128

# forward and backward shapes of tests/test_lstm_gpu.py
FWD_SHAPES = [(1, 1), (2, 1), (3, 5), (7, 40), (64, 16), (2, 257)]
BWD_SHAPES = [(1, 1), (3, 1), (2, 2), (5, 7), (2, 33), (64, 16)]
SHAPES = FWD_SHAPES + [s for s in BWD_SHAPES if s not in FWD_SHAPES]
SCALES = [1.6, 50.0, 2e-3]
W_RANGES = [0.25, 0.3]
SEEDS = [0, 1, 2, 3]
SWEEP = [(shape, scale, wr, seed) for shape in SHAPES for scale in SCALES for wr in W_RANGES for seed in SEEDS]


def gate_grid():
    """The finite arguments of the gate-function sweep, float32: +-0, subnormals, +-1e-6 .. +-1e-2, a dense grid on [-20, 20],
    the range where exp2 leaves float32 (+-44, 87, 89, 127) and huge values.  (+-inf and NaN are added by the tests.)"""
    small = [1e-45, 1e-41, 1.1754942e-38, 1e-30, 1e-6, 2e-6, 5e-6, 1e-5, 3e-5, 1e-4, 2.7e-4, 1e-3, 2.7e-3, 5e-3, 1e-2]
    dense = np.linspace(-20.0, 20.0, 4001)
    fine = np.geomspace(1e-6, 1e-2, 161)
    edge = [44.0, 87.0, 88.0, 88.8, 89.0, 103.0, 104.0, 127.0, 128.0, 150.0, 1e4, 1e30, 3e38]
    pos = np.concatenate([small, fine, edge])
    return np.concatenate([[0.0, -0.0], pos, -pos, dense]).astype(F32)


def derive_k(worst):
    """The smallest power of two at or above four times the yardstick's worst ratio."""
    return 2.0 ** math.ceil(math.log2(4.0 * worst))


def make_case(shape, scale, wr, seed):
    """(gx [B, T, 2, 512], w_hh [2, 512, 128], dout [B, T, 256]) float32: gx ~ scale N(0, 1), w_hh ~ U(-wr, wr), dout ~ N(0, 1)."""
    b, t = shape
    rng = np.random.default_rng([seed, b, t, int(round(wr * 100)), int(round(scale * 1000))])
    gx = (scale * rng.standard_normal((b, t, 2, 4 * H))).astype(F32)
    w_hh = rng.uniform(-wr, wr, (2, 4 * H, H)).astype(F32)
    dout = rng.standard_normal((b, t, 2 * H)).astype(F32)
    return gx, w_hh, dout


# ---------------------------------------------------------------------------
# float64: the definition
# ---------------------------------------------------------------------------
def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def tanh64(x):
    return np.tanh(np.asarray(x, np.float64))


def _steps(t, d):
    """Time indices in the order direction d walks them."""
    return range(t) if d == 0 else range(t - 1, -1, -1)


def bilstm_ref(gx, w_hh):
    """(out [B, T, 256], act [B, T, 2, 5, 128]) float64 by the definition."""
    gx, w = np.asarray(gx, np.float64), np.asarray(w_hh, np.float64)
    b, t = gx.shape[:2]
    assert gx.shape == (b, t, 2, 4 * H) and w.shape == (2, 4 * H, H)
    out, act = np.zeros((b, t, 2 * H)), np.zeros((b, t, 2, 5, H))
    for d in range(2):
        h, c = np.zeros((b, H)), np.zeros((b, H))
        for s in _steps(t, d):
            pre = gx[:, s, d] + h @ w[d].T
            gi, gf, go = sigmoid64(pre[:, :H]), sigmoid64(pre[:, H:2 * H]), sigmoid64(pre[:, 3 * H:])
            gg = tanh64(pre[:, 2 * H:3 * H])
            c = gf * c + gi * gg
            h = go * np.tanh(c)
            out[:, s, d * H:(d + 1) * H] = h
            for q, v in enumerate((gi, gf, gg, go, c)):
                act[:, s, d, q] = v
    return out, act


def bilstm_bwd_ref(dout, act, w_hh):
    """dgx [B, T, 2, 512] float64 from dout [B, T, 256], the activations `act` (taken as data) and w_hh."""
    dout, act, w = np.asarray(dout, np.float64), np.asarray(act, np.float64), np.asarray(w_hh, np.float64)
    b, t = dout.shape[:2]
    assert dout.shape == (b, t, 2 * H) and act.shape == (b, t, 2, 5, H) and w.shape == (2, 4 * H, H)
    dgx = np.zeros((b, t, 2, 4 * H))
    for d in range(2):
        order = list(_steps(t, d))
        dh_rec, dc_rec = np.zeros((b, H)), np.zeros((b, H))
        for n in range(t - 1, -1, -1):          # the forward order, walked backwards
            s = order[n]
            gi, gf, gg, go, ct = (act[:, s, d, q] for q in range(5))
            cprev = act[:, order[n - 1], d, 4] if n > 0 else np.zeros((b, H))
            dh = dout[:, s, d * H:(d + 1) * H] + dh_rec
            tc = np.tanh(ct)
            dc = dh * go * (1.0 - tc * tc) + dc_rec
            dp = np.concatenate([dc * gg * gi * (1.0 - gi), dc * cprev * gf * (1.0 - gf), dc * gi * (1.0 - gg * gg),
                                 dh * tc * go * (1.0 - go)], axis=1)
            dgx[:, s, d] = dp
            dc_rec = dc * gf
            dh_rec = dp @ w[d]
    return dgx


def h_prev(out):
    """[2, B, T, 128]: the hidden state each step of direction d started from = `out` shifted by one step of d, zeros first."""
    out = np.asarray(out)
    b, t = out.shape[:2]
    hp = np.zeros((2, b, t, H), out.dtype)
    hp[0, :, 1:] = out[:, :-1, :H]
    hp[1, :, :-1] = out[:, 1:, H:]
    return hp


def dw_hh_ref(dgx, out):
    """dW_hh [2, 512, 128] float64 from dgx [B, T, 2, 512] and out [B, T, 256]."""
    dgx, hp = np.asarray(dgx, np.float64), h_prev(np.asarray(out, np.float64))
    return np.stack([np.einsum("btj,btk->jk", dgx[:, :, d], hp[d]) for d in range(2)])


# ---------------------------------------------------------------------------
# float32: the yardstick (library exp / tanh, plain dot product)
# ---------------------------------------------------------------------------
def sigmoid32(x):
    """1 / (1 + exp(-x)), every operation rounded to float32."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x).astype(F32)).astype(F32)).astype(F32)


def tanh32(x):
    return np.tanh(np.asarray(x, F32)).astype(F32)


def _dot32(a, m):
    """a [B, K] . m [J, K]^T -> [B, J] in float32: every product rounded, then added in ascending k (np.cumsum adds in order)."""
    if a.shape[0] * m.size <= 1 << 19:
        prod = (a[:, None, :] * m[None, :, :]).astype(F32)
        return np.cumsum(prod, axis=2, dtype=F32)[:, :, -1]
    at, mt = np.ascontiguousarray(a.T), np.ascontiguousarray(m.T)   # the same sum, one k at a time (no [B, J, K] temporary)
    acc = np.zeros((a.shape[0], m.shape[0]), F32)
    for k in range(a.shape[1]):
        acc += at[k][:, None] * mt[k][None, :]
    return acc


def yardstick32(gx, w_hh):
    """(out, act) float32: `bilstm_ref` with every operation rounded to float32."""
    gx, w = np.asarray(gx, F32), np.asarray(w_hh, F32)
    b, t = gx.shape[:2]
    out, act = np.zeros((b, t, 2 * H), F32), np.zeros((b, t, 2, 5, H), F32)
    for d in range(2):
        h, c = np.zeros((b, H), F32), np.zeros((b, H), F32)
        for n, s in enumerate(_steps(t, d)):
            pre = gx[:, s, d] if n == 0 else (gx[:, s, d] + _dot32(h, w[d])).astype(F32)
            gi, gf, go = sigmoid32(pre[:, :H]), sigmoid32(pre[:, H:2 * H]), sigmoid32(pre[:, 3 * H:])
            gg = tanh32(pre[:, 2 * H:3 * H])
            c = ((gf * c).astype(F32) + (gi * gg).astype(F32)).astype(F32)
            h = (go * tanh32(c)).astype(F32)
            out[:, s, d * H:(d + 1) * H] = h
            for q, v in enumerate((gi, gf, gg, go, c)):
                act[:, s, d, q] = v
    return out, act


def yardstick32_bwd(dout, act, w_hh):
    """dgx float32: `bilstm_bwd_ref` with every operation rounded to float32."""
    dout, act, w = np.asarray(dout, F32), np.asarray(act, F32), np.asarray(w_hh, F32)
    b, t = dout.shape[:2]
    dgx = np.zeros((b, t, 2, 4 * H), F32)
    one = F32(1)
    for d in range(2):
        order = list(_steps(t, d))
        wt = np.ascontiguousarray(w[d].T)     # [128, 512]
        dh_rec, dc_rec = np.zeros((b, H), F32), np.zeros((b, H), F32)
        for n in range(t - 1, -1, -1):
            s = order[n]
            gi, gf, gg, go, ct = (act[:, s, d, q] for q in range(5))
            cprev = act[:, order[n - 1], d, 4] if n > 0 else np.zeros((b, H), F32)
            dh = (dout[:, s, d * H:(d + 1) * H] + dh_rec).astype(F32)
            tc = tanh32(ct)
            dc = (dh * go * (one - tc * tc) + dc_rec).astype(F32)
            dp = np.concatenate([dc * gg * gi * (one - gi), dc * cprev * gf * (one - gf), dc * gi * (one - gg * gg),
                                 dh * tc * go * (one - go)], axis=1).astype(F32)
            dgx[:, s, d] = dp
            dc_rec = (dc * gf).astype(F32)
            if n > 0:
                dh_rec = _dot32(dp, wt)
    return dgx


# ---------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------
def _ratio(got, ref, scale):
    """|got - ref| / (u scale) per element; where the reference is not finite the value must equal it (NaN for NaN)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), "a non-finite reference value must be reproduced"
    assert np.all(np.isfinite(got[fin])), "a finite reference value came out non-finite"
    r = np.zeros(ref.shape)
    r[fin] = np.abs(got[fin] - ref[fin]) / (U * np.broadcast_to(scale, ref.shape)[fin])
    return r


def gate_rule_ratio(got, ref):
    """|got - ref| / u for a gate function's values."""
    return _ratio(got, ref, 1.0)


def fwd_rule_ratio(out, act, out_ref, act_ref):
    """(ratio of out [B, T, 256], ratio of act [B, T, 2, 5, 128]): |. - ref| / u, the c plane over u max(1, |c_ref|)."""
    scale = np.ones(act_ref.shape)
    with np.errstate(invalid="ignore"):
        scale[:, :, :, 4] = np.maximum(1.0, np.nan_to_num(np.abs(act_ref[:, :, :, 4]), nan=1.0, posinf=1.0))
    return _ratio(out, out_ref, 1.0), _ratio(act, act_ref, scale)


def bwd_peaks(dgx_ref):
    """P [B, 1, 2, 1]: the peak of |ref| over each batch row and direction."""
    return np.abs(dgx_ref).max(axis=(1, 3), keepdims=True)


def bwd_rule_ratio(dgx, dgx_ref):
    """|dgx - ref| / (u P[b, d]); a row and direction whose reference is all zero must be exactly zero."""
    p = bwd_peaks(dgx_ref)
    zero = np.broadcast_to(p == 0, dgx_ref.shape)
    assert np.all(np.asarray(dgx)[zero] == 0), "a row / direction with an all-zero reference gradient must be exactly 0"
    return _ratio(dgx, dgx_ref, np.where(p > 0, p, 1.0))
