"""Reference forms of the training-mode BatchNorm + ReLU (+ MaxPool 2x2) passes and of the first layer that recomputes its
convolution inside them (csrc/k_elementwise.h, csrc/k_conv0_bn.h), a helper beside the tests.  Everything is written out in NumPy,
no autograd inside; `dtype` = float64 is the definition, `dtype` = float32 the same lines with every operation rounded to
float32 (the yardstick: NumPy's own sums, no fused multiply-add, none of the kernels' coefficient forms).

    bn_relu            z [B, H, W, C] channels-last -> y (or the pooled p), save_mean, save_rstd, running_mean, running_var
                           mean, var (biased) over the B H W rows;  rstd = 1 / sqrt(var + eps);  y = max(gamma (z - mean) rstd + beta, 0)
                           running_mean <- (1 - m) running_mean + m (mean + conv_bias)     (the bias only moves the mean)
                           running_var  <- (1 - m) running_var  + m var M / (M - 1)        (factor 1 for a single row)
                           pool: max over 2x2 / stride-2 windows, ceil mode (edge windows have 2 or 1 elements)
    bn_relu_backward   dz = a g + b z + d,  a = gamma rstd,  b = -a rstd sum(g xhat) / M,  d = -a sum(g) / M - b mean
                           g = dy [pre > 0]; pooled: dp scattered to the window's FIRST maximum in (h, w) scan order, and only
                           where that maximum is > 0;  dgamma = sum g xhat,  dbeta = sum g
    conv0_bn_relu      z = 3x3 'same' convolution of x [B, CIN, H, W] with w [C, CIN, 3, 3], no bias, then bn_relu
    conv0_bn_relu_backward   also dW [C, CIN, 3, 3] and dx [B, CIN, H, W]

Inputs (`make_bn_case`, `make_conv0_case`) sit on a grid, so that every decision a kernel takes is at a known distance from its
threshold and no comparison needs an exclusion mask:

    z = k / 8, |k| <= 16 (per channel k is uniform on [-s, s], s one of 2, 3, 5, 16: narrow channels tie often);
    first layer: x = k / 4, |x| <= 2, w = k / 4, |w| <= 1.5, so z is a multiple of 1/16 - exact in float32 in any order;
    gamma in +-[0.5, 1.5], mixed signs; beta = -gamma rstd (z* - mean) rounded to float32, z* halfway between two grid points of
    the channel: pre = gamma rstd (z - z*), |pre| >= |gamma| rstd / 16 (/ 32 for the first layer);
    two window elements are bit-equal or a grid step apart;
    two channels have gamma = 0, beta = +0.25 / -0.25: all elements tie, y = relu(beta), dz = 0, dgamma != 0.

The generators assert these margins.  `make_bn_case` also asserts, for a pooled case, that at least 10 % of the windows with more
than one element tie at their maximum (`tie_shares`; windows whose maximum is 0 and the gamma = 0 channels count - in the tiny
cases they are most of it), and where a case has 1000 such windows or more, that at least 10 % tie at a POSITIVE maximum, where the
first-maximum rule alone decides who gets the gradient (17-22 % in the cases as generated).

Bounds of tests/test_bn_gpu.py (`bound`): the ceiling is what these passes carry elsewhere in the suite, now against float64 -
2e-5 max|ref| + 1e-6 for outputs and saved statistics, 5x that for gradients, 1e-6 absolute for the running statistics - and
under it, for the quantities in TIGHT, 4x the float32 yardstick's worst error over the case list (YARDSTICK, re-measured by
tests/test_bn_host.py; in the same units, max|ref| + 0.05, without the gradients' factor 5)."""
import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24

EPS, MOMENTUM = 1e-5, 0.1          # torch's defaults; the model's own values are one more case (MODEL_EPS, MODEL_MOMENTUM)
MODEL_EPS, MODEL_MOMENTUM = 1e-3, 0.01

# (b, h, w, c) of the generic passes, each without and with pooling
BN_SHAPES = [(1, 1, 2, 4), (1, 1, 1, 8), (1, 1, 3, 8), (2, 3, 1, 8), (2, 5, 7, 32), (3, 9, 7, 64), (3, 7, 49, 32), (2, 3, 11, 12),
             (1, 3, 11, 1024), (1, 3, 11, 1028), (1, 2, 3, 4096)] + [(2, 33, 65, c) for c in (64, 68, 128, 132, 256, 260)]
BN_CASES = [(s, pool) for s in BN_SHAPES for pool in (False, True)] + [((4, 210, 210, 12), False), ((4, 257, 259, 32), True)]
# (cin, cout, b, h, w) of the first layer
CONV0_CASES = ([(cin, cout, 2, 5, 9) for cin in (1, 2) for cout in (4, 8, 16, 32, 64, 128, 256)]
               + [(1, 8, 1, 1, 2), (2, 16, 2, 1, 33), (1, 16, 2, 7, 1), (2, 256, 1, 2, 9), (1, 8, 3, 1400, 3), (2, 32, 1, 2, 2048)])
OFFSET_CASES = [(1, 32, 2, 64, 128), (2, 32, 2, 64, 128)]

# the float32 yardstick's worst error over the case list, in units of max|ref| + ABS_SHARE per tensor (running statistics: absolute)
YARDSTICK = {"y": 2.0e-7, "mean": 5.5e-8, "rstd": 2.3e-7, "dz": 4.2e-6, "dgamma": 4.5e-7, "dbeta": 3.1e-7, "dw": 4.0e-6, "dx": 9.8e-6,
             "running_mean": 6.3e-8, "running_var": 7.3e-7}
GRADIENTS = ("dz", "dgamma", "dbeta", "dw", "dx")
ABS_SHARE = 0.05   # the ceiling 2e-5 max|ref| + 1e-6 = 2e-5 (max|ref| + 0.05): errors are measured in units of max|ref| + 0.05
# Bounds that are 4x the yardstick instead of the ceiling: every quantity whose worst error on one MI355X is within it.
# Not listed: dx (4x its yardstick is above the ceiling) and running_var (2.9e-6 against the ceiling's 1e-6).  y is held to it
# wherever there is more than one row; with ONE row rstd = 1 / sqrt(eps) and the forward's shift beta - mean gamma rstd is rounded at
# the size of mean gamma rstd (hundreds to thousands): 7.8x / 142x the yardstick there, 0.2 of the ceiling, which stays.
TIGHT = ("y", "mean", "rstd", "dz", "dgamma", "dbeta", "dw", "running_mean")


def bound(name, ref, single_row=False):
    """The largest |got - ref| a kernel's tensor `name` may show against the float64 `ref`."""
    tight = name in TIGHT and not (name == "y" and single_row)
    if name in ("running_mean", "running_var"):
        return min(1e-6, 4.0 * YARDSTICK[name]) if tight else 1e-6
    peak = float(np.abs(ref).max()) if np.size(ref) else 0.0
    ceiling = 2e-5 * (peak + ABS_SHARE) * (5.0 if name in GRADIENTS else 1.0)
    return min(ceiling, 4.0 * YARDSTICK[name] * (peak + ABS_SHARE)) if tight else ceiling


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def _windows(a, fill):
    """[B, H, W, C] -> [B, Ho, Wo, 4, C]: the 2x2 / stride-2 ceil-mode windows, slots in (h, w) scan order, `fill` where the image ends."""
    b, h, w, c = a.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    pad = np.full((b, 2 * ho, 2 * wo, c), fill, a.dtype)
    pad[:, :h, :w] = a
    return pad.reshape(b, ho, 2, wo, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, ho, wo, 4, c)


def _unwindows(win, h, w):
    b, ho, wo, _, c = win.shape
    return win.reshape(b, ho, wo, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * ho, 2 * wo, c)[:, :h, :w]


def _colsum(rows, dtype):
    """Per-channel sum of [rows, C]: each channel's values laid out contiguously, so that NumPy adds them pairwise (a sum down the
    rows would be a running sum, whose rounding grows with the number of rows)."""
    return np.ascontiguousarray(rows.T).sum(axis=1, dtype=dtype)


def batch_stats(z, eps, dtype=F64):
    """(mean, biased var, rstd) per channel of z [B, H, W, C]."""
    z = np.asarray(z, dtype)
    rows = z.reshape(-1, z.shape[-1])
    m = dtype(rows.shape[0])
    mean = _colsum(rows, dtype) / m
    var = _colsum(np.square(rows - mean), dtype) / m
    rstd = (dtype(1) / np.sqrt(var + dtype(eps))).astype(dtype)
    return mean, var, rstd


def running_stats(mean, var, m_rows, conv_bias, rm, rv, momentum, dtype=F64):
    mom = dtype(momentum)
    bias = np.zeros_like(mean) if conv_bias is None else np.asarray(conv_bias, dtype)
    unbias = dtype(m_rows / (m_rows - 1.0)) if m_rows > 1 else dtype(1)
    new_rm = (dtype(1) - mom) * np.asarray(rm, dtype) + mom * (mean + bias)
    new_rv = (dtype(1) - mom) * np.asarray(rv, dtype) + mom * (var * unbias)
    return new_rm.astype(dtype), new_rv.astype(dtype)


def _pre(z, mean, rstd, gamma, beta):
    return (z - mean) * rstd * gamma + beta


def bn_relu(z, conv_bias, gamma, beta, rm, rv, eps, momentum, pool, dtype=F64):
    """-> (y [B, H, W, C] or p [B, ceil(H/2), ceil(W/2), C], save_mean, save_rstd, running_mean, running_var)"""
    z, gamma, beta = np.asarray(z, dtype), np.asarray(gamma, dtype), np.asarray(beta, dtype)
    mean, var, rstd = batch_stats(z, eps, dtype)
    y = np.maximum(_pre(z, mean, rstd, gamma, beta), dtype(0))
    if pool:
        y = _windows(y, -np.inf).max(axis=3)
    new_rm, new_rv = running_stats(mean, var, z.size // z.shape[-1], conv_bias, rm, rv, momentum, dtype)
    return y.astype(dtype), mean, rstd, new_rm, new_rv


def bn_relu_backward(z, dy, gamma, beta, eps, pool, dtype=F64):
    """-> (dz [B, H, W, C], dgamma, dbeta); dy has the shape of bn_relu's output."""
    z, dy, gamma, beta = np.asarray(z, dtype), np.asarray(dy, dtype), np.asarray(gamma, dtype), np.asarray(beta, dtype)
    b, h, w, c = z.shape
    m = dtype(b * h * w)
    mean, _, rstd = batch_stats(z, eps, dtype)
    pre = _pre(z, mean, rstd, gamma, beta)
    if pool:
        win = _windows(np.maximum(pre, dtype(0)), -np.inf)
        sel = win.argmax(axis=3)                                  # the FIRST maximum in scan order
        best = np.take_along_axis(win, sel[:, :, :, None], axis=3)[:, :, :, 0]
        gwin = np.zeros(win.shape, dtype)
        np.put_along_axis(gwin, sel[:, :, :, None], np.where(best > 0, dy, dtype(0))[:, :, :, None], axis=3)
        g = _unwindows(gwin, h, w)
    else:
        g = np.where(pre > 0, dy, dtype(0))
    xhat = (z - mean) * rstd
    rows = lambda a: a.reshape(-1, c)   # noqa: E731
    dbeta = _colsum(rows(g), dtype)
    dgamma = _colsum(rows(g * xhat), dtype)
    a = gamma * rstd
    bq = -a * rstd * dgamma / m
    d = -a * dbeta / m - bq * mean
    dz = a * g + bq * z + d
    return dz.astype(dtype), dgamma, dbeta


def conv3x3(x, w, dtype=F64):
    """z [B, H, W, C] = 3x3 'same' convolution (zero padding, no bias) of x [B, CIN, H, W] with w [C, CIN, 3, 3]."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    b, _, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    z = np.zeros((b, h, wd, w.shape[0]), dtype)
    for ky in range(3):
        for kx in range(3):
            z += np.einsum("bchw,oc->bhwo", xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx]).astype(dtype)
    return z


def conv0_bn_relu(x, w, conv_bias, gamma, beta, rm, rv, eps, momentum, dtype=F64):
    return bn_relu(conv3x3(x, w, dtype), conv_bias, gamma, beta, rm, rv, eps, momentum, False, dtype)


def conv0_bn_relu_backward(x, w, dy, gamma, beta, eps, dtype=F64):
    """-> (dz, dgamma, dbeta, dW [C, CIN, 3, 3], dx [B, CIN, H, W])"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    b, _, h, wd = x.shape
    dz, dgamma, dbeta = bn_relu_backward(conv3x3(x, w, dtype), dy, gamma, beta, eps, False, dtype)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dzp = np.pad(dz, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dw, dx = np.zeros(w.shape, dtype), np.zeros(x.shape, dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("bhwo,bchw->oc", dz, xp[:, :, ky:ky + h, kx:kx + wd])
            # dx[b, ci, h, w] += w[co, ci, ky, kx] dz[b, h + 1 - ky, w + 1 - kx, co]
            dx += np.einsum("bhwo,oc->bchw", dzp[:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + wd], w[:, :, ky, kx]).astype(dtype)
    return dz, dgamma, dbeta, dw, dx


# ---------------------------------------------------------------------------
# inputs on a grid
# ---------------------------------------------------------------------------
def zero_gamma_channels(c):
    """The two channels with gamma = 0 (beta = +0.25, -0.25): one in the middle, and the last one."""
    return c // 3, c - 1


def _affine(z64, grid, eps, rng):
    """gamma, beta (float32) that put every pre-activation of z64 [.., C] (on multiples of 1 / grid) half a grid step or more,
    times |gamma| rstd, from zero; conv bias and running statistics to go with them."""
    c = z64.shape[-1]
    rows = z64.reshape(-1, c)
    mean, _, rstd = batch_stats(z64, eps)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(F32)
    gamma[:2] = (abs(gamma[0]), -abs(gamma[1]))               # both signs in every case (a float4 holds both)
    q = np.quantile(rows, rng.uniform(0.25, 0.75), axis=0)    # somewhere inside the channel's values
    zstar = (np.floor(q * grid) + 0.5) / grid
    beta = (-gamma.astype(F64) * rstd * (zstar - mean)).astype(F32)
    c_pos, c_neg = zero_gamma_channels(c)
    gamma[[c_pos, c_neg]] = 0.0
    beta[c_pos], beta[c_neg] = 0.25, -0.25
    # what the construction promises, checked on the float32 parameters the kernels get
    pre = _pre(z64, mean, rstd, gamma.astype(F64), beta.astype(F64))
    margin = np.abs(gamma.astype(F64)) * rstd / (2 * grid)
    margin[[c_pos, c_neg]] = 0.25
    assert np.all(np.abs(pre).reshape(-1, c).min(axis=0) >= margin * (1 - 1e-5)), "a pre-activation is closer to 0 than promised"
    assert np.all(pre[..., c_pos] == 0.25) and np.all(pre[..., c_neg] == -0.25)
    return {"gamma": gamma, "beta": beta, "bias": rng.uniform(-0.5, 0.5, c).astype(F32),
            "rm": rng.uniform(-0.5, 0.5, c).astype(F32), "rv": rng.uniform(0.5, 1.5, c).astype(F32),
            "min_margin": float(margin.min())}


def make_bn_case(shape, pool, eps=EPS, momentum=MOMENTUM, seed=0):
    """{'z' [B, H, W, C], 'dy' (the output's shape), 'gamma', 'beta', 'bias', 'rm', 'rv'} float32, 'eps', 'momentum', 'pool'."""
    b, h, w, c = shape
    rng = np.random.default_rng([seed, b, h, w, c])
    spread = rng.choice([2, 3, 5, 16], c)
    k = rng.integers(-spread, spread + 1, (b, h, w, c))
    assert np.abs(k).max() <= 16
    z = (k / 8.0).astype(F32)
    assert np.array_equal(z.astype(F64) * 8, k)                   # on the grid, exactly
    case = {"z": z, "eps": eps, "momentum": momentum, "pool": bool(pool), **_affine(z.astype(F64), 8, eps, rng)}
    out = (b, (h + 1) // 2, (w + 1) // 2, c) if pool else shape
    case["dy"] = np.random.default_rng([seed + 1, b, h, w, c, int(pool)]).standard_normal(out).astype(F32)
    if pool:
        # of the windows with more than one element, at least 10 % tie at their maximum (the gamma = 0 channels and windows whose
        # maximum is 0 count); where there are 1000 or more, at least 10 % tie at a POSITIVE maximum - the first-maximum rule alone
        total, positive, n = tie_shares(case)
        assert n == 0 or total >= 0.10, (shape, total, n)
        assert n < 1000 or positive >= 0.10, (shape, positive, n)
    return case


def make_conv0_case(shape, eps=EPS, momentum=MOMENTUM, seed=0):
    """{'x' [B, CIN, H, W], 'w' [C, CIN, 3, 3], 'dy' [B, H, W, C], 'gamma', ...} float32."""
    cin, cout, b, h, w = shape
    rng = np.random.default_rng([seed, cin, cout, b, h, w])
    x = (rng.integers(-8, 9, (b, cin, h, w)) / 4.0).astype(F32)
    wt = (rng.integers(-6, 7, (cout, cin, 3, 3)) / 4.0).astype(F32)
    z = conv3x3(x, wt)
    assert np.array_equal(np.round(z * 16), z * 16) and np.abs(z).max() <= 54 and np.array_equal(z, z.astype(F32))
    case = {"x": x, "w": wt, "eps": eps, "momentum": momentum, **_affine(z, 16, eps, rng)}
    case["dy"] = rng.standard_normal((b, h, w, cout)).astype(F32)
    return case


def tie_shares(case):
    """Of the pooled windows (per channel) with more than one element: (the share whose maximum of y is reached by more than one
    element - the first-maximum or the zero rule decides there; the share where that tied maximum is > 0 - the first-maximum rule
    alone; the number of such windows)."""
    z = case["z"].astype(F64)
    mean, _, rstd = batch_stats(z, case["eps"])
    y = np.maximum(_pre(z, mean, rstd, case["gamma"].astype(F64), case["beta"].astype(F64)), 0.0)
    win = _windows(y, -np.inf)
    real = np.isfinite(win).sum(axis=3)
    best = win.max(axis=3)
    tied = ((win == best[:, :, :, None]).sum(axis=3) > 1) & (real > 1)
    n = int((real > 1).sum())
    if n == 0:
        return 0.0, 0.0, 0
    return float(tied.sum()) / n, float((tied & (best > 0)).sum()) / n, n


# ---------------------------------------------------------------------------
# the reference and the float32 yardstick of a case
# ---------------------------------------------------------------------------
def reference(case, dtype=F64):
    """Every quantity the GPU tests compare, by the definition in `dtype` (with the case's convolution bias)."""
    eps, mom = case["eps"], case["momentum"]
    if "x" in case:
        y, mean, rstd, rm, rv = conv0_bn_relu(case["x"], case["w"], case["bias"], case["gamma"], case["beta"], case["rm"], case["rv"],
                                              eps, mom, dtype)
        dz, dgamma, dbeta, dw, dx = conv0_bn_relu_backward(case["x"], case["w"], case["dy"], case["gamma"], case["beta"], eps, dtype)
        extra = {"dw": dw, "dx": dx}
    else:
        y, mean, rstd, rm, rv = bn_relu(case["z"], case["bias"], case["gamma"], case["beta"], case["rm"], case["rv"], eps, mom,
                                        case["pool"], dtype)
        dz, dgamma, dbeta = bn_relu_backward(case["z"], case["dy"], case["gamma"], case["beta"], eps, case["pool"], dtype)
        extra = {}
    return {"y": y, "mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv, "dz": dz, "dgamma": dgamma, "dbeta": dbeta, **extra}


def errors(got, ref):
    """{name: (max |got - ref|, max |ref|)} over the names of `got`."""
    out = {}
    for name, g in got.items():
        r = np.asarray(ref[name], F64)
        g = np.asarray(g, F64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        out[name] = (float(np.abs(g - r).max()), float(np.abs(r).max()))
    return out


def yardstick(case, ref):
    """{name: the float32 evaluation's error against `ref` over max|ref| + ABS_SHARE (running statistics: absolute)}."""
    out = {}
    for name, (err, peak) in errors(reference(case, F32), ref).items():
        out[name] = err if name.startswith("running") else err / (peak + ABS_SHARE)
    return out
