"""Reference forms of the 3x3 'same' convolution kernels (csrc/k_conv_wino.h, k_conv_wino_b3.h, k_conv_c32.h, k_conv_small.h,
k_conv_wino_wrw.h), a helper beside the tests.  NumPy only; activations are channels-last [B, H, W, C], weights [Cout, Cin, 3, 3].

The definition (float64)
    conv3x3(x, w, bias, relu, pool)   z[b, h, w, o] = sum_{c, ky, kx} x[b, h + ky - 1, w + kx - 1, c] w[o, c, ky, kx] (zero outside the
                                      image) + bias[o], then max(., 0), then the 2x2 / stride-2 / ceil-mode max over the window's IN-IMAGE
                                      elements.  A NaN stays: in the sum, through the ReLU (np.maximum) and through the pool (np.max).
    conv3x3_dx(dz, w)                 dx = conv3x3(dz, w'), w'[c, o, ky, kx] = w[o, c, 2 - ky, 2 - kx]
    conv3x3_dw(x, dz)                 dw[o, c, ky, kx] = sum_{b, h, w} dz[b, h, w, o] x[b, h + ky - 1, w + kx - 1, c]
    cond(x, w, bias, pool)            conv3x3(|x|, |w|) + |bias|: the size of what each output sums (pooled: the window's maximum);
    cond_dx, cond_dw                  the same of the two gradients (cond_dw: summed over the nine taps of a channel pair, see there)

The yardsticks (float32, none of the kernels' orderings, no fused multiply-add: every product and every sum rounded)
    direct_f32 / direct_dw_f32        the definition with ONE running float32 sum over taps and input channels (over pixels for dw)
    wino_f32 / wino_dw_f32            plain Winograd F(2x2, 3x3): U = G g G^T rounded once from float64, V = B^T d B and the output
                                      transform A^T M A in float32, M a running float32 sum over input channels (dw: dU a running
                                      float32 sum over the tiles of (B^T d B) (A dY A^T), dW = G^T dU G in float32)

The rule of tests/test_conv_gpu.py:  |got - ref| <= K[name] 2^-24 cond  per element, K = 4x the worse yardstick's worst ratio over
CASES x the continuous generators (tests/test_conv_host.py re-measures it), and under it the ceilings these kernels carry elsewhere
in the suite, now against float64 (CEILING, of the tensor's peak).

Inputs: `make_case(kind, shape, ...)`, kind one of
    grid       x = k / 4 (|k| <= 8), w = k / 4 (|k| <= 6), bias = k / 4, dz = k / 4: every product and every partial sum of ANY
               summation order - direct, Winograd forward, Winograd weight gradient - is a multiple of 2^-8 below 2^24 of them, so
               a float32 evaluation equals float64 bit for bit.  The generator proves it from the value ranges or from the absolute-value forms
               (wino_f32 / wino_dw_f32 with `absolute`) and halves its ranges until it holds; `bn`: also the per-lane sums of (z - K)^2 of a `_bn` epilogue.
    gauss      randn inputs, He-scaled randn weights (what tests/test_transforms_gpu.py draws)
    relu_like  max(randn, 0): about half the elements exactly zero, two whole zero channels
    offset     mean 30x spread, weights with a small common offset
    ranged     per-channel scales 2^-12 .. 2^12 (x by input channel and w by its inverse, w by output channel): small outputs
               beside large ones
"""
import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24

# (b, h, w, cin, cout): every tile geometry of the Winograd kernels (16, 32, 64 tile columns) with odd heights and widths, a single
# pixel, one-row images, tile rows that straddle images (B TH no multiple of TR), 8 / 16 / 24 -> 64, 64 -> 128, 512 -> 64 at 5 x 6
CASES = [(1, 1, 1, 8, 64), (2, 1, 13, 16, 64), (3, 5, 7, 24, 64), (3, 5, 41, 16, 64), (2, 7, 71, 8, 64), (2, 5, 9, 64, 128),
         (1, 5, 6, 512, 64)]
# the same for the split-bf16 family (16 | cin)
CASES_B3 = [(1, 1, 1, 16, 64), (2, 1, 13, 16, 64), (3, 5, 7, 48, 64), (3, 5, 41, 16, 64), (2, 7, 71, 16, 64), (2, 5, 9, 64, 128),
            (1, 5, 6, 512, 64)]
# 32 -> 32 (tiles of 4 x 64 pixels) and the first layer (cin 1 or 2; the contiguous output takes widths that are multiples of 4)
C32_CASES = [(1, 1, 1), (2, 1, 9), (3, 5, 70), (1, 9, 67), (2, 4, 64)]
SMALL_CASES = [(2, 5, 8, 1, 32), (1, 1, 4, 2, 8), (2, 3, 12, 2, 16), (3, 7, 9, 1, 32), (1, 6, 132, 2, 4)]
# weight gradient: 32 / 64 / 96 channels on either side; tile rows of the batch 4 (4 splits), 16, 18 and 40 (> 16: the two-stage sum)
WRW_CASES = [(2, 3, 5, 32, 32), (2, 4, 7, 64, 64), (8, 4, 7, 64, 32), (6, 5, 9, 32, 96), (20, 4, 6, 64, 64), (3, 1, 1, 96, 64),
             (5, 7, 33, 96, 96)]
CONTINUOUS = ("gauss", "relu_like", "offset", "ranged")

# K of the rule: 4x the worse yardstick's worst |err| / (2^-24 cond) over the case lists x CONTINUOUS (test_conv_host.py)
# (z: the running sum over 9 x 512 products of one sign - `offset`, 512 -> 64 - reads 66; every other case is below 38)
YARDSTICK = {"z": 66.3, "dx": 21.6, "dw": 4.0}
K = {name: 4.0 * v for name, v in YARDSTICK.items()}
# of the tensor's peak, as the existing tests state them
CEILING = {"wino": 2e-6, "wino_b3": 2e-6, "wrw": 2e-6, "c32": 2e-5, "small": 2e-6}

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], F64)     # B^T: V = B^T d B
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], F64)        # U = G g G^T
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], F64)                                   # Y = A^T M A


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def pool2x2(a):
    """[B, H, W, C] -> [B, ceil(H/2), ceil(W/2), C]: the maximum over each window's in-image elements (a NaN among them wins)."""
    b, h, w, c = a.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    pad = np.full((b, 2 * ho, 2 * wo, c), -np.inf, a.dtype)
    pad[:, :h, :w] = a
    return pad.reshape(b, ho, 2, wo, 2, c).max(axis=(2, 4))


def _pad(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _im2col(xp, h, wd):
    """[B, H + 2, W + 2, C] -> [B H W, 9 C]: the nine shifted views side by side, tap-major."""
    b, c = xp.shape[0], xp.shape[-1]
    cols = np.empty((b, h, wd, 9, c), xp.dtype)
    for ky in range(3):
        for kx in range(3):
            cols[:, :, :, 3 * ky + kx] = xp[:, ky:ky + h, kx:kx + wd]
    return cols.reshape(b * h * wd, 9 * c)


def conv3x3(x, w, bias=None, relu=False, pool=False):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    b, h, wd, _ = x.shape
    with np.errstate(invalid="ignore"):
        # one product of [B H W, 9 Cin] with [9 Cin, Cout]: an output row reads its own window only, so a NaN stays in its windows
        z = (_im2col(_pad(x), h, wd) @ w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0])).reshape(b, h, wd, w.shape[0])
        if bias is not None:
            z = z + np.asarray(bias, F64)
        if relu:
            z = np.maximum(z, 0.0)
        if pool:
            z = pool2x2(z)
    return z


def flip_transpose(w):
    """w'[c, o, ky, kx] = w[o, c, 2 - ky, 2 - kx]: the weights of the backward-data pass."""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def conv3x3_dx(dz, w):
    return conv3x3(dz, flip_transpose(w))


def conv3x3_dw(x, dz):
    x, dz = np.asarray(x, F64), np.asarray(dz, F64)
    b, h, wd, cin = x.shape
    cout = dz.shape[-1]
    return np.ascontiguousarray((dz.reshape(-1, cout).T @ _im2col(_pad(x), h, wd)).reshape(cout, 3, 3, cin).transpose(0, 3, 1, 2))


def cond(x, w, bias=None, pool=False):
    return conv3x3(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), False, pool)


def cond_dx(dz, w):
    return conv3x3_dx(np.abs(dz), np.abs(w))


def cond_dw(x, dz):
    """Per (o, c) pair, the sum over the nine taps of conv3x3_dw(|x|, |dz|), the same for each of them: a Winograd weight gradient
    forms every tap as G^T dU G, from sums over all 16 positions, so that a tap whose own sum is empty (the outer taps of a one-pixel
    image) or much smaller than its neighbours' (sparse activations) carries the rounding of the others.  Per tap, the Winograd
    yardstick reads 24 on `relu_like` and has no bound at all where a tap sums only zeros; per pair, both yardsticks stay below 4."""
    per_tap = conv3x3_dw(np.abs(x), np.abs(dz))
    return np.broadcast_to(per_tap.sum(axis=(2, 3), keepdims=True), per_tap.shape)


# ---------------------------------------------------------------------------
# the float32 yardsticks
# ---------------------------------------------------------------------------
def _epilogue_f32(z, bias, relu, pool):
    if bias is not None:
        z = z + np.asarray(bias, F32)
    if relu:
        z = np.maximum(z, F32(0))
    return pool2x2(z) if pool else z


def direct_f32(x, w, bias=None, relu=False, pool=False):
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    b, h, wd, cin = x.shape
    xp = _pad(x)
    z = np.zeros((b, h, wd, w.shape[0]), F32)
    for ky in range(3):
        for kx in range(3):
            for c in range(cin):
                z += xp[:, ky:ky + h, kx:kx + wd, c, None] * w[:, c, ky, kx]        # the product rounded, then the sum
    assert z.dtype == F32
    return _epilogue_f32(z, bias, relu, pool)


def direct_dw_f32(x, dz):
    x, dz = np.asarray(x, F32), np.asarray(dz, F32)
    b, h, wd, cin = x.shape
    xp = _pad(x)
    dw = np.zeros((dz.shape[-1], cin, 3, 3), F32)
    for bi in range(b):
        for i in range(h):
            for j in range(wd):
                dw += dz[bi, i, j, :, None, None, None] * xp[bi, i:i + 3, j:j + 3].transpose(2, 0, 1)[None]
    assert dw.dtype == F32
    return dw


def _tiles(a, absolute=False):
    """[B, H, W, C] -> the 4 x 4 input patches [B, TH, TW, 4, 4, C] of the 2 x 2 output tiles (zero outside the image)."""
    b, h, w, c = a.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((b, 2 * th + 2, 2 * tw + 2, c), a.dtype)
    pad[:, 1:h + 1, 1:w + 1] = a
    out = np.empty((b, th, tw, 4, 4, c), a.dtype)
    for i in range(4):
        for j in range(4):
            out[:, :, :, i, j] = pad[:, i:i + 2 * th:2, j:j + 2 * tw:2]
    return out


def _apply(mat, t, axis, dtype):
    """sum_j mat[i, j] t[.., j, ..] along `axis`, one rounded operation after another in `dtype` (mat holds 0, +-1, +-1/2)."""
    t = np.moveaxis(t, axis, 0)
    rows = []
    for row in mat:
        acc = None
        for coef, tj in zip(row, t):
            if coef == 0:
                continue
            term = (tj * dtype(coef)).astype(dtype)
            acc = term if acc is None else (acc + term).astype(dtype)
        rows.append(acc)
    return np.moveaxis(np.stack(rows), 0, axis)


def wino_f32(x, w, bias=None, relu=False, pool=False, absolute=False):
    """`absolute`: float64 with every coefficient and operand replaced by its absolute value - a bound on every partial sum of the form."""
    dt = F64 if absolute else F32
    fix = np.abs if absolute else (lambda m: m)
    x = np.asarray(x, dt)
    b, h, wd, cin = x.shape
    g = np.asarray(w, F64)
    if absolute:
        g = np.abs(g)
    u = np.einsum("ia,ocab,jb->ijoc", fix(G), g, fix(G)).astype(dt)             # rounded once from float64
    d = _tiles(fix(x))
    v = _apply(fix(BT), _apply(fix(BT), d, 3, dt), 4, dt)                       # [B, TH, TW, 4, 4, C]
    m = np.zeros(v.shape[:5] + (g.shape[0],), dt)
    for c in range(cin):
        m += v[..., c, None] * u[:, :, :, c]                                    # [.., 4, 4, 1] x [4, 4, Cout]
    y = _apply(fix(AT), _apply(fix(AT), m, 3, dt), 4, dt)                       # [B, TH, TW, 2, 2, Cout]
    th, tw = y.shape[1], y.shape[2]
    z = y.transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * th, 2 * tw, -1)[:, :h, :wd]
    assert z.dtype == dt
    return z if absolute else _epilogue_f32(z, bias, relu, pool)


def wino_dw_f32(x, dz, absolute=False):
    dt = F64 if absolute else F32
    fix = np.abs if absolute else (lambda m: m)
    x, dz = fix(np.asarray(x, dt)), fix(np.asarray(dz, dt))
    b, h, wd, cin = x.shape
    th, tw = (h + 1) // 2, (wd + 1) // 2
    v = _apply(fix(BT), _apply(fix(BT), _tiles(x), 3, dt), 4, dt)               # [B, TH, TW, 4, 4, Cin]
    dzp = np.zeros((b, 2 * th, 2 * tw, dz.shape[-1]), dt)
    dzp[:, :h, :wd] = dz
    dy = dzp.reshape(b, th, 2, tw, 2, -1).transpose(0, 1, 3, 2, 4, 5)           # [B, TH, TW, 2, 2, Cout]
    a = fix(AT.T)                                                               # A: 4 x 2
    e = _apply(a, _apply(a, dy, 3, dt), 4, dt)                                  # A dY A^T [B, TH, TW, 4, 4, Cout]
    du = np.zeros((4, 4, dz.shape[-1], cin), dt)
    v, e = v.reshape(-1, 4, 4, cin), e.reshape(-1, 4, 4, dz.shape[-1])
    for t in range(v.shape[0]):
        du += e[t][:, :, :, None] * v[t][:, :, None, :]
    dw = _apply(fix(G.T), _apply(fix(G.T), du, 0, dt), 1, dt)                   # G^T dU G: [3, 3, Cout, Cin]
    assert dw.dtype == dt
    return np.ascontiguousarray(dw.transpose(2, 3, 0, 1))


def ratio(got, ref, cnd):
    """The worst |got - ref| / (2^-24 cond) over the elements (0 / 0 = 0: what sums nothing must be exact)."""
    err = np.abs(np.asarray(got, F64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (U * cnd))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------
# the host's geometry, restated (csrc/host_wino.h, csrc/k_conv_c32.h)
# ---------------------------------------------------------------------------
def wino_geometry(b, h, w, cout, cus=256):
    """{'tc', 'tr', 'n_work', 'grid'} of iris_conv3x3_wino / _wino_b3: blocks of 64 tiles (tr rows x tc columns) x 64 output channels,
    a persistent grid of min(n_work, CUs) workgroups."""
    th, tw = (h + 1) // 2, (w + 1) // 2
    tc = 64 if tw > 32 else (32 if tw > 16 else 16)
    tr = 64 // tc
    n_work = ((b * th + tr - 1) // tr) * ((tw + tc - 1) // tc) * (cout // 64)
    return {"tc": tc, "tr": tr, "th": th, "tw": tw, "n_work": n_work, "grid": min(n_work, cus)}


def c32_geometry(b, h, w, cus=256):
    n_tiles = b * ((h + 3) // 4) * ((w + 63) // 64)
    return {"n_tiles": n_tiles, "grid": min(n_tiles, 2 * cus)}


def looping_batch(h, w, cout, cus=256, b0=1):
    """The smallest batch >= b0 at which every workgroup of the Winograd grid takes two items and some take three."""
    b = b0
    while wino_geometry(b, h, w, cout, cus)["n_work"] < 2 * cus + 3:
        b += 1
    return b


def looping_batch_c32(h, w, cus=256):
    b = 2 * cus + 5
    while c32_geometry(b, h, w, cus)["n_tiles"] < 2 * (2 * cus) + 3:
        b += 1
    return b


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _grid_ok(case, bn, dw):
    """Every partial sum of every form is a multiple of 2^-8 with fewer than 2^24 of them (so: exact in float32)."""
    x, w, dz = case["x"], case["w"], case["dz"]
    step = 2.0 ** -8            # x, dz in 1/4, w in 1/4, G g G^T in 1/16 of w's: 1/64 x 1/4 = 1/256; dW: 1/16 x 1/4 (G^T . G) = 1/64
    cout, cin = w.shape[:2]
    xm, wm = float(max(np.abs(x).max(), np.abs(dz).max())), float(max(np.abs(w).max(), np.abs(case["bias"]).max()))
    # without looking at the values: |V| <= 4 max|x|, |U| <= 2.25 max|w| (row sums of |B^T| and |G|: 2 and 1.5), |M| <= C 9 max|x| max|w|
    # over C channels, |Y| <= 9 |M|
    worst = 81.0 * max(cin, cout) * xm * wm + wm
    if worst / step >= 2.0 ** 24:        # ... or from the absolute-value forms of this very case
        worst = max(float(wino_f32(x, w, absolute=True).max()) + wm, float(wino_f32(dz, flip_transpose(w), absolute=True).max()))
    # (the absolute Winograd forms bound the direct forms too: every direct partial sum is at most cond <= its Winograd bound)
    assert float(cond(x, w, case["bias"]).max()) <= worst + 1e-9 and float(cond_dx(dz, w).max()) <= worst + 1e-9
    if dw:
        worst_dw = float(wino_dw_f32(x, dz, absolute=True).max())
        assert float(conv3x3_dw(np.abs(x), np.abs(dz)).max()) <= worst_dw + 1e-9
        worst = max(worst, worst_dw)
    if worst / step >= 2.0 ** 24:
        return False
    if bn:
        # a lane of a `_bn` epilogue sums d = z - K and d^2 over at most 64 of its channel's values in float32, K one of them:
        # |d| <= max z - min z of the channel, d^2 a multiple of 2^-8
        z = conv3x3(x, w)
        span = float((z.max(axis=(0, 1, 2)) - z.min(axis=(0, 1, 2))).max())
        if 64 * span * span / step >= 2.0 ** 24:
            return False
    return True


def make_case(kind, shape, seed=0, bn=False, dw=True):
    """{'x' [B, H, W, Cin], 'w' [Cout, Cin, 3, 3], 'bias' [Cout], 'dz' [B, H, W, Cout]} float32 + 'kind', 'shape'.
    grid: `bn` also proves the `_bn` epilogue's float32 sums exact; `dw` = False leaves the weight gradient's proof out (large batches
    that no weight-gradient test uses)."""
    b, h, wd, cin, cout = shape
    rng = np.random.default_rng([seed, CONTINUOUS.index(kind) + 1 if kind in CONTINUOUS else 0, b, h, wd, cin, cout])
    xs, ws, zs = (b, h, wd, cin), (cout, cin, 3, 3), (b, h, wd, cout)
    if kind == "grid":
        kx, kw = 8, 6
        while True:
            case = {"x": (rng.integers(-kx, kx + 1, xs) / 4.0).astype(F32), "w": (rng.integers(-kw, kw + 1, ws) / 4.0).astype(F32),
                    "bias": (rng.integers(-kw, kw + 1, cout) / 4.0).astype(F32), "dz": (rng.integers(-kx, kx + 1, zs) / 4.0).astype(F32)}
            if _grid_ok(case, bn, dw):
                break
            kx, kw = kx // 2, max(kw // 2, 1)
            assert kx >= 1, ("no grid for", shape)
        for name in ("x", "w", "bias", "dz"):
            assert np.array_equal(np.round(case[name].astype(F64) * 4), case[name].astype(F64) * 4)
        case["k_range"] = (kx, kw)
    elif kind == "gauss":
        case = {"x": rng.standard_normal(xs), "w": rng.standard_normal(ws) * (2.0 / (9 * cin)) ** 0.5,
                "bias": rng.standard_normal(cout) * 0.1, "dz": rng.standard_normal(zs)}
    elif kind == "relu_like":
        x = np.maximum(rng.standard_normal(xs), 0.0)
        zero = (0, cin // 2) if cin >= 8 else ()      # whole zero channels (the first layer's one or two stay)
        for c in zero:
            x[..., c] = 0.0
        dz = np.maximum(rng.standard_normal(zs), 0.0)
        dz[..., cout // 3] = 0.0
        case = {"x": x, "w": rng.standard_normal(ws) * (2.0 / (9 * cin)) ** 0.5, "bias": rng.standard_normal(cout) * 0.1, "dz": dz}
        share = float((x == 0).mean())
        assert (x.size < 256 or 0.4 <= share <= 0.65) and not any(x[..., c].any() for c in zero), share
    elif kind == "offset":
        case = {"x": rng.standard_normal(xs) + 30.0, "w": rng.standard_normal(ws) * (2.0 / (9 * cin)) ** 0.5 + 0.02,
                "bias": rng.standard_normal(cout) * 0.1, "dz": rng.standard_normal(zs) + 30.0}
        assert abs(float(case["x"].mean()) - 30.0) < 3.0
    elif kind == "ranged":
        s_in, s_out = 2.0 ** rng.integers(-12, 13, cin), 2.0 ** rng.integers(-12, 13, cout)
        if cin >= 2:
            s_in[:2] = (2.0 ** -12, 2.0 ** 12)
        s_out[:2] = (2.0 ** -12, 2.0 ** 12)
        case = {"x": rng.standard_normal(xs) * s_in,
                "w": rng.standard_normal(ws) * (2.0 / (9 * cin)) ** 0.5 / s_in[None, :, None, None] * s_out[:, None, None, None],
                "bias": rng.standard_normal(cout) * 0.1 * s_out, "dz": rng.standard_normal(zs) / s_out}
        assert s_out.max() / s_out.min() == 2.0 ** 24
    else:
        raise ValueError(kind)
    case = {k: (np.ascontiguousarray(v, F32) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    case["kind"], case["shape"] = kind, tuple(shape)
    return case


def nchw(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 3, 1, 2))


def chunked(a):
    """[B, H, W, C] -> the channel-chunked [B, C / 8, H, W, 8] of the Winograd layers."""
    b, h, w, c = a.shape
    return np.ascontiguousarray(np.asarray(a).reshape(b, h, w, c // 8, 8).transpose(0, 3, 1, 2, 4))


def unchunked(a):
    b, cb, h, w, _ = a.shape
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1, 4).reshape(b, h, w, cb * 8))
