"""GPU tests of the training-mode BatchNorm + ReLU (+ MaxPool) passes at their own boundary - iris_bn_stats / iris_bn_relu_apply /
iris_bn_relu_bwd_reduce / iris_bn_relu_bwd_dx, the four iris_bn_relu_pool_* passes (csrc/k_elementwise.h) and the first layer's
iris_conv0_stats / iris_conv0_bn_relu / iris_conv0_bn_relu_backward(_dx) (csrc/k_conv0_bn.h) - through
`hip_autograd._FusedBiasBNReLU.apply` and `_FusedConv0BNReLU.apply`, against the float64 definition of tests/bn_ref.py.  No MIOpen
is involved.  The inputs sit on a grid (bn_ref's generators): every ReLU and max-pool decision is far from its threshold or an exact
tie, so every element is compared - no mask.  Bounds: `bn_ref.bound`.  Each test prints, per quantity, the kernel's error and its
ratio to the float32 yardstick's error on the same case (the definition's own lines in NumPy float32); DESIGN.md records the worst."""
import functools

import numpy as np
import pytest
import torch

import bn_ref as R
from bn_ref import BN_CASES, CONV0_CASES, F32, F64, OFFSET_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(dev, a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def _nhwc(t):
    """A [B, C, H, W] device tensor -> NumPy [B, H, W, C]."""
    return t.detach().permute(0, 2, 3, 1).cpu().numpy()


@functools.lru_cache(maxsize=2)
def _bn_case(shape, pool, eps, momentum):
    case = R.make_bn_case(shape, pool, eps, momentum)
    ref = R.reference(case)
    return case, ref, R.errors(R.reference(case, F32), ref)


@functools.lru_cache(maxsize=2)
def _conv0_case(shape):
    case = R.make_conv0_case(shape)
    ref = R.reference(case)
    return case, ref, R.errors(R.reference(case, F32), ref)


def _compare(what, got, ref, yard, single_row=False):
    """Print every quantity's error and its ratio to the yardstick's, then assert the bounds."""
    errs = R.errors(got, ref)
    late = []
    for name, (err, peak) in errs.items():
        floor = 2.0 ** -25 * max(peak, 1e-30)              # rounding the exact value to float32
        lim = R.bound(name, ref[name], single_row)
        print(f"{what} {name}: |. - fp64| = {err:.3e} (peak {peak:.3e}, bound {lim:.3e}), "
              f"{err / max(yard[name][0], floor):.2f} x the float32 yardstick ({yard[name][0]:.3e})")
        if not err <= lim:
            late.append((name, err, lim))
    assert not late, (what, late)


def _run_bn(dev, case, with_bias, nchw_dy, sums0=None):
    """One forward + backward of _FusedBiasBNReLU on the case -> {name: NumPy array}."""
    from challenge_amd.hip_autograd import _FusedBiasBNReLU, record_activations
    z = _t(dev, case["z"]).permute(0, 3, 1, 2).requires_grad_(True)          # [B, C, H, W] in channels_last memory
    assert z.is_contiguous(memory_format=torch.channels_last)
    gamma, beta = _t(dev, case["gamma"], True), _t(dev, case["beta"], True)
    bias = _t(dev, case["bias"], True) if with_bias else None
    rm, rv = _t(dev, case["rm"]), _t(dev, case["rv"])
    with record_activations() as tap:
        y = _FusedBiasBNReLU.apply(z, bias, gamma, beta, rm, rv, case["eps"], case["momentum"], case["pool"], sums0)
    dy = _t(dev, case["dy"]).permute(0, 3, 1, 2)
    if nchw_dy:
        dy = dy.contiguous()
    y.backward(dy)
    torch.cuda.synchronize()
    assert len(tap) == 1 and tap[0]["pool"] == case["pool"]
    if with_bias:
        assert bias.grad.shape == bias.shape and int(torch.count_nonzero(bias.grad)) == 0      # exactly 0
    return {"y": _nhwc(y), "mean": tap[0]["mean"].cpu().numpy(), "rstd": tap[0]["rstd"].cpu().numpy(),
            "running_mean": rm.cpu().numpy(), "running_var": rv.cpu().numpy(), "dz": _nhwc(z.grad),
            "dgamma": gamma.grad.cpu().numpy(), "dbeta": beta.grad.cpu().numpy()}


def _ref_for(case, ref, with_bias):
    if with_bias:
        return ref
    rm, _ = R.running_stats(ref["mean"], 0.0, case["z"].size // case["z"].shape[-1], None, case["rm"], case["rv"], case["momentum"])
    return {**ref, "running_mean": rm}


def _closed_forms(case, got):
    """What needs no reference: the gamma = 0 channels."""
    c = case["gamma"].size
    pos, neg = R.zero_gamma_channels(c)
    assert np.all(got["y"][..., pos] == F32(0.25)) and not got["y"][..., neg].any()
    assert not got["dz"][..., [pos, neg]].any()                     # a = gamma rstd = 0: every term of dz has that factor
    assert got["dgamma"][neg] == 0 and got["dbeta"][neg] == 0


BN_PARAMS = [(s, p, R.EPS, R.MOMENTUM, bias, nchw) for s, p in BN_CASES for bias in (True, False) for nchw in (False, True)]
BN_PARAMS += [((3, 9, 7, 64), p, R.MODEL_EPS, R.MODEL_MOMENTUM, bias, nchw) for p in (False, True) for bias, nchw in ((True, False), (False, True))]


def _bn_id(v):
    s, p, eps, mom, bias, nchw = v
    return "-".join(str(k) for k in s) + ("-pool" if p else "") + f"-eps{eps}-m{mom}" + ("-bias" if bias else "") + ("-nchwdy" if nchw else "")


@pytest.mark.parametrize("param", BN_PARAMS, ids=_bn_id)
def test_bn_relu_passes_match_float64(dev, param):
    shape, pool, eps, momentum, with_bias, nchw_dy = param
    case, ref, yard = _bn_case(shape, pool, eps, momentum)
    got = _run_bn(dev, case, with_bias, nchw_dy)
    assert all(v.dtype == F32 for v in got.values())
    _closed_forms(case, got)
    if shape[0] * shape[1] * shape[2] == 1:      # one row: xhat = 0 and dz = 0 exactly (y = relu(beta) is left to the bound)
        assert not got["dgamma"].any() and not got["dz"].any()
    _compare(_bn_id(param), got, _ref_for(case, ref, with_bias), yard, shape[0] * shape[1] * shape[2] == 1)


def test_bn_channel_limit_is_stated(dev):
    """4096 channels run (the 4096-channel cases above); 4100 are refused with the limit in the text, before any launch."""
    from challenge_amd import _native as N
    z = torch.zeros(2 * 4100, device=dev)
    sums = torch.zeros(2 * 4100, dtype=torch.float64, device=dev)
    rc = N.lib().iris_bn_stats(z.data_ptr(), 2, 4100, sums.data_ptr(), None)
    assert rc != 0
    with pytest.raises(ValueError, match="4096"):
        N.check(rc, "iris_bn_stats")
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(sums)) == 0


@pytest.mark.parametrize("pool", [False, True])
def test_statistics_handed_in_by_the_convolution(dev, pool):
    """`sums0`: (sum z, sum z^2) in slot 0 of the first window of an otherwise zero iris_bn_sums_len(c) buffer - a convolution's epilogue
    leaves them split over the slots and windows, which the consumer adds up (about zero, no shift K).  The same result as the separate statistics pass: within the bounds everywhere, and bit for bit in
    the channels whose two means agree bit for bit."""
    from challenge_amd import _native as N
    shape = (2, 33, 65, 68)
    case, ref, yard = _bn_case(shape, pool, R.EPS, R.MOMENTUM)
    own = _run_bn(dev, case, True, False)
    c = shape[3]
    n = int(N.lib().iris_bn_sums_len(c))
    assert n == 3 * 4 * 2 * c                                      # 68 channels: four copies, in each of the three exponent windows
    rows = case["z"].reshape(-1, c).astype(F64)
    sums = np.zeros(n, F64)
    sums[:c], sums[c:2 * c] = rows.sum(axis=0), np.square(rows).sum(axis=0)
    got = _run_bn(dev, case, True, False, sums0=_t(dev, sums))
    _compare(f"sums0 {shape} pool={pool}", got, ref, yard)
    same = own["mean"].view(np.uint32) == got["mean"].view(np.uint32)
    print(f"sums0: {int(same.sum())} of {c} means agree bit for bit with the separate statistics pass")
    assert same.sum() > 0
    for name in ("y", "dz"):
        assert np.array_equal(own[name][..., same].view(np.uint32), got[name][..., same].view(np.uint32)), name
    for name in ("running_mean", "dgamma", "dbeta"):
        assert np.array_equal(own[name][same].view(np.uint32), got[name][same].view(np.uint32)), name


# ---------------------------------------------------------------------------
# the first layer
# ---------------------------------------------------------------------------
def _run_conv0(dev, case, input_grad, weight_cl, with_bias=True):
    from challenge_amd.hip_autograd import _FusedConv0BNReLU, record_activations
    x = _t(dev, case["x"], input_grad)
    w = _t(dev, case["w"])
    if weight_cl:
        w = w.contiguous(memory_format=torch.channels_last)
    w.requires_grad_(True)
    gamma, beta = _t(dev, case["gamma"], True), _t(dev, case["beta"], True)
    bias = _t(dev, case["bias"], True) if with_bias else None
    rm, rv = _t(dev, case["rm"]), _t(dev, case["rv"])
    with record_activations() as tap:
        y = _FusedConv0BNReLU.apply(x, w, bias, gamma, beta, rm, rv, case["eps"], case["momentum"])
    y.backward(_t(dev, case["dy"]).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert len(tap) == 1 and tap[0]["z"] is None
    if with_bias:
        assert int(torch.count_nonzero(bias.grad)) == 0
    assert w.grad.shape == w.shape
    got = {"y": _nhwc(y), "mean": tap[0]["mean"].cpu().numpy(), "rstd": tap[0]["rstd"].cpu().numpy(),
           "running_mean": rm.cpu().numpy(), "running_var": rv.cpu().numpy(), "dw": w.grad.cpu().numpy(),
           "dgamma": gamma.grad.cpu().numpy(), "dbeta": beta.grad.cpu().numpy()}
    if input_grad:
        got["dx"] = x.grad.cpu().numpy()
    else:
        assert x.grad is None
    return got


@pytest.mark.parametrize("weight_cl", [False, True], ids=["w-contiguous", "w-channels_last"])
@pytest.mark.parametrize("input_grad", [False, True], ids=["no-dx", "dx"])
@pytest.mark.parametrize("shape", CONV0_CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_first_layer_passes_match_float64(dev, shape, input_grad, weight_cl):
    case, ref, yard = _conv0_case(shape)
    got = _run_conv0(dev, case, input_grad, weight_cl)
    pos, neg = R.zero_gamma_channels(shape[1])
    assert np.all(got["y"][..., pos] == F32(0.25)) and not got["y"][..., neg].any() and not got["dw"][[pos, neg]].any()
    assert got["dgamma"][neg] == 0 and got["dbeta"][neg] == 0
    _compare(f"conv0 {shape} dx={input_grad} w_cl={weight_cl}", got, ref, yard)
    if input_grad:                                        # the gather has a fixed order: the same bits on a second run
        again = _run_conv0(dev, case, True, weight_cl)
        assert np.array_equal(got["dx"].view(np.uint32), again["dx"].view(np.uint32))


@pytest.mark.parametrize("cin", [1, 2])
def test_first_layer_single_pixel_has_no_gradient(dev, cin):
    """B H W = 1: the pixel is its own mean, so dz = 0 exactly - dW = 0, dx = 0, dgamma = 0, dbeta = dy [beta > 0]."""
    case = R.make_conv0_case((cin, 8, 1, 1, 1))
    ref = R.reference(case)
    assert not ref["dz"].any() and not ref["dw"].any() and not ref["dx"].any()
    got = _run_conv0(dev, case, True, False)
    assert not got["dw"].any() and not got["dx"].any() and not got["dgamma"].any()
    _compare(f"conv0 single pixel cin={cin}", got, ref, R.errors(R.reference(case, F32), ref), True)


@pytest.mark.parametrize("shape", OFFSET_CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_first_layer_statistics_under_an_offset(dev, shape):
    """k_conv0_stats sums raw z and z^2 in float32 per thread.  x = 50 + 0.1 randn with weights in [0, 0.3] puts every channel's
    mean tens of its spread away from 0 (the zero border is what spreads z at all); the variance, the running estimates and y
    must survive that, within the bounds test_fused_bn_statistics_with_a_large_channel_offset sets for the generic passes."""
    cin, cout, b, h, w = shape
    rng = np.random.default_rng([11, cin, b])
    case = {"x": (50 + 0.1 * rng.standard_normal((b, cin, h, w))).astype(F32), "w": rng.uniform(0, 0.3, (cout, cin, 3, 3)).astype(F32),
            "gamma": rng.uniform(0.5, 1.5, cout).astype(F32), "beta": rng.uniform(-0.3, 0.3, cout).astype(F32),
            "bias": rng.uniform(-0.5, 0.5, cout).astype(F32), "rm": np.zeros(cout, F32), "rv": np.ones(cout, F32),
            "dy": rng.standard_normal((b, h, w, cout)).astype(F32), "eps": R.MODEL_EPS, "momentum": R.MODEL_MOMENTUM}
    y, mean, rstd, rm, rv = R.conv0_bn_relu(case["x"], case["w"], None, case["gamma"], case["beta"], case["rm"], case["rv"],
                                            case["eps"], case["momentum"])
    var = 1 / rstd ** 2 - case["eps"]
    ratio = np.abs(mean) / np.sqrt(var)
    print(f"conv0 offset {shape}: |mean| / sigma of z per channel: min {ratio.min():.2f}, median {np.median(ratio):.2f}, max {ratio.max():.2f}; "
          f"mean {np.abs(mean).min():.1f} .. {np.abs(mean).max():.1f}, sigma {np.sqrt(var).min():.2f} .. {np.sqrt(var).max():.2f}")
    assert ratio.min() >= 10       # the case stays hard: every channel's mean is 10 sigma or more from 0 (11.5 .. 17.0 as generated)
    got = _run_conv0(dev, case, False, False, with_bias=False)
    n = b * h * w
    inc = case["momentum"] * var * n / (n - 1)
    e_var = float(np.abs((got["running_var"].astype(F64) - rv) / inc).max())
    e_mean = float(np.abs(got["running_mean"].astype(F64) - rm).max())
    e_y = float(np.abs(got["y"].astype(F64) - y).max())
    print(f"conv0 offset {shape}: running_var increment off by {e_var:.2e} of itself (bound 2e-3), running_mean by {e_mean:.2e} "
          f"(bound {1e-6 + 1e-7 * np.abs(mean).max():.2e}), y by {e_y / np.abs(y).max():.2e} of its peak (bound 4e-3), "
          f"rstd by {float(np.abs(got['rstd'] / rstd - 1).max()):.2e} relative")
    assert e_var <= 2e-3
    assert e_mean <= 1e-6 + 1e-7 * float(np.abs(mean).max())
    assert e_y <= 4e-3 * float(np.abs(y).max())
