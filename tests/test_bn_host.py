"""CPU tests of the BatchNorm + ReLU (+ MaxPool) references (tests/bn_ref.py; the kernels are the iris_bn_* passes of
csrc/k_elementwise.h and the iris_conv0_* passes of csrc/k_conv0_bn.h): the float64 definition against torch.double autograd
(conv2d, batch_norm(training=True), relu, max_pool2d(2, 2, ceil_mode=True)) for every case of tests/test_bn_gpu.py, the margins and
the share of tied windows the input generators promise, and the float32 yardstick.

The yardstick is `bn_ref.reference(case, float32)` - the definition's own lines in NumPy float32 - against float64, in units of
max|ref| + 0.05 per tensor (the shape of the ceiling 2e-5 max|ref| + 1e-6; running statistics: absolute), worst over BN_CASES +
CONV0_CASES.  Measured (bn_ref.YARDSTICK holds these figures with a fifth of headroom; `test_yardstick_is_what_is_committed`
re-measures them):

    y 1.7e-7   mean 4.5e-8   rstd 1.9e-7   dz 3.5e-6   dgamma 3.7e-7   dbeta 2.6e-7   dW 3.3e-6   dx 8.2e-6
    running_mean 5.2e-8 (absolute)   running_var 6.0e-7 (absolute)

dz, dW and dx are worst on the two-row cases ((1, 1, 2, 4) pooled, first layer (1, 8, 1, 1, 2)): with two rows the gradient cancels
down to eps / (delta^2 + eps) of its terms a g, and what is left of the terms' rounding is measured against that small remainder."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import bn_ref as R
from bn_ref import BN_CASES, CONV0_CASES, F64

EXTRA_BN = [((3, 9, 7, 64), False, R.MODEL_EPS, R.MODEL_MOMENTUM), ((3, 9, 7, 64), True, R.MODEL_EPS, R.MODEL_MOMENTUM)]
ALL_BN = [(s, p, R.EPS, R.MOMENTUM) for s, p in BN_CASES] + EXTRA_BN
_YARD = {}


def _close(got, ref, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, peak = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= 1e-12 * peak + 1e-13, (what, err, peak)


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64))).requires_grad_(grad)


def _torch_side(case, z_or_x, weight=None):
    """torch.double autograd of the same layer -> the quantities of bn_ref.reference (without mean / rstd)."""
    gamma, beta, bias = _t(case["gamma"], True), _t(case["beta"], True), _t(case["bias"])
    rm, rv = _t(case["rm"]), _t(case["rv"])
    inp = z_or_x.requires_grad_(True)
    if weight is not None:
        z = TF.conv2d(inp, weight, bias, padding=1)
    else:
        z = inp + bias.view(1, -1, 1, 1)
    y = torch.relu(TF.batch_norm(z, rm, rv, gamma, beta, training=True, momentum=case["momentum"], eps=case["eps"]))
    if case.get("pool"):
        y = TF.max_pool2d(y, 2, 2, ceil_mode=True)
    y.backward(_t(case["dy"]).permute(0, 3, 1, 2))
    return {"y": y.detach().permute(0, 2, 3, 1).numpy(), "running_mean": rm.numpy(), "running_var": rv.numpy(),
            "dgamma": gamma.grad.numpy(), "dbeta": beta.grad.numpy()}, inp.grad


def _check_generator(case):
    """The generator has asserted its margins and tie shares (bn_ref.make_bn_case); here they are printed."""
    if not case.get("pool"):
        return
    total, positive, n = R.tie_shares(case)
    print(f"  tied windows: {100 * total:.1f} % of {n} (maximum > 0: {100 * positive:.1f} %), margin >= {case['min_margin']:.3g}")
    assert n == 0 or total >= 0.10


def _bn(key):
    shape, pool, eps, momentum = key
    case = R.make_bn_case(shape, pool, eps, momentum)
    ref = R.reference(case)
    _YARD[("bn",) + key] = R.yardstick(case, ref)
    return case, ref


def _conv0(shape):
    case = R.make_conv0_case(shape)
    ref = R.reference(case)
    _YARD[("conv0",) + shape] = R.yardstick(case, ref)
    return case, ref


@pytest.mark.parametrize("key", ALL_BN, ids=lambda k: "-".join(str(v) for v in k[0]) + ("-pool" if k[1] else "") + f"-{k[2]}")
def test_definition_is_torch_double_autograd(key):
    case, ref = _bn(key)
    _check_generator(case)
    b, h, w, c = key[0]
    pos, neg = R.zero_gamma_channels(c)
    # the gamma = 0 channels by their closed form: y = relu(beta), dz = 0, dgamma != 0
    assert np.all(ref["y"][..., pos] == 0.25) and np.all(ref["y"][..., neg] == 0) and not ref["dz"][..., [pos, neg]].any()
    assert ref["dgamma"][neg] == 0 and ref["dbeta"][neg] == 0
    if np.ptp(case["z"][..., pos]) > 0:
        assert ref["dgamma"][pos] != 0
    if b * h * w == 1:
        # torch refuses a single value per channel: y = relu(beta), dz = 0, the variance estimate decays
        assert np.array_equal(ref["y"].reshape(-1), np.maximum(case["beta"].astype(F64), 0)) and not ref["dz"].any()
        _close(ref["running_var"], (1 - case["momentum"]) * case["rv"].astype(F64), "running_var")
        _close(ref["running_mean"], (1 - case["momentum"]) * case["rm"].astype(F64)
               + case["momentum"] * (case["z"].reshape(-1).astype(F64) + case["bias"]), "running_mean")
        _close(ref["dbeta"], np.where(case["beta"] > 0, case["dy"].reshape(-1), 0), "dbeta")
        assert not ref["dgamma"].any()
        return
    want, dz = _torch_side(case, _t(case["z"]).permute(0, 3, 1, 2))
    for name, v in want.items():
        _close(ref[name], v, (key, name))
    _close(ref["dz"], dz.permute(0, 2, 3, 1).numpy(), (key, "dz"))
    # without a convolution bias only the running mean moves
    rm, rv = R.running_stats(ref["mean"], 1 / ref["rstd"] ** 2 - case["eps"], b * h * w, None, case["rm"], case["rv"], case["momentum"])
    _close(rm, ref["running_mean"] - case["momentum"] * case["bias"].astype(F64), "running_mean without bias")
    _close(rv, ref["running_var"], "running_var")


@pytest.mark.parametrize("shape", CONV0_CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_first_layer_definition_is_torch_double_autograd(shape):
    case, ref = _conv0(shape)
    weight = _t(case["w"], True)
    want, dx = _torch_side(case, _t(case["x"]), weight)
    for name, v in want.items():
        _close(ref[name], v, (shape, name))
    _close(ref["dw"], weight.grad.numpy(), (shape, "dw"))
    _close(ref["dx"], dx.numpy(), (shape, "dx"))
    pos, neg = R.zero_gamma_channels(shape[1])
    assert np.all(ref["y"][..., pos] == 0.25) and np.all(ref["y"][..., neg] == 0) and not ref["dz"][..., [pos, neg]].any()
    assert not ref["dw"][[pos, neg]].any()


def test_first_maximum_and_zero_rules_on_a_hand_made_window():
    """One 3 x 3 image, one float4 of channels: ties at a positive maximum go to the first element in (h, w) order, a window whose
    maximum is 0 passes nothing, gamma < 0 turns the order of z around, edge windows have two elements / one."""
    z = np.zeros((1, 3, 3, 4))
    z[0, :, :, 0] = [[1, 2, 0], [2, 1, 0], [0, 0, 0]]       # gamma > 0: the two 2s tie, (0, 1) is first
    z[0, :, :, 1] = [[1, 2, 0], [2, 1, 0], [0, 0, 0]]       # gamma < 0: the two 1s tie, (0, 0) is first
    z[0, :, :, 2] = [[-1, -2, 0], [-2, -1, 0], [0, 0, 0]]   # all below the threshold: maximum 0, no gradient
    z[0, :, :, 3] = [[3, 3, 3], [3, 3, 3], [3, 3, 3]]       # constant channel: everything ties
    gamma = np.array([1.0, -1.0, 1.0, 1.0])
    mean, _, rstd = R.batch_stats(z, 0.0 + 1e-5)
    beta = np.array([-rstd[0] * (1.5 - mean[0]), rstd[1] * (1.5 - mean[1]), -rstd[2] * (0.5 - mean[2]), 0.25])
    dp = np.arange(1.0, 17.0).reshape(1, 2, 2, 4)
    dz, dgamma, dbeta = R.bn_relu_backward(z, dp, gamma, beta, 1e-5, True)
    a = gamma * rstd
    g = (dz - (-a * rstd * dgamma / 9) * z - (-a * dbeta / 9 + a * rstd * dgamma / 9 * mean)) / a     # dz = a g + b z + d, solved for g
    g = np.round(g, 9)
    want = np.zeros((1, 3, 3, 4))
    want[0, 0, 1, 0] = dp[0, 0, 0, 0]                         # first of the tied 2s; the other windows of channel 0 are below 1.5
    want[0, 0, 0, 1], want[0, 0, 2, 1], want[0, 2, 0, 1], want[0, 2, 2, 1] = dp[0, :, :, 1].reshape(-1)   # z < 1.5 wins: first 1, then the 0s
    want[0, 0, 0, 3], want[0, 0, 2, 3], want[0, 2, 0, 3], want[0, 2, 2, 3] = dp[0, :, :, 3].reshape(-1)   # all tie: the first of each window
    assert np.array_equal(g, want), g[0, :, :, 1]
    assert np.array_equal(dbeta, want.sum(axis=(0, 1, 2))) and dgamma[3] == 0
    y = R.bn_relu(z, None, gamma, beta, np.zeros(4), np.ones(4), 1e-5, 0.1, True)[0]
    assert y.shape == (1, 2, 2, 4) and np.all(y[..., 2] == 0) and np.all(y[..., 3] == 0.25) and y[0, 0, 0, 0] > 0 and y[0, 1, 1, 0] == 0


def test_yardstick_is_what_is_committed():
    """The float32 evaluation's worst error per quantity over the case list = bn_ref.YARDSTICK (at most that, and at least a third of it)."""
    for key in ALL_BN:
        if ("bn",) + key not in _YARD:
            _bn(key)
    for shape in CONV0_CASES:
        if ("conv0",) + shape not in _YARD:
            _conv0(shape)
    worst = {}
    for key, yard in _YARD.items():
        for name, v in yard.items():
            if v > worst.get(name, (-1.0, None))[0]:
                worst[name] = (v, key)
    for name, (v, key) in sorted(worst.items()):
        print(f"float32 yardstick {name}: {v:.3e} at {key} (committed {R.YARDSTICK[name]:.3e})")
    for name, (v, _) in worst.items():
        assert R.YARDSTICK[name] / 3 <= v <= R.YARDSTICK[name], (name, v, R.YARDSTICK[name])
