"""tests/conv_ref.py checked on the host: the float64 definition against torch's own float64 convolution, the float32 yardsticks
exact on every grid case, the constant K of the per-element rule re-measured from the yardsticks, the generators' premises, and
the restated host geometry (which shapes make a persistent workgroup take a second and a third work item)."""
import numpy as np
import pytest
import torch

import conv_ref as CR

ALL_Z_SHAPES = (CR.CASES + [s for s in CR.CASES_B3 if s not in CR.CASES] + [(b, h, w, 32, 32) for b, h, w in CR.C32_CASES] + [(b, h, w, cin, cout) for b, h, w, cin, cout in CR.SMALL_CASES])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 64), (1, 1, 1, 8, 64), (2, 4, 6, 2, 16), (3, 1, 9, 32, 32)])
def test_definition_matches_torch_float64(shape):
    case = CR.make_case("gauss", shape)
    x = _t(CR.nchw(case["x"])).requires_grad_(True)
    w = _t(case["w"]).requires_grad_(True)
    z = torch.nn.functional.conv2d(x, w, _t(case["bias"]), padding=1)
    for relu in (False, True):
        for pool in (False, True):
            want = torch.relu(z) if relu else z
            want = torch.nn.functional.max_pool2d(want, 2, 2, ceil_mode=True) if pool else want
            got = CR.conv3x3(case["x"], case["w"], case["bias"], relu, pool)
            assert np.abs(CR.nchw(got) - want.detach().numpy()).max() <= 1e-13 * max(1.0, float(want.detach().abs().max()))
    zb = torch.nn.functional.conv2d(x, w, None, padding=1)
    zb.backward(_t(CR.nchw(case["dz"])))
    assert np.abs(CR.nchw(CR.conv3x3_dx(case["dz"], case["w"])) - x.grad.numpy()).max() <= 1e-13 * float(x.grad.abs().max())
    assert np.abs(CR.conv3x3_dw(case["x"], case["dz"]) - w.grad.numpy()).max() <= 1e-13 * float(w.grad.abs().max())
    # cond bounds the sum it measures
    assert np.all(np.abs(CR.conv3x3(case["x"], case["w"], case["bias"])) <= CR.cond(case["x"], case["w"], case["bias"]) * (1 + 1e-12))


def test_a_nan_stays_in_the_definition():
    case = CR.make_case("gauss", (1, 5, 6, 8, 64))
    x = case["x"].copy()
    x[0, 2, 3, 5] = np.nan
    for relu in (False, True):
        z = CR.conv3x3(x, case["w"], case["bias"], relu, False)
        hit = np.zeros((1, 5, 6), bool)
        hit[0, 1:4, 2:5] = True
        assert np.isnan(z[hit]).all() and np.isfinite(z[~hit]).all()
        p = CR.conv3x3(x, case["w"], case["bias"], relu, True)
        assert np.isnan(p[0, 0:2, 1:3]).all() and np.isfinite(p[0, 2]).all() and np.isfinite(p[0, :, 0]).all()


@pytest.mark.parametrize("shape", ALL_Z_SHAPES)
def test_yardsticks_are_exact_on_the_grid(shape):
    """x, w, bias, dz on the grid: the direct and the Winograd form in float32 equal float64 bit for bit (so any summation order does)."""
    case = CR.make_case("grid", shape)
    x, w, bias, dz = case["x"], case["w"], case["bias"], case["dz"]
    for relu, pool in ((False, False), (True, False), (True, True)):
        ref = CR.conv3x3(x, w, bias, relu, pool)
        assert np.array_equal(CR.direct_f32(x, w, bias, relu, pool).astype(np.float64), ref)
        assert np.array_equal(CR.wino_f32(x, w, bias, relu, pool).astype(np.float64), ref)
    ref = CR.conv3x3_dx(dz, w)
    wt = CR.flip_transpose(w)
    assert np.array_equal(CR.direct_f32(dz, wt).astype(np.float64), ref) and np.array_equal(CR.wino_f32(dz, wt).astype(np.float64), ref)
    assert np.abs(ref).max() > 0 or shape[:3] == (1, 1, 1)


@pytest.mark.parametrize("shape", CR.WRW_CASES)
def test_weight_gradient_yardsticks_are_exact_on_the_grid(shape):
    case = CR.make_case("grid", shape)
    ref = CR.conv3x3_dw(case["x"], case["dz"])
    assert np.array_equal(CR.direct_dw_f32(case["x"], case["dz"]).astype(np.float64), ref)
    assert np.array_equal(CR.wino_dw_f32(case["x"], case["dz"]).astype(np.float64), ref)
    assert np.abs(ref).max() > 0


def test_bn_grid_keeps_the_epilogue_sums_exact():
    """The `bn` grid: 64 squares of (z - K), K any value of the channel, sum below 2^24 steps of 2^-8 - a lane's float32 partial sums
    of a `_bn` epilogue are exact, whichever of its values it takes as K."""
    for shape in CR.CASES + [(3, 5, 70, 32, 32)]:
        case = CR.make_case("grid", shape, bn=True)
        z = CR.conv3x3(case["x"], case["w"])
        span = (z.max(axis=(0, 1, 2)) - z.min(axis=(0, 1, 2))).max()
        assert 64 * span * span * 256 < 2 ** 24 and np.array_equal(z * 16, np.round(z * 16)), (shape, span)
        assert np.abs(z).max() > 0 or shape[:3] == (1, 1, 1)


def measure_yardsticks(verbose=False):
    worst = {"z": {"direct": 0.0, "wino": 0.0}, "dx": {"direct": 0.0, "wino": 0.0}, "dw": {"direct": 0.0, "wino": 0.0}}
    for kind in CR.CONTINUOUS:
        for shape in ALL_Z_SHAPES:
            case = CR.make_case(kind, shape)
            x, w, bias, dz = case["x"], case["w"], case["bias"], case["dz"]
            for relu, pool in ((False, False), (True, True)):
                ref, cnd = CR.conv3x3(x, w, bias, relu, pool), CR.cond(x, w, bias, pool)
                for name, fn in (("direct", CR.direct_f32), ("wino", CR.wino_f32)):
                    worst["z"][name] = max(worst["z"][name], CR.ratio(fn(x, w, bias, relu, pool), ref, cnd))
            wt = CR.flip_transpose(w)
            ref, cnd = CR.conv3x3_dx(dz, w), CR.cond_dx(dz, w)
            for name, fn in (("direct", CR.direct_f32), ("wino", CR.wino_f32)):
                worst["dx"][name] = max(worst["dx"][name], CR.ratio(fn(dz, wt), ref, cnd))
        for shape in CR.WRW_CASES:
            case = CR.make_case(kind, shape)
            ref, cnd = CR.conv3x3_dw(case["x"], case["dz"]), CR.cond_dw(case["x"], case["dz"])
            for name, fn in (("direct", CR.direct_dw_f32), ("wino", CR.wino_dw_f32)):
                worst["dw"][name] = max(worst["dw"][name], CR.ratio(fn(case["x"], case["dz"]), ref, cnd))
        if verbose:
            print(kind, {q: {n: round(v, 2) for n, v in d.items()} for q, d in worst.items()})
    return worst


def test_committed_K_is_four_times_the_yardstick():
    """K = 4x the worse yardstick's worst err / (2^-24 cond); the committed value must lie between 1x and 8x of what is measured here."""
    worst = measure_yardsticks()
    for name, per in worst.items():
        found = max(per.values())
        print(f"{name}: direct {per['direct']:.2f}  winograd {per['wino']:.2f}  committed yardstick {CR.YARDSTICK[name]}  K {CR.K[name]}")
        assert found > 0 and found <= CR.K[name] <= 8.0 * found, (name, per, CR.K[name])
        assert CR.K[name] == 4.0 * CR.YARDSTICK[name]


def test_generators_hold_their_premises():
    for kind in ("grid",) + CR.CONTINUOUS:
        for shape in CR.CASES[:4] + CR.WRW_CASES[:2]:
            case = CR.make_case(kind, shape)
            assert all(case[k].dtype == np.float32 and np.isfinite(case[k]).all() for k in ("x", "w", "bias", "dz"))
            again = CR.make_case(kind, shape)
            assert all(np.array_equal(case[k], again[k]) for k in ("x", "w", "bias", "dz"))       # seeded
    r = CR.make_case("ranged", (3, 5, 7, 24, 64))
    z = np.abs(CR.conv3x3(r["x"], r["w"])).max(axis=(0, 1, 2))
    assert z.max() / z.min() > 2.0 ** 20                      # small output channels beside large ones: a peak-relative bound sees only some
    o = CR.make_case("offset", (3, 5, 7, 24, 64))
    assert o["x"].mean() > 10 * o["x"].std()
    a = CR.make_case("relu_like", (3, 5, 41, 16, 64))
    assert a["x"].min() == 0.0 and 0.4 < (a["x"] == 0).mean() < 0.65
    g = CR.make_case("grid", (1, 5, 6, 512, 64))
    assert g["k_range"][0] >= 1 and np.abs(g["x"]).max() <= 2.0 and np.abs(g["w"]).max() <= 1.5
    assert np.array_equal(CR.unchunked(CR.chunked(g["x"])), g["x"])


def _cu_counts():
    counts = [256, 64, 104, 228, 304]
    if torch.cuda.is_available():
        counts.append(torch.cuda.get_device_properties(0).multi_processor_count)
    return sorted(set(counts))


@pytest.mark.parametrize("cus", _cu_counts())
def test_looping_shapes_loop(cus):
    """The restated geometry of csrc/host_wino.h and csrc/k_conv_c32.h, and the batches at which every workgroup of the persistent grid
    takes two work items and some take three."""
    assert CR.wino_geometry(3, 4, 32, 512)["n_work"] == 2 * 1 * 8 and CR.wino_geometry(2, 40, 256, 64)["n_work"] == 40 * 2 * 1
    assert [CR.wino_geometry(1, 5, w, 64)["tc"] for w in (5, 32, 33, 40, 64, 65, 70, 200)] == [16, 16, 32, 32, 32, 64, 64, 64]
    assert CR.c32_geometry(4, 64, 512)["n_tiles"] == 512 and CR.c32_geometry(1, 5, 70)["n_tiles"] == 4
    for w, tc in ((5, 16), (40, 32), (70, 64)):
        b = CR.looping_batch(5, w, 64, cus)
        geo = CR.wino_geometry(b, 5, w, 64, cus)
        assert geo["tc"] == tc and geo["tr"] == 64 // tc and geo["grid"] == cus and geo["n_work"] >= 2 * cus + 3
        assert CR.wino_geometry(b - 1, 5, w, 64, cus)["n_work"] < 2 * cus + 3
        assert geo["th"] % geo["tr"] or tc == 64                       # a block's tile rows straddle images
    b = CR.looping_batch_c32(3, 7, cus)
    geo = CR.c32_geometry(b, 3, 7, cus)
    assert b >= 2 * cus + 5 and geo["grid"] == 2 * cus and geo["n_tiles"] >= 2 * geo["grid"] + 3


if __name__ == "__main__":
    measure_yardsticks(verbose=True)
