"""CPU tests of the optimiser tail's reference (tests/agc_ref.py; the kernels are iris_agc_clip of csrc/k_elementwise.h and
iris_agc_clip_adam of csrc/k_agc_adam.h): the float64 definition against `hip_autograd.adaptive_clip_grad` on float64 tensors and
against torch.optim.Adam (single-tensor, float64) at 1e-13, the unit partition `FusedAGC._rows_of` makes of the v9, v8 and v1
models against `unitwise_norm`'s axes, and the error rule: the constants K_M, K_V, K_P re-derived from the two float32 evaluations
(this file's lines in NumPy float32; torch.optim.Adam in float32 fed the yardstick's x) over every case of tests/test_agc_gpu.py,
and the yardstick held inside every bound.

Measured here (worst over the 77 launches of the GPU file; `test_constants_come_from_the_two_float32_evaluations` prints them):

    x   NumPy float32 0.24 of its bound (its own pairwise sums; in the kernels' summation order the clip factor reads 0.12 of its bound)
    excess over the propagated part, in u x scale:   m' 1.05 | 1.05   v' 2.14 | 2.17   p' 0.99 | 0.99   (NumPy float32 | torch float32)
    -> K_M = 8, K_V = 16, K_P = 4; against the bounds so made the two evaluations read at most m' 0.18, v' 0.16, p' 0.25"""
import numpy as np
import pytest
import torch

import agc_ref as R
from agc_ref import F32, F64

_WORST = {}


def _rel(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)


# ---------------------------------------------------------------------------
# the definition against its two torch restatements
# ---------------------------------------------------------------------------
def _rows(t):
    """A parameter-shaped tensor -> NumPy [units, len] in the order of its memory (the kernels' rows)."""
    from challenge_amd.hip_autograd import FusedAGC
    rows, length = FusedAGC._rows_of(t)
    if t.dim() == 4 and not t.is_contiguous():
        t = t.permute(0, 2, 3, 1)
    return t.detach().contiguous().numpy().reshape(rows, length)


PARAM_SHAPES = [((16, 8, 3, 3), False), ((16, 8, 3, 3), True), ((32, 1, 3, 3), True), ((12, 40), False), ((7,), False), ((1,), False)]


@pytest.mark.parametrize("shape,channels_last", PARAM_SHAPES, ids=lambda v: str(v))
def test_definition_is_adaptive_clip_grad_in_float64(shape, channels_last):
    from challenge_amd.hip_autograd import adaptive_clip_grad
    rng = np.random.default_rng([7, len(shape), int(channels_last)])
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    p = torch.from_numpy(0.05 * rng.standard_normal(shape)).contiguous(memory_format=fmt)
    units = shape[0] if len(shape) > 1 else 1
    # per unit: far above, above, at about, below its threshold; one unit under the eps_agc floor, one with a tiny gradient
    scale = 10.0 ** rng.integers(-7, 1, units).reshape((units,) + (1,) * (len(shape) - 1))
    g = torch.from_numpy(rng.standard_normal(shape) * scale).contiguous(memory_format=fmt)
    if len(shape) > 1:
        with torch.no_grad():
            p[0] *= 1e-4
            g[1] *= 1e-9
    sc = R.scalars()
    cf, floor = float(F32(sc["clip_factor"])), float(F32(sc["eps_agc"]))
    want = adaptive_clip_grad([p], [g], cf, floor)[0]
    assert want.dtype == torch.float64
    s = R.clip_factor_of(_rows(p), _rows(g), sc)
    assert 0 < int((s == 1).sum()) < units or units == 1
    assert _rel(s * _rows(g), _rows(want)) <= 1e-13


def test_definition_is_torch_adam_in_float64():
    """Five steps, three parameters with counters 0, 3 and 40 at the start, betas (0.8, 0.95), the learning rate changed after the
    second step; clipvalue as the optimiser's clamp in front of it."""
    rng = np.random.default_rng(8)
    shapes, t0 = [(6, 5, 3, 3), (9, 20), (11,)], [0.0, 3.0, 40.0]
    sc = R.scalars(beta1=0.8, beta2=0.95, eps=1e-7, use_agc=0)
    lr, eps, cv = (float(F32(sc[k])) for k in ("lr", "eps", "clipvalue"))
    params = [torch.from_numpy(0.05 * rng.standard_normal(s)).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam(params, lr=lr, betas=(0.8, 0.95), eps=eps, foreach=False, fused=False)
    for p, t in zip(params, t0):
        opt.state[p] = {"step": torch.tensor(t, dtype=torch.float32), "exp_avg": torch.from_numpy(3e-4 * rng.standard_normal(p.shape)),
                        "exp_avg_sq": torch.from_numpy(np.square(3e-4 * rng.standard_normal(p.shape)))}
    mine = [{"p": p.detach().numpy().reshape(1, -1).copy(), "m": opt.state[p]["exp_avg"].numpy().reshape(1, -1).copy(),
             "v": opt.state[p]["exp_avg_sq"].numpy().reshape(1, -1).copy()} for p in params]
    for k in range(5):
        if k == 2:
            lr = float(F32(3e-4))
            opt.param_groups[0]["lr"] = lr
        for i, p in enumerate(params):
            g = 2e-3 * rng.standard_normal(p.shape)
            p.grad = torch.from_numpy(g).clamp_(-cv, cv)
            out = R.launch({**mine[i], "g": g.reshape(1, -1)}, {**sc, "lr": lr, "t": t0[i] + k + 1})
            assert np.array_equal(out["x"].reshape(p.shape), p.grad.numpy())
            mine[i] = {"p": out["p"], "m": out["m"], "v": out["v"]}
        opt.step()
        for i, p in enumerate(params):
            st = opt.state[p]
            assert float(st["step"]) == t0[i] + k + 1
            assert _rel(mine[i]["m"].reshape(p.shape), st["exp_avg"].numpy()) <= 1e-13, (k, i)
            assert _rel(mine[i]["v"].reshape(p.shape), st["exp_avg_sq"].numpy()) <= 1e-13, (k, i)
            assert _rel(mine[i]["p"].reshape(p.shape), p.detach().numpy()) <= 1e-13, (k, i)


def test_clip_factor_and_clamp_by_hand():
    """p = (3, 4) / 10, g = (0.6, 0.8): max_norm = 0.5 clip_factor, s = max_norm; eps_agc floor; the 1e-6 floor; NaN fills its unit."""
    sc = R.scalars(clip_factor=0.5, eps_agc=0.25, clipvalue=0.125)
    p = np.array([[0.3, 0.4], [0.03, 0.04], [0.3, 0.4], [0.0, 0.0], [0.3, 0.4]])
    g = np.array([[0.6, 0.8], [0.6, 0.8], [0.06, 0.08], [3e-7, 4e-7], [np.nan, 1.0]])
    s = R.clip_factor_of(p, g, sc)[:, 0]
    assert np.allclose(s[:4], [0.25, 0.125, 1.0, 1.0], rtol=1e-15) and np.isnan(s[4])
    assert R.clip_factor_of(p, g, R.scalars(clip_factor=0.5, eps_agc=1e-6))[3, 0] == float(F32(1e-6)) * 0.5 / 1e-6   # ||g|| = 5e-7: on the 1e-6 floor
    out = R.launch({"p": p, "g": g, "m": np.zeros_like(p), "v": np.zeros_like(p)}, sc)
    assert np.allclose(out["x"][:4], [[0.125, 0.125], [0.075, 0.1], [0.06, 0.08], [3e-7, 4e-7]], rtol=1e-15) and np.isnan(out["x"][4]).all()
    assert np.isnan(out["p"][4]).all() and np.isfinite(out["p"][:4]).all()


# ---------------------------------------------------------------------------
# the partition into units
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("v", ["9", "8", "1"])
def test_rows_are_the_reference_units(v):
    """`FusedAGC._rows_of` against `unitwise_norm`'s axes for every parameter of the model, channels_last as it trains: a row is one
    output unit, its elements are one contiguous run of the parameter's memory, and every element belongs to exactly one row.  (What
    `_build` makes of the rows - the device table - is checked where there is a device: tests/test_agc_gpu.py.)"""
    from challenge_amd import sj_train as S
    from challenge_amd.hip_autograd import FusedAGC
    from challenge_amd.utils import unitwise_norm
    cfg = S.ARGS().get(['--v', v, '--n_mels', '32', '--n_frame', '64', '--n_chan', '2', '--batch_size', '4'])
    torch.manual_seed(1)
    model = S.get_model(cfg).to(memory_format=torch.channels_last)
    dims = set()
    for name, p in model.named_parameters():
        rows, length = FusedAGC._rows_of(p)
        norm = unitwise_norm(p.detach())
        assert norm.numel() == rows and rows * length == p.numel(), name
        dims.add(p.dim())
        # element -> offset in the parameter's memory; row r must own exactly [r len, (r + 1) len)
        offs = torch.zeros(p.shape, dtype=torch.int64)
        for d in range(p.dim()):
            shape = [1] * p.dim()
            shape[d] = p.shape[d]
            offs = offs + torch.arange(p.shape[d]).view(shape) * p.stride(d)
        assert sorted(offs.reshape(-1).tolist()) == list(range(p.numel())), name           # dense: every element once
        unit = offs.reshape(rows, -1) if p.dim() > 1 else offs.reshape(1, -1)               # unit = index along axis 0 (or all of a 1-D tensor)
        assert torch.equal(unit.sort(dim=1).values, torch.arange(p.numel()).view(rows, length)), name
        # and the norm of that run of memory is the reference's norm of the unit
        flat = p.detach().double().as_strided((p.numel(),), (1,))
        mine = np.sqrt(np.square(flat.numpy().reshape(rows, length)).sum(axis=1))
        assert _rel(mine, norm.double().reshape(-1).numpy()) <= 1e-6, name
    assert dims == {1, 2, 4}


# ---------------------------------------------------------------------------
# the error rule
# ---------------------------------------------------------------------------
def _torch_float32_adam(grp, x, sc):
    """torch.optim.Adam (float32, CPU, single-tensor) on the group, fed the yardstick's x -> {'m', 'v', 'p'}."""
    p = torch.from_numpy(grp["p"].copy()).requires_grad_(True)
    p.grad = torch.from_numpy(np.ascontiguousarray(x, F32).copy())
    opt = torch.optim.Adam([p], lr=float(F32(sc["lr"])), betas=(sc["beta1"], sc["beta2"]), eps=float(F32(sc["eps"])), foreach=False, fused=False)
    opt.state[p] = {"step": torch.tensor(sc["t"] - 1.0, dtype=torch.float32), "exp_avg": torch.from_numpy(grp["m"].copy()),
                    "exp_avg_sq": torch.from_numpy(grp["v"].copy())}
    opt.step()
    return {"m": opt.state[p]["exp_avg"].numpy(), "v": opt.state[p]["exp_avg_sq"].numpy(), "p": p.detach().numpy()}


def _measure(case):
    """Both float32 evaluations of one case against its float64 reference: the bounds hold, the worst figures are kept."""
    ref = R.reference(case)
    yard = R.reference(case, F32)
    for grp, r, y in zip(case["groups"], ref, yard):
        got = {k: y[k] for k in R.QUANTITIES}
        tch = _torch_float32_adam(grp, y["x"], case["sc"])
        for who, ev in (("numpy", got), ("torch", tch)):
            for name, (ratio, _) in R.errors(ev, r, grp, case["sc"]).items():
                assert ratio <= 1.0, (case["name"], who, name, ratio)
                key = (who, name, "bound")
                _WORST[key] = max(_WORST.get(key, (0.0, "")), (ratio, case["name"]))
            for name, over in R.excess(ev, r, grp, case["sc"]).items():
                key = (who, name, "excess")
                _WORST[key] = max(_WORST.get(key, (0.0, "")), (over, case["name"]))
    return yard


def _all_cases():
    yield from R.single_launch_cases()
    for name, n in (("chain", 4), ("capture", 3)):
        start, state = R.chain_start(name), None
        for k in range(n):
            case = R.chain_next(start, state, k)
            yard = R.reference(case, F32)
            yield case
            state = [{q: y[q] for q in "pmv"} for y in yard]


def test_constants_come_from_the_two_float32_evaluations():
    """Every case of tests/test_agc_gpu.py: the float32 yardstick and torch's float32 Adam stay inside every bound, and K = the
    smallest power of two at or above four times the worse worst excess, per quantity - what agc_ref.K holds."""
    n = 0
    for case in _all_cases():
        _measure(case)
        n += 1
    for key in sorted(_WORST):
        print(f"{key[0]:5s} {key[1]} {key[2]:6s}: {_WORST[key][0]:.3f} at {_WORST[key][1]}")
    print(f"{n} cases")
    for name in ("m", "v", "p"):
        worst = max(_WORST[("numpy", name, "excess")][0], _WORST[("torch", name, "excess")][0])
        assert R.K[name] == R.pow2_at_or_above(4.0 * worst), (name, worst, R.K[name])


def test_clip_factor_bound_in_the_kernels_summation_order():
    """|s - s64| <= (ceil(len / 64) + 16) u s64 for float32 sums in the kernels' order (a lane's running sum over its stride, then the
    wave tree), both paths, lengths up to 2^16 here (2^20 x 20 seeds when the rule was set: 0.15)."""
    worst = 0.0
    for length in (1, 3, 18, 64, 260, 4608, 65536):
        for seed in range(3):
            rng = np.random.default_rng([9, length, seed])
            p, g = (0.05 * rng.standard_normal(length)).astype(F32), rng.standard_normal(length).astype(F32)
            sc = R.scalars()
            s64 = float(R.clip_factor_of(p[None], g[None], sc)[0, 0])
            for width in ((4, 1) if length % 4 == 0 else (1,)):
                norms = []
                for a in (p, g):
                    sq = np.zeros(-(-length // (64 * width)) * 64 * width, F32)
                    sq[:length] = a * a
                    sq = sq.reshape(-1, 64, width)
                    lane = np.zeros(64, F32)
                    for chunk in sq:                     # one trip of the lane loop
                        part = chunk[:, 0]
                        for j in range(1, width):
                            part = (part + chunk[:, j]).astype(F32)
                        lane = (lane + part).astype(F32)
                    while lane.size > 1:                 # the wave tree
                        lane = (lane[0::2] + lane[1::2]).astype(F32)
                    norms.append(np.sqrt(lane[0]))
                max_norm = F32(max(norms[0], F32(sc["eps_agc"])) * F32(sc["clip_factor"]))
                s = 1.0 if norms[1] < max_norm else float(F32(max_norm / max(norms[1], F32(1e-6))))
                worst = max(worst, abs(s - s64) / ((-(-length // 64) + 16) * R.U * s64))
    print(f"clip factor in the kernels' order: worst {worst:.3f} of the bound")
    assert worst <= 1.0
