"""Reference form of the optimiser tail of the training step - adaptive gradient clipping per output unit, the optimiser's clipvalue
and ATen's Adam (ORIGINAL mode, no weight decay, no amsgrad) - as `iris_agc_clip` (csrc/k_elementwise.h) and `iris_agc_clip_adam`
(csrc/k_agc_adam.h) take it: a helper beside the tests, NumPy only.  Units are the rows of a [rows, len] table - the kernels' own
boundary, not torch tensors.  `dtype` = float64 is the definition, `dtype` = float32 the same lines with every operation rounded
to float32 (the yardstick: NumPy's own sums, no fused multiply-add).

    max_norm = max(||p_unit||, eps_agc) * clip_factor
    s        = 1                                    if ||g_unit|| < max_norm
             = max_norm / max(||g_unit||, 1e-6)     otherwise
    x        = clamp(s * g, -clipvalue, +clipvalue)                (clamp only when clipvalue > 0; p.grad holds x afterwards)
    m' = m + (x - m)(1 - beta1);    v' = beta2 v + (1 - beta2) x^2
    p' = p - (lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

The scalars are what the kernel is handed: clip_factor, eps_agc, clipvalue, eps and a host lr are rounded to float32 first, the
betas stay doubles (1 - beta^t, 1 - beta are formed in double and then rounded to `dtype`, as ATen does), t is the value of the
float32 counter AFTER its increment.  A NaN anywhere in a unit's gradient makes that unit's norm, its factor and so all of its x
NaN (max(NaN, 1e-6) is NaN here, as in torch.clamp and tf.maximum).

A case is {'name', 'groups', 'sc'}: `groups` is a list of {'p', 'g', 'm', 'v': float32 [rows, len], 'mis': {quantity: 0 | 1},
'packed'}; `mis` puts the rows of that quantity one float (4 bytes) behind a 16-byte boundary, `packed` lays the rows out back to
back as a parameter tensor does (otherwise every row stands alone between sentinels); `sc` holds the scalars.

The error rule (u = 2^-24), none of it fitted to a kernel:

    clip factor   |s - s64| <= (ceil(len / 64) + 16) u s64.  The sums of squares have non-negative terms; a lane adds
                  ceil(len / 64) of them and the wave tree 6 more levels, so the sum is off by at most (ceil(len / 64) + 7) u of
                  itself; each square root halves that and adds u / 2; the division, the max (1e-6 as a float is 0.42 u away from
                  1e-6) and the product with clip_factor add a handful of u.  In NumPy float32 in the kernels' summation order,
                  lengths 1 .. 2^20, 20 seeds each, the worst is 0.15 of this bound.
    x             |x - x64| <= (ceil(len / 64) + 18) u |s64 g| on every element, whichever side of the threshold or of the clamp
                  either evaluation lands on: s is continuous at the threshold and the clamp is 1-Lipschitz.  (The one jump of the
                  definition - max_norm <= ||g|| < 1e-6 against ||g|| < max_norm - is kept a factor 3 or more away by the generators.)
                  Without AGC (use_agc = 0) x = clamp(g) exactly.                                                      =: ex
    m'            |.| <= (1 - beta1) ex                                         + K_M u (|m| + (1 - beta1)(|x| + |m|))  =: bm
    v'            |.| <= (1 - beta2)(2 |x| + ex) ex                             + K_V u v'      (a sum of non-negative terms)
    p'            |.| <= step / denom bm + |dp| (sqrt(v') / bc2) / denom bv / (2 v') + K_P u (|p| + |dp|)
                  the first-order image of bm and bv under the last line (step = lr / (1 - beta1^t), denom its denominator,
                  dp = step m' / denom, bc2 = sqrt(1 - beta2^t)) plus the float32 operations of that line.

K_M, K_V, K_P are not read off the kernels: they come from two float32 evaluations over every case of tests/test_agc_gpu.py - this
file's lines in NumPy float32, and torch.optim.Adam (float32, CPU, single-tensor) fed the yardstick's x - as the smallest power of
two at or above four times the worse of the two worst excesses over the propagated part, in units of u x the scale above (the
convention of the pcen_learn gradient rule).  tests/test_agc_host.py re-derives them and holds the yardstick inside
every bound."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24

# derived by tests/test_agc_host.py::test_constants_come_from_the_two_float32_evaluations (worst excesses: see there and DESIGN.md)
K = {"m": 8, "v": 16, "p": 4}

SCALARS = {"clip_factor": 0.01, "eps_agc": 1e-3, "clipvalue": 1e-3, "use_agc": 1, "lr": 1e-3, "lr_dev": False,
           "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "t": 3.0}
QUANTITIES = ("x", "m", "v", "p")
LENGTHS = (1, 3, 9, 18, 32, 252, 256, 260, 288, 4608)
LONG = 70000                                  # several trips per lane on both paths (70,000 / 256 = 274, / 64 = 1094)
TWINS = (32, 256, 288)                        # one more row each, 4 bytes off 16-byte alignment: len % 4 == 0 on the scalar path
ROWLOOP = {"clip": 16384 + 5, "adam": 32768 + 5}     # rows of length 5: one more than the grid's waves (4096 x 4, 8192 x 4)
T_VALUES = (1.0, 2.0, 10.0, 1000.0, 100000.0)
BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.99))
EPS_VALUES = (1e-8, 1e-3)
EDGE_ROWS = ("zero_p", "p_below_floor", "p_above_floor", "zero_g", "tiny_g", "at_threshold", "far_above", "far_below", "at_clipvalue",
             "above", "below")


def scalars(**kw):
    return {**SCALARS, **kw}


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def _norm(a, dtype):
    return np.sqrt(np.sum(a * a, axis=1, keepdims=True, dtype=dtype)).astype(dtype)


def clip_factor_of(p, g, sc, dtype=F64):
    """s [rows, 1] of the units p, g [rows, len]."""
    p, g = np.asarray(p, dtype), np.asarray(g, dtype)
    if not sc["use_agc"]:
        return np.ones((p.shape[0], 1), dtype)
    max_norm = np.maximum(_norm(p, dtype), dtype(F32(sc["eps_agc"]))) * dtype(F32(sc["clip_factor"]))
    g_norm = _norm(g, dtype)
    with np.errstate(invalid="ignore"):
        return np.where(g_norm < max_norm, dtype(1), max_norm / np.maximum(g_norm, dtype(1e-6))).astype(dtype)


def launch(grp, sc, dtype=F64):
    """One launch on the group's rows -> {'s' [rows, 1], 'x', 'm', 'v', 'p' [rows, len]} in `dtype`."""
    p, g, m, v = (np.asarray(grp[k], dtype) for k in "pgmv")
    s = clip_factor_of(p, g, sc, dtype)
    x = s * g
    cv = dtype(F32(sc["clipvalue"]))
    if cv > 0:
        x = np.clip(x, -cv, cv)
    t, b1, b2 = float(sc["t"]), float(sc["beta1"]), float(sc["beta2"])
    bc1, bc2 = dtype(1.0 - b1 ** t), np.sqrt(dtype(1.0 - b2 ** t))
    step = dtype(F32(sc["lr"])) / bc1
    m2 = m + (x - m) * dtype(1.0 - b1)
    v2 = dtype(b2) * v + dtype(1.0 - b2) * x * x
    p2 = p - step * m2 / (np.sqrt(v2) / bc2 + dtype(F32(sc["eps"])))
    out = {"s": s, "x": x, "m": m2, "v": v2, "p": p2}
    assert all(a.dtype == dtype for a in out.values())
    return out


def reference(case, dtype=F64):
    return [launch(grp, case["sc"], dtype) for grp in case["groups"]]


# ---------------------------------------------------------------------------
# the error rule
# ---------------------------------------------------------------------------
def parts(grp, ref, sc):
    """{name: (propagated part, scale of the float32 operations of that line)} per element, from the float64 `ref` of the group."""
    p, g, m = (np.asarray(grp[k], F64) for k in "pgm")
    x, m2, v2 = ref["x"], ref["m"], ref["v"]
    ex = (math.ceil(p.shape[1] / 64) + 18) * U * np.abs(ref["s"] * g) if sc["use_agc"] else np.zeros_like(g)
    t, b1, b2 = float(sc["t"]), float(sc["beta1"]), float(sc["beta2"])
    bc2 = math.sqrt(1.0 - b2 ** t)
    step = float(F32(sc["lr"])) / (1.0 - b1 ** t)
    s_m = np.abs(m) + (1.0 - b1) * (np.abs(x) + np.abs(m))
    b_m = (1.0 - b1) * ex + K["m"] * U * s_m
    p_v = (1.0 - b2) * (2.0 * np.abs(x) + ex) * ex
    b_v = p_v + K["v"] * U * v2
    sv = np.sqrt(v2) / bc2
    denom = sv + float(F32(sc["eps"]))
    dp = step * m2 / denom
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_v = np.where(v2 > 0, b_v / (2.0 * v2), 0.0)
    p_p = step / denom * b_m + np.abs(dp) * sv / denom * rel_v
    return {"x": (ex, np.zeros_like(ex)), "m": ((1.0 - b1) * ex, s_m), "v": (p_v, v2), "p": (p_p, np.abs(p) + np.abs(dp))}


def bounds(grp, ref, sc):
    """{name: the largest |got - ref| per element} for x, m', v', p'."""
    return {name: part + (K[name] * U * scale if name in K else 0.0) for name, (part, scale) in parts(grp, ref, sc).items()}


def _ratio(err, lim):
    """err / lim per element; 0 / 0 = 0, anything else over 0 = inf.  Where the reference is NaN the caller has put inf or 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, np.where(lim > 0, err / lim, np.inf))


def _err(got, ref):
    """|got - ref| per element; where the reference is NaN: 0 if `got` is NaN too, inf otherwise; a non-finite `got` elsewhere: inf."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    nan = np.isnan(ref)
    err[nan] = np.where(np.isnan(got[nan]), 0.0, np.inf)
    err[~nan & ~np.isfinite(got)] = np.inf
    return err


def errors(got, ref, grp, sc):
    """{name: (worst |got - ref| / bound over the group's elements, worst |got - ref|)} over the names of `got`."""
    lim = bounds(grp, ref, sc)
    out = {}
    for name, a in got.items():
        err = _err(a, ref[name])
        finite = err[np.isfinite(err)]
        out[name] = (float(_ratio(err, np.nan_to_num(lim[name], nan=0.0)).max()), float(finite.max()) if finite.size else 0.0)
    return out


def excess(got, ref, grp, sc):
    """{name: worst (|got - ref| - propagated part)+ / (u scale)} for m', v', p': what K has to cover."""
    out = {}
    for name, (part, scale) in parts(grp, ref, sc).items():
        if name == "x" or name not in got:
            continue
        over = np.maximum(_err(got[name], ref[name]) - np.nan_to_num(part, nan=0.0), 0.0)
        out[name] = float(_ratio(over, U * np.nan_to_num(scale, nan=0.0)).max())
    return out


def pow2_at_or_above(v):
    return 1 if v <= 1 else 2 ** math.ceil(math.log2(v))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def _units(rng, ratios, length, sc, p_scale=0.05, zero_moments=False):
    """Rows whose ||g|| is ratios[r] x the unit's max_norm; p ~ p_scale N(0, 1); running moments (m ~ 3e-4, v ~ m^2) or zeros."""
    rows = len(ratios)
    p = (p_scale * rng.standard_normal((rows, length))).astype(F32)
    g = rng.standard_normal((rows, length))
    max_norm = np.maximum(_norm(p.astype(F64), F64), float(F32(sc["eps_agc"]))) * float(F32(sc["clip_factor"]))
    g = (g / _norm(g, F64) * np.asarray(ratios, F64)[:, None] * max_norm).astype(F32)
    if zero_moments:
        m, v = np.zeros_like(p), np.zeros_like(p)
    else:
        m = (3e-4 * rng.standard_normal((rows, length))).astype(F32)
        v = np.square(3e-4 * rng.standard_normal((rows, length))).astype(F32)
    return {"p": p, "g": g, "m": m, "v": v, "mis": {k: 0 for k in "pgmv"}, "packed": False}


def _twin(grp, **mis):
    return {**{k: grp[k].copy() for k in "pgmv"}, "mis": {**grp["mis"], **mis}, "packed": grp["packed"]}


def lengths_case(sc=None):
    """Every length of LENGTHS (three rows each: below, above and far above the threshold), two rows of LONG, then the twins: for
    32, 256 and 288 the same rows 4 bytes off alignment, and for 256 with only exp_avg / only exp_avg_sq off.  `twins`: [(group,
    group of its aligned twin)]."""
    sc = sc or scalars()
    rng = np.random.default_rng(1)
    groups = [_units(rng, (0.3, 3.0, 100.0), n, sc) for n in LENGTHS] + [_units(rng, (0.3, 30.0), LONG, sc)]
    twins = []
    for n in TWINS:
        twins.append((len(groups), LENGTHS.index(n)))
        groups.append(_twin(groups[LENGTHS.index(n)], p=1, g=1, m=1, v=1))
    for only in "mv":
        twins.append((len(groups), LENGTHS.index(256)))
        groups.append(_twin(groups[LENGTHS.index(256)], **{only: 1}))
    return {"name": "lengths", "groups": groups, "sc": sc, "twins": twins}


def rowloop_case(kind, sc=None):
    """ROWLOOP[kind] rows of length 5, packed; ratios 0.3 .. 3 and a marked row, third from the end, 1e3 above its clip norm."""
    sc = sc or scalars()
    n = ROWLOOP[kind]
    rng = np.random.default_rng([2, n])
    ratios = np.exp(rng.uniform(np.log(0.3), np.log(3.0), n))
    ratios[n - 3] = 1e3
    grp = _units(rng, ratios, 5, sc)
    grp["packed"] = True
    return {"name": f"rowloop-{kind}", "groups": [grp], "sc": sc, "marked": n - 3}


def edges_case(sc=None, nan=False):
    """The edges of the definition, one row each (EDGE_ROWS), at length 8 (float4 path) and 6 (scalar path)."""
    sc = sc or scalars()
    cf, floor, cv = float(F32(sc["clip_factor"])), float(F32(sc["eps_agc"])), float(F32(sc["clipvalue"])) or 1e-3
    groups = []
    for length in (8, 6):
        rng = np.random.default_rng([3, length])
        grp = _units(rng, (100.0, 3.0, 3.0, 1.0, 1.0, 1.0, 1e3, 1e-3, 1.0, 3.0, 0.3), length, sc)
        p, g = grp["p"].astype(F64), grp["g"].astype(F64)
        row = EDGE_ROWS.index
        p[row("zero_p")] = 0                                               # the eps_agc floor decides
        g[row("zero_p")] *= floor * cf * 100 / np.linalg.norm(g[row("zero_p")])
        for name, f in (("p_below_floor", 1 - 1e-3), ("p_above_floor", 1 + 1e-3)):
            p[row(name)] *= floor * f / np.linalg.norm(p[row(name)])
            g[row(name)] *= 3 * floor * max(f, 1) * cf / np.linalg.norm(g[row(name)])
        g[row("zero_g")] = 0
        p[row("tiny_g")] = 0                                               # ||g|| < 1e-6: below max_norm = eps_agc clip_factor (s = 1), or
        g[row("tiny_g")] *= 5e-7 / np.linalg.norm(g[row("tiny_g")])         # - with eps_agc = 1e-5 - five times above it, on the 1e-6 floor
        p[row("at_threshold")] = 0                                         # ||p|| = 0.5 and ||g|| = 0.5 clip_factor, both exact in float64
        p[row("at_threshold"), :4] = 0.25
        g[row("at_threshold")] = 0
        g[row("at_threshold"), :4] = 0.25 * cf
        p[row("at_clipvalue")] *= 200                                      # far below its threshold, elements at exactly +-clipvalue
        g[row("at_clipvalue")] = cv * rng.uniform(-2, 2, length)
        g[row("at_clipvalue"), :2] = (cv, -cv)
        grp["p"], grp["g"] = p.astype(F32), g.astype(F32)
        if nan:
            grp["g"][row("above"), 1] = np.nan
        groups.append(grp)
    case = {"name": "edges" + ("-nan" if nan else ""), "groups": groups, "sc": sc}
    # what the construction promises, on the float32 inputs
    for grp, ref in zip(groups, reference(case)):
        if sc["use_agc"] and not nan:
            s = ref["s"][:, 0]
            g_norm, p_norm = _norm(grp["g"].astype(F64), F64)[:, 0], _norm(grp["p"].astype(F64), F64)[:, 0]
            assert p_norm[EDGE_ROWS.index("p_below_floor")] < floor < p_norm[EDGE_ROWS.index("p_above_floor")]
            assert p_norm[EDGE_ROWS.index("at_threshold")] == 0.5 and g_norm[EDGE_ROWS.index("at_threshold")] == 0.5 * cf
            assert 4e-7 < g_norm[EDGE_ROWS.index("tiny_g")] < 6e-7
            assert all(s[EDGE_ROWS.index(k)] == 1 for k in ("zero_g", "far_below", "at_clipvalue", "below", "at_threshold"))
            assert all(s[EDGE_ROWS.index(k)] < 0.5 for k in ("zero_p", "p_below_floor", "p_above_floor", "far_above", "above"))
            assert (s[EDGE_ROWS.index("tiny_g")] == 1) == (floor * cf > 1e-6)
    return case


def constants_case(sc, zero_moments):
    """A short table (lengths 3, 32, 260, 1024; one unit below and one far above its threshold) for the sweep over t, betas, eps, lr."""
    rng = np.random.default_rng([4, int(zero_moments)])
    return {"name": f"constants-t{sc['t']:g}-b{sc['beta1']}-{sc['beta2']}-eps{sc['eps']}-{'dev' if sc['lr_dev'] else 'host'}lr"
                    + ("-first" if zero_moments else ""),
            "groups": [_units(rng, (0.3, 30.0), n, sc, zero_moments=zero_moments) for n in (3, 32, 260, 1024)], "sc": sc}


def constants_cases(betas):
    """Every t x eps x lr source for one pair of betas; moments that start at zero where t = 1 (a first step), running ones otherwise."""
    out = []
    for t in T_VALUES:
        for eps in EPS_VALUES:
            for lr_dev in (False, True):
                sc = scalars(t=t, beta1=betas[0], beta2=betas[1], eps=eps, lr_dev=lr_dev, lr=3e-4 if lr_dev else 1e-3)
                out.append(constants_case(sc, zero_moments=t == 1.0))
    return out


CHAIN_LRS = (1e-3, 1e-3, 3e-4, 1e-4)


def chain_start(name):
    """The running state consecutive launches start from: 'chain' (four launches, t = 7 .. 10) or 'capture' (three replays)."""
    rng = np.random.default_rng([5, len(name)])
    sc = scalars(t=7.0, lr_dev=name == "capture", eps=1e-7)
    return {"name": name, "groups": [_units(rng, (0.3, 3.0, 100.0), n, sc) for n in (3, 32, 260, 1024)], "sc": sc}


def chain_next(case, state, k):
    """Launch k (0-based) of a chain: the case whose p, m, v are `state` (a list of {'p', 'm', 'v'} per group: what launch k - 1 left
    behind, or None for the start), with a new gradient, the counter at 7 + k and the learning rate CHAIN_LRS[k]."""
    sc = {**case["sc"], "t": 7.0 + k, "lr": CHAIN_LRS[k]}
    groups = []
    for i, grp in enumerate(case["groups"]):
        rng = np.random.default_rng([6, k, i])
        new = {**grp}
        if state is not None:
            new.update({q: np.asarray(state[i][q], F32) for q in "pmv"})
        fresh = _units(rng, (3.0, 0.3, 30.0), grp["p"].shape[1], sc)
        scale = _norm(new["p"].astype(F64), F64) / _norm(fresh["p"].astype(F64), F64)
        new["g"] = (fresh["g"].astype(F64) * scale).astype(F32)
        groups.append(new)
    return {"name": f"{case['name']}-{k}", "groups": groups, "sc": sc}


def single_launch_cases():
    """Every case of tests/test_agc_gpu.py that is one launch from given inputs (the chains are walked by their tests)."""
    out = [lengths_case(), lengths_case(scalars(clipvalue=0.0)), rowloop_case("clip"), rowloop_case("adam")]
    for sc in EDGE_SCALARS.values():
        out.append(edges_case(sc))
    out.append(edges_case(nan=True))
    for betas in BETAS:
        out += constants_cases(betas)
    return out


EDGE_SCALARS = {"default": scalars(), "no-clipvalue": scalars(clipvalue=0.0), "no-agc": scalars(use_agc=0),
                "floor-1e-6": scalars(eps_agc=1e-5), "t1": scalars(t=1.0)}
