"""Reference form of the optimiser tail for `--optimizer sgd` and `--optimizer rmsprop` - adaptive gradient clipping per output unit,
the optimiser's clipvalue, then torch.optim.SGD / torch.optim.RMSprop with momentum, then (optionally) the weight EMA - as
`iris_agc_clip_sgd`, `iris_agc_clip_rmsprop` and their `_ema` siblings (csrc/k_agc_optim.h) take it: tests/agc_ref.py's definition
of x, its groups and its cases, with the state rows read as these optimisers read them.  NumPy only.

    x  = clamp(s g, +-clipvalue)                                  agc_ref: s the unit's clip factor; p.grad holds x afterwards
    sgd      b' = mu b + x                                        p' = p - lr b'
    rmsprop  s' = alpha s + (1 - alpha) x x;  a = sqrt(s') + eps
             b' = mu b + x / a                                    p' = p - lr b'
    ema      e' = e + (p' - e) w,  w = (float)(1 - min(decay, (1 + t) / (10 + t)))      ema_ref's weight: float32 in every evaluation

A group is agc_ref's: 'p', 'g', 'm' (the momentum buffer b), 'v' (rmsprop's square average s; sgd never reads it), with the EMA also
'e'; the quantities that come back are x, m (= b'), v (= s', rmsprop only), p and e.  `sc` is agc_ref's scalars plus 'kind'
('sgd' | 'rmsprop'), 'mu', 'alpha' and - with the EMA - 'decay'; 'eps' is rmsprop's.  lr, eps, clip_factor, eps_agc and clipvalue are
rounded to float32 first (what the entry points are handed); mu and alpha stay doubles, 1 - alpha is formed in double and then
rounded to `dtype`, as agc_ref keeps Adam's betas.  t is only the EMA's counter: neither update has a bias correction.

The error rule (u = 2^-24), by agc_ref's method - the bound on x propagated to first order through the definition, plus K u times the
scale of the line's own float32 operations:

    x    ex = (ceil(len / 64) + 18) u |s64 g|                      agc_ref's; 0 without AGC
    s'   |.| <= (1 - alpha)(2 |x| + ex) ex                       + K_S u s'                             =: bs
    b'   sgd:      |.| <= ex                                     + K_B u (|mu b| + |x|)                 =: bb
         rmsprop:  |.| <= ex / a + |x| da / a^2                  + K_B u (|mu b| + |x / a|)             da = bs / (2 sqrt(s')), 0 at s' = 0
    p'   |.| <= lr bb                                            + K_P u (|p| + |lr b'|)                =: bp
    e'   |.| <= w bp + K_E u (|e| + w (|p'| + |e|))                                                     ema_ref's rule and K_E

(At s' = 0 the unit's x is 0, so is ex, and a = eps exactly: the derivative of the root is never needed there.)  The constants are
not read off the kernels: over every case of tests/test_optim_gpu.py, this file's lines in NumPy float32 and torch.optim.SGD /
torch.optim.RMSprop (float32, CPU, single-tensor) fed the yardstick's x are both held to the propagated part; K is the smallest
power of two at or above four times the worse of the two worst excesses, in units of u x the scale.  tests/test_optim_host.py
re-derives them and holds both evaluations inside every bound."""
import math

import numpy as np

import agc_ref as R
import ema_ref as E
from agc_ref import F32, F64, U

KINDS = ("sgd", "rmsprop")
# derived by tests/test_optim_host.py::test_constants_come_from_the_two_float32_evaluations (worst excesses: see there and DESIGN.md)
K = {"sgd": {"m": 16, "p": 4}, "rmsprop": {"v": 16, "m": 16, "p": 4}}
K_E = E.K_E

MUS = (0.0, 0.5, 0.9)
ALPHAS = (0.9, 0.99)
EPS_VALUES = (1e-7, 1e-3)


def quantities(kind, ema=False):
    return ("x", "m") + (("v",) if kind == "rmsprop" else ()) + ("p",) + (("e",) if ema else ())


def scalars(kind, **kw):
    return {**R.SCALARS, "kind": kind, "mu": 0.9, "alpha": 0.9, "eps": 1e-7, "decay": 0.999, **kw}


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def launch(grp, sc, dtype=F64, ema=False):
    """One launch on the group's rows -> {'s' [rows, 1], 'x', 'm', ('v',) 'p', ('e')} in `dtype`."""
    p, g, b = (np.asarray(grp[k], dtype) for k in "pgm")
    s = R.clip_factor_of(p, g, sc, dtype)
    x = s * g
    cv = dtype(F32(sc["clipvalue"]))
    if cv > 0:
        x = np.clip(x, -cv, cv)
    lr, mu = dtype(F32(sc["lr"])), dtype(float(sc["mu"]))
    out = {"s": s, "x": x}
    if sc["kind"] == "rmsprop":
        alpha = float(sc["alpha"])
        s2 = dtype(alpha) * np.asarray(grp["v"], dtype) + dtype(1.0 - alpha) * x * x
        out["v"] = s2
        step = x / (np.sqrt(s2) + dtype(F32(sc["eps"])))
    else:
        step = x
    out["m"] = mu * b + step
    out["p"] = p - lr * out["m"]
    if ema:
        e = np.asarray(grp["e"], dtype)
        out["e"] = e + (out["p"] - e) * dtype(E.weight(sc))
    assert all(a.dtype == dtype for a in out.values())
    return out


def reference(case, dtype=F64, ema=False):
    return [launch(grp, case["sc"], dtype, ema) for grp in case["groups"]]


# ---------------------------------------------------------------------------
# the error rule
# ---------------------------------------------------------------------------
def parts(grp, ref, sc, ema=False):
    """{name: (propagated part, scale of the float32 operations of that line)} per element, from the float64 `ref` of the group."""
    kind = sc["kind"]
    k = K[kind]
    p, g, b = (np.asarray(grp[q], F64) for q in "pgm")
    x, b2 = ref["x"], ref["m"]
    ex = (math.ceil(p.shape[1] / 64) + 18) * U * np.abs(ref["s"] * g) if sc["use_agc"] else np.zeros_like(g)
    lr, mu = float(F32(sc["lr"])), float(sc["mu"])
    out = {"x": (ex, np.zeros_like(ex))}
    if kind == "rmsprop":
        alpha, s2 = float(sc["alpha"]), ref["v"]
        p_s = (1.0 - alpha) * (2.0 * np.abs(x) + ex) * ex
        out["v"] = (p_s, s2)
        b_s = p_s + k["v"] * U * s2
        root = np.sqrt(s2)
        a = root + float(F32(sc["eps"]))
        with np.errstate(divide="ignore", invalid="ignore"):
            da = np.where(s2 > 0, b_s / (2.0 * root), 0.0)
            p_b = ex / a + np.abs(x) * da / (a * a)
            s_b = np.abs(mu * b) + np.abs(x / a)
    else:
        p_b, s_b = ex, np.abs(mu * b) + np.abs(x)
    out["m"] = (p_b, s_b)
    b_b = p_b + k["m"] * U * s_b
    out["p"] = (lr * b_b, np.abs(p) + np.abs(lr * b2))
    if ema:
        w = float(E.weight(sc))
        b_p = out["p"][0] + k["p"] * U * out["p"][1]
        e = np.abs(np.asarray(grp["e"], F64))
        out["e"] = (w * b_p, e + w * (np.abs(ref["p"]) + e))
    return out


def bounds(grp, ref, sc, ema=False):
    """{name: the largest |got - ref| per element}."""
    k = {**K[sc["kind"]], "e": K_E}
    return {name: part + (k[name] * U * scale if name in k else 0.0) for name, (part, scale) in parts(grp, ref, sc, ema).items()}


def errors(got, ref, grp, sc):
    """{name: (worst |got - ref| / bound over the group's elements, worst |got - ref|)} over the names of `got`."""
    lim = bounds(grp, ref, sc, ema="e" in got)
    out = {}
    for name, a in got.items():
        err = R._err(a, ref[name])
        finite = err[np.isfinite(err)]
        out[name] = (float(R._ratio(err, np.nan_to_num(lim[name], nan=0.0)).max()), float(finite.max()) if finite.size else 0.0)
    return out


def excess(got, ref, grp, sc):
    """{name: worst (|got - ref| - propagated part)+ / (u scale)} for the quantities of `got` but x: what K has to cover."""
    out = {}
    for name, (part, scale) in parts(grp, ref, sc, ema="e" in got).items():
        if name == "x" or name not in got:
            continue
        over = np.maximum(R._err(got[name], ref[name]) - np.nan_to_num(part, nan=0.0), 0.0)
        out[name] = float(R._ratio(over, U * np.nan_to_num(scale, nan=0.0)).max())
    return out


# ---------------------------------------------------------------------------
# cases: ema_ref's generators (agc_ref's with a shadow row), the state rows read as b and s
# ---------------------------------------------------------------------------
def _as(case, sc, state_scale=True):
    """`case` (an ema_ref case) under the scalars `sc`.  The generators' first-moment rows (~3e-4) serve sgd's momentum buffer as
    they are; rmsprop's buffer holds x / sqrt(s) terms, of order one: scaled up by 1e3 (exact: a float32 times a power-of-ten is
    rounded once, here, before anything reads it)."""
    for grp in case["groups"]:
        if sc["kind"] == "rmsprop" and state_scale and not grp.get("_scaled"):
            grp["m"] = (grp["m"].astype(F64) * 1e3).astype(F32)
            grp["_scaled"] = True
    case["sc"] = dict(sc)
    case["name"] = f"{sc['kind']}-{case['name']}" + ("" if sc["use_agc"] else "-noagc") + ("" if sc["clipvalue"] else "-noclipvalue")
    return case


def lengths_case(sc):
    """ema_ref.lengths_case: every length of agc_ref.LENGTHS, two rows of 70,000, and the twins 4 bytes off alignment - all pointers,
    only one state row, only the shadow."""
    return _as(E.lengths_case(dict(sc)), sc)


def rowloop_case(sc):
    return _as(E.rowloop_case(dict(sc)), sc)


def edges_case(sc, nan=False):
    return _as(E.edges_case(dict(sc), nan=nan), sc)


def zero_state_case(sc):
    """A first step: b = 0 everywhere (torch's first step is b' = x), and for rmsprop s = 0 - with the zero-gradient row of the
    edges that is s' = 0, a = eps, x / a = 0: b' stays finite."""
    case = edges_case(sc)
    for grp in case["groups"]:
        grp["m"], grp["v"] = np.zeros_like(grp["m"]), np.zeros_like(grp["v"])
    case["name"] += "-first"
    return case


def constants_cases(kind):
    """A short table (agc_ref.constants_case: lengths 3, 32, 260, 1024) for every mu x lr source - and for rmsprop x alpha x eps -,
    with the EMA's counter on the warm-up side (t = 2) and the capped side (t = 100000)."""
    out = []
    for mu in MUS:
        for lr_dev in (False, True):
            for alpha, eps in ([(a, e) for a in ALPHAS for e in EPS_VALUES] if kind == "rmsprop" else [(0.9, 1e-7)]):
                for t in (2.0, 100000.0):
                    sc = scalars(kind, mu=mu, alpha=alpha, eps=eps, lr_dev=lr_dev, lr=3e-4 if lr_dev else 1e-3, t=t)
                    base = R.constants_case({**R.scalars(t=t, lr_dev=lr_dev, lr=sc["lr"], eps=eps), "beta1": mu, "beta2": alpha}, False)
                    out.append(_as(E._with_shadow(base, 40 + len(out), sc["decay"]), sc))
    return out


EDGE_SCALARS = {"default": {}, "no-clipvalue": {"clipvalue": 0.0}, "no-agc": {"use_agc": 0}, "floor-1e-6": {"eps_agc": 1e-5}, "mu-0": {"mu": 0.0}}


def chain_start(kind, name):
    """The running state consecutive launches start from: 'chain' (four launches) or 'capture' (three replays, device lr)."""
    return _as(E.chain_start(name), scalars(kind, t=7.0, lr_dev=name == "capture"))


def chain_next(start, state, k):
    """Launch k of a chain (ema_ref.chain_next: a new gradient, the counter at 7 + k, the learning rate agc_ref.CHAIN_LRS[k])."""
    case = E.chain_next(start, state, k)
    case["sc"] = {**start["sc"], "t": 7.0 + k, "lr": R.CHAIN_LRS[k]}
    return case


def single_launch_cases(kind):
    """Every case of tests/test_optim_gpu.py that is one launch from given inputs (the chains are walked by their tests)."""
    out = [lengths_case(scalars(kind)), lengths_case(scalars(kind, use_agc=0)), rowloop_case(scalars(kind))]
    out += [edges_case(scalars(kind, **kw)) for kw in EDGE_SCALARS.values()]
    out += [edges_case(scalars(kind), nan=True), zero_state_case(scalars(kind))]
    return out + constants_cases(kind)
