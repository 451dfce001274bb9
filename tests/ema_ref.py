"""Reference form of the weight EMA that rides in the fused AGC + clipvalue + Adam launch (`iris_agc_clip_adam_ema`,
csrc/k_agc_adam.h): tests/agc_ref.py's definition, groups and cases with one more quantity, the shadow row `e`.  NumPy only.

    ... x, m', v', p' as in agc_ref ...
    d_t = min(decay, (1 + t) / (10 + t))        formed in double; t the counter the bias corrections read
    w   = (float)(1 - d_t)                       the kernel's weight: rounded to float32 in EVERY evaluation, the float64 one too
    e'  = e + (p' - e) w

A group is agc_ref's plus 'e' (float32 [rows, len]) and 'mis'['e']; `sc` gains 'decay'.

The error rule (u = 2^-24):

    |e' - e64'| <= w b_p + K_E u (|e| + w (|p'| + |e|))

b_p is agc_ref's bound on p' (the line is linear in p' with slope w), the second term the float32 operations of the line itself: a
subtraction, a product, a sum - the form and the scale of K_M's term for Adam's first moment.  K_E follows agc_ref's convention and is
not read off the kernel: the smallest power of two at or above four times the worst excess over the propagated part, in units of
u x that scale, of two float32 evaluations over every case of tests/test_ema_gpu.py - this file's lines in NumPy float32, and
torch.lerp (float32, CPU) fed the yardstick's p'.  tests/test_ema_host.py re-derives it and holds both inside the bound."""
import numpy as np

import agc_ref as R
from agc_ref import F32, F64, U

# derived by tests/test_ema_host.py::test_constant_comes_from_the_two_float32_evaluations (worst excesses: see there and DESIGN.md)
K_E = 4

DECAYS = (0.999, 0.9, 0.0)
QUANTITIES = R.QUANTITIES + ("e",)


def scalars(**kw):
    return {**R.SCALARS, "decay": 0.999, **kw}


def decay_at(t, decay):
    """d_t, in double."""
    t = float(t)
    return min(float(decay), (1.0 + t) / (10.0 + t))


def weight(sc):
    """w as the kernel forms it: float32."""
    return F32(1.0 - decay_at(sc["t"], sc["decay"]))


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def launch(grp, sc, dtype=F64):
    out = R.launch(grp, sc, dtype)
    e = np.asarray(grp["e"], dtype)
    out["e"] = e + (out["p"] - e) * dtype(weight(sc))
    assert out["e"].dtype == dtype
    return out


def reference(case, dtype=F64):
    return [launch(grp, case["sc"], dtype) for grp in case["groups"]]


# ---------------------------------------------------------------------------
# the error rule
# ---------------------------------------------------------------------------
def parts_e(grp, ref, sc):
    """(propagated part, scale of the line's float32 operations) per element of e', from the float64 `ref` of the group."""
    w = float(weight(sc))
    b_p = R.bounds(grp, ref, sc)["p"]
    e = np.abs(np.asarray(grp["e"], F64))
    return w * b_p, e + w * (np.abs(ref["p"]) + e)


def bounds(grp, ref, sc):
    """agc_ref's bounds for x, m', v', p' and the rule above for e'."""
    out = R.bounds(grp, ref, sc)
    part, scale = parts_e(grp, ref, sc)
    out["e"] = part + K_E * U * scale
    return out


def errors(got, ref, grp, sc):
    """{name: (worst |got - ref| / bound, worst |got - ref|)} over the names of `got` (agc_ref.errors with 'e')."""
    out = R.errors({k: a for k, a in got.items() if k != "e"}, ref, grp, sc)
    if "e" in got:
        err = R._err(got["e"], ref["e"])
        finite = err[np.isfinite(err)]
        out["e"] = (float(R._ratio(err, np.nan_to_num(bounds(grp, ref, sc)["e"], nan=0.0)).max()), float(finite.max()) if finite.size else 0.0)
    return out


def excess_e(got_e, ref, grp, sc):
    """Worst (|got - ref| - propagated part)+ / (u scale) for e': what K_E has to cover."""
    part, scale = parts_e(grp, ref, sc)
    over = np.maximum(R._err(got_e, ref["e"]) - np.nan_to_num(part, nan=0.0), 0.0)
    return float(R._ratio(over, U * np.nan_to_num(scale, nan=0.0)).max())


def recurrence_check(what, e0, recorded, got, decay, t0=0):
    """The float64 recurrence over the RECORDED parameters (so b_p = 0) against the shadows `got` after len(recorded) steps; the
    bound is the rule carried forward: B' = (1 - w) B + K_E u (|e| + w (|p'| + |e|)).  -> the worst ratio."""
    worst = 0.0
    for i in range(len(e0)):
        e, bound = e0[i].astype(F64), np.zeros(e0[i].shape)
        for k, params in enumerate(recorded):
            w = float(weight({"t": float(t0 + k + 1), "decay": decay}))
            p = params[i].astype(F64)
            bound = (1.0 - w) * bound + K_E * U * (np.abs(e) + w * (np.abs(p) + np.abs(e)))
            e = e + (p - e) * w
        ratio = float(R._ratio(R._err(got[i], e), bound).max())
        assert ratio <= 1.0, (what, i, ratio)
        worst = max(worst, ratio)
    print(f"{what}: shadow after {len(recorded)} steps at most {worst:.3f} of the carried bound")
    return worst


# ---------------------------------------------------------------------------
# cases: agc_ref's generators, a shadow row beside every parameter row
# ---------------------------------------------------------------------------
def _with_shadow(case, seed, decay=0.999):
    """`e` = the parameter plus N(0, 5e-3) - an average trails its parameter closely - aligned like the parameter row."""
    rng = np.random.default_rng([7, seed])
    for grp in case["groups"]:
        grp["e"] = (grp["p"].astype(F64) + 5e-3 * rng.standard_normal(grp["p"].shape)).astype(F32)
        grp["mis"] = {**grp["mis"], "e": grp["mis"]["p"]}
    case["sc"] = {**case["sc"], "decay": decay}
    return case


def lengths_case(sc=None):
    """agc_ref.lengths_case with shadows: the all-misaligned twins have `e` misaligned too, the exp_avg-only and exp_avg_sq-only
    twins keep it aligned, and one more twin of the 256 group has ONLY `e` 4 bytes off.  Twins share their aligned group's values."""
    sc = sc or scalars()
    case = _with_shadow(R.lengths_case({k: v for k, v in sc.items()}), 1, sc["decay"])
    base = R.LENGTHS.index(256)
    case["twins"] = list(case["twins"]) + [(len(case["groups"]), base)]
    g = case["groups"][base]
    case["groups"].append({**{k: g[k].copy() for k in "pgmve"}, "mis": {**g["mis"], "e": 1}, "packed": g["packed"]})
    for gi, twin in case["twins"]:
        case["groups"][gi]["e"] = case["groups"][twin]["e"].copy()
    assert [case["groups"][gi]["mis"]["e"] for gi, _ in case["twins"]] == [1, 1, 1, 0, 0, 1]
    return case


def edges_case(sc=None, nan=False):
    sc = sc or scalars()
    return _with_shadow(R.edges_case(sc, nan=nan), 3, sc["decay"])


def rowloop_case(sc=None):
    sc = sc or scalars()
    return _with_shadow(R.rowloop_case("adam", sc), 2, sc["decay"])


def constants_cases():
    """agc_ref.constants_cases (every t of T_VALUES x eps x lr source, the first pair of betas) for every decay of DECAYS: at 0.999
    t = 1, 2, 10, 1000 are on the warm-up side and 100000 on the capped side; at 0.9, t = 100000 and 1000 are capped; 0.0: e' = p'."""
    out = []
    for di, decay in enumerate(DECAYS):
        for ci, case in enumerate(R.constants_cases(R.BETAS[0])):
            case = _with_shadow(case, 100 * di + ci + 10, decay)
            case["name"] += f"-decay{decay}"
            out.append(case)
    return out


def chain_start(name):
    return _with_shadow(R.chain_start(name), 5 + len(name))


def chain_next(start, state, k):
    """agc_ref.chain_next with the shadow carried forward: `state` is a list of {'p', 'm', 'v', 'e'} per group, or None."""
    case = R.chain_next(start, state, k)
    for i, grp in enumerate(case["groups"]):
        grp["e"] = start["groups"][i]["e"] if state is None else np.asarray(state[i]["e"], F32)
        grp["mis"] = start["groups"][i]["mis"]
    case["sc"] = {**case["sc"], "decay": start["sc"]["decay"]}
    return case


def single_launch_cases():
    """Every case of tests/test_ema_gpu.py that is one launch from given inputs (the chains are walked by their tests)."""
    return [lengths_case(), edges_case(), edges_case(nan=True), rowloop_case()] + constants_cases()
