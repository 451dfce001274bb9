"""CPU tests of the weight EMA (tests/ema_ref.py; the kernel is iris_agc_clip_adam_ema of csrc/k_agc_adam.h, the torch side
challenge_amd/ema.py): the constant K_E re-derived from the two float32 evaluations (this file's lines in NumPy float32; torch.lerp in
float32 fed the yardstick's p') over every case of tests/test_ema_gpu.py with both held inside the bound, the warm-up, `WeightEMA`'s
torch fallback against the float64 recurrence, checkpoints, `recalibrate_bn` against torch.optim.swa_utils.update_bn, the entry
point's argument checks and `fit(..., ema=)`.

Measured here (`test_constant_comes_from_the_two_float32_evaluations` prints them; 71 launches):

    excess of e' over the propagated part, in u x scale:   NumPy float32 0.99 | torch.lerp 0.99   ->  K_E = 4
    against the bound so made the two evaluations read at most 0.30 | 0.25"""
import ctypes as C
import copy
import io

import numpy as np
import pytest
import torch

import agc_ref as R
import ema_ref as E
from agc_ref import F32, F64, U

_WORST = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------
# the error rule
# ---------------------------------------------------------------------------
def _measure(case):
    """Both float32 evaluations of e' for one case against its float64 reference: inside the bound; the worst figures are kept."""
    ref = E.reference(case)
    yard = E.reference(case, F32)
    w = torch.tensor(float(E.weight(case["sc"])), dtype=torch.float32)
    for grp, r, y in zip(case["groups"], ref, yard):
        lerp = torch.lerp(torch.from_numpy(grp["e"].copy()), torch.from_numpy(np.ascontiguousarray(y["p"], F32)), w).numpy()
        for who, got in (("numpy", y["e"]), ("torch", lerp)):
            ratio, _ = E.errors({"e": got}, r, grp, case["sc"])["e"]
            assert ratio <= 1.0, (case["name"], who, ratio)
            _WORST[(who, "bound")] = max(_WORST.get((who, "bound"), (0.0, "")), (ratio, case["name"]))
            _WORST[(who, "excess")] = max(_WORST.get((who, "excess"), (0.0, "")), (E.excess_e(got, r, grp, case["sc"]), case["name"]))
    return yard


def _all_cases():
    yield from E.single_launch_cases()
    for name, n in (("chain", 4), ("capture", 3)):
        start, state = E.chain_start(name), None
        for k in range(n):
            case = E.chain_next(start, state, k)
            yield case
            state = [{q: y[q] for q in "pmve"} for y in E.reference(case, F32)]


def test_constant_comes_from_the_two_float32_evaluations():
    """Every case of tests/test_ema_gpu.py: the float32 yardstick and torch.lerp stay inside the bound on e', and K_E = the smallest
    power of two at or above four times the worse worst excess - what ema_ref.K_E holds."""
    n = 0
    for case in _all_cases():
        _measure(case)
        n += 1
    for key in sorted(_WORST):
        print(f"{key[0]:5s} e {key[1]:6s}: {_WORST[key][0]:.3f} at {_WORST[key][1]}")
    print(f"{n} cases")
    worst = max(_WORST[("numpy", "excess")][0], _WORST[("torch", "excess")][0])
    assert E.K_E == R.pow2_at_or_above(4.0 * worst), (worst, E.K_E)


def test_cases_cover_what_they_promise():
    case = E.lengths_case()
    assert [g["p"].shape[1] for g in case["groups"][:11]] == list(R.LENGTHS) + [R.LONG]
    assert len(case["twins"]) == 6
    only_e = case["groups"][case["twins"][-1][0]]
    assert only_e["mis"] == {"p": 0, "g": 0, "m": 0, "v": 0, "e": 1} and only_e["p"].shape[1] == 256
    for gi, twin in case["twins"]:
        assert all(np.array_equal(case["groups"][gi][q], case["groups"][twin][q]) for q in "pgmve")
    assert E.rowloop_case()["groups"][0]["p"].shape == (32773, 5)
    cases = E.constants_cases()
    assert len(cases) == 60 and {c["sc"]["decay"] for c in cases} == set(E.DECAYS) and {c["sc"]["t"] for c in cases} == set(R.T_VALUES)
    side = {t: (1.0 + t) / (10.0 + t) < 0.999 for t in R.T_VALUES}
    assert side == {1.0: True, 2.0: True, 10.0: True, 1000.0: True, 100000.0: False}      # warm-up side / capped side at 0.999
    nan = E.edges_case(nan=True)
    assert any(np.isnan(r["e"]).any() for r in E.reference(nan)) and not any(np.isnan(g["e"]).any() for g in nan["groups"])


def test_warm_up_values():
    """d_1 = 2 / 11 whatever the decay allows; 0.999 takes over where (1 + t) / (10 + t) reaches it, between t = 8989 and 8990; a decay
    of 0 makes the shadow the parameter; and `ema.ema_weight` - the torch fallback's w, formed from a counter tensor - has the bits
    of the reference's (and so of the kernel's) at every t of the cases."""
    from challenge_amd.ema import ema_weight
    assert E.decay_at(1.0, 0.999) == 2.0 / 11.0 and E.decay_at(1.0, 0.1) == 0.1
    assert E.decay_at(8989.0, 0.999) == 8990.0 / 8999.0 < 0.999 and E.decay_at(8990.0, 0.999) == 0.999 == E.decay_at(1e5, 0.999)
    assert float(E.weight(E.scalars(t=1.0))) == float(F32(9.0 / 11.0))
    assert float(E.weight(E.scalars(t=5.0, decay=0.0))) == 1.0
    for decay in E.DECAYS + (0.9999,):
        for t in R.T_VALUES + (8989.0, 8990.0, 8991.0):
            got = ema_weight(torch.tensor(t, dtype=torch.float32), decay)
            assert got.dtype == torch.float32 and got.dim() == 0
            assert _bits(got.numpy()) == _bits(E.weight({"t": t, "decay": decay})), (decay, t)
    grp = {k: np.full((1, 4), v, F32) for k, v in (("p", 1.0), ("g", 0.0), ("m", 0.0), ("v", 0.0), ("e", 3.0))}
    out = E.launch(grp, E.scalars(t=1.0, use_agc=0))                       # zero gradient and moments: p' = p = 1
    assert np.array_equal(out["p"], grp["p"]) and np.allclose(out["e"], 3.0 + (1.0 - 3.0) * float(F32(9.0 / 11.0)), rtol=1e-15)


# ---------------------------------------------------------------------------
# WeightEMA on a CPU model: the torch fallback, checkpoints
# ---------------------------------------------------------------------------
def _small(optimizer="adam", seed=3):
    from challenge_amd import sj_train as S
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4', '--optimizer', optimizer])
    torch.manual_seed(seed)
    return S, cfg, S.get_model(cfg)


def _batches(n, seed, rows=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(rows, 32, 64, 1, generator=g), (torch.rand(rows, 2, 3, generator=g) > 0.5).float()) for _ in range(n)]


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "rmsprop"])
def test_torch_fallback_follows_the_float64_recurrence(optimizer):
    """4 train_steps of a small CPU model with a WeightEMA compiled in: the shadow against the recurrence over the parameters
    recorded after each step.  adam keeps a counter tensor the fallback reads; sgd keeps none and rmsprop's is the same kind, so
    all three count 1, 2, 3, 4.  The shadow module takes no gradient, stays in eval mode and is no submodule of the live model."""
    from challenge_amd.ema import WeightEMA
    S, cfg, model = _small(optimizer)
    ema = WeightEMA(model, 0.999)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=ema)
    keys = list(model.state_dict())
    e0 = [e.detach().numpy().copy() for e in ema.shadow]
    assert all(np.array_equal(_bits(a), _bits(p.detach().numpy())) for a, p in zip(e0, model.parameters()))
    recorded = []
    for batch in _batches(4, 7):
        model.train_step(batch)
        recorded.append([p.detach().numpy().copy() for p in model.parameters()])
    E.recurrence_check(f"torch fallback ({optimizer})", e0, recorded, [e.detach().numpy() for e in ema.shadow], 0.999)
    assert sum(not np.array_equal(a, e.detach().numpy()) for a, e in zip(e0, ema.shadow)) > len(e0) // 2      # the shadows DID move
    assert not ema.module.training and not any(p.requires_grad for p in ema.module.parameters())
    assert list(model.state_dict()) == keys and list(ema.state_dict()) == keys and not any(m is ema.module for m in model.modules())


def test_state_dict_round_trip_is_bit_identical():
    from challenge_amd.ema import WeightEMA
    S, cfg, model = _small()
    ema = WeightEMA(model, 0.99)
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=ema)
    for batch in _batches(2, 8):
        model.train_step(batch)
    buf = io.BytesIO()
    torch.save(ema.state_dict(), buf)
    buf.seek(0)
    _, _, other = _small(seed=4)
    other.load_state_dict(torch.load(buf))                                   # an ordinary checkpoint: a plain model reads it
    again = WeightEMA(other, 0.5)
    want = ema.state_dict()
    for holder in (other, again):
        got = holder.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
            if want[k].is_floating_point():
                assert np.array_equal(_bits(got[k].numpy()), _bits(want[k].numpy())), k
    with pytest.raises(ValueError):
        WeightEMA(model, 1.0)
    with pytest.raises(ValueError):
        WeightEMA(model, -0.1)


# ---------------------------------------------------------------------------
# BatchNorm recalibration
# ---------------------------------------------------------------------------
def bn_statistics(model):
    return {n: b.detach().double().cpu().numpy().copy() for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))}


def update_bn_yardstick(model, xs):
    """torch.optim.swa_utils.update_bn on copies of `model` in float32 and in float64 -> (statistics32, statistics64, tolerance per
    buffer = four times the largest distance between the two)."""
    from torch.optim.swa_utils import update_bn
    out = []
    for dtype in (torch.float32, torch.float64):
        m = copy.deepcopy(model).to(dtype)
        update_bn([x.to(dtype) for x in xs], m)
        out.append(bn_statistics(m))
    tol = {n: 4.0 * float(np.abs(out[0][n] - out[1][n]).max()) for n in out[0]}
    return out[0], out[1], tol


def test_recalibrate_bn_is_update_bn():
    """3 batches of 4 (32 mel x 64 frames, mono) through a CPU model whose statistics start from garbage: `recalibrate_bn` against
    torch.optim.swa_utils.update_bn on the same module, within four times that float32 result's own distance from float64
    (measured here, printed); momentum and mode come back as they were, in train and in eval mode."""
    from challenge_amd.ema import recalibrate_bn
    S, cfg, model = _small()
    xs = [x for x, _ in _batches(3, 9)]
    with torch.no_grad():
        for n, b in model.named_buffers():
            if n.endswith("running_mean"):
                b.fill_(7.0)
            elif n.endswith("running_var"):
                b.fill_(0.3)
    s32, s64, tol = update_bn_yardstick(model, xs)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(s32) == 2 * len(bns) == 36 and all(t > 0 for t in tol.values())
    model.eval()
    assert recalibrate_bn(model, [(x, None) for x in xs]) == 3                 # (input, target) pairs, as a dataset yields them
    assert not model.training and all(bn.momentum == 0.01 and not bn.training for bn in bns)
    got = bn_statistics(model)
    worst = max(float(np.abs(got[n] - s32[n]).max()) / tol[n] for n in got)
    far = max(float(np.abs(s32[n] - s64[n]).max()) for n in got)
    print(f"recalibrate_bn vs update_bn (float32): worst {worst:.3f} of the tolerance (4 x |float32 - float64|, at most {4 * far:.3e})")
    assert worst <= 1.0
    assert all(np.abs(got[n] - 7.0).min() > 1.0 for n in got if n.endswith("running_mean"))           # nothing of the garbage is left
    model.train()
    recalibrate_bn(model, iter(xs))
    assert model.training and all(bn.momentum == 0.01 for bn in bns)
    again = bn_statistics(model)
    assert all(np.array_equal(again[n], got[n]) for n in got)


def test_swa_finalize_resets_bn_only_when_asked():
    from challenge_amd.swa import SWA
    S, cfg, model = _small()
    xs = [x for x, _ in _batches(3, 10)]
    swa = SWA(start_epoch=0)
    swa.on_epoch_end(0, model)
    plain = {k: v.clone() for k, v in swa.finalize(model).items()}
    assert all(torch.equal(plain[k], v) for k, v in model.state_dict().items())
    s32, _, tol = update_bn_yardstick(model, xs)
    state = swa.finalize(model, reset_bn=xs)
    got = bn_statistics(model)
    assert all(float(np.abs(got[n] - s32[n]).max()) <= tol[n] for n in got)
    for k, v in model.state_dict().items():
        assert torch.equal(state[k], v)
        if not k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(plain[k], v), k


# ---------------------------------------------------------------------------
# the entry point's argument checks (no GPU: nothing may be launched)
# ---------------------------------------------------------------------------
def test_entry_point_validates_before_any_launch():
    from challenge_amd import _native as N
    lib = N.lib()
    p8 = C.c_void_p(8)

    def call(rows=p8, n=1, beta1=0.9, beta2=0.999, eps=1e-7, step=p8, decay=0.999):
        return lib.iris_agc_clip_adam_ema(rows, n, 0.01, 1e-3, 0.01, 1, None, 1e-3, beta1, beta2, eps, step, decay, None)
    assert call(n=0) == 0                                                      # nothing to do, as iris_agc_clip_adam
    assert call(rows=None) == -1 and b"NULL" in lib.iris_last_error()
    assert call(step=None) == -1
    for decay in (1.0, 1.5, -1e-9, float("nan"), float("inf")):
        assert call(decay=decay) == -1, decay
        assert b"decay" in lib.iris_last_error()
    assert call(beta1=1.0) == -1 and call(beta2=-0.1) == -1 and call(eps=-1.0) == -1
    assert lib.iris_agc_clip_adam(None, 1, 0.01, 1e-3, 0.01, 1, None, 1e-3, 0.9, 0.999, 1e-7, p8, None) == -1   # the sibling, unchanged


def test_fused_agc_without_a_device_keeps_its_tables():
    """`attach_ema` refuses CPU shadows (and detaches); the column count follows what is attached."""
    from challenge_amd.hip_autograd import FusedAGC
    params = [torch.nn.Parameter(torch.randn(3, 4))]
    agc = FusedAGC(params)
    assert agc._cols() == 3 and not agc.ema_attached
    assert agc.attach_ema([torch.zeros(3, 4)], 0.9) is False and not agc.ema_attached and agc._cols() == 3
    with pytest.raises(ValueError):
        agc.attach_ema([torch.zeros(3, 4)], 1.0)


# ---------------------------------------------------------------------------
# fit(..., ema=)
# ---------------------------------------------------------------------------
def _fit_once(tmp_path, tag, with_ema):
    from challenge_amd import metrics as M
    from challenge_amd.dataset import Dataset
    from challenge_amd.ema import WeightEMA
    S, cfg, model = _small(seed=5)
    ema = None
    if with_ema:
        ema = WeightEMA(model, 0.9)
        ema.compile(S.binary_crossentropy, metrics=[M.cos_sim, M.f1_score(), M.er_score(smoothing=False)])
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  metrics=[M.cos_sim, M.f1_score(), M.er_score(smoothing=False)], ema=ema)
    train, val = _batches(3, 11), _batches(2, 12)
    ds = Dataset.from_generator(lambda: iter(train)).repeat()
    vds = Dataset.from_generator(lambda: iter(val)).repeat()
    (tmp_path / tag).mkdir()                                                   # (torch.save writes the file's name into the archive)
    ckpt, eckpt = tmp_path / tag / "model.pt", tmp_path / tag / "model_EMA.pt"
    extra = {"ema": ema, "ema_checkpoint_path": str(eckpt)} if with_ema else {}
    hist = S.fit(model, ds, epochs=2, steps_per_epoch=2, validation_data=vds, validation_steps=2, checkpoint_path=str(ckpt),
                 csv_path=str(tmp_path / f"{tag}.csv"), checkpoint_monitor="val_er", verbose=False, **extra)
    return hist, ckpt, eckpt, ema, model


def test_fit_validates_the_ema_beside_the_live_model(tmp_path):
    """2 epochs x 2 steps on the CPU, with and without `ema`, same seeds: the rows' existing entries and the live checkpoint are
    byte-identical; with it the rows carry val_ema_loss and the val_ema_* metrics, and the EMA checkpoint is an ordinary one."""
    plain, ckpt0, eckpt0, _, _ = _fit_once(tmp_path, "plain", False)
    hist, ckpt1, eckpt1, ema, model = _fit_once(tmp_path, "ema", True)
    assert len(plain) == len(hist) == 2
    new = {"val_ema_loss", "val_ema_cos_sim", "val_ema_f1_score", "val_ema_er"}
    for a, b in zip(plain, hist):
        assert set(b) - set(a) == new and set(a) <= set(b)
        assert all(np.isfinite(b[k]) for k in new)
        for k in a:
            if k != "time":
                assert a[k] == b[k], (k, a[k], b[k])
        assert b["val_ema_loss"] != b["val_loss"]
    assert ckpt0.read_bytes() == ckpt1.read_bytes()
    assert not eckpt0.exists() and eckpt1.exists()
    saved = torch.load(str(eckpt1))
    S, cfg, fresh = _small(seed=6)
    fresh.load_state_dict(saved)
    best = min(range(2), key=lambda i: (hist[i]["val_ema_er"], i))          # strictly better only: ties keep the earlier epoch
    if best == 1:                                                              # the file is the EMA as the last epoch left it
        assert all(torch.equal(saved[k], v) for k, v in ema.state_dict().items())
    # the pass ran on the EMA's weights under the LIVE BatchNorm statistics
    live, shadow = model.state_dict(), ema.state_dict()
    assert all(torch.equal(live[k], shadow[k]) for k in live if "running_" in k or "num_batches" in k)
    assert any(not torch.equal(live[k], shadow[k]) for k in live if k.endswith("weight"))
    with pytest.raises(ValueError):
        S.fit(fresh, [], epochs=1, steps_per_epoch=1, ema=ema, verbose=False)
