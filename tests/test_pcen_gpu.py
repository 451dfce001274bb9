"""GPU tests of per-channel energy normalisation (iris_pcen, csrc/k_pcen.h): parity with the fp64 restatement of
tests/test_pcen_host.py under its error rule at the training, odd-length and long-recording shapes; exact zeros, NaN
propagation, in-place / repeat / graph-replay bit equality; and the pipelines that select it by a 'pcen' run name."""
import math

import numpy as np
import pytest
import torch

from test_pcen_host import K_M, U, out_bound, params32, pcen_ref

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_MEL = {}


def _real_mel(seed=0):
    """[64, 80, 512, 2] mel magnitudes from the fused frontend (min-max / log off) on synthetic stereo audio: noise under
    a drone-like harmonic hum plus bursts of tones, per clip its own level."""
    if seed in _MEL:
        return _MEL[seed]
    from challenge_amd import frontend as FE
    dev = _dev()
    rng = np.random.default_rng(seed)
    b, length = 64, 511 * 256
    t = np.arange(length) / 16000.0
    hum = sum(np.sin(2 * np.pi * f0 * k * t) / k for k in range(1, 6) for f0 in (97.0,))
    wav = rng.standard_normal((b, 2, length)) * 0.05 + 0.2 * hum[None, None]
    env = np.repeat(rng.random((b, 1, length // 4000 + 1)) < 0.3, 4000, axis=2)[..., :length]
    wav += env * np.sin(2 * np.pi * rng.uniform(300, 3000, (b, 2, 1)) * t) * 0.5
    wav *= np.exp(rng.normal(0.0, 1.5, (b, 1, 1)))
    plan = FE.FrontendPlan(512, 256, 80, 16000, 2, b, length, dev)
    mel = plan.wav_to_logmel(torch.from_numpy(wav.astype(np.float32)).to(dev), minmax=False, log=False)
    _MEL[seed] = mel
    return mel


def _shape_from(mel, shape):
    """A tensor of `shape` ([..., T, C] batched or [M, T, C]) cut from the real mel; long T joins clips along time."""
    *lead, t, c = shape
    flat = mel[..., :c].permute(1, 0, 2, 3).reshape(mel.shape[1], -1, c)          # [80, 64 * 512, c]
    if len(lead) == 1:
        return flat[:lead[0], :t].contiguous()
    b, m = lead
    need = b * t
    reps = -(-need // flat.shape[1])
    flat = flat.repeat(1, reps, 1) if reps > 1 else flat
    return flat[:m, :need].reshape(m, b, t, c).permute(1, 0, 2, 3).contiguous()


def _inject(x, rng):
    """All-zero rows, masked bands (zeroed time ranges) and one NaN, in place; returns the NaN's index or None."""
    if x.dim() == 4:
        b, m, t, c = x.shape
        x[rng.integers(b), rng.integers(m)] = 0.0
        if t > 8:
            i, j = rng.integers(b), rng.integers(m)
            t0 = int(rng.integers(0, t - 4))
            x[i, j, t0:t0 + min(24, t - t0)] = 0.0
            x[i, :, t0:t0 + min(5, t - t0)] = 0.0                               # a SpecAugment-like time mask
            x[rng.integers(b), rng.integers(m // 2, m)] = 0.0                   # a masked mel band of one clip
        nan = (int(rng.integers(b)), int(rng.integers(m)), int(rng.integers(t)), int(rng.integers(c)))
    else:
        m, t, c = x.shape
        x[rng.integers(m)] = 0.0
        t0 = int(rng.integers(0, t - 30))
        x[:, t0:t0 + 30] = 0.0
        nan = (int(rng.integers(m)), int(rng.integers(t)), int(rng.integers(c)))
    x[nan] = float('nan')
    return nan


def _check(x, out, m32, params, time_axis=-2):
    """Assert the error rule on M and on the output; returns the worst (|dM| / (u W), |d out| / bound, rel on ordinary)."""
    E = x.cpu().numpy().astype(np.float64)
    M, ref, W = pcen_ref(E, *params, time_axis=time_axis)
    with np.errstate(invalid='ignore', divide='ignore'):
        return _ratios(E, M, ref, W, out, m32, params)


def _ratios(E, M, ref, W, out, m32, params):
    got, gm = out.cpu().numpy().astype(np.float64), m32.cpu().numpy().astype(np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), ~fin) and np.array_equal(np.isnan(gm), ~np.isfinite(M))
    dm = np.abs(gm - M)[fin]
    assert np.all(dm <= K_M * U * W[fin]), float(np.max(dm / (U * W[fin] + 1e-300)))
    dout = np.abs(got - ref)[fin]
    bound = out_bound(M, ref, W, E, *params)[fin]
    assert np.all(dout <= bound), float(np.max(dout / bound))
    assert np.all(got[(E == 0) & fin] == 0.0)                                      # masked / zero input: exactly 0
    ordinary = ref[fin] > 1e-30
    rel = float(np.max(dout[ordinary] / ref[fin][ordinary])) if ordinary.any() else 0.0
    return (float(np.max(dm / (U * W[fin]), initial=0.0, where=W[fin] > 0)), float(np.max(dout / np.maximum(bound, 1e-300))), rel)


SHAPES = [(64, 80, 512, 2), (8, 64, 512, 1), (3, 7, 1, 2), (4, 80, 513, 2), (2, 16, 4099, 2), (80, 15000, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_fp64(shape):
    from challenge_amd import frontend as FE
    rng = np.random.default_rng(len(shape) * 1000 + shape[-2])
    x = _shape_from(_real_mel(), shape).clone()
    nan = _inject(x, rng)
    params = params32()
    out = FE.pcen(x)
    m32 = FE.pcen_smoother(x)
    stats = _check(x, out, m32, params)
    print("pcen parity", shape, "max |dM|/(u W) %.3f  max |dout|/bound %.3f  max rel (ordinary) %.2e" % stats)
    # NaN: forward along its own sequence only
    got = out.cpu().numpy()
    seq = got[nan[:-2]][:, nan[-1]] if len(shape) == 4 else got[nan[0], :, nan[-1]]
    t_nan = nan[-2]
    assert np.all(np.isnan(seq[t_nan:])) and not np.any(np.isnan(seq[:t_nan]))
    assert int(np.isnan(got).sum()) == shape[-2] - t_nan


@pytest.mark.parametrize("params", [(0.2, 0.5, 1.0, 1.0, 1e-3), (1.0, 0.0, 0.5, 0.25, 1e-4), (0.005, 2.0, 10.0, 0.8, 1e-8),
                                    (0.04, 8.0, 2.0, 0.5, 1e-6)])
def test_parity_other_parameters(params):
    """Other corners of the accepted ranges: s = 1 (no memory), a = 0 (no gain control), a slow smoother, and a gain whose
    (eps + M)^-a overflows fp32 (the log-domain branch)."""
    from challenge_amd import frontend as FE
    x = _shape_from(_real_mel(), (6, 80, 700, 2)).clone()
    x[1, 3] = 0.0
    p = params32(*params)
    out = FE.pcen(x, *params)
    m32 = FE.pcen_smoother(x, params[0])
    _check(x, out, m32, p)


def test_seed_sweep_worst_case():
    """20 seeds of real mel at the training shape: the worst case of each ratio, printed for DESIGN.md."""
    from challenge_amd import frontend as FE
    worst = np.zeros(3)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        x = _real_mel(seed % 4).clone() * float(np.exp(rng.normal(0, 2)))
        x = x[:, :, :, :] if seed % 2 else x.flip(2).contiguous()
        _inject(x, rng)
        worst = np.maximum(worst, _check(x, FE.pcen(x), FE.pcen_smoother(x), params32()))
    print("pcen 20-seed sweep: max |dM|/(u W) %.3f  max |dout|/bound %.3f  max rel (ordinary) %.2e" % tuple(worst))
    assert worst[2] <= 1e-5


def test_zero_input_gives_exact_zero():
    from challenge_amd import frontend as FE
    x = torch.zeros((5, 9, 1000, 2), device=_dev())
    assert torch.count_nonzero(FE.pcen(x)) == 0 and torch.count_nonzero(FE.pcen_smoother(x)) == 0


def test_in_place_repeat_and_graph_replay_are_bitwise_equal():
    from challenge_amd import frontend as FE
    for shape in [(64, 80, 512, 2), (80, 15000, 2)]:
        x = _shape_from(_real_mel(1), shape).clone()
        a = FE.pcen(x)
        b = FE.pcen(x)
        assert torch.equal(a, b)
        y = x.clone()
        r = FE.pcen(y, out=y)
        assert r.data_ptr() == y.data_ptr() and torch.equal(y, a)
        # capture into a hipGraph, replay, compare with eager
        src, dst = x.clone(), torch.empty_like(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            FE.pcen(src, out=dst)
        torch.cuda.current_stream().wait_stream(side)
        dst.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            FE.pcen(src, out=dst)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, a)
        src.copy_(x.flip(-2))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, FE.pcen(x.flip(-2).contiguous()))


def test_time_axis_and_wide_inner_axis():
    """time_axis on other axes (n_inner 1 and n_inner > 256, several workgroups per row) against the restatement."""
    from challenge_amd import frontend as FE
    base = _shape_from(_real_mel(2), (80, 3000, 2)).clone()
    x = base[:, :, 0].contiguous()                                                  # [80, 3000], time last
    _check(x, FE.pcen(x, time_axis=-1), FE.pcen_smoother(x, time_axis=-1), params32(), time_axis=-1)
    w = base[:, :1000].permute(1, 0, 2).reshape(1000, 160).repeat(1, 3).reshape(1, 1000, 480).contiguous()  # n_inner 480
    M, ref, W = pcen_ref(w.cpu().numpy(), *params32(), time_axis=1)
    got = FE.pcen(w, time_axis=1).cpu().numpy()
    assert np.all(np.abs(got - ref) <= out_bound(M, ref, W, w.cpu().numpy().astype(np.float64), *params32()))


def test_bad_parameters_raise_value_error():
    from challenge_amd import frontend as FE
    x = torch.ones((1, 2, 3, 1), device=_dev())
    for kw in ({'smooth': 0.0}, {'gain': -1.0}, {'bias': 0.0}, {'power': 1.5}, {'eps': float('nan')}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            FE.pcen(x, **kw)
    with pytest.raises(ValueError):
        FE.pcen(x, out=torch.empty((1, 2, 3, 2), device=x.device))


# ---------------------------------------------------------------------------
# pipelines
# ---------------------------------------------------------------------------
def _cfg(name, *extra):
    from challenge_amd import sj_train as S
    return S.ARGS().get(['--name', name, '--v', '9', '--n_mels', '32', '--n_frame', '128', '--batch_size', '4',
                         '--synthetic', *extra])


def test_device_dataset_yields_pcen_of_the_raw_mel(monkeypatch):
    from challenge_amd import data_utils as D
    from challenge_amd import frontend as FE
    from challenge_amd import sj_train as S
    dev = _dev()
    got = next(iter(S.make_device_dataset(_cfg('pcen'), training=True, device=dev, seed=5)))
    monkeypatch.setattr(D, 'minmax_log_on_mel', lambda mel, labels=None: (mel, labels))   # the same batch, stage off
    raw = next(iter(S.make_device_dataset(_cfg(''), training=True, device=dev, seed=5)))
    assert torch.equal(got[1], raw[1])
    assert torch.equal(got[0], FE.pcen(raw[0]))


def test_wave_dataset_and_wave_frontend_yield_pcen_of_the_raw_mel(monkeypatch):
    from challenge_amd import frontend as FE
    from challenge_amd import sj_train as S
    dev = _dev()
    got = next(iter(S.make_wave_dataset(_cfg('pcen'), training=True, device=dev, seed=6)))
    real = FE.FrontendPlan.wav_to_logmel

    def raw_mel(self, wav, **kw):
        kw.update(minmax=False, log=False)
        return real(self, wav, **kw)

    monkeypatch.setattr(FE.FrontendPlan, 'wav_to_logmel', raw_mel)
    raw = next(iter(S.make_wave_dataset(_cfg(''), training=True, device=dev, seed=6)))
    monkeypatch.undo()
    assert torch.equal(got[1], raw[1])
    assert torch.equal(got[0], FE.pcen(raw[0]))
    # the default name is untouched: min-max + log as before
    dflt = next(iter(S.make_wave_dataset(_cfg(''), training=True, device=dev, seed=6)))
    assert float(dflt[0].max()) <= 1e-6 and not torch.equal(dflt[0], got[0])

    wav = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 1, 255 * 256)).astype(np.float32) * 0.1).to(dev)
    fe = S.WaveFrontend(1024, 256, 64, 16000, 1, 4, 255 * 256, dev, training=False, compression='pcen')
    plain = S.WaveFrontend(1024, 256, 64, 16000, 1, 4, 255 * 256, dev, training=False)
    assert torch.equal(fe(wav), FE.pcen(fe.plan.wav_to_logmel(wav, minmax=False, log=False)))
    assert torch.equal(plain(wav), plain.plan.wav_to_logmel(wav))
    # the captured frontend + forward of InferenceEngine takes the same features
    model = S.get_model(S.ARGS().get(['--v', '9', '--n_mels', '64', '--n_chan', '1', '--n_frame', '256'])).to(dev)
    model = model.to(memory_format=torch.channels_last).eval()
    eng = S.InferenceEngine(model, fe, wav)
    assert eng.graph_ok, eng.graph_error
    torch.testing.assert_close(eng.replay(), eng.eager(), rtol=1e-4, atol=1e-5)


def test_features_for_eval_selects_pcen():
    from challenge_amd import data_utils as D
    from challenge_amd import frontend as FE
    from challenge_amd import inference as I
    from challenge_amd import transforms as T
    dev = _dev()
    wav = np.random.default_rng(4).standard_normal((2, 16000 * 7)).astype(np.float32) * 0.1
    spec = D.load_wav_array(wav, 16000, dev)
    cfg = _cfg('pcen', '--n_chan', '2')
    inputs = D.stft_filter(int(round(256 * 1000 / 16000)))(spec)
    mel = T.magphase_to_mel(32, spec.shape[0])(T.complex_to_magphase(inputs))
    assert torch.equal(I.features_for_eval(spec, cfg), FE.pcen(mel))
    assert torch.equal(I.features_for_eval(spec, _cfg('', '--n_chan', '2')), D.log_on_mel(D.minmax(mel)))
    with pytest.raises(ValueError):
        I.features_for_eval(spec, _cfg('pcen_nominmax'))


def test_train_pcen_run_then_detect(tmp_path, monkeypatch):
    """Smoke check only (no accuracy claim): a short sj_train run with a 'pcen' name, then detection with its model."""
    from challenge_amd import detect as DT
    from challenge_amd import eval as E
    from challenge_amd import sj_train as S
    monkeypatch.chdir(tmp_path)
    S.main(['--synthetic', '--epochs', '1', '--steps_per_epoch', '2', '--validation_steps', '1', '--batch_size', '8',
            '--n_frame', '128', '--v', '9', '--n_mels', '32', '--name', 'pcen'])
    stem = 'pcen_vad_v9_lr0.001_batch8_opt_adam_mel32_chan2_BCE_framelen128'
    cfg = E.parse_name(S.ARGS().get(['--name', stem]))
    model = E.load_model(cfg, str(tmp_path), _dev())
    rng = np.random.default_rng(8)
    items = [("a", rng.standard_normal((2, 16000 * 9)).astype(np.float32) * 0.1),
             ("b", rng.standard_normal((2, 16000 * 4)).astype(np.float32) * 0.1)]
    res = DT.detect(model, items, cfg, overlap_hop=64)
    assert [r.name for r in res] == ["a", "b"]
    assert all(len(r.events) == 3 and r.n_frames == 1 + (16000 * s) // 256 for r, s in zip(res, (9, 4)))
    assert math.isfinite(float(sum(len(c) for r in res for c in r.events)))
