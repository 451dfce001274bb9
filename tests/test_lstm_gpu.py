"""GPU tests of the BiLSTM recurrence kernels at their own boundary (k_bilstm128_fwd / k_bilstm128_bwd, csrc/k_lstm.h, through
`frontend.bilstm128_forward(..., save=True)` / `bilstm128_backward`): the gate functions evaluated through a T = 1 launch, `out`
and all five saved planes against the float64 definition per element, `dgx` against the float64 backward (fed the kernel's own
activations, and end to end), row / direction independence and untouched guard floats bit for bit, the parameter gradients of
`bilstm128()` against nn.LSTM.double(), bit reproducibility (repeat, second stream, after another shape, graph replay) and the
refusals of `bilstm128_backward`.

The rules and their constants K_G, K_F, K_B come from tests/lstm_ref.py / tests/test_lstm_host.py (an fp32 yardstick, not this
kernel).  The kernel's own worst ratios on one MI355X (profiles/lstm/kernel_error_ratios.log): gates
sigmoid 1.47 u, tanh 2.95 u; forward 14.7 u (g plane, (7, 40), scale 2e-3; 13.1 u at scale 1.6, where the yardstick reads 20.5);
backward 7.4 u P fed its own activations, 50.2 u P end to end ((3, 1), scale 50; the yardstick: 14.7 / 26.1).  Every test prints
its figures per case."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import lstm_ref as L
from lstm_ref import BWD_SHAPES, F32, FWD_SHAPES, H, K_B, K_F, K_G, U

pytestmark = pytest.mark.gpu

SEED = 7     # not one of the yardstick sweep's seeds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fwd(dev, gx, w_hh):
    from challenge_amd import frontend as FE
    out, act = FE.bilstm128_forward(_t(dev, gx), _t(dev, w_hh), save=True)
    return out.cpu().numpy(), act.cpu().numpy()


def _bwd(dev, dout, act, w_hh):
    from challenge_amd import frontend as FE
    return FE.bilstm128_backward(_t(dev, dout), _t(dev, act), _t(dev, w_hh)).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------
# 1. the gate functions, through the kernel
# ---------------------------------------------------------------------------
def test_gate_functions_through_a_single_step(dev):
    """T = 1: h_0 = 0 makes the recurrent dot product exactly 0, so the four gate planes are lstm_sigmoid / lstm_tanh of gx element
    by element.  One launch sweeps `gate_grid()` and +-inf, placed in all four gate blocks."""
    vals = np.concatenate([L.gate_grid(), np.array([np.inf, -np.inf], F32)])
    b = -(-vals.size // (2 * H)) | 1                       # odd: the last workgroup has a padding row
    rng = np.random.default_rng(SEED)
    vals = np.concatenate([vals, rng.uniform(-20, 20, b * 2 * H - vals.size).astype(F32)]).reshape(b, 2, H)
    gx = np.ascontiguousarray(np.broadcast_to(vals[:, None, :, None, :], (b, 1, 2, 4, H))).reshape(b, 1, 2, 4 * H)
    w_hh = rng.uniform(-0.3, 0.3, (2, 4 * H, H)).astype(F32)
    out, act = _fwd(dev, gx, w_hh)
    gi, gf, gg, go, c = (act[:, 0, :, q] for q in range(5))
    sig, tanh = L.sigmoid64(vals), L.tanh64(vals)
    fin = np.isfinite(vals)
    worst = {}
    for name, got, ref in (("i", gi, sig), ("f", gf, sig), ("o", go, sig), ("g", gg, tanh)):
        worst[name] = float(L.gate_rule_ratio(got, ref).max())
        assert worst[name] <= K_G, (name, worst[name])
        lo, hi = (0.0, 1.0) if name != "g" else (-1.0, 1.0)
        assert np.all(np.isfinite(got[fin]) & (got[fin] >= lo) & (got[fin] <= hi)), name     # finite in, finite in range out
    yard = (float(L.gate_rule_ratio(L.sigmoid32(vals), sig).max()), float(L.gate_rule_ratio(L.tanh32(vals), tanh).max()))
    print(f"lstm_sigmoid: |s - s64| <= {max(worst['i'], worst['f'], worst['o']):.3f} u, lstm_tanh: {worst['g']:.3f} u "
          f"(library-form fp32 on the same arguments: {yard[0]:.3f} / {yard[1]:.3f} u; K_G = {K_G})")
    # the bound k_lstm.h states for its own formulas
    assert max(worst.values()) * U <= 3e-7, worst
    # exact limits
    pinf, ninf = vals == np.inf, vals == -np.inf
    assert pinf.sum() == 1 and ninf.sum() == 1
    for s in (gi, gf, go):
        assert np.all(s[pinf] == 1) and np.all(s[ninf] == 0)
    assert np.all(gg[pinf] == 1) and np.all(gg[ninf] == -1)
    assert np.all(gi[vals == 0] == 0.5) and np.all(gg[vals == 0] == 0)
    # the cell state of the first step is the fp32 product i g, and out obeys the forward rule
    assert np.array_equal(c, gi * gg) and (gi * gg).dtype == F32
    out_ref, act_ref = L.bilstm_ref(gx, w_hh)
    ro, ra = L.fwd_rule_ratio(out, act, out_ref, act_ref)
    print(f"T = 1 grid: out {ro.max():.3f} u, planes (i, f, g, o, c) {np.round(ra.max(axis=(0, 1, 2, 4)), 3)} (K_F = {K_F})")
    assert ro.max() <= K_F and ra.max() <= K_F
    # tanh = 2 sigmoid(2x) - 1 cancels for small arguments: the relative error there is reported, only the absolute rule is asserted
    small = (np.abs(vals) >= 1e-6) & (np.abs(vals) <= 1e-2)
    rel = lambda got: float((np.abs(got[small].astype(np.float64) - tanh[small]) / np.abs(tanh[small])).max())   # noqa: E731
    at = float(np.abs(vals[small][np.argmax(np.abs(gg[small].astype(np.float64) - tanh[small]) / np.abs(tanh[small]))]))
    print(f"lstm_tanh on 1e-6 <= |x| <= 1e-2 ({int(small.sum())} arguments): relative error <= {rel(gg):.3e} (at |x| = {at:.3g}), "
          f"absolute <= {float(np.abs(gg[small] - tanh[small]).max()) / U:.3f} u; library tanhf form: {rel(L.tanh32(vals)):.3e}")


def test_a_nan_argument_stays_in_its_element(dev):
    gx, w_hh, _ = L.make_case((3, 1), 1.6, 0.3, SEED)
    clean_out, clean_act = _fwd(dev, gx, w_hh)
    planted = [(1, 0, 0, 5), (1, 1, 1, 7), (2, 0, 2, 9), (0, 1, 3, 11), (2, 1, 0, 127)]       # (row, direction, gate, unit)
    bad = gx.copy()
    for b, d, q, u in planted:
        bad[b, 0, d, q * H + u] = np.nan
    out, act = _fwd(dev, bad, w_hh)
    want_gate = np.zeros((3, 1, 2, 5, H), bool)
    want_out = np.zeros((3, 1, 2 * H), bool)
    for b, d, q, u in planted:
        want_gate[b, 0, d, q, u] = True
        want_gate[b, 0, d, 4, u] |= q != 3                   # c = f c_prev + i g; the output gate does not enter it
        want_out[b, 0, d * H + u] = True
    assert np.array_equal(np.isnan(act), want_gate) and np.array_equal(np.isnan(out), want_out)
    assert np.array_equal(_bits(act)[~want_gate], _bits(clean_act)[~want_gate])
    assert np.array_equal(_bits(out)[~want_out], _bits(clean_out)[~want_out])


# ---------------------------------------------------------------------------
# 2. forward parity, per element
# ---------------------------------------------------------------------------
FWD_CASES = [(s, 1.6) for s in FWD_SHAPES] + [(s, sc) for s in ((3, 5), (7, 40), (2, 257)) for sc in (50.0, 2e-3)]


@pytest.mark.parametrize("shape,scale", FWD_CASES)
def test_forward_meets_the_rule_per_element(dev, shape, scale):
    gx, w_hh, _ = L.make_case(shape, scale, 0.3, SEED)
    out, act = _fwd(dev, gx, w_hh)
    assert out.shape == shape + (2 * H,) and act.shape == shape + (2, 5, H) and out.dtype == act.dtype == F32
    out_ref, act_ref = L.bilstm_ref(gx, w_hh)
    ro, ra = L.fwd_rule_ratio(out, act, out_ref, act_ref)
    print(f"k_bilstm128_fwd {shape} scale {scale}: out {ro.max():.3f} u, planes (i, f, g, o, c) {np.round(ra.max(axis=(0, 1, 2, 4)), 3)}, "
          f"directions {np.round(ra.max(axis=(0, 1, 3, 4)), 3)} (K_F = {K_F})")
    assert ro.max() <= K_F, (shape, scale, float(ro.max()))
    assert ra.max() <= K_F, (shape, scale, ra.max(axis=(0, 1, 2, 4)))


# ---------------------------------------------------------------------------
# 3. independence and indexing, bit for bit
# ---------------------------------------------------------------------------
def test_rows_and_directions_are_independent_bit_for_bit(dev):
    from challenge_amd import frontend as FE
    gx, w_hh, _ = L.make_case((5, 6), 1.6, 0.3, SEED)
    out, act = _fwd(dev, gx, w_hh)
    # every row of the batch == that row alone (first / second row of a workgroup, and the row beside the padding row)
    for r in range(5):
        o1, a1 = _fwd(dev, gx[r:r + 1], w_hh)
        assert _same_bits(o1[0], out[r]) and _same_bits(a1[0], act[r]), r
    # the reverse direction == the forward direction on the time-flipped input with the two recurrent matrices swapped
    o2, a2 = _fwd(dev, gx[:, ::-1, ::-1], w_hh[::-1])
    assert _same_bits(o2[:, ::-1, :H], out[:, :, H:]) and _same_bits(o2[:, ::-1, H:], out[:, :, :H])
    assert _same_bits(a2[:, ::-1, ::-1], act)
    # a NaN row changes no other row's bits, its workgroup partner's included
    for r, partner in ((2, 3), (1, 0), (4, None)):
        bad = gx.copy()
        bad[r] = np.nan
        o3, a3 = _fwd(dev, bad, w_hh)
        keep = [k for k in range(5) if k != r]
        assert np.isnan(o3[r]).all() and np.isnan(a3[r]).all()
        assert _same_bits(o3[keep], out[keep]) and _same_bits(a3[keep], act[keep]), (r, partner)
    # save = False returns the same bits
    plain = FE.bilstm128_forward(_t(dev, gx), _t(dev, w_hh)).cpu().numpy()
    assert _same_bits(plain, out)


def test_floats_beyond_the_tensors_stay_untouched(dev):
    """Odd B: the last workgroup's second row does not exist; nothing may be written for it."""
    from challenge_amd import _native as N
    lib = N.lib()
    for b, t in ((3, 5), (1, 1), (5, 2)):
        gx, w_hh, dout = L.make_case((b, t), 1.6, 0.3, SEED)
        out, act = _fwd(dev, gx, w_hh)
        dgx = _bwd(dev, dout, act, w_hh)
        pad = 2 * t * 5 * H + 64                              # more than a whole row of the largest tensor
        gx_d, w_d, dout_d, act_d = _t(dev, gx), _t(dev, w_hh), _t(dev, dout), _t(dev, act)
        n_out, n_act, n_dgx = b * t * 2 * H, b * t * 2 * 5 * H, b * t * 2 * 4 * H
        out_b = torch.full((n_out + pad,), -7.0, device=dev)
        act_b = torch.full((n_act + pad,), -7.0, device=dev)
        dgx_b = torch.full((n_dgx + pad,), -7.0, device=dev)
        torch.cuda.synchronize()
        N.check(lib.iris_bilstm128_forward(gx_d.data_ptr(), w_d.data_ptr(), out_b.data_ptr(), act_b.data_ptr(), b, t, None), "forward")
        N.check(lib.iris_bilstm128_backward(dout_d.data_ptr(), act_d.data_ptr(), w_d.data_ptr(), dgx_b.data_ptr(), b, t, None), "backward")
        torch.cuda.synchronize()
        for buf, n, want in ((out_b, n_out, out), (act_b, n_act, act), (dgx_b, n_dgx, dgx)):
            assert bool((buf[n:] == -7.0).all()), (b, t, n)
            assert _same_bits(buf[:n].cpu().numpy(), want.reshape(-1)), (b, t, n)
        # the launch without saved activations writes `out` only
        out_c = torch.full((n_out + pad,), -7.0, device=dev)
        N.check(lib.iris_bilstm128_forward(gx_d.data_ptr(), w_d.data_ptr(), out_c.data_ptr(), None, b, t, None), "forward")
        torch.cuda.synchronize()
        assert torch.equal(out_c, out_b)


# ---------------------------------------------------------------------------
# 4. backward parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.6, 50.0])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_backward_meets_the_rule_per_element(dev, shape, scale):
    gx, w_hh, dout = L.make_case(shape, scale, 0.3, SEED)
    out, act = _fwd(dev, gx, w_hh)
    dgx = _bwd(dev, dout, act, w_hh)
    assert dgx.shape == shape + (2, 4 * H) and dgx.dtype == F32
    own = L.bwd_rule_ratio(dgx, L.bilstm_bwd_ref(dout, act, w_hh))               # fed the kernel's own activations
    e2e = L.bwd_rule_ratio(dgx, L.bilstm_bwd_ref(dout, L.bilstm_ref(gx, w_hh)[1], w_hh))
    print(f"k_bilstm128_bwd {shape} scale {scale}: fed its own act {own.max():.3f} u P (gates i, f, g, o "
          f"{np.round(own.reshape(shape + (2, 4, H)).max(axis=(0, 1, 2, 4)), 3)}), end to end {e2e.max():.3f} u P (K_B = {K_B})")
    assert own.max() <= K_B, (shape, scale, float(own.max()))
    assert e2e.max() <= K_B, (shape, scale, float(e2e.max()))
    if shape[1] == 1:     # c_{-1} = 0: no gradient into the forget gate's pre-activation
        assert np.count_nonzero(dgx[:, :, :, H:2 * H]) == 0


def test_backward_zero_and_nan_gradients_stay_where_they_are(dev):
    gx, w_hh, dout = L.make_case((5, 7), 1.6, 0.3, SEED)
    _, act = _fwd(dev, gx, w_hh)
    full = _bwd(dev, dout, act, w_hh)
    assert np.count_nonzero(full) > 0.9 * full.size     # (the forget gate's plane of each direction's first step is 0)
    for d in range(2):     # dout zero in one direction: exactly no gradient there, the other direction's bits unchanged
        part = dout.copy()
        part[:, :, d * H:(d + 1) * H] = 0
        got = _bwd(dev, part, act, w_hh)
        assert np.count_nonzero(got[:, :, d]) == 0 and _same_bits(got[:, :, 1 - d], full[:, :, 1 - d]), d
    for r in (2, 3, 4):    # dout zero for one row (first / second row of a workgroup, the row beside the padding row)
        part = dout.copy()
        part[r] = 0
        got = _bwd(dev, part, act, w_hh)
        keep = [k for k in range(5) if k != r]
        assert np.count_nonzero(got[r]) == 0 and _same_bits(got[keep], full[keep]), r
    for r, t, col in ((3, 4, 10), (2, 6, 200), (4, 0, 255)):    # one NaN in row r stays in row r, and in its direction
        part = dout.copy()
        part[r, t, col] = np.nan
        got = _bwd(dev, part, act, w_hh)
        keep = [k for k in range(5) if k != r]
        d = col // H
        assert np.isnan(got[r, t, d]).any() and not np.isnan(got[keep]).any() and not np.isnan(got[r, :, 1 - d]).any()
        assert _same_bits(got[keep], full[keep]) and _same_bits(got[r, :, 1 - d], full[r, :, 1 - d]), r


def test_single_step_has_no_recurrent_gradient(dev):
    from challenge_amd.hip_autograd import _BiLSTM128
    gx, w_hh, dout = L.make_case((3, 1), 1.6, 0.3, SEED)
    gx_d, w_d = _t(dev, gx).requires_grad_(True), _t(dev, w_hh).requires_grad_(True)
    out = _BiLSTM128.apply(gx_d, w_d)
    out.backward(_t(dev, dout))
    assert w_d.grad.shape == (2, 4 * H, H) and int(torch.count_nonzero(w_d.grad)) == 0
    dgx = gx_d.grad.cpu().numpy()
    assert np.count_nonzero(dgx[:, :, :, H:2 * H]) == 0 and np.count_nonzero(dgx[:, :, :, :H]) > 0
    # dW_hh of _BiLSTM128 for T > 1 is the reference's h_prev shift applied to the kernel's own dgx and out
    gx, w_hh, dout = L.make_case((3, 4), 1.6, 0.3, SEED)
    gx_d, w_d = _t(dev, gx).requires_grad_(True), _t(dev, w_hh).requires_grad_(True)
    out = _BiLSTM128.apply(gx_d, w_d)
    out.backward(_t(dev, dout))
    ref = L.dw_hh_ref(gx_d.grad.cpu().numpy(), out.detach().cpu().numpy())
    err = np.abs(w_d.grad.cpu().numpy() - ref).max()
    print(f"_BiLSTM128 dW_hh (3, 4): |dW - ref| <= {err / np.abs(ref).max():.2e} of the peak")
    assert err <= 2e-5 * np.abs(ref).max() + 1e-6


# ---------------------------------------------------------------------------
# 5. parameter gradients through bilstm128()
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lstm_pair(dev):
    torch.manual_seed(12)
    lstm = torch.nn.LSTM(128, 128, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for p in lstm.parameters():
            p.uniform_(-0.3, 0.3)
    ref64 = copy.deepcopy(lstm).double()
    return lstm.to(dev), ref64


@pytest.mark.parametrize("b,t", [(3, 1), (2, 2), (5, 7), (64, 16)])
def test_parameter_gradients_match_float64(dev, lstm_pair, b, t):
    from challenge_amd import sj_train as S
    lstm, ref64 = lstm_pair
    stock = copy.deepcopy(lstm)
    g = torch.Generator().manual_seed(1000 * b + t)
    x, dy = torch.randn(b, t, 128, generator=g), torch.randn(b, t, 256, generator=g)
    x64 = x.double().requires_grad_(True)
    ref64.zero_grad()
    y64, _ = ref64(x64)
    y64.backward(dy.double())
    want = {"y": y64.detach(), "dx": x64.grad, **{n: p.grad for n, p in ref64.named_parameters()}}

    def run(module, call):
        module.zero_grad()
        xd = x.to(dev).requires_grad_(True)
        y = call(module, xd)
        y.backward(dy.to(dev))
        got = {"y": y.detach(), "dx": xd.grad, **{n: p.grad for n, p in module.named_parameters()}}
        return y, {n: float((v.double().cpu() - want[n]).abs().max()) for n, v in got.items()}

    y, hip = run(lstm, S.bilstm128)
    assert y.grad_fn.name().startswith("_BiLSTM128")
    _, miopen = run(stock, lambda m, v: m(v)[0])
    for n, ref in want.items():
        peak = float(ref.abs().max())
        print(f"bilstm128 ({b}, {t}) {n}: |. - fp64| = {hip[n]:.2e} = {hip[n] / max(peak, 1e-30):.2e} of the peak "
              f"(torch.nn.LSTM fp32 on the device: {miopen[n]:.2e})")
        assert hip[n] <= 2e-5 * peak + 1e-6, (n, b, t, hip[n], peak)


# ---------------------------------------------------------------------------
# 6. reproducibility
# ---------------------------------------------------------------------------
def test_repeat_second_stream_other_shape_and_graph_replay_are_bitwise_equal(dev):
    from challenge_amd import _native as N
    from challenge_amd import frontend as FE
    gx, w_hh, dout = (_t(dev, a) for a in L.make_case((5, 9), 1.6, 0.3, SEED))

    def both():
        out, act = FE.bilstm128_forward(gx, w_hh, save=True)
        return out, act, FE.bilstm128_backward(dout, act, w_hh)

    first = both()
    again = both()
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = both()
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(first, other))
    gx2, w2, dout2 = (_t(dev, a) for a in L.make_case((2, 3), 50.0, 0.25, SEED))     # another shape in between
    o2, a2 = FE.bilstm128_forward(gx2, w2, save=True)
    FE.bilstm128_backward(dout2, a2, w2)
    assert all(torch.equal(a, b) for a, b in zip(first, both()))
    # both launches captured into one graph (a single chain) and replayed
    out_g, act_g, dgx_g = (torch.zeros_like(v) for v in first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc1 = N.lib().iris_bilstm128_forward(gx.data_ptr(), w_hh.data_ptr(), out_g.data_ptr(), act_g.data_ptr(), 5, 9, stream)
        rc2 = N.lib().iris_bilstm128_backward(dout.data_ptr(), act_g.data_ptr(), w_hh.data_ptr(), dgx_g.data_ptr(), 5, 9, stream)
    assert rc1 == 0 and rc2 == 0
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, (out_g, act_g, dgx_g)))
    gx.copy_(gx.flip(1))                                     # a replay reads the new contents of the same addresses
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(both(), (out_g, act_g, dgx_g))) and not torch.equal(out_g, first[0])


# ---------------------------------------------------------------------------
# 7. refusals of bilstm128_backward
# ---------------------------------------------------------------------------
def test_backward_refuses_before_any_launch(dev):
    """Every tensor float32, on the device, on ONE device, exact shapes: a host `act` or `w_hh` used to reach the kernel as a
    host pointer.  Each call raises in the wrapper's checks (ValueError), before `.contiguous()` and before the launch."""
    from challenge_amd import frontend as FE
    dout, act, w_hh = torch.zeros(2, 3, 256, device=dev), torch.zeros(2, 3, 2, 5, 128, device=dev), torch.zeros(2, 512, 128, device=dev)
    assert FE.bilstm128_backward(dout, act, w_hh).shape == (2, 3, 2, 512)
    bad = [(dout, act.cpu(), w_hh), (dout, act, w_hh.cpu()), (dout.cpu(), act, w_hh), (dout, act, w_hh.double()),
           (dout, act.double(), w_hh), (dout, act.view(2, 3, 2, 640), w_hh), (dout, act.view(2, 3, 10, 128), w_hh),
           (dout, act[:, :2], w_hh), (dout.view(6, 256), act, w_hh)]
    if torch.cuda.device_count() > 1:
        far = torch.device("cuda", 1)
        bad += [(dout, act, w_hh.to(far)), (dout, act.to(far), w_hh)]
    for args in bad:
        with pytest.raises(ValueError):
            FE.bilstm128_backward(*args)
