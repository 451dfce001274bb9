"""GPU tests of the weight EMA inside the fused AGC + clipvalue + Adam launch: iris_agc_clip_adam_ema (csrc/k_agc_adam.h) called
through `_native.lib()` on six-column row tables built by hand between sentinels - as tests/test_agc_gpu.py builds the five-column
ones - against the float64 definition of tests/ema_ref.py; then `FusedAGC.attach_ema`, `WeightEMA`, `GraphedTrainStep` and
`recalibrate_bn` on a small model.  Every element of x, m', v', p' and e' of every row is held to its bound (`ema_ref.bounds`; K_E
from two float32 evaluations on the CPU, tests/test_ema_host.py), and x, m', v', p' must have the bits iris_agc_clip_adam leaves on
the same inputs.  Each comparison prints, per quantity, the kernel's worst ratio to its bound and its worst error over the float32
yardstick's on the same case; DESIGN.md records the worst.

Twins.  A row that starts 4 bytes off alignment takes the scalar path, its aligned twin the float4 path.  Everything after the
clip factor is the same element-wise arithmetic on both, so twins have equal bits wherever their clip factors do: in every row
whose factor is 1, and in every row when AGC is off - both asserted.  The factor itself comes from two sums of squares that the two
paths add up in different orders (iris_agc_clip_adam's own, unchanged here); where it differs by a rounding the twins are held to
twice the bound, as tests/test_agc_gpu.py holds them, and the number of such elements is printed."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import agc_ref as R
import ema_ref as E
from agc_ref import EDGE_ROWS, F32, F64

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0xC2F6E979], np.uint32).view(F32)[0]      # -123.456
NAMES = {"x": "g", "m": "m", "v": "v", "p": "p", "e": "e"}     # quantity -> the buffer it comes back in
BUFS = "pgmve"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Table:
    """The case's rows in five device buffers (p, g, m, v, e) between sentinels, and a row table over them: six columns for
    iris_agc_clip_adam_ema (`ema`), or the first five for iris_agc_clip_adam, which must leave the e buffer alone."""

    def __init__(self, dev, case, ema=True):
        self.dev, self.case, self.ema = dev, case, ema
        self.slots, cursor = [], 8                          # (group, first row, rows, base float index); the base is a multiple of 4
        for gi, grp in enumerate(case["groups"]):
            rows, length = grp["p"].shape
            for r0, n in ([(0, rows)] if grp["packed"] else [(r, 1) for r in range(rows)]):
                self.slots.append((gi, r0, n, cursor))
                cursor = -(-(cursor + 1 + n * length) // 4) * 4 + 4
        self.host = {q: np.full(cursor + 8, SENTINEL, F32) for q in BUFS}
        self.rows_at = {q: np.zeros(cursor + 8, bool) for q in BUFS}
        cols, lens = {q: [] for q in BUFS}, []
        for gi, r0, n, base in self.slots:
            grp = case["groups"][gi]
            length = grp["p"].shape[1]
            for q in BUFS:
                start = base + grp["mis"][q]
                self.host[q][start:start + n * length] = grp[q][r0:r0 + n].reshape(-1)
                self.rows_at[q][start:start + n * length] = True
                cols[q].append(start + np.arange(n, dtype=np.int64) * length)
            lens.append(np.full(n, length, np.int64))
        self.start = {q: np.concatenate(cols[q]) for q in BUFS}
        self.len = np.concatenate(lens)
        self.buf = {q: torch.from_numpy(self.host[q]).to(dev) for q in BUFS}
        assert all(b.data_ptr() % 16 == 0 for b in self.buf.values())
        table = np.empty((self.len.size, 6 if ema else 5), np.int64)
        table[:, 2] = self.len
        for col, q in ((0, "p"), (1, "g"), (3, "m"), (4, "v")) + (((5, "e"),) if ema else ()):
            table[:, col] = self.buf[q].data_ptr() + 4 * self.start[q]
        # every row inside its buffer, no two rows of a buffer overlapping: checked before anything runs
        for q in BUFS:
            assert self.start[q].min() >= 4 and (self.start[q] + self.len).max() <= self.host[q].size - 4
            assert int(self.rows_at[q].sum()) == int(self.len.sum())
            order = np.argsort(self.start[q])
            assert np.all((self.start[q] + self.len)[order][:-1] <= self.start[q][order][1:])
        self.table_host, self.table = table, torch.from_numpy(table).to(dev)
        sc = case["sc"]
        self.step = torch.tensor(float(sc["t"]), dtype=torch.float32, device=dev)
        self.lr = torch.tensor(float(sc["lr"]), dtype=torch.float32, device=dev) if sc["lr_dev"] else None

    def set_gradient(self, groups):
        """A new gradient into the same buffer (the rows keep their addresses)."""
        for gi, r0, n, base in self.slots:
            g, length = groups[gi]["g"], groups[gi]["g"].shape[1]
            start = base + self.case["groups"][gi]["mis"]["g"]
            self.host["g"][start:start + n * length] = g[r0:r0 + n].reshape(-1)
        self.buf["g"].copy_(torch.from_numpy(self.host["g"]))

    def launch(self, sc=None):
        from challenge_amd import _native as N
        sc = sc or self.case["sc"]
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        head = (self.table.data_ptr(), int(self.table.shape[0]), float(sc["clip_factor"]), float(sc["eps_agc"]), float(sc["clipvalue"]),
                int(sc["use_agc"]), self.lr.data_ptr() if self.lr is not None else None, 0.0 if self.lr is not None else float(sc["lr"]),
                float(sc["beta1"]), float(sc["beta2"]), float(sc["eps"]), self.step.data_ptr())
        with torch.cuda.device(self.dev):
            if self.ema:
                N.check(N.lib().iris_agc_clip_adam_ema(*head, float(sc["decay"]), stream), "iris_agc_clip_adam_ema")
            else:
                N.check(N.lib().iris_agc_clip_adam(*head, stream), "iris_agc_clip_adam")

    def read(self):
        """-> per group {'x', 'm', 'v', 'p' and with `ema` 'e'} [rows, len]; the sentinels around every row bit for bit, the row
        table unchanged, and without `ema` the whole e buffer unchanged."""
        torch.cuda.synchronize(self.dev)
        back = {q: self.buf[q].cpu().numpy() for q in BUFS}
        for q in BUFS:
            off = ~self.rows_at[q]
            assert np.array_equal(_bits(back[q][off]), _bits(self.host[q][off])), f"a float beside a row of {q} was written"
        assert np.array_equal(self.table.cpu().numpy(), self.table_host), "the row table was written"
        if not self.ema:
            assert np.array_equal(_bits(back["e"]), _bits(self.host["e"])), "iris_agc_clip_adam wrote e"
        out = [dict() for _ in self.case["groups"]]
        for name, q in NAMES.items():
            if name == "e" and not self.ema:
                continue
            for gi, grp in enumerate(self.case["groups"]):
                out[gi][name] = np.empty(grp["p"].shape, F32)
            for gi, r0, n, base in self.slots:
                grp = self.case["groups"][gi]
                length = grp["p"].shape[1]
                start = base + grp["mis"][q]
                out[gi][name][r0:r0 + n] = back[q][start:start + n * length].reshape(n, length)
        return out


def _run(dev, case, ema=True):
    tab = Table(dev, case, ema)
    tab.launch()
    return tab.read()


def _same_bits(what, a, b, names=None):
    """Two runs of a case: equal bits in every quantity (or in `names`) of every row."""
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        for name in (names or ga):
            assert np.array_equal(_bits(ga[name]), _bits(gb[name])), (what, name)


_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """After the module's tests: the worst ratio of every quantity to its bound, in one place (print only; `_compare` asserts)."""
    yield
    for name, (ratio, what) in sorted(_SEEN.items()):
        print(f"\nworst {name}: {ratio:.3f} of its bound at {what}", end="")
    print()


def _compare(what, case, got, ref=None):
    """Print, per quantity, the kernel's worst ratio to its bound and its worst error over the yardstick's; then assert the bounds."""
    ref = ref or E.reference(case)
    yard = E.reference(case, F32)
    worst, late = {}, []
    for gi, (grp, r, y, g) in enumerate(zip(case["groups"], ref, yard, got)):
        mine = E.errors(g, r, grp, case["sc"])
        theirs = E.errors({k: y[k] for k in g}, r, grp, case["sc"])
        for name, (ratio, err) in mine.items():
            w = worst.setdefault(name, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], ratio), max(w[1], err), max(w[2], theirs[name][1])
            if not ratio <= 1.0:
                late.append((gi, grp["p"].shape, name, ratio))
    for name, (ratio, err, yerr) in worst.items():
        print(f"{what} {name}: {ratio:.3f} of its bound; |. - fp64| = {err:.3e}, {err / yerr if yerr > 0 else float(err > 0):.2f} x the float32 yardstick ({yerr:.3e})")
        seen = _SEEN.setdefault(name, [0.0, ""])
        if ratio > seen[0]:
            seen[0], seen[1] = ratio, what
    assert not late, (what, late)


def _both(dev, what, case):
    """One case through iris_agc_clip_adam_ema twice and through iris_agc_clip_adam once: all five quantities inside their bounds,
    two runs equal bits, and x, m', v', p' the bits of the launch without the EMA.  -> (what came back, the float64 reference)."""
    got, ref = _run(dev, case), E.reference(case)
    assert all(set(g) == set(E.QUANTITIES) for g in got)
    _compare(what, case, got, ref)
    _same_bits(what + ": two runs", got, _run(dev, case))
    _same_bits(what + ": against iris_agc_clip_adam", got, _run(dev, case, ema=False), names=R.QUANTITIES)
    return got, ref


# ---------------------------------------------------------------------------
# lengths, alignment, the row loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_agc", [1, 0], ids=["agc", "no-agc"])
def test_lengths_and_alignment(dev, use_agc):
    """Lengths 1 .. 4608 and two rows of 70,000 on both paths; the twins that start 4 bytes off alignment - all five pointers, only
    one moment's, only the shadow's - take the scalar path (see the module docstring for what twins must share)."""
    case = E.lengths_case(E.scalars(use_agc=use_agc))
    got, ref = _both(dev, f"lengths use_agc={use_agc}", case)
    for gi, twin in case["twins"]:
        lim = E.bounds(case["groups"][gi], ref[gi], case["sc"])
        same = ref[gi]["s"][:, 0] == 1
        assert same.any() and (use_agc or same.all())
        apart = 0
        for name in got[gi]:
            assert np.array_equal(_bits(got[gi][name][same]), _bits(got[twin][name][same])), (gi, name)
            assert np.all(np.abs(got[gi][name].astype(F64) - got[twin][name]) <= 2 * lim[name]), (gi, name)
            apart += int((_bits(got[gi][name]) != _bits(got[twin][name])).sum())
        print(f"twin {gi} (mis {case['groups'][gi]['mis']}) of group {twin}: {apart} elements with other bits than the aligned rows'")


def test_row_loop_takes_a_second_trip(dev):
    """32,773 rows of 5: five more than the grid has waves (8192 x 4), so the last five are a wave's second row."""
    case = E.rowloop_case()
    assert case["groups"][0]["p"].shape == (32768 + 5, 5)
    _both(dev, "row loop", case)


# ---------------------------------------------------------------------------
# the edges of the definition, NaN
# ---------------------------------------------------------------------------
def test_edges_and_a_nan(dev):
    """agc_ref's edge rows without and with one NaN in one unit's gradient: that unit's x, m', v', p' and - the parameter being lost
    - its e' turn NaN; every other row, shadow included, equals the run without it bit for bit."""
    clean, dirty = E.edges_case(), E.edges_case(nan=True)
    a, _ = _both(dev, "edges", clean)
    b, _ = _both(dev, "edges with a NaN", dirty)
    hit = EDGE_ROWS.index("above")
    others = np.arange(len(EDGE_ROWS)) != hit
    for ga, gb in zip(a, b):
        assert all(np.isfinite(v).all() for v in ga.values())
        for name in ga:
            assert np.isnan(gb[name][hit]).all(), (name, gb[name][hit])
            assert np.array_equal(_bits(ga[name][others]), _bits(gb[name][others])), name


# ---------------------------------------------------------------------------
# the counter and the decay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("decay", E.DECAYS, ids=lambda d: f"decay-{d}")
def test_counter_and_decay(dev, decay):
    """t in {1, 2, 10, 1000, 100000} x eps x lr source for one decay: the warm-up side and the capped side of min(decay, (1 + t) /
    (10 + t)).  A decay of 0 gives w = 1: e' = e + (p' - e), p' to the rounding of that difference."""
    cases = [c for c in E.constants_cases() if c["sc"]["decay"] == decay]
    assert len(cases) == 20
    for case in cases:
        got, _ = _both(dev, case["name"], case)
        if decay == 0.0:
            assert float(E.weight(case["sc"])) == 1.0
            assert all(np.all(np.abs(g["e"].astype(F64) - g["p"]) <= 2.0 ** -23 * np.maximum(np.abs(g["p"]), np.abs(grp["e"])))
                       for g, grp in zip(got, case["groups"]))


def _walk(dev, name, n, captured):
    """`n` consecutive launches on one table (t = 7 ..., a new gradient each, the learning rate changing), eagerly or as replays of
    ONE captured launch behind the counter's increment: each is held to the definition applied to what the launch before left in
    the buffers - the shadow's bound carried forward in that sense.  -> everything that came back."""
    start = E.chain_start(name)
    first = E.chain_next(start, None, 0)
    tab = Table(dev, first)
    graph = None
    if captured:
        assert start["sc"]["lr_dev"]
        tab.step.fill_(6.0)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tab.step.add_(1)
            tab.launch(first["sc"])
        torch.cuda.synchronize(dev)
        back = {q: tab.buf[q].cpu().numpy() for q in BUFS}
        assert all(np.array_equal(_bits(back[q]), _bits(tab.host[q])) for q in BUFS) and float(tab.step) == 6.0   # nothing has run yet
    state, seen = None, []
    for k in range(n):
        case = E.chain_next(start, state, k)
        if k or captured:
            tab.set_gradient(case["groups"])
        if captured:
            tab.lr.fill_(float(case["sc"]["lr"]))
            graph.replay()
        else:
            if k:
                tab.step.add_(1)
            tab.launch(case["sc"])
        got = tab.read()
        assert float(tab.step) == 7.0 + k
        _compare(f"{name} {k + 1} of {n}", case, got)
        state = [{q: g[q] for q in "pmve"} for g in got]
        for q in "pmve":                               # what the next launch starts from is what this one left (sentinel check: `read`)
            tab.host[q] = tab.buf[q].cpu().numpy()
        seen += got
    return seen


def test_four_launches_from_a_running_state(dev):
    _same_bits("four launches", _walk(dev, "chain", 4, False), _walk(dev, "chain", 4, False))


def test_captured_launch_replays_with_new_counter_and_lr(dev):
    """One launch captured into a torch.cuda.graph (a single chain, no parallel branches) and replayed three times: the weight of
    the average follows the device-side counter with nothing re-recorded."""
    _same_bits("captured launch", _walk(dev, "capture", 3, True), _walk(dev, "capture", 3, True))


# ---------------------------------------------------------------------------
# FusedAGC.attach_ema, WeightEMA and GraphedTrainStep on a model
# ---------------------------------------------------------------------------
DECAY = 0.999


def _model(dev, capturable=False, ema=True, seed=3):
    from challenge_amd import sj_train as S
    from challenge_amd.ema import WeightEMA
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(seed)
    m = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    avg = WeightEMA(m, DECAY) if ema else None
    m.compile(S.make_optimizer(cfg, m.parameters(), capturable=capturable), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=avg)
    return m, avg


def _batches(dev, n, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 32, 64, 1, generator=g).to(dev), (torch.rand(4, 2, 3, generator=g) < 0.3).float().to(dev)) for _ in range(n)]


def _flat(tensors):
    """Dense parameter-shaped device tensors -> NumPy, each in the order of its memory."""
    return [t.detach().as_strided((t.numel(),), (1,)).cpu().numpy().copy() for t in tensors]


def _three_steps(dev, how, probe=None):
    """3 steps of the small model with a WeightEMA compiled in -> (model, ema, shadows before, parameters recorded after each
    step, shadows after, `predict(probe)` of the EMA module before the steps)."""
    from challenge_amd import sj_train as S
    model, ema = _model(dev, capturable=how == "graph")
    before = None
    if probe is not None:
        before = ema.module.predict(probe).clone()
        assert torch.equal(before, ema.module.predict(probe))
    e0, recorded = _flat(ema.shadow), []
    batches = _batches(dev, 3)
    if how == "graph":
        step = S.GraphedTrainStep(model, batches[0], preserve_state=True)
        torch.cuda.synchronize(dev)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(e0, _flat(ema.shadow))), "the warm-up steps left a trace in the shadow"
        assert step._agc.ema_attached and step._agc._table.shape[1] == 6
    else:
        step = model.train_step
    for batch in batches:
        step(batch)
        torch.cuda.synchronize(dev)
        recorded.append(_flat(model.parameters()))
    assert float(model.optimizer.state[next(model.parameters())]["step"]) == 3.0
    return model, ema, e0, recorded, _flat(ema.shadow), before


@pytest.mark.parametrize("how", ["eager", "graph", "torch"])
def test_shadow_follows_the_float64_recurrence(dev, how):
    """Model v9 at 32 mel x 64 frames, mono, batch 4, 3 steps: after eager fused steps, after GraphedTrainStep replays and after the
    torch fallback (the fused Adam launch switched off) the shadow is held to the float64 recurrence over that run's own recorded
    parameters; `predict` on the EMA module sees the new average."""
    from challenge_amd import sj_train as S
    x = _batches(dev, 1, seed=22)[0][0]
    assert S.FUSED_ADAM
    try:
        S.FUSED_ADAM = how != "torch"
        model, ema, e0, recorded, got, before = _three_steps(dev, how, probe=x)
        if how == "eager":
            assert model._fused_agc._adam is model.optimizer and model._fused_agc.ema_attached and model._fused_agc._table.shape[1] == 6
        elif how == "torch":
            assert model._fused_agc._adam is None and model._fused_agc._table.shape[1] == 3
    finally:
        S.FUSED_ADAM = True
    E.recurrence_check(f"model, {how}", e0, recorded, got, DECAY)
    assert sum(not np.array_equal(a, b) for a, b in zip(e0, got)) > len(e0) // 2
    after = ema.module.predict(x)
    assert not ema.module.training and torch.isfinite(after).all() and not torch.equal(after, before)   # its engine was rebuilt


def test_live_model_does_not_notice_the_ema(dev):
    """The live parameters after 3 eager steps are bit-identical with and without an EMA attached; without one FusedAGC still
    builds the five-column table and calls the old entry point."""
    with_ema, _, _, recorded, _, _ = _three_steps(dev, "eager")
    plain, none = _model(dev, ema=False)
    assert none is None
    for batch in _batches(dev, 3):
        plain.train_step(batch)
    torch.cuda.synchronize(dev)
    assert plain._fused_agc._adam is plain.optimizer and not plain._fused_agc.ema_attached and plain._fused_agc._table.shape[1] == 5
    for (name, _), a, b in zip(plain.named_parameters(), _flat(plain.parameters()), recorded[-1]):
        assert np.array_equal(_bits(a), _bits(b)), name
    for (name, a), b in zip(plain.named_buffers(), with_ema.buffers()):
        assert torch.equal(a, b), name
    # detaching puts the five-column table back
    agc = with_ema._fused_agc
    assert agc._cols() == 6 and agc.attach_ema(None) is False and agc._cols() == 5


# ---------------------------------------------------------------------------
# BatchNorm recalibration on the device
# ---------------------------------------------------------------------------
def test_recalibrate_bn_on_the_device(dev):
    """3 batches of 4 (32 mel x 64 frames, mono): `recalibrate_bn` on the device model - the fused conv + BatchNorm passes, momentum
    1 / (k + 1) per call - against torch.optim.swa_utils.update_bn on a float64 CPU copy, within four times the distance of the
    float32 CPU result from that float64 one (measured here, printed)."""
    from torch.optim.swa_utils import update_bn
    from challenge_amd import sj_train as S
    from challenge_amd.ema import recalibrate_bn
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(3)
    host = S.get_model(cfg)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(4, 32, 64, 1, generator=g) for _ in range(3)]

    def stats(m):
        return {n: b.detach().double().cpu().numpy().copy() for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var"))}
    yard = []
    for dtype in (torch.float32, torch.float64):
        m = copy.deepcopy(host).to(dtype)
        update_bn([x.to(dtype) for x in xs], m)
        yard.append(stats(m))
    tol = {n: 4.0 * float(np.abs(yard[0][n] - yard[1][n]).max()) for n in yard[0]}
    S.configure_miopen()
    model = copy.deepcopy(host).to(dev).to(memory_format=torch.channels_last).eval()
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert recalibrate_bn(model, [x.to(dev) for x in xs]) == 3
    torch.cuda.synchronize(dev)
    assert not model.training and all(bn.momentum == 0.01 for bn in bns)
    got = stats(model)
    ratios = {n: float(np.abs(got[n] - yard[1][n]).max()) / tol[n] for n in got}
    worst = max(ratios, key=ratios.get)
    print(f"recalibrate_bn on the device vs float64: worst {ratios[worst]:.3f} of the tolerance at {worst} "
          f"(|.| = {ratios[worst] * tol[worst]:.3e}, 4 x |float32 - float64| = {tol[worst]:.3e})")
    assert len(got) == 36 and ratios[worst] <= 1.0, {n: r for n, r in ratios.items() if r > 1.0}
