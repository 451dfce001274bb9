"""GPU tests of the sgd / rmsprop optimiser tail in one launch: iris_agc_clip_sgd, iris_agc_clip_rmsprop and their _ema siblings
(csrc/k_agc_optim.h) called through `_native.lib()` on row tables built by hand between sentinels - as tests/test_ema_gpu.py builds
them - against the float64 definition of tests/optim_ref.py; then `FusedAGC.attach_optimizer` / `optimizer_step`, `make_optimizer`,
`GraphedTrainStep` and `fit` on a small model.  Every element of x, b', s', p' and e' of every row is held to its bound
(`optim_ref.bounds`; the constants from two float32 evaluations on the CPU, tests/test_optim_host.py), and the launch without the EMA
must leave the bits of the launch with it.  Each comparison prints, per quantity, the kernel's worst ratio to its bound; the module
prints the worst per kernel at its end.

Quantities come back under agc_ref's names: 'm' is the momentum buffer b', 'v' rmsprop's square average s'.  For sgd the row's
`exp_avg_sq` slot points at the v buffer, which the launch must hand back untouched, bit for bit.  Twins (rows 4 bytes off
alignment) are held as tests/test_ema_gpu.py holds them."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import agc_ref as R
import ema_ref as E
import optim_ref as O
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
    """The case's rows in five device buffers (p, g, m, v, e) between sentinels and a row table over them: six columns for the
    _ema entry points (`ema`), else the first five.  Buffers the entry point has no business with - e without `ema`, v for sgd -
    must come back whole."""

    def __init__(self, dev, case, ema=True):
        self.dev, self.case, self.ema, self.kind = dev, case, ema, case["sc"]["kind"]
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
        args = (self.table.data_ptr(), int(self.table.shape[0]), float(sc["clip_factor"]), float(sc["eps_agc"]), float(sc["clipvalue"]),
                int(sc["use_agc"]), self.lr.data_ptr() if self.lr is not None else None, 0.0 if self.lr is not None else float(sc["lr"]),
                float(sc["mu"]))
        if self.kind == "rmsprop":
            args += (float(sc["alpha"]), float(sc["eps"]))
        if self.ema:
            args += (self.step.data_ptr(), float(sc["decay"]))
        name = "iris_agc_clip_" + self.kind + ("_ema" if self.ema else "")
        with torch.cuda.device(self.dev):
            N.check(getattr(N.lib(), name)(*args, stream), name)

    def read(self):
        """-> per group {'x', 'm', ('v',) 'p', ('e')} [rows, len]; the sentinels around every row bit for bit, the row table
        unchanged; without `ema` the whole e buffer unchanged, for sgd the whole v buffer."""
        torch.cuda.synchronize(self.dev)
        back = {q: self.buf[q].cpu().numpy() for q in BUFS}
        for q in BUFS:
            off = ~self.rows_at[q]
            assert np.array_equal(_bits(back[q][off]), _bits(self.host[q][off])), f"a float beside a row of {q} was written"
        assert np.array_equal(self.table.cpu().numpy(), self.table_host), "the row table was written"
        if not self.ema:
            assert np.array_equal(_bits(back["e"]), _bits(self.host["e"])), "an entry point without the EMA wrote e"
        if self.kind == "sgd":
            assert np.array_equal(_bits(back["v"]), _bits(self.host["v"])), "sgd wrote the state slot it does not use"
        out = [dict() for _ in self.case["groups"]]
        for name in O.quantities(self.kind, self.ema):
            q = NAMES[name]
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
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        for name in (names or ga):
            assert np.array_equal(_bits(ga[name]), _bits(gb[name])), (what, name)


_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """After the module's tests: the worst ratio of every quantity to its bound per kernel, in one place (`_compare` asserts)."""
    yield
    for (kernel, name), (ratio, what) in sorted(_SEEN.items()):
        print(f"\nworst {kernel} {name}: {ratio:.3f} of its bound at {what}", end="")
    print()


def _compare(what, case, got, ref=None):
    """Print, per quantity, the kernel's worst ratio to its bound and its worst error over the yardstick's; then assert the bounds."""
    sc = case["sc"]
    ema = "e" in got[0]
    ref = ref or O.reference(case, ema=ema)
    yard = O.reference(case, F32, ema=ema)
    kernel = "iris_agc_clip_" + sc["kind"] + ("_ema" if ema else "")
    worst, late = {}, []
    for gi, (grp, r, y, g) in enumerate(zip(case["groups"], ref, yard, got)):
        mine = O.errors(g, r, grp, sc)
        theirs = O.errors({k: y[k] for k in g}, r, grp, sc)
        for name, (ratio, err) in mine.items():
            w = worst.setdefault(name, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], ratio), max(w[1], err), max(w[2], theirs[name][1])
            if not ratio <= 1.0:
                late.append((gi, grp["p"].shape, name, ratio))
    for name, (ratio, err, yerr) in worst.items():
        print(f"{what} {name}: {ratio:.3f} of its bound; |. - fp64| = {err:.3e}, {err / yerr if yerr > 0 else float(err > 0):.2f} x the float32 yardstick ({yerr:.3e})")
        seen = _SEEN.setdefault((kernel, name), [0.0, ""])
        if ratio > seen[0]:
            seen[0], seen[1] = ratio, what
    assert not late, (what, late)


def _both(dev, what, case):
    """One case through the _ema entry point twice and through the plain one twice: every quantity inside its bound, two runs
    equal bits, and x, b', s', p' the same bits with and without the EMA.  -> (what came back, the float64 reference)."""
    kind = case["sc"]["kind"]
    got, ref = _run(dev, case), O.reference(case, ema=True)
    assert all(set(g) == set(O.quantities(kind, True)) for g in got)
    _compare(what, case, got, ref)
    _same_bits(what + ": two runs", got, _run(dev, case))
    plain = _run(dev, case, ema=False)
    _compare(what, case, plain)
    _same_bits(what + ": two runs without the EMA", plain, _run(dev, case, ema=False))
    _same_bits(what + ": with and without the EMA", got, plain, names=O.quantities(kind))
    return got, ref


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------
def test_arguments_are_checked_before_anything_runs(dev):
    """NULL table, mu / alpha / decay outside [0, 1), eps < 0, a NULL counter: IRIS_E_INVALID and nothing launched (the table
    handed over with the bad scalars is a valid one whose buffers must come back whole); n_rows == 0 is IRIS_OK whatever else."""
    from challenge_amd import _native as N
    lib = N.lib()
    for kind in O.KINDS:
        case = O.edges_case(O.scalars(kind))
        tab = Table(dev, case)
        t, n, step = tab.table.data_ptr(), int(tab.table.shape[0]), tab.step.data_ptr()
        head = (0.01, 1e-3, 1e-3, 1, None, 1e-3)
        tail = (0.9, 1e-7) if kind == "rmsprop" else ()
        plain, ema = getattr(lib, "iris_agc_clip_" + kind), getattr(lib, "iris_agc_clip_" + kind + "_ema")
        bad = [plain(None, n, *head, 0.9, *tail, None), ema(None, n, *head, 0.9, *tail, step, 0.999, None)]
        for mu in (-0.1, 1.0, float("nan")):
            bad += [plain(t, n, *head, mu, *tail, None), ema(t, n, *head, mu, *tail, step, 0.999, None)]
        if kind == "rmsprop":
            for alpha, eps in ((-0.1, 1e-7), (1.0, 1e-7), (0.9, -1e-7)):
                bad += [plain(t, n, *head, 0.9, alpha, eps, None), ema(t, n, *head, 0.9, alpha, eps, step, 0.999, None)]
        bad += [ema(t, n, *head, 0.9, *tail, None, 0.999, None), ema(t, n, *head, 0.9, *tail, step, 1.0, None),
                ema(t, n, *head, 0.9, *tail, step, -0.1, None)]
        assert all(rc == -1 for rc in bad), bad              # IRIS_E_INVALID
        assert plain(None, 0, *head, 7.0, *tail, None) == 0 and ema(None, 0, *head, 7.0, *tail, None, 7.0, None) == 0
        torch.cuda.synchronize(dev)
        back = {q: tab.buf[q].cpu().numpy() for q in BUFS}
        assert all(np.array_equal(_bits(back[q]), _bits(tab.host[q])) for q in BUFS)


# ---------------------------------------------------------------------------
# lengths, alignment, the row loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_agc", [1, 0], ids=["agc", "no-agc"])
@pytest.mark.parametrize("kind", O.KINDS)
def test_lengths_and_alignment(dev, kind, use_agc):
    """Lengths 1 .. 4608 and two rows of 70,000 on both paths; the twins that start 4 bytes off alignment - all pointers, only one
    state row, only the shadow - take the scalar path (for sgd the twin with only the unused slot off stays on the float4 path)."""
    case = O.lengths_case(O.scalars(kind, use_agc=use_agc))
    got, ref = _both(dev, f"{kind} lengths use_agc={use_agc}", case)
    for gi, twin in case["twins"]:
        lim = O.bounds(case["groups"][gi], ref[gi], case["sc"], ema=True)
        same = ref[gi]["s"][:, 0] == 1
        assert same.any() and (use_agc or same.all())
        apart = 0
        for name in got[gi]:
            assert np.array_equal(_bits(got[gi][name][same]), _bits(got[twin][name][same])), (gi, name)
            assert np.all(np.abs(got[gi][name].astype(F64) - got[twin][name]) <= 2 * lim[name]), (gi, name)
            apart += int((_bits(got[gi][name]) != _bits(got[twin][name])).sum())
        print(f"twin {gi} (mis {case['groups'][gi]['mis']}) of group {twin}: {apart} elements with other bits than the aligned rows'")


@pytest.mark.parametrize("kind", O.KINDS)
def test_row_loop_takes_a_second_trip(dev, kind):
    """32,773 rows of 5: five more than the grid has waves (8192 x 4), so the last five are a wave's second row; the marked row,
    third from the end, sits 1e3 above its clip norm."""
    case = O.rowloop_case(O.scalars(kind))
    assert case["groups"][0]["p"].shape == (32768 + 5, 5) and case["marked"] == 32768 + 2
    got, ref = _both(dev, f"{kind} row loop", case)
    assert ref[0]["s"][case["marked"], 0] < 2e-3


# ---------------------------------------------------------------------------
# the edges of the definition, NaN, a first step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(O.EDGE_SCALARS))
@pytest.mark.parametrize("kind", O.KINDS)
def test_edges_of_the_definition(dev, kind, which):
    _both(dev, f"{kind} edges {which}", O.edges_case(O.scalars(kind, **O.EDGE_SCALARS[which])))


@pytest.mark.parametrize("kind", O.KINDS)
def test_a_nan_stays_in_its_unit(dev, kind):
    """One NaN in one unit's gradient: that unit's x, state, parameter and shadow turn NaN; every other row equals the run without
    it bit for bit."""
    a, _ = _both(dev, f"{kind} edges", O.edges_case(O.scalars(kind)))
    b, _ = _both(dev, f"{kind} edges with a NaN", O.edges_case(O.scalars(kind), nan=True))
    hit = EDGE_ROWS.index("above")
    others = np.arange(len(EDGE_ROWS)) != hit
    for ga, gb in zip(a, b):
        assert all(np.isfinite(v).all() for v in ga.values())
        for name in ga:
            assert np.isnan(gb[name][hit]).all(), (name, gb[name][hit])
            assert np.array_equal(_bits(ga[name][others]), _bits(gb[name][others])), name


@pytest.mark.parametrize("kind", O.KINDS)
def test_first_step_from_zero_state(dev, kind):
    """b = 0 (and s = 0): b' = x / a exactly as torch's first step has it; rmsprop's zero-gradient row has s' = 0, a = eps and
    stays finite."""
    case = O.zero_state_case(O.scalars(kind))
    got, _ = _both(dev, f"{kind} first step", case)
    row = EDGE_ROWS.index("zero_g")
    for g, grp in zip(got, case["groups"]):
        assert all(np.isfinite(v).all() for v in g.values())
        assert not g["m"][row].any() and np.array_equal(_bits(g["p"][row]), _bits(grp["p"][row]))
        if kind == "sgd":
            assert np.array_equal(_bits(g["m"]), _bits(g["x"] + F32(0)))      # mu 0 + x


# ---------------------------------------------------------------------------
# the scalars of the call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", O.KINDS)
def test_optimiser_constants(dev, kind):
    """mu in {0, 0.5, 0.9} x host / device lr (x alpha x eps for rmsprop), the EMA's counter on its warm-up and its capped side."""
    cases = O.constants_cases(kind)
    assert len(cases) == (12 if kind == "sgd" else 48)
    for case in cases:
        _both(dev, case["name"], case)


def _walk(dev, kind, name, n, captured):
    """`n` consecutive launches on one table (t = 7 ..., a new gradient each, the learning rate changing), eagerly or as replays of
    ONE captured launch behind the counter's increment: each is held to the definition applied to what the launch before left."""
    start = O.chain_start(kind, name)
    first = O.chain_next(start, None, 0)
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
        case = O.chain_next(start, state, k)
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
        _compare(f"{kind} {name} {k + 1} of {n}", case, got)
        state = [{"p": g["p"], "m": g["m"], "v": g.get("v", grp["v"]), "e": g["e"]} for g, grp in zip(got, case["groups"])]
        for q in "pmve":                               # what the next launch starts from is what this one left (sentinel check: `read`)
            tab.host[q] = tab.buf[q].cpu().numpy()
        seen += got
    return seen


@pytest.mark.parametrize("kind", O.KINDS)
def test_four_launches_from_a_running_state(dev, kind):
    _same_bits("four launches", _walk(dev, kind, "chain", 4, False), _walk(dev, kind, "chain", 4, False))


@pytest.mark.parametrize("kind", O.KINDS)
def test_captured_launch_replays_with_new_gradient_counter_and_lr(dev, kind):
    """One launch + the counter's increment captured into a torch.cuda.graph (a single chain, no parallel branches) and replayed
    three times with a new gradient and learning rate."""
    _same_bits("captured launch", _walk(dev, kind, "capture", 3, True), _walk(dev, kind, "capture", 3, True))


# ---------------------------------------------------------------------------
# make_optimizer, FusedAGC, GraphedTrainStep and fit on a model
# ---------------------------------------------------------------------------
DECAY = 0.999
STATE = {"sgd": {"momentum_buffer"}, "rmsprop": {"step", "square_avg", "momentum_buffer"}}


def _cfg(kind):
    from challenge_amd import sj_train as S
    S.configure_miopen()
    return S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4', '--optimizer', kind])


@pytest.fixture(scope="module")
def base_state(dev):
    """One initial state for every model of this module (computed once, never written)."""
    from challenge_amd import sj_train as S
    torch.manual_seed(3)
    m = S.get_model(_cfg("sgd")).to(dev).to(memory_format=torch.channels_last)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(dev, base_state, kind, capturable=False, ema=False):
    from challenge_amd import sj_train as S
    from challenge_amd.ema import WeightEMA
    cfg = _cfg(kind)
    m = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    m.load_state_dict(base_state)
    avg = WeightEMA(m, DECAY) if ema else None
    m.compile(S.make_optimizer(cfg, m.parameters(), capturable=capturable), S.binary_crossentropy, clipvalue=cfg.clipvalue, ema=avg)
    return m, avg, cfg


def _batches(dev, n, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 32, 64, 1, generator=g).to(dev), (torch.rand(4, 2, 3, generator=g) < 0.3).float().to(dev)) for _ in range(n)]


def _set_lr(m, lr):
    for g in m.optimizer.param_groups:
        if torch.is_tensor(g['lr']):
            g['lr'].fill_(lr)
        else:
            g['lr'] = lr


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _layout(t):
    """The strides that place an element: those of the dimensions longer than 1 (a [32, 1, 3, 3] weight is the same memory with
    stride 9 or 1 on its second dimension; torch's first sgd step clones the gradient, whichever of the two it carries)."""
    return tuple(s for s, n in zip(t.stride(), t.shape) if n > 1)


@pytest.mark.parametrize("kind", O.KINDS)
def test_make_optimizer_on_a_device(dev, base_state, kind):
    """The class and hyper-parameters of each form; the capturable one holds its rate in a device tensor and passes the predicate
    GraphedTrainStep and fit ask."""
    from challenge_amd import sj_train as S
    m, _, cfg = _model(dev, base_state, kind)
    g = m.optimizer.param_groups[0]
    assert type(m.optimizer) is (torch.optim.SGD if kind == "sgd" else torch.optim.RMSprop)
    assert g["lr"] == cfg.lr and g["momentum"] == 0.9 and g["foreach"] and not S.optimizer_capturable(m.optimizer) and not S.graph_step_possible(m)
    m, _, cfg = _model(dev, base_state, kind, capturable=True)
    opt = m.optimizer
    g = opt.param_groups[0]
    assert type(opt) is (torch.optim.SGD if kind == "sgd" else torch.optim.RMSprop) and g["momentum"] == 0.9
    assert torch.is_tensor(g["lr"]) and g["lr"].is_cuda and g["lr"].dtype == torch.float32 and float(g["lr"]) == float(F32(cfg.lr))
    if kind == "sgd":
        assert g["fused"] and not g["foreach"] and not g["nesterov"] and not g["dampening"] and not g["weight_decay"]
    else:
        assert g["capturable"] and (g["alpha"], g["eps"]) == (0.9, 1e-7) and not g["centered"] and not g["weight_decay"]
    assert S.optimizer_capturable(opt) and S.graph_step_possible(m)


@pytest.mark.parametrize("capturable", [False, True], ids=["host-lr", "capturable"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("kind", O.KINDS)
def test_one_launch_matches_the_steps_apart(dev, base_state, kind, ema, capturable):
    """`FusedAGC.optimizer_step` against iris_agc_clip, then torch's step, then `WeightEMA.update`, from the same state on the same
    synthetic gradients (some units far above their clip norm, some elements above clipvalue, some tiny) over three steps with
    a learning-rate change, in the form and with the bounds of test_agc_clip_adam_in_one_launch_matches_the_two_steps: clipped
    gradients to one ulp of the clip factor (3e-7 of the tensor's peak), parameters, state and shadows to 1e-6 of each tensor's
    peak; the state has torch's keys, dtypes, devices and layouts; then the fused run's state_dict() loads into a fresh torch-only
    optimiser, which continues beside it."""
    from challenge_amd import sj_train as S
    from challenge_amd.hip_autograd import FusedAGC
    gen = torch.Generator(device=dev).manual_seed(8)
    assert S.FUSED_OPTIM
    a, ea, cfg = _model(dev, base_state, kind, capturable, ema)
    b, eb, _ = _model(dev, base_state, kind, capturable, ema)
    fa, fb = FusedAGC(list(a.parameters())), FusedAGC(list(b.parameters()))
    if ema:
        assert ea.attach(fa)
    assert fa.attach_optimizer(a.optimizer) and fa._kind == kind and fa._cols() == (6 if ema else 5)
    assert all(set(a.optimizer.state[p]) == STATE[kind] for p in a.parameters())       # created by the attach, zero
    assert all(not a.optimizer.state[p]["momentum_buffer"].any() for p in a.parameters())

    def gradients(models):
        for ps in zip(*[m.parameters() for m in models]):
            p = ps[0]
            gr = torch.randn(p.shape, generator=gen, device=dev).contiguous(memory_format=torch.channels_last if p.dim() == 4 else torch.contiguous_format)
            gr = gr * float(10.0 ** float(torch.randint(-6, 1, (1,), generator=gen, device=dev)))
            for q in ps:
                q.grad = gr.clone(memory_format=torch.preserve_format)

    def apart(model, agc, avg):
        agc(0.01, 1e-3, cfg.clipvalue)
        model.optimizer.step()
        if avg is not None:
            avg.update(model.optimizer)

    def compare(what, ma, mb, sha, shb):
        for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
            sa, sb = ma.optimizer.state[p], mb.optimizer.state[q]
            assert _rel(p.grad, q.grad) <= 3e-7, (what, n)
            assert _rel(p, q) <= 1e-6, (what, n, _rel(p, q))
            assert set(sa) == set(sb) == STATE[kind], (what, n, set(sa), set(sb))
            for key in sa:
                assert sa[key].dtype == sb[key].dtype and sa[key].device == sb[key].device and sa[key].shape == sb[key].shape, (what, n, key)
                assert _layout(sa[key]) == _layout(sb[key]), (what, n, key, sa[key].stride(), sb[key].stride())
                if key == "step":
                    assert float(sa[key]) == float(sb[key]), (what, n)
                else:
                    assert _rel(sa[key], sb[key]) <= 1e-6, (what, n, key, _rel(sa[key], sb[key]))
        if sha is not None:
            assert float(sha._t) == float(shb._t)
            for u, v in zip(sha.shadow, shb.shadow):
                assert _rel(u, v) <= 1e-6

    for k in range(3):
        gradients([a, b])
        if k == 2:
            _set_lr(a, 3e-4), _set_lr(b, 3e-4)
        assert fa.optimizer_step(0.01, 1e-3, cfg.clipvalue) is True
        apart(b, fb, eb)
        compare(k, a, b, ea, eb)
        if kind == "rmsprop":
            assert float(a.optimizer.state[next(a.parameters())]["step"]) == k + 1
        if ema:
            assert float(ea._t) == (0.0 if kind == "rmsprop" and capturable else k + 1)     # the counter WeightEMA._counter hands out
    # the fused run's state in a fresh optimiser that only ever runs torch's step
    c, ec, _ = _model(dev, base_state, kind, capturable, ema)
    c.load_state_dict(a.state_dict())
    c.optimizer.load_state_dict(copy.deepcopy(a.optimizer.state_dict()))   # (load_state_dict keeps the tensors it is handed)
    if ema:
        ec.load_state_dict(ea.state_dict())
        ec._t.copy_(ea._t)
    fc = FusedAGC(list(c.parameters()))
    gradients([a, c])
    assert fa.optimizer_step(0.01, 1e-3, cfg.clipvalue) is True
    apart(c, fc, ec)
    compare("continued", a, c, ea, ec)


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("kind", O.KINDS)
def test_train_step_takes_the_one_launch(dev, base_state, kind, ema, monkeypatch):
    """Three `train_step`s with the switch on and off from the same state: with it on `optimizer_step` ran and returned True every
    step (five- or six-column table, state created by the attach), with it off the three-column table of iris_agc_clip and torch's
    step; from the same state and batch the clipped gradients agree (the form of the Adam test: 1e-4 of each tensor's peak behind
    MIOpen's atomically reduced passes); counters agree every step."""
    from challenge_amd import sj_train as S
    from challenge_amd.hip_autograd import FusedAGC
    calls = []
    inner = FusedAGC.optimizer_step

    def spy(self, *args, **kw):
        calls.append(inner(self, *args, **kw))
        return calls[-1]
    monkeypatch.setattr(FusedAGC, "optimizer_step", spy)
    a, ea, cfg = _model(dev, base_state, kind, ema=ema)
    b, eb, _ = _model(dev, base_state, kind, ema=ema)
    try:
        for k, batch in enumerate(_batches(dev, 3)):
            S.FUSED_OPTIM = True
            la = a.train_step(batch)['loss']
            assert calls == [True] * (k + 1) and a._fused_agc._adam is a.optimizer and a._fused_agc._table.shape[1] == (6 if ema else 5)
            S.FUSED_OPTIM = False
            lb = b.train_step(batch)['loss']
            assert calls == [True] * (k + 1) and b._fused_agc._adam is None and b._fused_agc._table.shape[1] == 3
            if k == 0:
                assert abs(float(la) - float(lb)) <= 1e-6
                for (n, p), q in zip(a.named_parameters(), b.parameters()):
                    assert _rel(p.grad, q.grad) <= 1e-4, (n, _rel(p.grad, q.grad))
            for (n, p), q in zip(a.named_parameters(), b.parameters()):
                sa, sb = a.optimizer.state[p], b.optimizer.state[q]
                assert set(sa) == set(sb) == STATE[kind] and torch.isfinite(p).all() and torch.isfinite(q).all(), n
                if kind == "rmsprop":
                    assert float(sa["step"]) == float(sb["step"]) == k + 1
            if ema:
                assert float(ea._t) == float(eb._t) == k + 1     # neither optimiser keeps a counter on the device here
    finally:
        S.FUSED_OPTIM = True


def _flat(tensors):
    return [t.detach().as_strided((t.numel(),), (1,)).cpu().numpy().copy() for t in tensors]


def _everything(model, avg):
    """Parameters, floating-point buffers, optimiser state tensors and shadows, in a fixed order -> [(name, NumPy)]."""
    out = [("p:" + n, p) for n, p in model.named_parameters()] + [("b:" + n, b) for n, b in model.named_buffers()]
    for n, p in model.named_parameters():
        out += [(f"s:{n}:{k}", v) for k, v in sorted(model.optimizer.state.get(p, {}).items()) if torch.is_tensor(v)]
    if avg is not None:
        out += [(f"e:{i}", t) for i, t in enumerate(avg.state_tensors())]
    return [(n, t.detach().cpu().numpy().copy()) for n, t in out]


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("kind", O.KINDS)
def test_graphed_train_step(dev, base_state, kind, ema):
    """GraphedTrainStep with a capturable sgd / rmsprop: `preserve_state=True` leaves parameters, momentum_buffer, square_avg, step
    and the shadows where they were (state the warm-up created: a fresh zero); the captured step holds the one launch; three
    replays - the third after `set_lr` - equal three eager one-launch steps from the same state bit for bit."""
    from challenge_amd import sj_train as S
    batches = _batches(dev, 3)
    g, eg, _ = _model(dev, base_state, kind, capturable=True, ema=ema)
    e, ee, _ = _model(dev, base_state, kind, capturable=True, ema=ema)
    before = _everything(g, eg)
    step = S.GraphedTrainStep(g, batches[0], preserve_state=True)
    torch.cuda.synchronize(dev)
    assert step._agc._kind == kind and step._agc._adam is g.optimizer and step._agc._table.shape[1] == (6 if ema else 5)
    after = dict(_everything(g, eg))
    for n, was in before:
        assert np.array_equal(was, after[n]), f"the warm-up steps left a trace in {n}"
    for n, now in after.items():
        if n.startswith("s:"):
            assert not now.any(), f"{n} was created by the warm-up and is not a fresh zero"
    assert {n.rsplit(":", 1)[1] for n in after if n.startswith("s:")} == STATE[kind]
    for k, batch in enumerate(batches):
        if k == 2:
            step.set_lr(3e-4), _set_lr(e, 3e-4)
        step(batch)
        e.train_step(batch)
        assert e._fused_agc._adam is e.optimizer and e._fused_agc._kind == kind
    torch.cuda.synchronize(dev)
    assert float(g.optimizer.param_groups[0]['lr']) == float(F32(3e-4))
    got, want = _everything(g, eg), _everything(e, ee)
    moved = sum(not np.array_equal(a, b) for (_, a), (_, b) in zip(before, got) if _.startswith("p:"))
    assert moved > len(list(g.parameters())) // 2
    for (n, a), (_, b) in zip(got, want):
        assert np.array_equal(a, b), (n, float(np.abs(a.astype(F64) - b).max()))
    if kind == "rmsprop":
        assert float(g.optimizer.state[next(g.parameters())]["step"]) == 3.0
    if ema:
        assert float(eg._t) == (3.0 if kind == "sgd" else 0.0)


def test_fit_takes_the_graph_path_with_sgd(dev, base_state, monkeypatch):
    """fit(..., graph=None) on two epochs of two steps with `--optimizer sgd`: the capturable optimiser makes the graph step
    possible and all four steps are replays."""
    from challenge_amd import sj_train as S
    m, _, cfg = _model(dev, base_state, "sgd", capturable=True)
    assert S.graph_step_possible(m) and S.GRAPH_STEP
    replays = []
    inner = S.GraphedTrainStep.__call__
    monkeypatch.setattr(S.GraphedTrainStep, "__call__", lambda self, data: (replays.append(1), inner(self, data))[1])
    batches = _batches(dev, 4)

    def forever():
        i = 0
        while True:
            yield batches[i % len(batches)]
            i += 1
    start = _flat(m.parameters())
    S.fit(m, forever(), epochs=2, steps_per_epoch=2, verbose=False, graph=None)
    torch.cuda.synchronize(dev)
    assert len(replays) == 4
    assert sum(not np.array_equal(a, b) for a, b in zip(start, _flat(m.parameters()))) > len(start) // 2
    assert all(torch.isfinite(p).all() for p in m.parameters())
