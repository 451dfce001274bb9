"""GPU tests of the optimiser tail at the kernels' own boundary: iris_agc_clip (csrc/k_elementwise.h) and iris_agc_clip_adam
(csrc/k_agc_adam.h) called through `_native.lib()` on row tables built by hand - int64 device tensors of addresses, as
`FusedAGC._build` makes them - against the float64 definition of tests/agc_ref.py.  Every element of every row is compared, no mask
and no tolerance on a share of elements; every row stands between sentinel floats that must come back bit for bit.  Bounds:
`agc_ref.bounds` (derived there, constants from two float32 evaluations on the CPU: tests/test_agc_host.py).  Each comparison prints,
per quantity, the kernel's worst ratio to its bound and its worst error over the float32 yardstick's on the same case; DESIGN.md
records the worst.  Then the state around the launch: per-parameter step counters and the Winograd pack book (`FusedAGC.adam_step`)."""
import ctypes as C

import numpy as np
import pytest
import torch

import agc_ref as R
from agc_ref import EDGE_ROWS, F32, F64

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0xC2F6E979], np.uint32).view(F32)[0]      # -123.456
NAMES = {"x": "g", "m": "m", "v": "v", "p": "p"}                # quantity -> the buffer it comes back in


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Table:
    """The case's rows in four device buffers (p, g, m, v) between sentinels, and the kernels' row table over them."""

    def __init__(self, dev, case, adam):
        self.dev, self.case, self.adam = dev, case, adam
        self.slots, cursor = [], 8                          # (group, first row, rows, base float index); the base is a multiple of 4
        for gi, grp in enumerate(case["groups"]):
            rows, length = grp["p"].shape
            for r0, n in ([(0, rows)] if grp["packed"] else [(r, 1) for r in range(rows)]):
                self.slots.append((gi, r0, n, cursor))
                cursor = -(-(cursor + 1 + n * length) // 4) * 4 + 4
        self.host = {q: np.full(cursor + 8, SENTINEL, F32) for q in "pgmv"}
        self.rows_at = {q: np.zeros(cursor + 8, bool) for q in "pgmv"}
        cols = {q: [] for q in "pgmv"}
        lens = []
        for gi, r0, n, base in self.slots:
            grp = case["groups"][gi]
            length = grp["p"].shape[1]
            for q in "pgmv":
                start = base + grp["mis"][q]
                self.host[q][start:start + n * length] = grp[q][r0:r0 + n].reshape(-1)
                self.rows_at[q][start:start + n * length] = True
                cols[q].append(start + np.arange(n, dtype=np.int64) * length)
            lens.append(np.full(n, length, np.int64))
        self.start = {q: np.concatenate(cols[q]) for q in "pgmv"}
        self.len = np.concatenate(lens)
        self.buf = {q: torch.from_numpy(self.host[q]).to(dev) for q in "pgmv"}
        assert all(b.data_ptr() % 16 == 0 for b in self.buf.values())
        order = "pg" + ("mv" if adam else "")
        table = np.empty((self.len.size, 3 + 2 * int(adam)), np.int64)
        table[:, 0], table[:, 1], table[:, 2] = (self.buf["p"].data_ptr() + 4 * self.start["p"], self.buf["g"].data_ptr() + 4 * self.start["g"],
                                                 self.len)
        if adam:
            table[:, 3], table[:, 4] = self.buf["m"].data_ptr() + 4 * self.start["m"], self.buf["v"].data_ptr() + 4 * self.start["v"]
        # every row inside its buffer, no two rows of a written buffer overlapping: checked before anything runs
        for q in order:
            assert self.start[q].min() >= 4 and (self.start[q] + self.len).max() <= self.host[q].size - 4
            assert int(self.rows_at[q].sum()) == int(self.len.sum())
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
        with torch.cuda.device(self.dev):
            if self.adam:
                rc = N.lib().iris_agc_clip_adam(self.table.data_ptr(), int(self.table.shape[0]), float(sc["clip_factor"]), float(sc["eps_agc"]),
                                                float(sc["clipvalue"]), int(sc["use_agc"]), self.lr.data_ptr() if self.lr is not None else None,
                                                0.0 if self.lr is not None else float(sc["lr"]), float(sc["beta1"]), float(sc["beta2"]),
                                                float(sc["eps"]), self.step.data_ptr(), stream)
                N.check(rc, "iris_agc_clip_adam")
            else:
                assert sc["use_agc"]
                rc = N.lib().iris_agc_clip(self.table.data_ptr(), int(self.table.shape[0]), float(sc["clip_factor"]), float(sc["eps_agc"]),
                                           float(sc["clipvalue"]), stream)
                N.check(rc, "iris_agc_clip")

    def read(self):
        """-> per group {'x', and for the Adam kernel 'm', 'v', 'p'} [rows, len]; the sentinels around every row bit for bit, and
        whatever the kernel must not write (iris_agc_clip: the parameters; both: the row table) unchanged."""
        torch.cuda.synchronize(self.dev)
        back = {q: self.buf[q].cpu().numpy() for q in "pgmv"}
        for q in "pgmv":
            off = ~self.rows_at[q]
            assert np.array_equal(_bits(back[q][off]), _bits(self.host[q][off])), f"a float beside a row of {q} was written"
        assert np.array_equal(self.table.cpu().numpy(), self.table_host), "the row table was written"
        for q in ("pmv" if not self.adam else ""):
            assert np.array_equal(_bits(back[q]), _bits(self.host[q])), f"iris_agc_clip wrote {q}"
        out = [dict() for _ in self.case["groups"]]
        for name, q in NAMES.items():
            if name != "x" and not self.adam:
                continue
            for gi, grp in enumerate(self.case["groups"]):
                out[gi][name] = np.empty(grp["p"].shape, F32)
            for gi, r0, n, base in self.slots:
                grp = self.case["groups"][gi]
                length = grp["p"].shape[1]
                start = base + grp["mis"][q]
                out[gi][name][r0:r0 + n] = back[q][start:start + n * length].reshape(n, length)
        return out


def _run(dev, case, adam):
    tab = Table(dev, case, adam)
    tab.launch()
    return tab.read()


def _same_bits(what, a, b):
    """Two runs of a case: equal bits in every quantity of every row."""
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        assert set(ga) == set(gb)
        for name in ga:
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
    ref = ref or R.reference(case)
    yard = R.reference(case, F32)
    worst, late = {}, []
    for gi, (grp, r, y, g) in enumerate(zip(case["groups"], ref, yard, got)):
        mine = R.errors(g, r, grp, case["sc"])
        theirs = R.errors({k: y[k] for k in g}, r, grp, case["sc"])
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


KINDS = [pytest.param(False, id="clip"), pytest.param(True, id="adam")]


# ---------------------------------------------------------------------------
# lengths, alignment, the row loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("clipvalue", [1e-3, 0.0], ids=["clipvalue", "no-clipvalue"])
@pytest.mark.parametrize("adam", KINDS)
def test_lengths_and_alignment(dev, adam, clipvalue):
    """Lengths 1 .. 4608 and two rows of 70,000 on both paths; rows with len % 4 == 0 that start 4 bytes off alignment (all four
    pointers, or only one moment's) take the scalar path and agree with their aligned twins; two runs give equal bits."""
    case = R.lengths_case(R.scalars(clipvalue=clipvalue))
    got = _run(dev, case, adam)
    ref = R.reference(case)
    _compare(f"lengths adam={adam} clipvalue={clipvalue}", case, got, ref)
    for gi, twin in case["twins"]:
        lim = R.bounds(case["groups"][gi], ref[gi], case["sc"])
        for name in got[gi]:
            assert np.all(np.abs(got[gi][name].astype(F64) - got[twin][name]) <= 2 * lim[name]), (gi, name)
    _same_bits("lengths", got, _run(dev, case, adam))
    if not clipvalue:                      # a unit below its threshold comes back bit for bit
        for grp, r, g in zip(case["groups"], ref, got):
            same = r["s"][:, 0] == 1
            assert same.any() and np.array_equal(_bits(g["x"][same]), _bits(grp["g"][same]))


@pytest.mark.parametrize("adam", KINDS)
def test_row_loop_takes_a_second_trip(dev, adam):
    """More rows than the grid has waves (4096 x 4 for iris_agc_clip, 8192 x 4 for iris_agc_clip_adam) + 5: the last five rows are a
    wave's second row.  Every row is checked; the marked one, third from the end, sits 1e3 above its clip norm."""
    case = R.rowloop_case("adam" if adam else "clip")
    n, marked = case["groups"][0]["p"].shape[0], case["marked"]
    assert n == (32768 if adam else 16384) + 5 and marked >= n - 5
    got = _run(dev, case, adam)
    ref = R.reference(case)
    assert ref[0]["s"][marked, 0] < 1.01e-3
    ratio = np.abs(got[0]["x"][marked].astype(F64)).max() / np.abs(case["groups"][0]["g"][marked].astype(F64)).max()
    assert ratio < 2e-3, ratio                                             # it WAS clipped
    _compare(f"row loop adam={adam}", case, got, ref)
    _same_bits("row loop", got, _run(dev, case, adam))


# ---------------------------------------------------------------------------
# the edges of the definition
# ---------------------------------------------------------------------------
EDGE_RUNS = [(False, k) for k in R.EDGE_SCALARS if k != "no-agc"] + [(True, k) for k in R.EDGE_SCALARS]


@pytest.mark.parametrize("adam,which", EDGE_RUNS, ids=lambda v: v if isinstance(v, str) else ("adam" if v else "clip"))
def test_edges_of_the_definition(dev, adam, which):
    sc = R.EDGE_SCALARS[which]
    case = R.edges_case(sc)
    got = _run(dev, case, adam)
    ref = R.reference(case)
    _compare(f"edges {which} adam={adam}", case, got, ref)
    _same_bits(f"edges {which}", got, _run(dev, case, adam))
    cv = F32(sc["clipvalue"])
    for grp, r, g in zip(case["groups"], ref, got):
        row = EDGE_ROWS.index
        assert not _bits(g["x"][row("zero_g")]).any()                                      # exactly +0, and finite everywhere
        assert all(np.isfinite(a).all() for a in g.values())
        if cv > 0:
            assert np.abs(g["x"]).max() <= cv
            assert g["x"][row("at_clipvalue"), 0] == cv and g["x"][row("at_clipvalue"), 1] == -cv
            inside = np.abs(grp["g"][row("at_clipvalue")]) <= cv
            assert np.array_equal(_bits(g["x"][row("at_clipvalue")][inside]), _bits(grp["g"][row("at_clipvalue")][inside]))
        else:                                                                              # s = 1 and no clamp: the gradient's own bits
            same = r["s"][:, 0] == 1
            same[row("at_threshold")] = False                                              # (either branch is right there)
            assert same.sum() >= 4 and np.array_equal(_bits(g["x"][same]), _bits(grp["g"][same]))
        if adam:                                                                           # zero gradient: the moments decay, p moves by m alone
            z = row("zero_g")
            assert np.all(np.abs(g["m"][z]) < np.abs(grp["m"][z])) and np.all(g["v"][z] < grp["v"][z]) and np.any(g["p"][z] != grp["p"][z])


@pytest.mark.parametrize("adam", KINDS)
def test_a_nan_stays_in_its_unit(dev, adam):
    """One NaN in one unit's gradient: that unit's clipped gradient (and, with Adam, its moments and parameters) turns NaN - the
    definition's max(NaN, 1e-6) is NaN - and every other row equals the run without it bit for bit."""
    clean, dirty = R.edges_case(), R.edges_case(nan=True)
    a, b = _run(dev, clean, adam), _run(dev, dirty, adam)
    hit = EDGE_ROWS.index("above")
    for ga, gb in zip(a, b):
        others = np.arange(len(EDGE_ROWS)) != hit
        for name in ga:
            assert np.isnan(gb[name][hit]).all(), (name, gb[name][hit])
            assert np.array_equal(_bits(ga[name][others]), _bits(gb[name][others])), name
    _compare(f"edges with a NaN adam={adam}", dirty, b)
    _same_bits("edges with a NaN", b, _run(dev, dirty, adam))


# ---------------------------------------------------------------------------
# the optimiser's constants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("betas", R.BETAS, ids=lambda b: f"betas-{b[0]}-{b[1]}")
def test_optimiser_constants(dev, betas):
    """t in {1, 2, 10, 1000, 100000} x eps in {1e-8, 1e-3} x lr from the host float / from a device tensor, for one pair of betas;
    t = 1 starts from zero moments.  After each launch `grad` holds x."""
    cases = R.constants_cases(betas)
    assert len(cases) == 20
    for case in cases:
        got = _run(dev, case, True)
        assert all(set(g) == {"x", "m", "v", "p"} for g in got)
        _compare(case["name"], case, got)
        _same_bits(case["name"], got, _run(dev, case, True))


def test_four_launches_from_a_running_state(dev):
    """Four consecutive launches (t = 7 .. 10, a new gradient each, the learning rate changed twice) on one table: each launch is
    held to the definition applied to the state the launch before left in the buffers."""
    start = R.chain_start("chain")
    first = R.chain_next(start, None, 0)

    def walk():
        tab = Table(dev, first, True)
        state, seen = None, []
        for k in range(4):
            case = R.chain_next(start, state, k)
            if k:
                tab.set_gradient(case["groups"])
                tab.step.add_(1)
            tab.launch(case["sc"])
            got = tab.read()
            assert float(tab.step) == 7.0 + k
            _compare(f"launch {k + 1} of 4", case, got)
            state = [{q: g[q] for q in "pmv"} for g in got]
            for q in "pmv":                               # what the next launch starts from is what this one left (sentinel check: `read`)
                tab.host[q] = tab.buf[q].cpu().numpy()
            seen += got
        return seen
    _same_bits("four launches", walk(), walk())


def test_captured_launch_replays_with_new_gradient_counter_and_lr(dev):
    """One iris_agc_clip_adam launch behind the counter's increment, captured on a side stream into a torch.cuda.graph (a single
    chain, no parallel branches) and replayed three times with a new gradient and a changed device learning rate in between: all
    three steps are held to the definition."""
    start = R.chain_start("capture")
    assert start["sc"]["lr_dev"]
    first = R.chain_next(start, None, 0)

    def walk():
        tab = Table(dev, first, True)
        tab.step.fill_(6.0)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tab.step.add_(1)
            tab.launch(first["sc"])
        torch.cuda.synchronize(dev)
        back = {q: tab.buf[q].cpu().numpy() for q in "pgmv"}
        assert all(np.array_equal(_bits(back[q]), _bits(tab.host[q])) for q in "pgmv") and float(tab.step) == 6.0   # nothing has run yet
        state, seen = None, []
        for k in range(3):
            case = R.chain_next(start, state, k)
            tab.set_gradient(case["groups"])
            tab.lr.fill_(float(case["sc"]["lr"]))
            graph.replay()
            got = tab.read()
            assert float(tab.step) == 7.0 + k
            _compare(f"replay {k + 1} of 3", case, got)
            state = [{q: g[q] for q in "pmv"} for g in got]
            for q in "pmv":
                tab.host[q] = tab.buf[q].cpu().numpy()
            seen += got
        return seen
    _same_bits("captured launch", walk(), walk())


# ---------------------------------------------------------------------------
# FusedAGC on a model: the table, the step counters, the pack book
# ---------------------------------------------------------------------------
def _model(dev, v="9", capturable=False, seed=3):
    from challenge_amd import sj_train as S
    S.configure_miopen()
    cfg = S.ARGS().get(['--v', v, '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '4'])
    torch.manual_seed(seed)
    m = S.get_model(cfg).to(dev).to(memory_format=torch.channels_last)
    m.compile(S.make_optimizer(cfg, m.parameters(), capturable=capturable), S.binary_crossentropy, clipvalue=cfg.clipvalue)
    return m, cfg


def _synthetic_gradients(model, gen):
    """Per parameter N(0, 1) x 10^U{-6 .. 0} in the parameter's own layout: some units far above their clip norm, some tiny."""
    for p in model.parameters():
        g = torch.randn(p.shape, generator=gen, device=p.device) * float(10.0 ** float(torch.randint(-6, 1, (1,), generator=gen, device=p.device)))
        p.grad = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)


def _as_rows(t):
    """A dense parameter-shaped device tensor -> NumPy [units, len] in the order of its memory."""
    from challenge_amd.hip_autograd import FusedAGC
    rows, length = FusedAGC._rows_of(t)
    return t.detach().as_strided((t.numel(),), (1,)).cpu().numpy().reshape(rows, length).copy()


@pytest.mark.parametrize("v", ["9", "8", "1"])
def test_built_table_is_the_partition_into_units(dev, v):
    """`FusedAGC._build` with an optimiser attached: row r of a parameter is [r len, (r + 1) len) of its memory, of its gradient's and
    of both moments'; the rows are disjoint and cover every element of the model exactly once."""
    from challenge_amd.hip_autograd import FusedAGC
    model, _ = _model(dev, v)
    _synthetic_gradients(model, torch.Generator(device=dev).manual_seed(1))
    params = list(model.parameters())
    agc = FusedAGC(params)
    assert agc.attach_adam(model.optimizer)
    agc._build()
    torch.cuda.synchronize(dev)
    assert not agc._slow
    table = agc._table.cpu().numpy()
    assert table.shape == (sum(FusedAGC._rows_of(p)[0] for p in params), 5)
    at = 0
    for p in params:
        rows, length = FusedAGC._rows_of(p)
        st = model.optimizer.state[p]
        want = np.arange(rows, dtype=np.int64) * length * 4
        for col, t in ((0, p), (1, p.grad), (3, st["exp_avg"]), (4, st["exp_avg_sq"])):
            assert t.stride() == p.stride() and np.array_equal(table[at:at + rows, col], t.data_ptr() + want)
        assert np.all(table[at:at + rows, 2] == length)
        at += rows
    order = np.argsort(table[:, 0])
    begin, end = table[order, 0], table[order, 0] + 4 * table[order, 2]
    assert np.all(end[:-1] <= begin[1:]) and int(table[:, 2].sum()) == sum(p.numel() for p in params)


@pytest.mark.parametrize("how,capturable", [("in_place", False), ("replaced", False), ("in_place", True)])
def test_per_parameter_step_counters(dev, how, capturable):
    """torch's Adam keeps a step counter per parameter; the launch reads one.  With one parameter's counter 5 ahead (a loaded state, or
    an earlier step that went through `optimizer.step()` while a gradient was missing), what `train_step` does - `attach_adam`,
    `adam_step`, and `FusedAGC.__call__` + `optimizer.step()` where those decline - must give every parameter ITS bias correction:
    parameters, both moments, the clipped gradients and every counter against agc_ref with per-parameter t.  With equal counters
    the one-launch path runs."""
    from challenge_amd import sj_train as S
    from challenge_amd.hip_autograd import FusedAGC
    assert S.FUSED_ADAM
    model, cfg = _model(dev, capturable=capturable)
    opt, params = model.optimizer, list(model.parameters())
    gen = torch.Generator(device=dev).manual_seed(8)
    agc = FusedAGC(params)

    def counters():
        return [float(opt.state[p]["step"]) if "step" in opt.state[p] else 0.0 for p in params]

    def step():
        before = counters()
        stepped = agc.attach_adam(opt) and agc.adam_step(0.01, 1e-3, cfg.clipvalue)
        if not stepped:
            assert counters() == before                                                    # declined BEFORE any increment
            agc(0.01, 1e-3, cfg.clipvalue)
            assert counters() == before
            opt.step()
        return stepped

    for _ in range(2):                                                                     # equal counters: one launch
        _synthetic_gradients(model, gen)
        assert step() and agc._adam is opt
    odd = params[5]
    if how == "in_place":
        opt.state[odd]["step"] += 5
    else:
        opt.state[odd]["step"] = opt.state[odd]["step"] + 5
    for k in range(2):                                                                     # the second: the verdict is remembered
        _synthetic_gradients(model, gen)
        before = [{"p": _as_rows(p), "g": _as_rows(p.grad), "m": _as_rows(opt.state[p]["exp_avg"]), "v": _as_rows(opt.state[p]["exp_avg_sq"]),
                   "t": float(opt.state[p]["step"])} for p in params]
        assert before[5]["t"] == 7.0 + k and before[4]["t"] == 2.0 + k
        stepped = step()
        print(f"counters apart ({how}, capturable={capturable}), step {k}: {'one launch, a counter per row' if stepped else 'declined: torch path'}")
        lr = opt.param_groups[0]["lr"]
        worst = {}
        for i, p in enumerate(params):
            st = opt.state[p]
            assert float(st["step"]) == before[i]["t"] + 1, i
            sc = R.scalars(clipvalue=cfg.clipvalue, lr=float(lr), beta1=0.9, beta2=0.999, eps=opt.param_groups[0]["eps"], t=before[i]["t"] + 1)
            ref = R.launch(before[i], sc)
            got = {"x": _as_rows(p.grad), "m": _as_rows(st["exp_avg"]), "v": _as_rows(st["exp_avg_sq"]), "p": _as_rows(p)}
            for name, (ratio, _) in R.errors(got, ref, before[i], sc).items():
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert ratio <= 1.0, (i, name, ratio, before[i]["t"])
        print("   worst ratio to the bound: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))


def _forward_backward(model, x, grad):
    """model.train(); model(x): with gradients and a backward -> (output, input gradient, weight gradients), or under no_grad."""
    model.train()
    if not grad:
        with torch.no_grad():
            return [model(x).clone()]
    for p in model.parameters():
        p.grad = None
    xx = x.clone().requires_grad_(True)
    out = model(xx)
    out.square().sum().backward()
    return [out.detach().clone(), xx.grad.clone()] + [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("how", ["train_step", "adam_step"])
def test_pack_book_follows_the_fused_update(dev, how):
    """The one-launch update writes the weights behind their autograd versions.  After an eager fused `train_step` (or a bare
    `FusedAGC.adam_step` on a model whose forward has filled the book), a training-mode forward outside `train_step` - with
    gradients and a backward, and under no_grad - must convolve with the NEW weights: bit for bit what a second model in the same
    state computes with the book cleared and FUSED_PACK off (the same kernels on the same weights): the output, the input gradient
    and all 84 weight gradients."""
    from challenge_amd import hip_autograd as HA
    from challenge_amd import sj_train as S
    gen = torch.Generator(device=dev).manual_seed(11)
    x = torch.rand(4, 32, 64, 1, generator=gen, device=dev)
    y = (torch.rand(4, 2, 3, generator=gen, device=dev) < 0.3).float()
    x2 = torch.rand(4, 32, 64, 1, generator=gen, device=dev)
    try:
        assert S.FUSED_ADAM and S.FUSED_PACK
        HA._PACKS.clear()
        a, cfg = _model(dev)
        # The input wants a gradient here.  The first layer hands it back from its own fused passes, as it does behind a trainable
        # PCEN layer (`input_grad`, model.py:49-55).  Without that flag an input that requires a gradient sends this one layer to
        # torch's conv2d, and MIOpen's weight-gradient kernel for the 1 -> 32 convolution does not give the same bits twice: over six
        # runs of ONE model from one state `features.0.convs.0.0.weight.grad` moved by 1e-6 of its peak and nothing else of the 86
        # tensors moved; with the flag none moved, so every tensor is compared by bits.
        a.features[0].convs[0].input_grad = True
        agc = HA.FusedAGC(list(a.parameters()))
        for grad in (True, False):
            if how == "train_step":
                a.train_step((x, y))
                assert a._fused_agc._adam is a.optimizer                 # the one-launch path ran
            else:
                a.train()
                a.optimizer.zero_grad(set_to_none=True)
                a.loss_fn(y, a(x)).backward()                            # fills the book with this step's weights
                assert agc.attach_adam(a.optimizer) and agc.adam_step(0.01, 1e-3, cfg.clipvalue)
            assert len(HA._PACKS.entries) > 0
            state = {k: v.detach().clone() for k, v in a.state_dict().items()}         # parameters and BatchNorm buffers just before the call
            got = _forward_backward(a, x2, grad)
            HA._PACKS.clear()
            S.FUSED_PACK = False
            try:
                b, _ = _model(dev, seed=4)
                b.features[0].convs[0].input_grad = True
                b.load_state_dict(state)
                want = _forward_backward(b, x2, grad)
            finally:
                S.FUSED_PACK = True
            names = ["output", "input gradient"] + [n for n, _ in a.named_parameters()]
            assert len(got) == len(want) == (len(names) if grad else 1)
            for name, u, w in zip(names, got, want):
                assert torch.equal(u, w), (how, grad, name, float((u - w).abs().max()))
    finally:
        S.FUSED_PACK = True
        HA._PACKS.clear()
