"""Optimiser, run name, MIOpen configuration, the training step as one replayed hipGraph (`GraphedTrainStep`, also under
DistributedDataParallel over RCCL) and the Keras-fit equivalent of sj_train.py:489-519 upstream (`fit`)."""
from __future__ import annotations

import csv
import math
import os
import time
from typing import Optional

import torch

from . import frontend as _fe
from . import switches as SW
from .distributed import _gradient_buckets, average_bn_statistics, collectives_on
from .hip_autograd import FusedAGC, _IN_STEP, _ZERO_POOL
from .model import CustomModel


def make_optimizer(config, params, capturable: bool = False):
    """`capturable`: the optimiser with its learning rate (and, where it keeps one, its step count) in device tensors and a
    `step()` that is legal inside a hipGraph capture, for `GraphedTrainStep`: Adam and RMSprop with capturable=True; SGD with
    fused=True - torch.optim.SGD has no `capturable` key, its foreach form reads a tensor rate back to the host
    (`_foreach_add_(..., alpha=-lr)`), its fused form hands the tensor to the kernel."""
    params = list(params)
    if capturable:
        if config.optimizer == 'adabelief':
            raise ValueError('adabelief is deprecated')
        if not (params and params[0].is_cuda):
            raise ValueError("make_optimizer(capturable=True): adam, sgd or rmsprop on a GPU")
        lr = torch.tensor(float(config.lr), device=params[0].device)
        if config.optimizer == 'adam':
            return torch.optim.Adam(params, lr=lr, eps=1e-7, fused=True, capturable=True)
        if config.optimizer == 'sgd':
            return torch.optim.SGD(params, lr=lr, momentum=0.9, fused=True)
        if config.optimizer == 'rmsprop':
            return torch.optim.RMSprop(params, lr=lr, momentum=0.9, alpha=0.9, eps=1e-7, foreach=True, capturable=True)
        raise ValueError(f"make_optimizer: unknown optimizer {config.optimizer!r}")
    # foreach=True on a GPU: the update AND zero_grad run as a handful of multi-tensor kernels instead of one per
    # parameter (86 fills of ~3.6 us each per step otherwise)
    fe = bool(params) and params[0].is_cuda
    if config.optimizer == 'adam':
        if fe and os.environ.get("IRIS_ADAM_FUSED", "1") != "0":  # the whole update in one multi-tensor launch
            return torch.optim.Adam(params, lr=config.lr, eps=1e-7, fused=True)
        return torch.optim.Adam(params, lr=config.lr, eps=1e-7, foreach=fe)  # Keras Adam epsilon
    if config.optimizer == 'sgd':
        return torch.optim.SGD(params, lr=config.lr, momentum=0.9, foreach=fe)
    if config.optimizer == 'rmsprop':
        return torch.optim.RMSprop(params, lr=config.lr, momentum=0.9, alpha=0.9, eps=1e-7, foreach=fe)
    raise ValueError('adabelief is deprecated')


def optimizer_capturable(opt) -> bool:
    """Can `opt.step()` run inside a hipGraph capture, and will a replay see a new learning rate?  The rate of every group in a
    device tensor, and a step that reads nothing back to the host: torch's `capturable=True` (Adam, RMSprop), or - torch.optim.SGD
    has no such key - its fused form, which takes the rate tensor as a kernel argument."""
    if opt is None:
        return False
    for g in opt.param_groups:
        if not (torch.is_tensor(g['lr']) and g['lr'].is_cuda):
            return False
        if not (g.get('capturable', False) or (type(opt) is torch.optim.SGD and g.get('fused'))):
            return False
    return True


def run_name(config) -> str:
    """Run name encoding of sj_train.py:416-429."""
    name = (config.name + '_') if config.name != '' else ''
    first = {'eff': f'B{config.model}', 'se': 'se', 'vad': 'vad'}[config.model_type]
    name += '_'.join([first, f'v{config.v}', f'lr{config.lr}', f'batch{config.batch_size}',
                      f'opt_{config.optimizer}', f'mel{config.n_mels}', f'chan{config.n_chan}',
                      f'{config.loss.upper()}', f'framelen{config.n_frame}'])
    return name if name.endswith('.h5') else name + '.h5'


def configure_miopen() -> None:
    """MIOpen defaults for this model's fp32 conv shapes (only set when the user has not):
    NORMAL find benchmarks the applicable solvers once per shape - the FAST heuristic picks a CK
    backward-weight kernel that is ~60x slower here - and the naive reference solvers (hundreds of
    ms per call, never the winner) are kept out of that benchmark."""
    os.environ.setdefault("MIOPEN_FIND_MODE", "NORMAL")
    for d in ("FWD", "BWD", "WRW"):
        os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + d, "0")
    _use_shipped_miopen_db()


def _use_shipped_miopen_db() -> None:
    """challenge_amd/miopen_db/ holds MIOpen's user perf-db / find-db after an exhaustive search (MIOPEN_FIND_ENFORCE=3,
    scripts/gpu_miopen_tune.sh) over this model's convolution shapes at batch 64 on an MI355X: tuned kernel parameters for
    the solvers MIOpen already has, 16.2 -> 15.1 ms per training step (profiles/r3/miopen_tune.log).  MIOpen also WRITES to
    its user db, so a per-user, per-rank copy (miopen_db/_run/, named after the shipped content) is what MIOPEN_USER_DB_PATH points at.
    Skipped when the user has set MIOPEN_USER_DB_PATH, or with IRIS_MIOPEN_DB=0; the files are keyed by MIOpen build and
    GPU, so any other build / GPU simply does not find them."""
    if "MIOPEN_USER_DB_PATH" in os.environ or os.environ.get("IRIS_MIOPEN_DB", "1") == "0":
        return
    import hashlib
    import shutil
    import tempfile
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "miopen_db")
    try:
        files = sorted(f for f in os.listdir(src) if f.endswith("db.txt"))
        if not files:
            return
        digest = hashlib.sha256()
        for f in files:
            with open(os.path.join(src, f), "rb") as fh:
                digest.update(f.encode() + b"\0" + fh.read())
        uid = os.getuid() if hasattr(os, "getuid") else 0
        name = f"u{uid}_r{os.environ.get('LOCAL_RANK', '0')}_{digest.hexdigest()[:12]}"
        dst = os.path.join(src, "_run", name)  # beside the shipped files (git- and gpurun-ignored) ...
        try:
            os.makedirs(dst, exist_ok=True)
        except OSError:  # ... or, for a read-only installation, in the temp dir
            dst = os.path.join(tempfile.gettempdir(), "iris_miopen_db_" + name)
            os.makedirs(dst, exist_ok=True)
        for f in files:
            if not os.path.exists(os.path.join(dst, f)):
                tmp = os.path.join(dst, f + f".{os.getpid()}.tmp")
                shutil.copyfile(os.path.join(src, f), tmp)
                os.replace(tmp, os.path.join(dst, f))
        os.environ["MIOPEN_USER_DB_PATH"] = dst
    except OSError:
        pass  # no shipped db / unwritable temp dir: MIOpen's own defaults


def miopen_db_status() -> str:
    """Did MIOpen pick up the shipped perf-db / find-db (`_use_shipped_miopen_db`)?  Call AFTER the model's convolutions have
    run once.  The files are keyed by MIOpen's build string and the GPU (arch + CU count) in their NAMES: a matching MIOpen
    reads and appends to the shipped names, any other build ignores them and - having had to search - writes files under its
    own name next to them.  'used' / 'ignored: ...' / 'off: ...' (bench.py records it as extra.miopen_db: the tuned db is
    worth 13.7 vs 15.1 ms per training step, so a line must say which of the two it measured)."""
    path = os.environ.get("MIOPEN_USER_DB_PATH")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "miopen_db")
    if os.environ.get("IRIS_MIOPEN_DB", "1") == "0":
        return "off: IRIS_MIOPEN_DB=0"
    try:
        shipped = {f for f in os.listdir(src) if f.endswith("db.txt")}
    except OSError:
        shipped = set()
    if not path or not shipped:
        return "off: no shipped db in use"
    if not (os.path.basename(os.path.dirname(path)) == "_run" or os.path.basename(path).startswith("iris_miopen_db_")):
        return "off: MIOPEN_USER_DB_PATH set by the user"
    try:
        present = {f for f in os.listdir(path) if f.endswith("db.txt")}
    except OSError:
        return "off: " + path + " unreadable"
    foreign = sorted(present - shipped)
    if foreign:
        return ("ignored: this MIOpen build wrote " + ", ".join(foreign[:2]) + " - its build string / GPU differs from the shipped "
                + sorted(shipped)[-1])
    return "used"


class GraphCaptureError(RuntimeError):
    """The training step could not be captured as a hipGraph.  Raised by GraphedTrainStep on EVERY rank of a job alike (the ranks
    agree on the outcome before anyone replays) and with the model's state as it was before the attempt: the caller may go on
    with the eager step."""


class GraphedTrainStep:
    """`model.train_step` (forward, loss, backward, gradient all-reduce, AGC + clipvalue, optimiser) as ONE replayed hipGraph -
    fixed batch shape.  The gradients live in the graph's memory pool and are dropped inside the capture, so the replay has
    neither the zero fills nor autograd's accumulate launches; the host enqueues two copies and one graph launch per step
    however many kernels the step has (~260), which is what keeps eight ranks sharing one host off each other's toes.

        opt = make_optimizer(config, model.parameters(), capturable=True)      # learning rate held in a device tensor
        model.compile(opt, loss, clipvalue=..., ddp=wrap_ddp(...))
        step = GraphedTrainStep(model, (x, y))                                   # 3 eager warm-up steps (they train), then the capture
                                                                                 # (preserve_state=True: the warm-up leaves no trace)
        for x, y in data: loss = step((x, y))['loss']                            # inputs are copied into the static buffers
        step.set_lr(value)                                                       # schedulers write the tensor

    MIOpen must already know its kernels for these shapes (the warm-up steps see to that).
    **Under DistributedDataParallel** (round 6; RCCL only) the capture does not go through DDP's reducer - host-side bucket
    bookkeeping that a replay would skip - but issues the same exchange itself: the plain module runs forward and backward, a
    post-accumulate hook per parameter copies each finished gradient bucket (DDP's own bucket order and size, `_gradient_buckets`)
    into a flat buffer, pre-divides it by the world size and starts `all_reduce` on it asynchronously (RCCL's stream joins the
    capture as a parallel branch: the collective of one bucket overlaps the backward kernels of the layers below, as under DDP);
    after backward the capture waits for the collectives, the gradients become views of the flat buffers, and AGC, clipvalue and
    the optimiser act on the averaged gradients - identically on every rank.  Whether the capture succeeded is agreed on by ALL ranks
    (one MIN all-reduce of a flag) before anyone replays: a rank never replays a graph while another one runs eager DDP."""

    def __init__(self, model: "CustomModel", example, warmup: int = 3, preserve_state: bool = False):
        """`preserve_state`: parameters, buffers and the optimiser's state are put back after the warm-up steps - also when a
        warm-up step or the capture fails -, so that the first replay (or the first eager step of the fallback) is the FIRST
        update the example batch causes (what `fit` wants: one update per batch, as the reference)."""
        x, y = example
        if not x.is_cuda:
            raise RuntimeError("GraphedTrainStep: a GPU tensor is required (hipGraph capture; no CPU fallback)")
        opt = model.optimizer
        if not optimizer_capturable(opt):
            raise ValueError("GraphedTrainStep: the optimiser must be capturable - make_optimizer(config, params, capturable=True)")
        self.world = 0   # > 0: the capture holds the gradient all-reduce of that many ranks
        if model._ddp is not None:
            dist = torch.distributed
            if dist.get_backend() != 'nccl':
                raise GraphCaptureError(f"GraphedTrainStep: under DistributedDataParallel only with RCCL (backend 'nccl'); the "
                                        f"'{dist.get_backend()}' backend's collectives cannot be captured into a hipGraph")
            self.world = dist.get_world_size()
        self.model, self.x, self.y = model, x.clone(), y.clone()
        dev = x.device
        saved = None
        self.metrics = model._metrics   # compiled metrics: one captured iris_event_metrics launch per replay
        self.metric_out, self.y_pred = {}, None
        if preserve_state:
            tensors = list(model.parameters()) + list(model.buffers())
            saved = ([t.detach().clone() for t in tensors], tensors,
                     {id(p): {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in opt.state.get(p, {}).items()}
                      for g in opt.param_groups for p in g['params']},
                     {id(t): t.clone() for t in (self.metrics.state_tensors() if self.metrics is not None else [])},
                     [(t, t.detach().clone()) for t in (model._ema.state_tensors() if model._ema is not None else [])])

        def restore():
            opt.zero_grad(set_to_none=True)
            if saved is None:
                return
            with torch.no_grad():   # undo the warm-up in place (the graph is captured on these very tensors)
                for t, old in zip(saved[1], saved[0]):
                    t.copy_(old)
                for g in opt.param_groups:
                    for p in g['params']:
                        before, now = saved[2][id(p)], opt.state.get(p, {})
                        for k, v in now.items():
                            if torch.is_tensor(v):   # moments and the step count: back to their old values, or to a fresh 0
                                v.copy_(before[k]) if k in before else v.zero_()
                if self.metrics is not None:   # F1 counts and epoch accumulators: the warm-up steps counted nothing
                    for t in self.metrics.state_tensors():
                        t.copy_(saved[3][id(t)]) if id(t) in saved[3] else t.zero_()
                for t, old in saved[4]:   # the weight EMA's shadows: the warm-up steps averaged nothing
                    t.copy_(old)
                if model._ema is not None:
                    model._ema.bump_generation()
            model.bump_generation()
            torch.cuda.synchronize(dev)

        # `warmup` eager steps in all (they train the model; under DDP they go through DDP): all but the last on the current
        # stream - without them the capture was invalidated on this stack (some first-use initialisation that a side stream
        # alone does not trigger) - and the last one on a side stream, as torch's capture recipe asks
        try:
            for _ in range(max(warmup, 2) - 1):
                model.train_step((self.x, self.y))
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            # (under DDP this one step runs the reducer's AccumulateGrad nodes - default stream - from a side stream: torch warns
            # about the extra synchronisation, which is all it costs here; the capture itself goes through parameter aliases)
            quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None) if self.world else None
            if quiet is not None:
                quiet(False)
            try:
                with torch.cuda.stream(side):
                    model.train_step((self.x, self.y))
            finally:
                if quiet is not None:
                    quiet(True)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
        finally:
            object.__setattr__(model, '_fused_agc', None)  # its table holds the eager gradients' addresses
            restore()
        # The captured AGC launch reads a table whose pinned staging buffer is the source of a captured copy node: this
        # object owns both for as long as the graph lives, and the model's own `_fused_agc` stays None - an eager
        # `model.train_step` later (e.g. a ragged last batch) builds a SEPARATE FusedAGC instead of rebuilding - and
        # freeing - the buffers the graph replays from.
        self._agc = FusedAGC(list(model.parameters())) if model.use_agc else None
        if self._agc is not None:
            self._agc.attach_optimizer(opt)   # (before `reserve`: an attached optimiser makes the table five columns wide)
            if model._ema is not None:   # (and a weight EMA six)
                model._ema.attach(self._agc)
            self._agc.reserve()
        self._flats, self._buckets = [], []
        if self.world:
            self._buckets = _gradient_buckets(model.parameters(), SW.DDP_BUCKET_MB << 20)
            self._flats = [torch.zeros(sum(p.numel() for p in b), dtype=b[0].dtype, device=dev) for b in self._buckets]
        torch.cuda.synchronize(dev)
        if self.world:
            # The process group's watchdog thread polls the end events of the EAGER collectives it still holds (the warm-up steps'
            # bucket all-reduces) every 100 ms.  Once the capture below has pulled RCCL's stream in, such a poll fails with
            # "operation not permitted on an event last recorded in a capturing stream" and takes the process down (seen once in
            # four runs: profiles/r6/rccl_watchdog_event_query_during_capture.log).  The device is idle now: give the watchdog three of
            # its periods to retire every finished collective, so that it holds nothing while the capture runs.
            time.sleep(0.35)
        self.graph = torch.cuda.CUDAGraph()
        self._pool_marks = {}
        ok, error = True, None
        try:
            # (thread_local: another thread's harmless queries - RCCL's watchdog polling the events of earlier collectives when
            # a process group is alive in this process - must not invalidate the capture, nor be killed by it)
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._capture_body(model, opt, dev)
            torch.cuda.synchronize(dev)
        except Exception as exc:   # nothing of the capture has RUN: the model is where `restore` left it
            ok, error = False, exc
            opt.zero_grad(set_to_none=True)
        if self.world:   # every rank replays, or none does
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            if ok and not int(flag.item()):
                ok, error = False, RuntimeError("the capture failed on another rank of this job")
        if not ok:
            self.graph = None
            raise GraphCaptureError(f"GraphedTrainStep: {error!r:.300}") from error

    def _capture_body(self, model, opt, dev):
        model.train()
        if SW.ZERO_POOL:
            _ZERO_POOL.begin_step(dev)
        handles, works, aliases = [], [], None
        if self.world:
            # The exchange DDP's reducer would do, issued from inside the capture (see the class docstring).  The forward runs on
            # ALIASES of the parameters - fresh leaves on the same storage (torch.func.functional_call): DDP's reducer keeps the
            # real parameters' AccumulateGrad nodes alive, and those belong to the stream DDP was constructed on (the default
            # stream, whose implicit synchronisation a capture forbids: a capture through them dies inside capture_end on this
            # stack); an alias gets its node inside the capture, on the capture stream, like the parameters of a model without DDP.
            world, index, left = self.world, {}, [len(b) for b in self._buckets]
            alias_of = {id(p): p.detach().requires_grad_(True) for p in model.parameters()}
            aliases = {n: alias_of[id(p)] for n, p in model.named_parameters()}
            views, alias_buckets = [], []
            for k, (bucket, flat) in enumerate(zip(self._buckets, self._flats)):
                off, vs = 0, []
                for p in bucket:
                    n = p.numel()
                    dense = p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)
                    vs.append(flat[off:off + n].as_strided(p.shape, p.stride()) if dense else flat[off:off + n].view(p.shape))
                    index[id(alias_of[id(p)])] = k
                    off += n
                views.append(vs)
                alias_buckets.append([alias_of[id(p)] for p in bucket])

            def ready(a):
                k = index[id(a)]
                left[k] -= 1
                if left[k]:
                    return
                flat = self._flats[k]
                torch._foreach_copy_(views[k], [q.grad for q in alias_buckets[k]])
                if world > 1:
                    flat.div_(world)          # DDP's order: divide, then sum over the ranks
                for q, a_, v in zip(self._buckets[k], alias_buckets[k], views[k]):
                    q.grad = v                # AGC and the optimiser read (and AGC rewrites) the averaged gradients in place
                    a_.grad = None            # the alias's own gradient goes back to the graph's pool
                works.append(torch.distributed.all_reduce(flat, async_op=True))
            handles = [a.register_post_accumulate_grad_hook(ready) for b in alias_buckets for a in b]
        was_in_step, _IN_STEP[0] = _IN_STEP[0], True
        try:
            if aliases is None:
                out = model(self.x)
            else:   # the plain module on the aliases: DDP's reducer stays out of the capture
                out = torch.func.functional_call(model, aliases, (self.x,))
            loss = model.loss_fn(self.y, out)
            if self.metrics is not None:   # (before backward: from the same predictions the loss used, into preallocated outputs)
                self.y_pred = out.detach()
                self.metric_out = self.metrics(self.y, self.y_pred, 'train')
            loss.backward()
        finally:
            _IN_STEP[0] = was_in_step
            for h in handles:
                h.remove()
        if self.world:
            if any(n for n in left):
                raise RuntimeError("GraphedTrainStep: a parameter received no gradient - its bucket was never exchanged")
            for w in works:
                w.wait()                      # the capture stream joins RCCL's stream again
        stepped, averaged = False, False
        if model.use_agc:
            if self._agc.attach_optimizer(opt):   # AGC + clipvalue + the optimiser (+ the weight EMA) in one launch (FusedAGC.optimizer_step)
                stepped = self._agc.optimizer_step(0.01, 1e-3, model.clipvalue)
                averaged = stepped and self._agc.ema_attached
            if not stepped:
                self._agc(0.01, 1e-3, model.clipvalue)
            self._agc.freeze()
        elif model.clipvalue:
            torch.nn.utils.clip_grad_value_([p for p in model.parameters() if p.grad is not None], model.clipvalue)
        if not stepped:
            opt.step()
        if model._ema is not None and not averaged:   # the same definition with torch ops: captured like everything else
            model._ema.update(opt)
        opt.zero_grad(set_to_none=True)
        self.loss = loss.detach()
        self._pool_marks = _ZERO_POOL.marks(dev) if SW.ZERO_POOL else {}

    def __call__(self, data):
        x, y = data
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        self.graph.replay()
        if self._pool_marks:
            _ZERO_POOL.mark_dirty(self._pool_marks)   # the replay has written into the zero pool behind its back
        self.model.bump_generation()  # a replay moves parameters and BatchNorm statistics behind ATen's back
        if self.model._ema is not None:
            self.model._ema.bump_generation()   # and the weight EMA's shadows
        if self.metric_out:
            return {'loss': self.loss, **self.metric_out}
        return {'loss': self.loss}

    def set_lr(self, value: float) -> None:
        for g in self.model.optimizer.param_groups:
            if torch.is_tensor(g['lr']):
                g['lr'].fill_(float(value))
            else:
                g['lr'] = float(value)


def graph_step_possible(model: "CustomModel") -> bool:
    """Can `fit` try GraphedTrainStep for this compiled model?  A capturable optimiser, and - under DDP - the RCCL backend."""
    if not optimizer_capturable(model.optimizer):
        return False
    return model._ddp is None or torch.distributed.get_backend() == 'nccl'


def monitor_maximised(name: Optional[str]) -> bool:
    """Is a row entry better when LARGER?  The entries of the compiled count metrics behind 'val_' / 'val_ema_' are
    (metrics.VAL_MAXIMISED: score_curves()'s, sed_eval()'s two F1, psds()'s); every other name (losses, er, seg_er, ...) keeps
    Keras' mode min."""
    if not name:
        return False
    for prefix in ('val_ema_', 'val_'):
        if name.startswith(prefix):
            name = name[len(prefix):]
            break
    from .metrics import VAL_MAXIMISED
    return name in VAL_MAXIMISED


def fit(model: CustomModel, train_set, epochs, steps_per_epoch, validation_data=None, validation_steps=16,
        scheduler=None, csv_path=None, checkpoint_path=None, patience=None, rank=0, world=1, verbose=True,
        swa=None, graph: Optional[bool] = None, checkpoint_monitor: Optional[str] = None, callbacks=(), ema=None,
        ema_checkpoint_path=None):
    """Minimal Keras-fit equivalent for this path: per-epoch LR schedule, CSV log,
    best-val-loss checkpoint, early stopping, TerminateOnNaN (sj_train.py:489-519).
    Compiled metrics (`model.compile(metrics=...)`) are accumulated on the device and read once per epoch: rows gain their names
    and 'val_' twins, Keras' means (per-clip metrics weighted by clips, f1_score by batches).  `checkpoint_monitor` (e.g.
    'val_er', mode min as Keras' 'auto' for these names): the checkpoint follows that row entry while early stopping keeps
    val_loss / loss; None: one monitor for both, as before.  `callbacks`: further objects with on_epoch_end(epoch, model),
    called after the checkpoint is written (metrics.eval_callback).
    `graph` (default: on, IRIS_GRAPH_STEP=0 switches it off): run the training step as ONE replayed hipGraph (GraphedTrainStep) - a
    capturable optimiser (make_optimizer(..., capturable=True)), batches of one shape, under DDP the RCCL backend; a batch of
    another shape (a ragged last one) takes the eager step.  The step then costs what its kernels cost (10 ms per batch of 64)
    however slow the host is at launching ~260 kernels.  A capture that fails is reported ONCE (warnings.warn, every rank) and
    the run goes on eagerly - on every rank alike, from the state the model had before the attempt.
    `ema`: the ema.WeightEMA the model was compiled with (`model.compile(..., ema=ema)`; its module compiled by `ema.compile`).
    After the live model's validation pass a second one runs over the same validation batches (copies: nothing more is drawn from
    `validation_data`) on the EMA module with the live BatchNorm statistics copied in, all-reduced like the first; the row gains
    'val_ema_loss' and the 'val_ema_*' metrics.  Everything the
    live model's row, early stopping and checkpoint depend on is computed as without it.  `ema_checkpoint_path` is written when
    'val_ema_<the checkpoint's monitor>' improves strictly.
    The compiled count metrics add their entries (and the 'val_ema_' twins) after the validation pass, from the validation counts
    summed over the ranks (`MetricSet.val_values`): metrics.score_curves() 'val_auc', 'val_map', 'val_best_f1'; metrics.sed_eval()
    'val_seg_f1', 'val_seg_er', 'val_event_f1'; metrics.psds() 'val_psds'.  A `checkpoint_monitor` with such a name is MAXIMISED
    (strictly larger saves), and so is the EMA's twin of it - but for seg_er, which is minimised."""
    best, bad, history = math.inf, 0, []
    ckpt_sign = -1.0 if monitor_maximised(checkpoint_monitor) else 1.0   # best_ckpt / best_ema hold sign * value: smaller is better
    best_ckpt = math.inf
    best_ema = math.inf
    if ema is not None and model._ema is not ema:
        raise ValueError("fit: `ema` must be the WeightEMA the model was compiled with (model.compile(..., ema=ema))")
    ms = model._metrics

    def metric_sums(phase, dev):
        """The phase's metric accumulator (sums and counts), all-reduced over the ranks - every rank logs and decides alike.
        Still on the device: the caller reads it together with the loss, in one transfer."""
        acc = ms.accum(dev, phase)
        if coll:
            acc = acc.clone()
            torch.distributed.all_reduce(acc)
        return acc
    coll = collectives_on(world)  # world > 1, or a forced process group at world 1 (IRIS_FORCE_PG=1)
    it = iter(train_set)
    graph = SW.GRAPH_STEP if graph is None else bool(graph)
    graph = graph and graph_step_possible(model)
    gstep = None

    def one_step(data):
        nonlocal gstep
        x, y = data
        if not (graph and x.is_cuda):
            return model.train_step(data)
        if gstep is None:
            try:   # the warm-up steps run on this batch and are undone: the first replay is its first update
                gstep = GraphedTrainStep(model, data, preserve_state=True)
            except GraphCaptureError as exc:   # must not take the training run down: eager from here on (all ranks alike)
                import warnings
                warnings.warn(f"fit (rank {rank}): the training step could not be captured as a hipGraph ({exc!s:.300}); "
                              "running it eagerly", RuntimeWarning, stacklevel=2)
                gstep = False
        if gstep and x.shape == gstep.x.shape and y.shape == gstep.y.shape and x.dtype == gstep.x.dtype:
            return gstep(data)
        return model.train_step(data)

    for epoch in range(epochs):
        if scheduler is not None:
            lr = scheduler(epoch)
            for g in model.optimizer.param_groups:
                if torch.is_tensor(g['lr']):
                    g['lr'].fill_(float(lr))   # capturable optimiser: the rate lives in a device tensor (a graph reads it)
                else:
                    g['lr'] = lr
        t0, losses = time.time(), []
        if ms is not None:
            ms.reset()   # (a device fill, outside any graph)
        for _ in range(steps_per_epoch):
            losses.append(one_step(next(it))['loss'].clone() if graph else one_step(next(it))['loss'])
        loss = torch.stack(losses).mean()
        if ema is not None:
            ema.bump_generation()   # the shadows moved behind ATen's back all epoch: `predict` on the EMA module rebuilds its engine
        # The one place per epoch where the frontend plans' status words are read for certain (the hot path also reports a
        # failed earlier launch at the plan's next call, without a sync): EpilogueTimeout naming the plan instead of training
        # on NaN features.  Under DDP the failure of ONE rank must not leave the others waiting in the collectives below, so
        # the verdict rides along with the epoch loss in the same all-reduce and every rank raises after it.
        plan_failure = None
        if loss.is_cuda or SW._PLAN_CHECK_ON_CPU:
            try:
                _fe.check_plans(loss.device)
            except _fe.N.EpilogueTimeout as exc:
                plan_failure = exc
        host = None   # with compiled metrics: [loss, (failed ranks,) 5 metric sums] read in ONE transfer
        if coll:
            pack = torch.stack([loss, loss.new_tensor(1.0 if plan_failure is not None else 0.0)])
            torch.distributed.all_reduce(pack)  # two scalars per epoch
            if ms is None:
                loss, failed_ranks = pack[0] / world, int(round(float(pack[1])))
            else:
                loss = pack[0] / world
                host = torch.cat([torch.stack([loss, pack[1]]).double(), metric_sums('train', loss.device)]).tolist()
                failed_ranks = int(round(host.pop(1)))
            if failed_ranks and plan_failure is None:
                plan_failure = _fe.N.EpilogueTimeout(f"{failed_ranks} other rank(s) of this job reported a failed fused min-max / "
                                                     "log epilogue (NaN features); stopping with them")
        if plan_failure is not None:
            raise plan_failure
        if ms is not None and host is None:
            host = torch.cat([loss.double().view(1), metric_sums('train', loss.device)]).tolist()
        row = {'epoch': epoch, 'loss': float(loss) if host is None else host[0], 'lr': float(model.optimizer.param_groups[0]['lr']),
               'time': time.time() - t0}
        if ms is not None:
            row.update(ms.epoch_values(host[1:]))
        if coll:
            average_bn_statistics(model, world)
        if not math.isfinite(row['loss']):
            if verbose and rank == 0:
                print('NaN loss, terminating')
            break
        if validation_data is not None:
            vit = iter(validation_data)
            kept = [] if ema is not None else None   # the EMA pass sees the SAME batches: copies, and no further draw from the set

            def vbatch():
                batch = next(vit)
                if kept is not None:
                    kept.append(tuple(t.clone() if torch.is_tensor(t) else t for t in batch) if isinstance(batch, (tuple, list)) else batch)
                return batch
            vl = torch.stack([model.test_step(vbatch())['loss'] for _ in range(validation_steps)]).mean()
            if coll:  # every rank validates its own shard: the monitored value is the mean over ranks
                torch.distributed.all_reduce(vl)
                vl = vl / world
            if ms is None:
                row['val_loss'] = float(vl)
            else:
                host = torch.cat([vl.double().view(1), metric_sums('val', vl.device)]).tolist()
                row['val_loss'] = host[0]
                row.update(ms.epoch_values(host[1:], 'val_'))
                row.update(ms.val_values('val_', all_reduce=coll))
            if ema is not None:   # the second pass: the averaged weights under the live model's BatchNorm statistics
                ema.copy_buffers(model)
                ems = ema.module._metrics
                if ems is not None:
                    ems.reset()
                evl = torch.stack([ema.module.test_step(batch)['loss'] for batch in kept]).mean()
                if coll:
                    torch.distributed.all_reduce(evl)
                    evl = evl / world
                if ems is None:
                    row['val_ema_loss'] = float(evl)
                else:
                    acc = ems.accum(evl.device, 'val')
                    if coll:
                        acc = acc.clone()
                        torch.distributed.all_reduce(acc)
                    host = torch.cat([evl.double().view(1), acc]).tolist()
                    row['val_ema_loss'] = host[0]
                    row.update(ems.epoch_values(host[1:], 'val_ema_'))
                    row.update(ems.val_values('val_ema_', all_reduce=coll))
        history.append(row)
        if swa is not None:
            swa.on_epoch_end(epoch, model)
        # The monitored value is identical on every rank (all-reduced above), so best / bad / stop are
        # computed by all ranks alike and they leave the loop together; only file I/O is rank 0's.
        monitor = row.get('val_loss', row['loss'])
        improved = monitor < best
        if improved:
            best, bad = monitor, 0
        else:
            bad += 1
        save = improved
        if checkpoint_monitor is not None:   # Keras ModelCheckpoint(save_best_only=True): strictly better, mode min
            cm = row.get(checkpoint_monitor)
            save = cm is not None and ckpt_sign * cm < best_ckpt
            if save:
                best_ckpt = ckpt_sign * cm
        save_ema = False
        if ema is not None:   # the EMA's own best-only checkpoint, on the EMA pass's twin of the checkpoint's monitor
            name = checkpoint_monitor if checkpoint_monitor is not None else 'val_loss'
            em = row.get('val_ema_' + name[len('val_'):]) if name.startswith('val_') else None
            save_ema = em is not None and ckpt_sign * em < best_ema
            if save_ema:
                best_ema = ckpt_sign * em
        if rank == 0:
            if verbose:
                print(row)
            if csv_path:
                new = not os.path.exists(csv_path)
                with open(csv_path, 'a', newline='') as f:
                    w = csv.DictWriter(f, fieldnames=list(row))
                    if new:
                        w.writeheader()
                    w.writerow(row)
            if save and checkpoint_path:
                torch.save(model.state_dict(), checkpoint_path)
            if save_ema and ema_checkpoint_path:
                torch.save(ema.state_dict(), ema_checkpoint_path)
        for cb in callbacks:
            cb.on_epoch_end(epoch, model)
        stop = patience is not None and not improved and bad >= patience  # Keras EarlyStopping: wait >= patience, tested on a non-improving epoch
        if coll:  # belt and braces: one int per epoch, rank 0's decision wins
            flag = torch.tensor([1 if stop else 0], dtype=torch.int32, device=loss.device)
            torch.distributed.broadcast(flag, src=0)
            stop = bool(int(flag.item()))
        if stop:
            break
    return history
