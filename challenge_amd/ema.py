"""Exponential moving average of the weights, updated every training step and evaluated beside the live model (model EMA / mean
teacher), and BatchNorm recalibration for averaged weights.

    d_t = min(decay, (1 + t) / (10 + t))            t = the optimiser's step counter after its increment (TensorFlow's
    e'  = e + (p' - e) (float)(1 - d_t)                 ExponentialMovingAverage(num_updates) warm-up); p' the updated parameter

On a GPU with the optimisers `make_optimizer` builds the update rides in the one launch that already does AGC, clipvalue and the
optimiser's update (`FusedAGC.attach_ema`, iris_agc_clip_adam_ema of csrc/k_agc_adam.h and its sgd / rmsprop siblings of
csrc/k_agc_optim.h: the updated parameter is still in a register, the shadow costs 8 more bytes of traffic per parameter and no
launch); everywhere else - a CPU model, IRIS_FUSED_ADAM_AGC=0 / IRIS_FUSED_OPTIM_AGC=0, a step the
kernel declines - `WeightEMA.update` applies the same definition with torch ops after `optimizer.step()`.  Both are capturable: the
weight is formed on the device from the counter, so a replayed hipGraph sees every step.  Only parameters are averaged; buffers
(BatchNorm running statistics) are copied from the live model (`copy_buffers`) or recomputed (`recalibrate_bn`)."""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

# attributes of a CustomModel that are not submodules and stay with the original when a shadow is made of it
_NOT_COPIED = ('optimizer', '_ddp', '_fused_agc', '_predict_engine', '_metrics', '_ema')


def ema_weight(t, decay: float) -> torch.Tensor:
    """(float)(1 - min(decay, (1 + t) / (10 + t))) for a counter tensor `t`, formed in double on t's device (no host read)."""
    t = t.detach().to(torch.float64)
    d = torch.clamp((1.0 + t) / (10.0 + t), max=float(decay))
    return (1.0 - d).to(torch.float32)


class WeightEMA:
    """`module`: a second instance of the live model - same construction, layout and device, loaded with the live state, in eval
    mode, taking no gradient - whose parameters are the shadow rows.  `state_dict()` / `load_state_dict()` go through it, so a saved
    EMA is an ordinary checkpoint that `evaluate`, `detect` and `--pretrain` read unchanged.

        ema = WeightEMA(model, 0.999)
        ema.compile(loss, metrics=[...])                  # its own MetricSet: fit's second validation pass
        model.compile(opt, loss, ..., ema=ema)            # train_step / GraphedTrainStep keep it up to date
        fit(model, ..., ema=ema, ema_checkpoint_path=...)"""

    def __init__(self, model: nn.Module, decay: float):
        if not (0.0 <= float(decay) < 1.0):
            raise ValueError(f"WeightEMA: decay {decay} outside [0, 1)")
        self.decay = float(decay)
        keep = {k: model.__dict__.get(k) for k in _NOT_COPIED if k in model.__dict__}
        try:   # (the copy is the model as it was built: same classes, memory formats, device; none of its training surface)
            for k in keep:
                object.__setattr__(model, k, None)
            self.module = copy.deepcopy(model)
        finally:
            for k, v in keep.items():
                object.__setattr__(model, k, v)
        self.module.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        self.module.eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.live = [p for p in model.parameters()]
        self.shadow = [p for p in self.module.parameters()]      # ONE list for good: FusedAGC recognises it by identity
        assert len(self.live) == len(self.shadow)
        # the fallback's own counter, for optimisers that keep none on the parameters' device (sgd; a host-side step count)
        self._t = torch.zeros((), dtype=torch.float32, device=self.shadow[0].device) if self.shadow else None

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        return self.module.load_state_dict(*args, **kwargs)

    def compile(self, loss, metrics=None) -> None:
        """The shadow's `test_step`: the live model's loss and a MetricSet of its own.  Hand it FRESH metric objects - an f1_score()
        shared with the live model would add this pass's counts to the live model's."""
        self.module.compile(None, loss, metrics=metrics)

    def state_tensors(self):
        """Everything a step advances (GraphedTrainStep saves / restores them around its warm-up)."""
        return list(self.shadow) + ([self._t] if self._t is not None else [])

    # ---- the update ----------------------------------------------------------------------------------------------------------
    def attach(self, agc) -> bool:
        """Let `agc` (a FusedAGC over the live parameters) carry the update in its launch."""
        return agc.attach_ema(self.shadow, self.decay, self._t)

    def _counter(self, optimizer):
        """The optimiser's step counter where it is a tensor on the parameters' device (after `step()`: already incremented);
        else this object's own, incremented here."""
        if optimizer is not None and self.live:
            step = optimizer.state.get(self.live[0], {}).get('step')
            if torch.is_tensor(step) and step.device == self.shadow[0].device:
                return step
        self._t.add_(1)
        return self._t

    @torch.no_grad()
    def update(self, optimizer=None) -> None:
        """The definition with torch ops, after `optimizer.step()`: one lerp per parameter, the weight a device scalar."""
        if not self.shadow:
            return
        w = ema_weight(self._counter(optimizer), self.decay)
        for e, p in zip(self.shadow, self.live):
            e.lerp_(p.detach(), w)

    # ---- buffers -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def copy_buffers(self, model: nn.Module) -> None:
        """The live model's buffers (BatchNorm running statistics, batch counts) into the shadow module."""
        for dst, src in zip(self.module.buffers(), model.buffers()):
            dst.copy_(src)
        self.bump_generation()

    def bump_generation(self) -> None:
        """The shadows move behind ATen's version counters (the fused launch, a graph replay): `predict` on `module` rebuilds."""
        if hasattr(self.module, 'bump_generation'):
            self.module.bump_generation()


@torch.no_grad()
def recalibrate_bn(model: nn.Module, batches, world: int = 1) -> int:
    """BatchNorm running statistics for weights that no forward pass has seen (an average of weights): every layer's statistics
    are set to (0, 1), then `batches` (inputs, or (input, target) pairs) run forward in training mode under no_grad with
    momentum 1 / (k + 1) at batch k - the plain mean of the per-batch statistics, what torch.optim.swa_utils.update_bn computes.
    Momentum and mode are restored; under DDP the result is averaged over the ranks.  Returns the number of batches."""
    from .distributed import average_bn_statistics
    bns = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats]
    if not bns:
        return 0
    was_training, momenta = model.training, [bn.momentum for bn in bns]
    for bn in bns:
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0)
    n = 0
    try:
        model.train()
        for k, batch in enumerate(batches):
            x = batch[0] if isinstance(batch, (tuple, list)) else batch
            for bn in bns:
                bn.momentum = 1.0 / (k + 1)
            model(x)
            n += 1
    finally:
        for bn, mom in zip(bns, momenta):
            bn.momentum = mom
        model.train(was_training)
    average_bn_statistics(model, world)
    if hasattr(model, 'bump_generation'):
        model.bump_generation()
    return n
