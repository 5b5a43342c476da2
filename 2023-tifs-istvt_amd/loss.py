"""The training criterion on the HIP path: ``nn.BCEWithLogitsLoss`` with per-sample weights,
``pos_weight`` and label smoothing in one launch forward and one launch backward, and the epoch's loss / accuracy /
confusion counts kept in a device block that the same launch adds to.

    criterion = BCEWithLogitsLoss(meter=TrainMeter('cuda'))          # train_CNN.py:148
    loss = criterion(outputs.view(-1), labels)                        # train_CNN.py:526 (labels as they come: no .float())
    loss.backward()
    ...
    snap = criterion.meter.snapshot()                                 # where the loop prints; no device-wide sync
    print(snap.loss_mean, snap.accuracy)

``bce_logits_ref`` is the float64 host restatement of the same definition, for tests and tools/loss_bench.py."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .parallel import HostScalar

METER_COUNTS = ('seen', 'correct', 'tp', 'tn', 'fp', 'fn', 'calls')


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else float('nan')


class MeterSnapshot:
    """The meter block on the host.  ``TrainMeter.snapshot()`` returns one whose values arrive behind an event: the first
    attribute read waits for that copy alone.  Ratios with an empty denominator are NaN."""

    def __init__(self, loss_sum: float = 0.0, batch_loss_sum: float = 0.0, seen: int = 0, correct: int = 0, tp: int = 0,
                 tn: int = 0, fp: int = 0, fn: int = 0, calls: int = 0):
        self._buf = self._done = None
        self._set(float(loss_sum), float(batch_loss_sum), [seen, correct, tp, tn, fp, fn, calls])

    def _set(self, loss_sum, batch_loss_sum, counts):
        self._loss_sum, self._batch_loss_sum = loss_sum, batch_loss_sum
        self._counts = {k: int(v) for k, v in zip(METER_COUNTS, counts)}

    @classmethod
    def _pending(cls, buf: torch.Tensor, done) -> 'MeterSnapshot':
        s = cls()
        s._buf, s._done = buf, done
        return s

    def _get(self):
        if self._done is not None:
            self._done.synchronize()
            words = self._buf
            sums = words[:2].view(torch.float64).tolist()
            self._set(sums[0], sums[1], words[2:2 + len(METER_COUNTS)].tolist())
            self._buf = self._done = None
        return self

    @property
    def counts(self) -> dict:
        return dict(self._get()._counts)

    @property
    def loss_sum(self) -> float:
        return self._get()._loss_sum

    @property
    def batch_loss_sum(self) -> float:
        """the sum of the values the calls returned: the reference's ``train_loss += loss.item()``"""
        return self._get()._batch_loss_sum

    @property
    def loss_mean(self) -> float:
        """mean per-sample loss over everything seen"""
        c = self._get()._counts
        return _ratio(self._loss_sum, c['seen'])

    @property
    def accuracy(self) -> float:
        c = self._get()._counts
        return _ratio(c['correct'], c['seen'])

    @property
    def apcer(self) -> float:
        """attacks (label 1) taken for real: fn / (tp + fn), train_CNN.py:885"""
        c = self._get()._counts
        return _ratio(c['fn'], c['tp'] + c['fn'])

    @property
    def bpcer(self) -> float:
        """real samples (label 0) taken for attacks: fp / (tn + fp), train_CNN.py:886"""
        c = self._get()._counts
        return _ratio(c['fp'], c['tn'] + c['fp'])

    @property
    def acer(self) -> float:
        return (self.apcer + self.bpcer) / 2

    def __repr__(self):
        return 'MeterSnapshot(loss_mean=%.6g, accuracy=%.6g, counts=%r)' % (self.loss_mean, self.accuracy, self.counts)


class TrainMeter:
    """The device block the criterion's forward launch adds every call to (include/istvt_hip.h, istvt_loss_meter): sums of
    the per-sample and of the returned losses in fp64, samples seen, correct, tp / tn / fp / fn, calls.  One writer, ordered
    by the stream the criterion runs on.  ``tensor`` is the raw block (int64 (10,), the first two words float64 bits) for a
    caller that reduces it across ranks itself."""

    def __init__(self, device='cuda'):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('istvt_amd: a TrainMeter must be on a ROCm device (no CPU fallback exists for the ISTVT hot path)')
        self.tensor = torch.zeros((ops.METER_WORDS,), dtype=torch.int64, device=device)

    def reset(self) -> None:
        """one asynchronous fill"""
        self.tensor.zero_()

    def snapshot(self) -> MeterSnapshot:
        """The block as it is at this point of the current stream, read without draining the stream: HostScalar's mechanism
        (pinned buffer, event, HostScalar's side stream).  The block is first copied on the current stream, so a criterion call
        enqueued later cannot change what the side stream reads."""
        stage = self.tensor.clone()
        dev = stage.device
        side = HostScalar._streams.get(dev.index)
        if side is None:
            side = HostScalar._streams[dev.index] = torch.cuda.Stream(device=dev)
        buf = torch.empty((ops.METER_WORDS,), dtype=torch.int64).pin_memory()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            side.wait_event(ready)
            buf.copy_(stage, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        stage.record_stream(side)
        return MeterSnapshot._pending(buf, done)


class _BCELogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y, weight, pos_weight, label_smoothing, reduction, threshold, meter, want_grad):
        # want_grad comes from the caller: in here grad mode is always off, and needs_input_grad says what the logits
        # require, not whether anything is being recorded (torch.no_grad() around a validation loop)
        none = reduction == 'none'
        loss, reduced, d = ops.bce_logits(z, y, weight, pos_weight, label_smoothing, reduction, threshold, want_loss=none,
                                          want_reduced=not none, want_grad=want_grad, meter=meter)
        if want_grad:
            ctx.save_for_backward(d)
        return loss if none else reduced.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d, = ctx.saved_tensors
        return (ops.bce_logits_bwd(d, g),) + (None,) * 8


class BCEWithLogitsLoss(torch.nn.Module):
    """``torch.nn.BCEWithLogitsLoss`` on the HIP path, with torch's argument names: ``crit(outputs.view(-1), labels)``.

    weight           per-sample weights, float32 (n,) on the logits' device (a buffer of the module), or None
    reduction        'mean' (divides by n, as torch), 'sum', 'none'
    pos_weight       a number or a one-element tensor, read ONCE here
    label_smoothing  eps in [0, 1): targets become y (1 - eps) + eps / 2; the meter's counts use the unsmoothed y
    threshold        prediction = logit > threshold (the reference's ``outputs > 0``)
    meter            a TrainMeter: every call adds its losses and counts, also under torch.no_grad()

    Logits: CUDA float32, 1-D, any stride (a column of (B, nc) needs no copy).  Targets: float32, int64, int32, uint8 or
    bool, (n,).  One launch forward (which also fills the unscaled logit gradient when one is needed), one launch backward;
    nothing synchronises, so the call can be captured in a torch.cuda.graph."""

    def __init__(self, weight: Optional[torch.Tensor] = None, reduction: str = 'mean', pos_weight=None,
                 label_smoothing: float = 0.0, threshold: float = 0.0, meter: Optional[TrainMeter] = None):
        super().__init__()
        if reduction not in ops.BCE_REDUCTIONS:
            raise ValueError("BCEWithLogitsLoss: reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError('BCEWithLogitsLoss: label_smoothing must be in [0, 1), got %r' % (label_smoothing,))
        if torch.is_tensor(pos_weight):
            if pos_weight.numel() != 1:
                raise ValueError('BCEWithLogitsLoss: pos_weight is one number (one logit per sample), got %s'
                                 % (tuple(pos_weight.shape),))
            pos_weight = pos_weight.item()
        if meter is not None and not isinstance(meter, TrainMeter):
            raise TypeError('BCEWithLogitsLoss: meter must be a TrainMeter, got %s' % type(meter).__name__)
        if weight is not None and (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.dim() != 1):
            raise TypeError('BCEWithLogitsLoss: weight must be a float32 (n,) tensor')
        self.register_buffer('weight', weight)
        self.reduction = reduction
        self.pos_weight = 1.0 if pos_weight is None else float(pos_weight)
        self.label_smoothing = float(label_smoothing)
        self.threshold = float(threshold)
        self.meter = meter

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return _BCELogits.apply(input, target, self.weight, self.pos_weight, self.label_smoothing, self.reduction,
                                self.threshold, None if self.meter is None else self.meter.tensor,
                                torch.is_grad_enabled() and input.requires_grad)

    def extra_repr(self):
        return 'reduction=%r, pos_weight=%g, label_smoothing=%g, threshold=%g, meter=%s' % (
            self.reduction, self.pos_weight, self.label_smoothing, self.threshold, self.meter is not None)


def bce_logits_ref(z, y, weight=None, pos_weight: float = 1.0, label_smoothing: float = 0.0, reduction: str = 'mean',
                   threshold: float = 0.0) -> dict:
    """Float64 restatement on the host of what istvt_bce_logits computes (include/istvt_hip.h), written in torch's own
    order of operations: per-sample ``loss``, ``reduced`` (the sum for 'none' and 'sum', sum / n for 'mean'), ``grad`` = the
    gradient of ``reduced`` by the logits, and the ``counts`` seen / correct / tp / tn / fp / fn of one call."""
    z = torch.as_tensor(z).detach().cpu().double().reshape(-1)
    y = torch.as_tensor(y).detach().cpu().double().reshape(-1)
    n = z.shape[0]
    w = torch.ones(n, dtype=torch.float64) if weight is None else torch.as_tensor(weight).detach().cpu().double().reshape(-1)
    ys = y * (1.0 - label_smoothing) + 0.5 * label_smoothing
    coef = 1.0 + (pos_weight - 1.0) * ys
    log_sigmoid = torch.clamp(z, max=0.0) - torch.log1p(torch.exp(-z.abs()))
    loss = ((1.0 - ys) * z - coef * log_sigmoid) * w
    # (1 - y') - coef sigmoid(-z) with 1 - sigmoid(-z) = sigmoid(z) taken first: exact where sigmoid(-z) rounds to 1
    grad = w * ((1.0 - ys) * torch.sigmoid(z) - pos_weight * ys * torch.sigmoid(-z))
    total = loss.sum()
    if reduction == 'mean':
        total, grad = total / n, grad / n
    elif reduction not in ('sum', 'none'):
        raise ValueError('reduction %r' % (reduction,))
    pred, pos = z > threshold, y > 0.5
    tp, tn = int((pred & pos).sum()), int((~pred & ~pos).sum())
    fp, fn = int((pred & ~pos).sum()), int((~pred & pos).sum())
    return {'loss': loss, 'reduced': total, 'grad': grad,
            'counts': {'seen': n, 'correct': tp + tn, 'tp': tp, 'tn': tn, 'fp': fp, 'fn': fn}}
