"""Data parallelism for the ISTVT path: one process per GPU, clips sharded over the batch axis,
ONE all-reduce (RCCL over xGMI when the backend is "nccl", gloo on CPU for tests) of a flat
gradient bucket per step.

The reference's only multi-GPU mode is single-process nn.DataParallel (train_CNN.py:185-186):
per-replica BatchNorm statistics, gradients summed onto device 0.  The equivalent here keeps
per-rank BN statistics (no SyncBN, as the reference) and averages gradients: the loss is a
batch mean, so mean-of-rank-means == global mean for equal shards.

Only parameters that can receive a gradient go in the bucket: the Xception wrapper holds 19.7 M
parameters (block4..fc) that ``low_level_features`` never touches.
"""
from __future__ import annotations

import itertools
import operator
import os
import weakref
from typing import Iterable, List, Tuple

import torch
import torch.distributed as dist

from . import stem as _stem


def _single_rank(group=None) -> bool:
    """True when the collectives can be skipped: a world of one rank.  ISTVT_FORCE_COLLECTIVES=1 runs them anyway -- on a
    one-GPU box that is the only way to drive RCCL through exactly the calls, streams and waits of the N > 1 path
    (`bench.py --rccl-rehearsal`); a one-rank all-reduce leaves the values unchanged."""
    return dist.get_world_size(group) == 1 and os.environ.get('ISTVT_FORCE_COLLECTIVES') != '1'


def live_named_parameters(model: torch.nn.Module) -> List[Tuple[str, torch.nn.Parameter]]:
    """Parameters on the hot path (everything except the never-executed Xception tail)."""
    keep = set('xcep.model.' + n for n in _stem.param_names())
    out = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if name.startswith('xcep.') and name not in keep:
            continue
        out.append((name, p))
    return out


class GradBucket:
    """Flat fp32 gradient buffer; every live parameter's ``.grad`` is a view into it."""

    def __init__(self, params: Iterable[torch.nn.Parameter], fuse_accumulate: bool = False,
                 flatten_params: bool = False):
        """fuse_accumulate: let the HIP weight-gradient kernels add straight into the bucket
        (functional._target) instead of returning fresh tensors for autograd to add.
        flatten_params: also move the parameters themselves into one flat fp32 buffer (``flat_params``; each
        ``p.data`` becomes a view of it, values preserved) -- what FusedSGD / FusedAdamW step over."""
        self.params = list(params)
        for p in self.params:
            p._istvt_fused_grad = bool(fuse_accumulate)
        if not self.params:
            raise ValueError('GradBucket needs at least one parameter')
        dev = self.params[0].device
        self.numel = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            off += n
        self.defer_scale = False        # set by the fused optimizers: all_reduce() then only sums, the step kernel scales
        self.grad_scale = 1.0           # what the next fused optimizer step multiplies the gradients by (1 / world size)
        self._early = None
        self._early_work = None
        # CUs left to the collective's kernels while the early all-reduce overlaps the stem backward (RCCL runs one
        # workgroup per channel; the persistent GEMM kernels need whole CUs).  ISTVT_RCCL_CU_RESERVE overrides.
        self.cu_reserve = int(os.environ.get('ISTVT_RCCL_CU_RESERVE', '32'))
        self._reserved = None           # (device index, value before ours) while the reserve is raised
        self._on_ready = None
        self.flat_params = None
        if flatten_params:
            if any(p.dtype != torch.float32 for p in self.params):
                raise TypeError('flatten_params needs float32 parameters')
            self.flat_params = torch.empty(self.numel, dtype=torch.float32, device=dev)
            off = 0
            for p in self.params:
                n = p.numel()
                view = self.flat_params[off:off + n].view_as(p)
                view.copy_(p.data)
                p.data = view
                off += n

    def zero(self):
        # weight gradients of a backward pass that aborted may still be queued on the side stream: they must land
        # before the zero fill, not after it; so must an early all-reduce that such a backward started and no
        # all_reduce() call collected (it also still holds the CU reserve)
        from . import functional as Fn
        Fn.flush_stale_joins()
        self._drop_early_work()
        self.flat.zero_()

    def enable_early_all_reduce(self, first_param: int, group=None):
        """Overlap the gradient all-reduce with the stem backward: the gradients of ``params[first_param:]`` (the
        transformer, when the parameters are in model order: stem first) are complete when the backward pass reaches
        the token assembly, long before the stem's are.  Their slice of the bucket is then all-reduced asynchronously
        (functional.grad_ready_hooks); ``all_reduce()`` later waits for it and reduces the rest.  Needs every gradient
        of the slice to be written by the kernels themselves (fuse_accumulate=True): a gradient handed back to autograd
        could still be accumulated after the hook.  No effect without an initialised process group of size > 1."""
        from . import functional as Fn
        if not all(getattr(p, '_istvt_fused_grad', False) for p in self.params[first_param:]):
            raise ValueError('enable_early_all_reduce needs GradBucket(..., fuse_accumulate=True)')
        lo = sum(p.numel() for p in self.params[:first_param])
        self._drop_early_work()
        self.disable_early_all_reduce()
        self._early = (lo, self.numel, group)
        ref = weakref.ref(self)          # the global hook list must not keep a dropped bucket (and its collectives) alive

        def on_ready(device):
            me = ref()
            if me is None:
                if on_ready in Fn.grad_ready_hooks:
                    Fn.grad_ready_hooks.remove(on_ready)
                return
            if not (dist.is_available() and dist.is_initialized()):
                return
            if _single_rank(group) or device != me.flat.device:
                return
            if me._early_work is not None:
                # a second backward before all_reduce() (gradient accumulation): its kernels would add into the slice
                # while the asynchronous collective is still reducing it, and its gradients would never be summed
                raise RuntimeError('GradBucket: early all-reduce still in flight; there must be exactly one backward per '
                                   'all_reduce() (call disable_early_all_reduce() for gradient accumulation)')
            if device.type == 'cuda':
                Fn.join_side_stream(device.index)       # the side-stream weight gradients are part of the slice
            me._early_work = (dist.all_reduce(me.flat[lo:me.numel], op=dist.ReduceOp.SUM, group=group, async_op=True), lo)
            # the collective's kernels hold CUs until it is done: the persistent GEMMs of the stem backward, which runs
            # beside it, are launched on the CUs that are left (ops.set_cu_reserve), reset in all_reduce()
            if device.type == 'cuda' and me.cu_reserve > 0:
                from . import ops
                me._reserved = (device.index, ops.set_cu_reserve(me.cu_reserve, device.index))

        self._on_ready = on_ready
        Fn.grad_ready_hooks.append(on_ready)

    def _release_cus(self):
        """put back the CU reserve that the early all-reduce hook raised (the value found then, not 0)"""
        if self._reserved is not None:
            from . import ops
            idx, prev = self._reserved
            self._reserved = None
            ops.set_cu_reserve(prev, idx)

    def _drop_early_work(self):
        """an early collective nobody will wait for through all_reduce() (re-arming, a backward that aborted after the
        hook): wait for it here so it cannot write into the bucket later, and give the CUs back"""
        if self._early_work is not None:
            work, _ = self._early_work
            self._early_work = None
            try:
                work.wait()
            except Exception:       # noqa: BLE001  (a torn-down process group)
                pass
        self._release_cus()

    def disable_early_all_reduce(self):
        """No early collective is started from the next backward on.  One already in flight stays owned by the
        all_reduce() call that follows (which also returns its CUs)."""
        from . import functional as Fn
        if self._on_ready is not None and self._on_ready in Fn.grad_ready_hooks:
            Fn.grad_ready_hooks.remove(self._on_ready)
        self._on_ready = None
        self._early = None
        if self._early_work is None:
            self._release_cus()

    def __del__(self):
        try:
            self.disable_early_all_reduce()
            self._release_cus()
        except Exception:           # noqa: BLE001  (interpreter shutdown)
            pass

    def _scale(self, world: int):
        if self.defer_scale:
            self.grad_scale = 1.0 / world           # folded into the fused optimizer step: no pass over the bucket
        else:
            self.flat.mul_(1.0 / world)

    def apply_deferred_scale(self):
        """multiply the bucket by the pending 1 / world-size factor now (one pass) instead of inside the next fused
        optimizer step: afterwards ``p.grad`` are the global-batch mean gradients, as after a plain all-reduce"""
        if self.grad_scale != 1.0:
            self.flat.mul_(self.grad_scale)
            self.grad_scale = 1.0

    def all_reduce(self, group=None, chunks: int = 1):
        """sum over ranks then divide by world size (== DataParallel's global-batch mean).

        With a fused optimizer attached (``defer_scale``) the division happens inside its step kernel: between this call
        and ``optimizer.step()`` every ``p.grad`` holds the cross-rank SUM (``world`` times the mean).  Gradient clipping
        and gradient-norm logging need nothing in between: ``FusedSGD / FusedAdamW(..., max_grad_norm=...)`` clip against,
        and ``optimizer.grad_norm()`` reports, the norm of the global-batch MEAN gradient (the pending ``grad_scale`` is
        part of the norm kernel).  Only code that reads ``p.grad`` itself -- torch's ``clip_grad_norm_``, a non-fused
        optimizer over ``bucket.params`` -- must call ``apply_deferred_scale()`` first."""
        if not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(group)
        if _single_rank(group):
            return
        if self._early_work is not None:    # the transformer's slice is already in flight (enable_early_all_reduce)
            work, lo = self._early_work     # (lo travels with the work: disable_early_all_reduce() may have run since)
            self._early_work = None
            self._release_cus()                 # what is launched from here on runs after the collective (work.wait())
            if lo > 0:
                dist.all_reduce(self.flat[:lo], op=dist.ReduceOp.SUM, group=group)
            work.wait()
            self._scale(world)
            return
        if chunks <= 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
        else:
            works = [dist.all_reduce(c, op=dist.ReduceOp.SUM, group=group, async_op=True)
                     for c in self.flat.chunk(chunks)]
            for w in works:
                w.wait()
        self._scale(world)


class HostScalar:
    """The value of a device scalar on the host WITHOUT draining the launch queue.

    ``loss.item()`` (train_CNN.py:534) copies on the current stream: it returns when everything enqueued before it -- the
    whole backward pass and the optimizer step -- has run, and the next step then starts from an empty queue (measured at
    C2: +1.4 ... 2.1 ms per step; the copy itself is nothing).  ``HostScalar(loss)`` created where the value is PRODUCED
    (right after the loss / the accuracy count, before ``backward()``) records an event there and copies device -> pinned
    host memory on a stream of its own behind that event; ``.item()`` -- called where the loop needs the number, after
    ``optimizer.step()`` -- waits for that copy only, which finished while the backward pass was still running.  Same
    values at the same program points as the reference loop, no device-wide sync (tools/host_boundary_probe.py, round 6 with
    the probe's upload race fixed: 52.86 ms per step against 53.22 with ``.item()``, 52.33 with resident inputs and no
    readback; round 5, before the host work at the head of a step moved behind the optimizer step: 53.5 / 54.9 / 53.1)."""

    _streams: dict = {}

    def __init__(self, t: torch.Tensor):
        if t.numel() != 1:
            raise ValueError('HostScalar takes a one-element tensor')
        t = t.detach().reshape(1)
        if not t.is_cuda:                       # nothing to overlap: a host tensor is its own value
            self._value, self._done, self._buf = t[0].item(), None, None
            return
        idx = t.device.index
        side = HostScalar._streams.get(idx)
        if side is None:
            side = HostScalar._streams[idx] = torch.cuda.Stream(device=t.device)
        self._buf = torch.empty((1,), dtype=t.dtype).pin_memory()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(t.device))
        with torch.cuda.stream(side):
            side.wait_event(ready)
            self._buf.copy_(t, non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(side)
        t.record_stream(side)                   # the allocator must not hand t's block out before the copy has read it
        self._value = None

    def item(self):
        if self._value is None:
            self._done.synchronize()
            self._value = self._buf[0].item()
        return self._value

    def __float__(self):
        return float(self.item())

    def __int__(self):
        return int(self.item())


def broadcast_parameters(model: torch.nn.Module, src: int = 0, group=None):
    """identical weights/buffers on every rank (DataParallel replicates module 0 each step)."""
    if not (dist.is_available() and dist.is_initialized()) or _single_rank(group):
        return
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, src, group=group)
    # `.data` has its own version counter: the cached bf16 / transposed operand copies of any weight that was already
    # used in a forward would survive the overwrite.  (Anyone writing parameters through `.data` or raw pointers calls
    # ops.invalidate_weight_cache() likewise.)
    from . import ops
    ops.invalidate_weight_cache()


def shard_batch(x: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """rank r gets clips [r*B/W, (r+1)*B/W)."""
    b = x.shape[0]
    if b % world != 0:
        raise ValueError('global batch %d is not divisible by world size %d' % (b, world))
    per = b // world
    return x[rank * per:(rank + 1) * per]


MAX_PARAM_GROUPS = 8            # the by-value {lr, weight_decay} table of the grouped step kernels
GRAD_NORM_CHUNK = 16384         # elements one workgroup of istvt_grad_norm reduces (istvt_grad_norm_ws_elems(n) = chunks of n)


def segment_table(params, groups):
    """The segment table of the grouped step kernels, on the host (no GPU needed).

    ``params``: the bucket's parameters in bucket order; ``groups``: one list of parameters per named group, in any order
    and not necessarily contiguous in the bucket.  Parameters no group names form a last group of their own.  Returns
    ``(ends, group_ids, group_of)``: the sorted end offsets of the segments (the last one is the bucket's size), the group of
    each segment -- consecutive parameters of one group are merged into one segment -- and the group index of every parameter.
    ValueError: a parameter in two groups, a parameter that is not in the bucket, more than MAX_PARAM_GROUPS groups."""
    params = list(params)
    index = {id(p): i for i, p in enumerate(params)}
    group_of = [None] * len(params)
    groups = [list(g) for g in groups]
    for gi, members in enumerate(groups):
        for q in members:
            i = index.get(id(q))
            if i is None:
                raise ValueError('param group %d names a parameter that is not in the bucket' % gi)
            if group_of[i] is not None:
                raise ValueError('parameter %d of the bucket appears in more than one param group' % i)
            group_of[i] = gi
    count = len(groups)
    if any(g is None for g in group_of):
        group_of = [count if g is None else g for g in group_of]
        count += 1
    if count > MAX_PARAM_GROUPS:
        raise ValueError('%d param groups (the default group included): the fused optimizers take at most %d'
                         % (count, MAX_PARAM_GROUPS))
    ends, gids, off = [], [], 0
    for q, gi in zip(params, group_of):
        if q.numel() == 0:
            continue
        off += q.numel()
        if gids and gids[-1] == gi:
            ends[-1] = off
        else:
            ends.append(off)
            gids.append(gi)
    return ends, gids, group_of


class _FusedOptimizer(torch.optim.Optimizer):
    """Common part of the fused optimizers: one HIP launch over GradBucket's flat parameter / gradient buffers
    (reference optimizers: train_CNN.py:196-201).  ``zero_grad=True`` makes the step kernel
    write zeros over the gradients it has just consumed, so the training loop needs no zero-grad pass.

    They are torch.optim.Optimizer objects with real ``param_groups`` whose hyper-parameters (``lr`` ...) are read at every
    step, so ``lr_scheduler.CosineAnnealingLR(optimizer, ...)`` (train_CNN.py:202) works; ``state_dict()`` /
    ``load_state_dict()`` carry the step count and the flat state buffers.

    ``param_groups``: a list of dicts as torch takes them (``{'params': [...], 'lr': ..., 'weight_decay': ...}``), at most
    MAX_PARAM_GROUPS with the default group that collects every parameter no dict names.  ``lr`` and ``weight_decay`` are
    per group; the other hyper-parameters must agree.  ``max_grad_norm``: clip the global L2 norm of the global-batch mean
    gradient, as ``clip_grad_norm_(params, max_grad_norm)`` in front of the step would (the pending ``bucket.grad_scale``
    is included: no ``apply_deferred_scale()``).  ``skip_nonfinite``: a step whose gradient norm is inf / NaN changes no
    parameter and no state, and is not counted (SGD's first-step rule and AdamW's bias corrections follow the applied
    steps).  Either of the two adds one pass that reads the bucket (istvt_grad_norm); ``step()`` still never synchronises
    and never copies to the host -- ``grad_norm()`` / ``skipped_steps()`` hand out HostScalars.  With none of the three the
    optimizer launches exactly the one-group kernel it always launched."""

    _state_names: Tuple[str, ...] = ()
    _shared_keys: Tuple[str, ...] = ()      # hyper-parameters the kernels take once: they must agree across the groups

    def __init__(self, bucket: GradBucket, defaults: dict, zero_grad: bool, param_groups=None, max_grad_norm=None,
                 skip_nonfinite: bool = False):
        if bucket.flat_params is None:
            raise ValueError('the fused optimizers need GradBucket(..., flatten_params=True)')
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError('max_grad_norm must be positive (None: no clipping)')
        table = None
        if param_groups is not None:
            param_groups = [dict(g) for g in param_groups]
            for g in param_groups:
                g['params'] = list(g['params']) if not isinstance(g['params'], torch.Tensor) else [g['params']]
            table = segment_table(bucket.params, [g['params'] for g in param_groups])
            rest = [q for q, gi in zip(bucket.params, table[2]) if gi == len(param_groups)]
            if rest:
                param_groups = param_groups + [{'params': rest}]
            self._check_shared([dict(defaults, **g) for g in param_groups])
        if not bucket.flat.is_cuda:
            raise RuntimeError('the fused optimizers run on the GPU only (no CPU fallback)')
        super().__init__(bucket.params if param_groups is None else param_groups, defaults)
        self.bucket = bucket
        bucket.defer_scale = True           # all_reduce() leaves the sum; step() applies 1 / world size
        self.fused_zero_grad = bool(zero_grad)
        self.steps = 0                      # step() calls (what zero_grad() goes by); skip mode: see applied_steps()
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        # torch numbers parameters group by group: _order[torch index] = bucket index
        index = {id(q): i for i, q in enumerate(bucket.params)}
        self._order = [index[id(q)] for g in self.param_groups for q in g['params']]
        self._seg = self._info = self._norm_ws = None
        dev = bucket.flat.device
        if len(self.param_groups) > 1 or self._uses_info():
            ends, gids, _ = table if table is not None else segment_table(bucket.params, [])
            self._seg = (torch.tensor(ends, dtype=torch.int64, device=dev), torch.tensor(gids, dtype=torch.int32, device=dev))
        if self._uses_info():
            from . import _lib
            self._info = torch.zeros(8, dtype=torch.int32, device=dev)          # the step-info block (include/istvt_hip.h)
            self._norm_ws = torch.empty(_lib.lib().istvt_grad_norm_ws_elems(bucket.numel), dtype=torch.float64, device=dev)

    @property
    def hyper(self) -> dict:
        return self.param_groups[0]

    def _uses_info(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _check_shared(self, groups):
        def same(a, b):
            return tuple(a) == tuple(b) if isinstance(a, (list, tuple)) else a == b
        for g in groups[1:]:
            for k in self._shared_keys:
                if not same(g[k], groups[0][k]):
                    raise ValueError('fused optimizer: %r must be the same in every param group (%r in group 0, %r in group '
                                     '%d); only lr and weight_decay are per group' % (k, groups[0][k], g[k], groups.index(g)))

    def _group_args(self):
        """the kernels' by-value {lr, weight_decay} table, read from the param groups at every step"""
        from ctypes import c_float
        groups = self.param_groups
        if len(groups) > MAX_PARAM_GROUPS:
            raise ValueError('the fused optimizers take at most %d param groups' % MAX_PARAM_GROUPS)
        self._check_shared(groups)
        arr = c_float * len(groups)
        return arr(*[g['lr'] for g in groups]), arr(*[g['weight_decay'] for g in groups]), len(groups)

    def _norm_pass(self):
        """istvt_grad_norm over the bucket when clipping or skipping is on: the address of the step-info block the
        step kernel then reads its gradient scale (and, in skip mode, its step count) from; otherwise None"""
        if self._info is None:
            return None
        from . import _lib, ops
        b = self.bucket
        _lib.check(_lib.lib().istvt_grad_norm(b.flat.data_ptr(), b.numel, float(b.grad_scale), self.max_grad_norm or 0.0,
                                              int(self.skip_nonfinite), self._norm_ws.data_ptr(), self._norm_ws.numel(),
                                              self._info.data_ptr(), ops._stream()), 'istvt_grad_norm')
        return self._info.data_ptr()

    def _info_scalar(self, word: int, dtype) -> 'HostScalar':
        if self._info is None:
            raise RuntimeError('needs max_grad_norm=... or skip_nonfinite=True: without them no norm is computed')
        # a copy on the current stream: the next step's norm kernel overwrites the block
        return HostScalar(self._info[word:word + 1].view(dtype).clone())

    def grad_norm(self) -> 'HostScalar':
        """L2 norm of the last step's global-batch mean gradient (before clipping), without a sync in the loop: take it
        after ``step()``, call ``.item()`` where the number is needed"""
        return self._info_scalar(0, torch.float32)

    def skipped_steps(self) -> 'HostScalar':
        """how many steps ``skip_nonfinite`` has skipped so far (the device counter)"""
        return self._info_scalar(4, torch.int32)

    def applied_steps(self) -> int:
        """steps that changed the parameters.  In skip mode the count lives on the device: reading it synchronises."""
        return int(self._info[3].item()) if self.skip_nonfinite else self.steps

    def zero_grad(self, set_to_none: bool = False):
        if set_to_none:
            raise ValueError('gradients are views of the flat bucket: they cannot be set to None')
        # A backward pass that aborted behind the grad-ready hook leaves an early all-reduce nobody collected (and the CU
        # reserve raised): it is waited for and dropped HERE, on every call -- the fused step's re-zeroing skips
        # bucket.zero(), which used to be the only way to reach this recovery -- and the half-reduced bucket of
        # such a step is really zeroed.
        aborted = self.bucket._early_work is not None
        self.bucket._drop_early_work()
        if aborted or not (self.fused_zero_grad and self.steps > 0):
            self.bucket.zero()

    def _done(self):
        from . import ops
        self.steps += 1
        self.bucket.grad_scale = 1.0
        ops.invalidate_weight_cache()       # the kernel wrote parameters without bumping their version counters
        # Re-cast the bf16 operand copies NOW, right behind the update: the bookkeeping (~0.7 ms of Python for ~40 operands)
        # and the grouped cast launch then happen while the GPU is still working through the backward pass, instead of at
        # the head of the next forward pass -- where, in a loop that syncs every step (loss.item(), train_CNN.py:534), the
        # GPU sat idle for it (tools/sync_gap_probe.py: 0.65 ms per step).  The forward's own call finds nothing stale.
        ops.refresh_stale_operands()

    def _slices(self):
        """(torch's parameter index, parameter, offset in the flat buffers, elements), in torch's order"""
        offs, off = [], 0
        for q in self.bucket.params:
            offs.append(off)
            off += q.numel()
        for i, bi in enumerate(self._order):
            q = self.bucket.params[bi]
            yield i, q, offs[bi], q.numel()

    def _extra_state(self, steps) -> dict:  # per-parameter entries beside the flat buffers (AdamW's step count)
        return {}

    def state_dict(self):
        """torch.optim's format -- ``{'state': {index: {name: tensor}}, 'param_groups': [{..., 'params': [indices]}]}``
        -- with the per-parameter tensors cut out of the flat state buffers and the parameters numbered group by group as
        torch numbers them, so a checkpoint written here loads into torch.optim.SGD / AdamW built with the same groups and
        the other way round.  ``fused_steps`` (ignored by torch) keeps the step count for SGD, whose torch state has none;
        in skip mode it is the applied count."""
        steps = self.applied_steps()
        state = {}
        if steps > 0:                       # torch optimizers have no state before their first step either
            for i, p, off, n in self._slices():
                st = {name: getattr(self, name)[off:off + n].view_as(p).detach().clone() for name in self._state_names}
                st.update(self._extra_state(steps))
                state[i] = st
        groups, first = [], 0
        for g in self.param_groups:
            out = {k: v for k, v in g.items() if k != 'params'}
            out['params'] = list(range(first, first + len(g['params'])))
            first += len(g['params'])
            groups.append(out)
        return {'state': state, 'param_groups': groups, 'fused_steps': steps}

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if len(groups) != len(self.param_groups) or \
                any(len(g['params']) != len(mine['params']) for g, mine in zip(groups, self.param_groups)):
            raise ValueError('fused optimizer: expected %d param group(s) over %s parameters, the checkpoint has %s'
                             % (len(self.param_groups), [len(g['params']) for g in self.param_groups],
                                [len(g['params']) for g in groups]))
        # every saved key, as torch.optim does (a checkpoint written with an LR scheduler attached carries
        # 'initial_lr', which CosineAnnealingLR(last_epoch=E) needs on resume); the kernels read only the keys they know
        for g, mine in zip(groups, self.param_groups):
            mine.update({k: v for k, v in g.items() if k != 'params'})
        state = sd['state']
        steps = 0
        for i, p, off, n in self._slices():
            st = state.get(i, state.get(str(i)))
            for name in self._state_names:
                dst = getattr(self, name)[off:off + n]
                src = None if st is None else st.get(name)
                if src is None:
                    dst.zero_()
                else:
                    if src.numel() != n:
                        raise ValueError('optimizer state %r of parameter %d has %d elements, expected %d' % (name, i, src.numel(), n))
                    dst.copy_(src.reshape(-1))
            if st is not None:
                steps = max(steps, int(float(st['step'])) if 'step' in st else 1)
        self.steps = int(sd.get('fused_steps', steps))
        if self.skip_nonfinite:
            self._info[3:4].fill_(self.steps)       # the device's applied-step count goes on from the checkpoint's


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov) over the flat buffers."""

    _state_names = ('momentum_buffer',)
    _shared_keys = ('momentum', 'dampening', 'nesterov')

    def __init__(self, bucket: GradBucket, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, zero_grad: bool = False, param_groups=None,
                 max_grad_norm=None, skip_nonfinite: bool = False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(bucket, dict(lr=float(lr), momentum=float(momentum), dampening=float(dampening),
                                      weight_decay=float(weight_decay), nesterov=bool(nesterov)), zero_grad,
                         param_groups, max_grad_norm, skip_nonfinite)
        self.momentum_buffer = torch.zeros_like(bucket.flat)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib, ops
        b, h = self.bucket, self.hyper
        if len(self.param_groups) == 1 and self._info is None:
            _lib.check(_lib.lib().istvt_sgd_momentum(b.flat_params.data_ptr(), b.flat.data_ptr(), self.momentum_buffer.data_ptr(),
                                                     b.numel, h['lr'], h['momentum'], h['dampening'], h['weight_decay'],
                                                     int(h['nesterov']), int(self.steps == 0), int(self.fused_zero_grad),
                                                     float(b.grad_scale), ops._stream()), 'istvt_sgd_momentum')
        else:
            lrs, wds, count = self._group_args()
            info = self._norm_pass()
            _lib.check(_lib.lib().istvt_sgd_momentum_groups(
                b.flat_params.data_ptr(), b.flat.data_ptr(), self.momentum_buffer.data_ptr(), b.numel,
                self._seg[0].data_ptr(), self._seg[1].data_ptr(), self._seg[0].numel(), lrs, wds, count, h['momentum'],
                h['dampening'], int(h['nesterov']), int(self.steps == 0), int(self.fused_zero_grad), float(b.grad_scale),
                info, int(self.skip_nonfinite), ops._stream()), 'istvt_sgd_momentum_groups')
        self._done()


class FusedAdamW(_FusedOptimizer):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) (amsgrad off) over the flat buffers."""

    _state_names = ('exp_avg', 'exp_avg_sq')
    _shared_keys = ('betas', 'eps')

    def _extra_state(self, steps):
        return {'step': torch.tensor(float(steps))}

    def __init__(self, bucket: GradBucket, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, zero_grad: bool = False, param_groups=None, max_grad_norm=None,
                 skip_nonfinite: bool = False):
        super().__init__(bucket, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                      weight_decay=float(weight_decay)), zero_grad, param_groups, max_grad_norm,
                         skip_nonfinite)
        self.exp_avg = torch.zeros_like(bucket.flat)
        self.exp_avg_sq = torch.zeros_like(bucket.flat)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib, ops
        b, h = self.bucket, self.hyper
        if len(self.param_groups) == 1 and self._info is None:
            _lib.check(_lib.lib().istvt_adamw(b.flat_params.data_ptr(), b.flat.data_ptr(), self.exp_avg.data_ptr(),
                                              self.exp_avg_sq.data_ptr(), b.numel, h['lr'], h['betas'][0], h['betas'][1],
                                              h['eps'], h['weight_decay'], self.steps + 1, int(self.fused_zero_grad),
                                              float(b.grad_scale), ops._stream()), 'istvt_adamw')
        else:
            lrs, wds, count = self._group_args()
            info = self._norm_pass()
            _lib.check(_lib.lib().istvt_adamw_groups(
                b.flat_params.data_ptr(), b.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), b.numel,
                self._seg[0].data_ptr(), self._seg[1].data_ptr(), self._seg[0].numel(), lrs, wds, count, h['betas'][0],
                h['betas'][1], h['eps'], self.steps + 1, int(self.fused_zero_grad), float(b.grad_scale), info,
                int(self.skip_nonfinite), ops._stream()), 'istvt_adamw_groups')
        self._done()


# ------------------------------------------------------------------------------------------------------------------------
# HIP-graph replay of the training forward / backward (round 6)
# ------------------------------------------------------------------------------------------------------------------------
class _ReplayBackward(torch.autograd.Function):
    """Puts a replayed forward graph's output into the caller's autograd graph: its backward copies the incoming gradient
    into the static buffer and replays the captured backward graph (parameter gradients land in the flat bucket, as they
    do when the kernels are launched one by one)."""

    @staticmethod
    def forward(ctx, anchor, entry, token):
        ctx.entry = entry
        ctx.token = token            # alive until this node has run its backward or has been dropped: StepGraphs' "pending" flag
        return entry.static_out.detach().clone()

    @staticmethod
    def backward(ctx, g):
        from . import functional as Fn
        entry, ctx.entry, ctx.token = ctx.entry, None, None
        entry.static_gout.copy_(g)
        # A launch-by-launch backward pass may share this autograd pass (a second forward that fell back): its weight-gradient
        # launches sit on the side stream and read-modify-write the same .grad buffers as the graph's.  Order them: what the
        # side stream has so far, then the graph, then whatever it gets later.  (No-ops in the all-graph loop.)
        cur = torch.cuda.current_stream(g.device)
        side = Fn._overlap['streams'].get(g.device.index)
        if side is not None:
            cur.wait_stream(side)
        entry.g_bwd.replay()
        if side is not None:
            side.wait_stream(cur)
        return None, None, None


class _GraphEntry:
    __slots__ = ('static_x', 'static_out', 'static_gout', 'g_fwd', 'g_bwd', 'keep', 'fingerprint', 'live', 'calls', 'pool')


def env_switches() -> tuple:
    """The switches stem.py and functional.py read from the environment on EVERY call and that select launch sequences,
    each as its reader sees it (so a value that means the default is the default): ISTVT_STEM_MATERIALISE_A2 (stem forward),
    ISTVT_STEM_WGRAD_SIDE and ISTVT_STEM_PW_BWD_FUSED (stem backward), ISTVT_BGRAD_SIDE (functional._bgrad)."""
    env = os.environ.get
    return (env('ISTVT_STEM_MATERIALISE_A2', '0') == '1', env('ISTVT_STEM_WGRAD_SIDE', '1') != '0',
            env('ISTVT_STEM_PW_BWD_FUSED', '1') != '0', env('ISTVT_BGRAD_SIDE', '0') == '1')


_training_of = operator.attrgetter('training')


class ModuleIndex:
    """One walk over a model's module tree, kept: what StepGraphs reads on the host at every call -- the mode flags that
    select launch sequences and the parameters the backward differentiates -- comes from these lists instead of a new
    ``modules()`` / ``named_parameters()`` walk per step.  No device work: it is built and read on a host model as well.

    ``stale()`` says whether the tree has changed since (a submodule replaced, added or removed, a parameter registered or
    deleted); the owner then builds a new index.  A parameter REPLACED in its module, or frozen, needs no new index:
    ``live()`` reads every slot and ``requires_grad`` anew."""

    def __init__(self, model: torch.nn.Module):
        keep = set('xcep.model.' + n for n in _stem.param_names())
        mods, self.slots = [], []                       # slots: (the owner's _parameters dict, leaf name), in model order
        for prefix, mod in model.named_modules():
            mods.append(mod)
            for leaf in mod._parameters:
                name = prefix + '.' + leaf if prefix else leaf
                if name.startswith('xcep.') and name not in keep:       # the never-executed Xception tail
                    continue
                self.slots.append((mod._parameters, leaf))
        self._child_dicts = [mod._modules for mod in mods]
        self._param_dicts = [mod._parameters for mod in mods]
        self._children = self._walk()
        self._param_count = sum(map(len, self._param_dicts))
        # The model itself is held weakly: it owns the StepGraphs that owns this index, and a cycle through it would keep the
        # graphs' memory pools and static-address mode alive until the garbage collector runs (submodules do not point back).
        self._root = weakref.ref(model)
        self.modules = mods[1:]
        self.dropouts = [mod for mod in self.modules if isinstance(mod, torch.nn.Dropout)]
        self.fp8 = [mod for mod in self.modules if hasattr(mod, 'attn_fp8')]
        self.dre = [mod for mod in self.modules if hasattr(mod, 'dead_row_elimination')]

    def _walk(self):
        return list(itertools.chain.from_iterable(map(dict.values, self._child_dicts)))

    def stale(self) -> bool:
        # (list equality compares by identity first; nn.Module defines no __eq__)
        return self._walk() != self._children or sum(map(len, self._param_dicts)) != self._param_count

    def flags(self) -> tuple:
        """every module's train / eval flag, every nn.Dropout's ``p > 0``, every attn_fp8 and dead_row_elimination flag"""
        root = self._root()
        return ((root.training, bool(getattr(root, 'attn_fp8', False)), bool(getattr(root, 'dead_row_elimination', False))),
                tuple(map(_training_of, self.modules)), tuple([d.p > 0 for d in self.dropouts]),
                tuple([bool(q.attn_fp8) for q in self.fp8]), tuple([bool(q.dead_row_elimination) for q in self.dre]))

    def live(self) -> List[torch.nn.Parameter]:
        """the parameters ``live_named_parameters(model)`` names, in its order, from the slots' current contents"""
        out = [p for p in [params[leaf] for params, leaf in self.slots] if p is not None and p.requires_grad]
        if len(set(map(id, out))) != len(out):          # a tied parameter once, as named_parameters() lists it
            seen = set()
            out = [p for p in out if not (id(p) in seen or seen.add(id(p)))]
        return out


class StepGraphs:
    """The launch sequences of ``model(x)`` and of its backward pass, captured once per (input shape, mode) as HIP graphs
    (hipGraph via torch.cuda.CUDAGraph; the kernels are launched through the C ABI on torch's current stream, which is the
    capturing stream inside ``torch.cuda.graph``) and replayed from then on: ~1 400 launches per training step at C2 become
    two graph launches, the per-step host time falls from 14-23 ms of Python to ~3 ms, and a launch-bound configuration (C1,
    small batches) runs at the speed of its kernels.

    Transparent to the caller's loop (train_CNN.py:497-537 runs unchanged): ``model.enable_step_graphs()`` makes
    ``model(x)`` return logits that are part of the caller's autograd graph; ``loss.backward()`` replays the backward graph.
    A forward under ``torch.no_grad()`` (the validation loop, train_CNN.py:837-944) is a forward-only graph of its own.
    Falls back to the launch-by-launch path whenever the preconditions do not hold:
      * a CUDA input that does not require a gradient;
      * with gradients enabled: every live parameter's gradient is a view of a ``GradBucket(fuse_accumulate=True)`` (the
        kernels write the bucket directly; a torch optimizer's ``zero_grad(set_to_none=True)`` breaks that and is detected);
      * no early all-reduce hook (N > 1 with the overlapped schedule stays launch-by-launch: the collective's handle is host state);
      * no per-kernel instrumentation (bench.py's profiled step);
      * the forward draws no dropout seed: an applied ``nn.Dropout`` with ``p > 0`` in train mode takes a Philox key from
        torch's CPU generator at every forward (functional._new_seed), a host value a graph would freeze.  Seen on the
        warm-up forwards (functional.seed_draws); such a key is never captured, ``last_reason`` says so.  The same model in
        eval mode, or with every ``p`` back at 0, is another key and is captured;
      * the previous graphed forward of this entry has had its backward (or was dropped): an entry owns ONE set of saved
        activations.
    Everything else the launch-by-launch path reads on the host at every call is in an entry's KEY (``key()``): the input's
    shape / dtype / device, grad / no_grad, the compute dtype, the train / eval flag of EVERY module (the stem goes by
    ``xcep``'s, each block and transformer module by its own: ``model.xcep.eval()`` for frozen BatchNorm statistics is
    another launch sequence), every ``nn.Dropout``'s ``p > 0``, every ``attn_fp8`` and ``dead_row_elimination`` flag, the
    weight-gradient stream / grouping, the GELU backward form, ISTVT_GEMM_TM and the four environment switches stem.py and
    functional.py read per call (``env_switches()``).  A toggle captures a new entry, it never replays the old one; undoing
    it finds the old entry again.  The flags are read in one pass over a cached module list (``ModuleIndex``); a changed
    module tree (a new head) is noticed at the next call, drops the graphs and rebuilds the list.
    The FINGERPRINT covers what an entry's graphs hold by address: the set of differentiated parameters -- recomputed at every
    call, so ``requires_grad_()`` after a capture and a parameter swapped in are seen --, the identity and ``data_ptr`` of each and
    of its gradient view.  A change (a new bucket, staged unfreezing) drops the graphs and captures again.  Every cached
    operand copy is refreshed in place (the static-address mode of weights.py).  The first ``warmup`` calls of an entry (at
    least one) run launch by launch (they fill the operand caches, the statistics arena, the side stream, the kernels'
    one-time attribute calls).  Every entry has a memory pool of its own: replaying one never touches what another saved
    for its backward."""

    def __init__(self, model: torch.nn.Module, forward_eager, warmup: int = 2, max_entries: int = 4):
        self.model = weakref.ref(model)
        # (a bound method of the model would make model -> StepGraphs -> model a cycle only the garbage collector breaks:
        #  the graphs' memory pools, and static-address mode, would outlive the model for as long as that takes)
        self._fwd = weakref.WeakMethod(forward_eager) if hasattr(forward_eager, '__self__') else (lambda f=forward_eager: f)
        # at least one launch-by-launch forward per key: it shows whether the configuration draws dropout seeds on the host
        self.warmup = max(int(warmup), 1)
        self.max_entries = int(max_entries)
        self.entries = {}
        self.seen = {}
        self.nocapture = {}             # entry key -> why this configuration is never captured (its forward draws seeds)
        self.pending = {}               # entry key -> weakref to the token of a graphed forward whose backward has not run
        self.anchor = None
        self.live = None                # the differentiated parameters as of the last call
        self._tree = None               # ModuleIndex of the model, rebuilt when the module tree changes
        self.stats = {'captures': 0, 'replays': 0, 'eager': 0, 'recaptures': 0}
        self.last_reason = None
        from . import ops
        ops._static_holders.add(self)   # static-address mode is on exactly while some StepGraphs holds a captured graph

    def forward_eager(self, x):
        return self._fwd()(x)

    def note_eager(self, reason: str):
        """a call the model runs launch by launch without asking (an input kind no graph is captured for)"""
        self.last_reason = reason
        self.stats['eager'] += 1

    # -- host side: the entry key, the live set, the fingerprint (no device work; they run on a host model too) ---------
    def index(self) -> ModuleIndex:
        """the model's ModuleIndex; a changed module tree (a swapped head) drops every graph and every warm-up count --
        they belong to another model -- and builds a new one"""
        idx = self._tree
        if idx is None or idx.stale():
            if idx is not None:
                if self.entries:
                    self.stats['recaptures'] += 1
                self.drop()
            idx = self._tree = ModuleIndex(self.model())
        return idx

    def _config(self, m):
        from . import functional as Fn
        if m is None:
            return None
        return (str(getattr(m, 'compute_dtype', None)), self.index().flags(), env_switches(), bool(Fn._overlap['on']),
                int(Fn._overlap['group']), bool(Fn.GELU_SAVE_DERIV[0]), os.environ.get('ISTVT_GEMM_TM', ''))

    def key(self, x, grads: bool):
        """The key of the entry ``model(x)`` belongs to.  It names everything that selects a launch sequence: the input,
        grad / no_grad, the compute dtype, EVERY module's train / eval flag (the stem and each block branch on their own),
        every nn.Dropout's ``p > 0``, every attn_fp8 and dead_row_elimination flag, the weight-gradient stream / grouping and
        the environment switches read per call.  A toggle after a capture is another key, never a replay of the old sequence;
        undoing it finds the old entry again."""
        m = self.model()
        return (tuple(x.shape), x.dtype, x.device.index, self._config(m), bool(m is not None and m.training), bool(grads))

    def live_parameters(self):
        """the parameters the backward differentiates NOW: read at every call (requires_grad_() after a capture, a parameter
        or submodule swapped in), in the order of live_named_parameters()"""
        self.live = self.index().live()
        return self.live

    def _live(self):
        return self.live if self.live is not None else self.live_parameters()

    def _fingerprint(self, grads: bool, live=None):
        """identity and address of every live parameter (and, with gradients, the address of its fused gradient view); None
        when a live gradient is not a view of a fused bucket.  An entry keeps its parameters alive, so an identity in its
        fingerprint cannot come back as another tensor's."""
        fp = []
        for p in (self._live() if live is None else live):
            fp.append(id(p))
            fp.append(p.data_ptr())
            if grads:
                g = p.grad
                if g is None or not getattr(p, '_istvt_fused_grad', False):
                    return None
                fp.append(g.data_ptr())
        return tuple(fp)

    def why_not(self, x, key):
        from . import functional as Fn
        from . import ops
        if self.model() is None:
            return 'model gone'
        if not x.is_cuda or x.requires_grad:
            return 'input on the host or requiring a gradient'
        if ops.kernel_profile is not None or ops.gemm_profile is not None:
            return 'per-kernel instrumentation on'
        if torch.cuda.is_current_stream_capturing():
            return 'already inside a capture'
        if key[-1]:                     # gradients enabled
            if Fn.grad_ready_hooks:
                return 'early all-reduce hook registered'
            pend = self.pending.get(key)
            if pend is not None and pend() is not None:
                return 'a graphed forward is still waiting for its backward'
        return None

    # -- the call ----------------------------------------------------------------------------------------------------
    def __call__(self, x):
        from . import functional as Fn
        from . import ops
        grads = torch.is_grad_enabled()
        key = self.key(x, grads)
        reason = self.why_not(x, key)
        fp = live = None
        if reason is None:
            live = self.live_parameters()
            fp = self._fingerprint(grads, live)
            if fp is None:
                reason = 'a live gradient is not a fused-bucket view'
        if reason is None:
            reason = self.nocapture.get(key)
        warming = False
        if reason is None:
            n = self.seen.get(key, 0)
            self.seen[key] = n + 1
            if n < self.warmup:
                reason, warming = 'warm-up', True
            elif key not in self.entries and len(self.entries) >= self.max_entries:
                reason = 'more (shape, mode) entries than max_entries'
        if reason is not None:
            self.last_reason = reason
            self.stats['eager'] += 1
            if not warming:
                return self.forward_eager(x)
            # A forward that draws a dropout seed (functional._new_seed: a host integer from torch's CPU generator, handed to
            # the kernel by value) would replay the masks of its capture for ever.  The warm-up forwards run launch by launch
            # anyway: if the draw counter moves across one, this key is never captured.  Nothing is captured and thrown away,
            # and the generator sees exactly the draws of the launch-by-launch loop.
            draws = Fn.seed_draws[0]
            out = self.forward_eager(x)
            if Fn.seed_draws[0] != draws:
                self.nocapture[key] = self.last_reason = \
                    'dropout is active: its seeds are drawn on the host at every forward (not captured)'
            return out
        ent = self.entries.get(key)
        if ent is not None and ent.fingerprint != fp:
            # a parameter or gradient moved (a new bucket, load_state_dict into new storage, .to()), or the set of
            # differentiated parameters changed (requires_grad_(), a parameter swapped in): the captured pointers are dead,
            # or the captured backward differentiates the wrong set -- drop every graph and start over
            self.drop()
            self.stats['recaptures'] += 1
            ent = None
        if ent is None:
            ent = self._capture(x, key, fp, grads, live)
        # operand copies the optimizer step (or a load_state_dict) made stale: in place, before the graph reads them
        ops.refresh_stale_operands()
        if ent.static_x.data_ptr() != x.data_ptr():
            ent.static_x.copy_(x)
        ent.g_fwd.replay()
        ent.calls += 1
        self.stats['replays'] += 1
        if not grads:
            return ent.static_out.detach().clone()

        class _Token:
            __slots__ = ('__weakref__',)
        token = _Token()
        self.pending[key] = weakref.ref(token)
        return _ReplayBackward.apply(self.anchor, ent, token)

    def _capture(self, x, key, fp, grads, live):
        from . import functional as Fn
        from . import ops
        from . import stem as stem_mod
        from . import weights
        Fn.flush_stale_joins()
        if self.anchor is None or self.anchor.device != x.device:
            self.anchor = torch.zeros((), device=x.device, requires_grad=True)
        ent = _GraphEntry()
        ent.calls = 0
        ent.fingerprint = fp
        ent.live = live                 # the captured backward differentiates these; alive as long as the entry is
        ent.static_x = x.detach().clone()
        ent.static_gout = ent.g_bwd = None
        self.entries[key] = ent         # from here on ops.static_addresses() is true: every refresh is in place
        ops.refresh_stale_operands()
        ent.pool = torch.cuda.graph_pool_handle()
        ent.g_fwd = torch.cuda.CUDAGraph()
        # The statistics arena of the launch-by-launch path (stem._arena: one buffer, zeroed once per forward, the backward's
        # accumulators cut from it behind the forward's) must not be shared with a graph: a launch-by-launch forward between
        # this entry's forward and backward would zero and re-cut what the captured backward accumulates into.  The capture
        # starts from an empty arena: the captured forward then allocates one of its own from the graph's pool.
        arena_saved = dict(stem_mod._arena)
        stem_mod._arena.update(buf=None, off=0, need=max(arena_saved['need'], arena_saved['off']))
        try:
            self._capture_graphs(ent, grads)
        except BaseException:
            self.entries.pop(key, None)
            raise
        finally:
            arena_private = stem_mod._arena.get('buf')
            stem_mod._arena.clear()
            stem_mod._arena.update(arena_saved)
        # everything outside the graphs' pool whose ADDRESS they captured stays alive with them
        ent.keep = weights.cache.tensors() + [arena_private]
        self.entries[key] = ent
        self.stats['captures'] += 1
        return ent

    def _capture_graphs(self, ent, grads):
        with torch.set_grad_enabled(grads):
            with torch.cuda.graph(ent.g_fwd, pool=ent.pool, capture_error_mode='thread_local'):
                out = self.forward_eager(ent.static_x)
            ent.static_out = out
            if grads:
                ent.static_gout = torch.zeros_like(out)
                ent.g_bwd = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ent.g_bwd, pool=ent.pool, capture_error_mode='thread_local'):
                    # autograd.grad, not backward(): no AccumulateGrad node runs (those of the warm-up steps live on the
                    # default stream, and the engine's stream hand-over to them is illegal inside a capture -- it crashed
                    # the process); the kernels write the fused bucket themselves and the Functions return None for their
                    # parameters
                    got = torch.autograd.grad(out, ent.live, grad_outputs=ent.static_gout, allow_unused=True)
                    # a Function that does hand a gradient tensor back is accumulated here, inside the capture, as
                    # AccumulateGrad would have done
                    for p, g in zip(ent.live, got):
                        if g is not None:
                            p.grad.add_(g)
                del got

    def drop(self):
        """forget every captured graph (each entry's pool is released once the last reference is gone)"""
        self.entries.clear()
        self.seen.clear()
        self.nocapture.clear()
        self.pending.clear()
        self.live = None
