"""Everything derived from a parameter: the compute-dtype GEMM operand, its transpose for the input-gradient GEMM, the
stacked [w_0; w_1; ...] operand, the layouts the stem builds with a few torch ops.

One cache (WeightCache), one entry type (Entry), one dict.  What makes "forward A -> optimizer step -> forward B ->
backward A", the fused optimizers (which write parameters through raw pointers) and parallel.StepGraphs (which captures
addresses) correct is decided here and nowhere else:

  * fresh:    an entry is valid while the version counters of its parameters, and the epoch of the raw-pointer writers
              (invalidate_weight_cache), are what they were when it was made;
  * in place: refresh_stale_operands() rewrites a stale (operand, transpose) pair into its own buffers only if nothing but
              the cache holds them (WeightCache.held); otherwise the pair is dropped and stays intact for whoever holds it.
              Derived layouts are re-made as fresh tensors;
  * address:  in static-address mode (captured HIP graphs hold raw pointers) every kind is rewritten into the buffer it
              already lives in, always, and nothing is re-made at a new address;
  * death:    when a parameter dies its copies are released at once (weakref callback -> WeightCache.drop).

The live cache is `cache`; ops re-exports its methods under the names the rest of the package uses.
"""
from __future__ import annotations

import sys
import weakref

import torch

from . import _lib
from ._common import G256_MIN, Tensor, _c, _DT, _stream, cast, dtype_code, empty_rows, pad_ld

_wepoch = [0]          # bumped by writers that modify parameters behind autograd's back (parallel.FusedSGD / FusedAdamW)


def invalidate_weight_cache():
    """A kernel wrote parameters through raw pointers (no ``_version`` bump): every cached copy is stale."""
    _wepoch[0] += 1


def _versions(ws) -> tuple:
    return tuple(w._version for w in ws) + (_wepoch[0],)


# Static-address mode (parallel.StepGraphs: the forward / backward launch sequences captured as HIP graphs hold raw
# pointers): every cached copy derived from a parameter -- bf16 operand pairs, plain casts, stacked operands, derived
# layouts -- is then refreshed IN PLACE, always, by refresh_stale_operands(); nothing is ever re-made at a new address.
# The price is the guarantee the eager mode gives a live autograd graph (its saved operand copies stay intact when the
# parameter changes before backward): with graphs on, parameters must not be modified between a forward and its backward
# -- which the graphs' own static activations forbid anyway.
_static = [False]
_static_holders = weakref.WeakSet()     # parallel.StepGraphs objects: the mode is on while any of them holds a captured graph


def set_static_addresses(on: bool) -> bool:
    """explicit switch (beside the automatic one: on while a parallel.StepGraphs holds captured graphs)"""
    prev = _static[0]
    _static[0] = bool(on)
    return prev


def static_addresses() -> bool:
    return _static[0] or any(h.entries for h in _static_holders)


def _holders(t: Tensor) -> tuple:
    """(Python references, C++ references to the TensorImpl -- autograd SavedVariables --, tensors sharing the storage --
    views and slices) of `t`, each including what THIS call adds.  Only differences between two calls made the same way
    mean anything: WeightCache._pair_holders() is the one place that calls it.  AttributeError where this torch build
    lacks the private introspection (Tensor._use_count, torch._C._storage_Use_Count)."""
    return (sys.getrefcount(t), t._use_count(), torch._C._storage_Use_Count(t.untyped_storage()._cdata))


class Entry:
    """One cached copy of one parameter (or one stack of parameters).
    kind     'plain' (cast), 'padded' (cast with line-aligned rows), 'cat' (stacked operand), 'derived' (builder(w)), or
             'loose' (the transpose of a tensor that is not a cached operand: `refs` is that tensor, `out` is None)
    refs     weakrefs to the sources; the death of any of them drops the entry
    version  _versions(sources) when `out` was last written
    out      the copy;  wt: its transpose (made by the fused pass, or lazily by _transposed_operand), or None
    grouped  out / wt came from the fused cast + transpose pass: refresh_stale_operands() re-casts the pair in its one
             grouped launch
    builder  derived layouts only"""
    __slots__ = ('kind', 'refs', 'version', 'out', 'wt', 'grouped', 'builder')


COPIES = ('plain', 'padded', 'cat')


class WeightCache:
    _idle: dict = {}            # view? -> holder counts of a pair only a cache holds (a property of Entry, not of an instance)
    _introspection_warned = False

    def __init__(self):
        self.entries = {}       # (kind, id of the source | tuple of ids of the stacked sources | derived()'s key) -> Entry
        self.by_out = {}        # id(entry.out) -> Entry: _transposed_operand() is handed the operand, not the parameter

    # -- the two places that change what the cache holds -------------------------------------------------------------------
    def insert(self, key, ws, version, out, wt=None, grouped=False, builder=None) -> Entry:
        self.drop(key)
        e = Entry()
        e.kind = key[0]
        # (the parameter's death drops the copies at once, not at the next refresh_stale_operands())
        e.refs = tuple(weakref.ref(w, lambda _r, k=key, c=self: c.drop(k)) for w in ws)
        e.version, e.out, e.wt, e.grouped, e.builder = version, out, wt, grouped, builder
        self.entries[key] = e
        if out is not None:
            self.by_out[id(out)] = e
        return e

    def drop(self, key):
        """a source died, a live graph holds the copies, or the entry is being replaced: the cache lets go of it (the tensors
        live on with whoever else holds them)"""
        e = self.entries.pop(key, None)
        if e is not None and self.by_out.get(id(e.out)) is e:
            del self.by_out[id(e.out)]

    # -- read-only inspection (parallel.StepGraphs, the tests, tools/refresh_probe.py) ----------------------------------
    @staticmethod
    def key(kind, source):
        """source: the parameter ('plain' / 'padded'), the tuple of parameters ('cat'), the tensor ('loose'), or the key
        given to derived()"""
        if kind != 'derived':
            source = tuple(id(w) for w in source) if isinstance(source, tuple) else id(source)
        return (kind, source)

    def entry(self, kind, source):
        return self.entries.get(self.key(kind, source))

    def grouped_count(self) -> int:
        return sum(1 for e in self.entries.values() if e.grouped)

    def tensors(self) -> list:
        """every tensor the cache currently holds"""
        return [t for e in self.entries.values() for t in (e.out, e.wt) if t is not None]

    # -- who else holds an (operand, transpose) pair -----------------------------------------------------------------------
    @staticmethod
    def _pair_holders(e) -> tuple:
        return _holders(e.out) + _holders(e.wt)

    @classmethod
    def _idle_holders(cls, view: bool) -> tuple:
        """what _pair_holders() returns for a pair that NOTHING but a cache holds: measured, not assumed -- a throw-away pair
        is put through insert() on a private cache and through the same call (so another Python version's reference
        accounting, or a change of Entry, moves the baseline and the check together)."""
        if view not in cls._idle:
            mk = (lambda: torch.empty((2, 16))[:, :8]) if view else (lambda: torch.empty((2, 8)))
            # Under the mode real operands are made in (a normal forward): the first stale refresh runs inside the optimizer
            # step, possibly under torch.inference_mode() / no_grad, where a slice carries no ._base and its storage has one
            # holder fewer -- a baseline taken there made every later refresh look "held" and silently fell back to 84 lazy
            # casts per step.
            with torch.inference_mode(False), torch.enable_grad():
                out, wt = mk(), mk()
            if (out._base is not None) != bool(view) or (wt._base is not None) != bool(view):
                raise RuntimeError('istvt_amd.weights: calibration operand is %sa view (expected view=%r)'
                                   % ('' if out._base is not None else 'not ', view))
            private = cls()
            e = private.insert(('padded', 0), (), None, out, wt, grouped=True)
            del out, wt
            cls._idle[view] = cls._pair_holders(e)
        return cls._idle[view]

    def held(self, e) -> bool:
        """whether anything but this cache holds e.out or e.wt.  Holders are counted three ways (_holders: Python references,
        C++ references such as SavedVariable, tensors sharing the storage such as views / slices) and compared with the
        counts of a pair that only a cache holds (_idle_holders)."""
        try:
            idle = self._idle_holders(e.out._base is not None)[:3] + self._idle_holders(e.wt._base is not None)[3:]
            return any(a > b for a, b in zip(self._pair_holders(e), idle))
        except AttributeError:
            # no introspection in this torch build: "held by somebody", so that no operand is ever rewritten in place (it is
            # re-made instead: correct, one launch per weight slower)
            if not WeightCache._introspection_warned:
                WeightCache._introspection_warned = True
                import warnings
                warnings.warn('istvt_amd.weights: torch lacks the reference-count introspection used to refresh bf16 operand '
                              'copies in place; falling back to re-making them (slower, still correct)')
            return True

    # -- the copies ------------------------------------------------------------------------------------------------------------
    def weight_as(self, w: Tensor, dtype: torch.dtype, pad: bool = False) -> Tensor:
        """2-D view of a (fp32) parameter in the compute dtype; bf16 copies are cached until the parameter is modified
        in place (optimizer step bumps ``_version``).  pad=True: the copy has line-aligned rows (a [N, K] view of a
        [N, pad_ld(K)] buffer), the layout the DMA-staged GEMMs want for their B operand."""
        w2 = w.detach()
        if w2.dim() != 2:
            w2 = w2.reshape(w2.shape[0], -1)
        if w2.dtype == dtype:
            return _c(w2)
        pad = pad and w2.shape[1] % 8 == 0 and pad_ld(w2.shape[1]) != w2.shape[1]
        key = ('padded' if pad else 'plain', id(w))     # id-keyed: Tensor.__eq__ is elementwise, so tensors cannot be dict keys
        e = self.entries.get(key)
        if e is not None and e.refs[0]() is w and e.version == _versions((w,)) and e.out.dtype == dtype:
            return e.out
        wt = None
        if pad:
            w2 = _c(w2)
            R, C = w2.shape
            out = empty_rows(R, C, dtype, w2.device)
            if w2.dtype == torch.float32 and dtype == torch.bfloat16 and R % 8 == 0 and R >= G256_MIN and C >= G256_MIN:
                # the operand of the input-gradient GEMM (W^T, k-contiguous) comes out of the same pass over the fp32 weight
                wt = empty_rows(C, R, dtype, w2.device)
                _lib.check(_lib.lib().istvt_cast_transpose(w2.data_ptr(), C, out.data_ptr(), out.stride(0), wt.data_ptr(),
                                                           wt.stride(0), R, C, _stream()), 'istvt_cast_transpose')
            else:
                _lib.check(_lib.lib().istvt_cast2d(w2.data_ptr(), dtype_code(w2), C, out.data_ptr(), _DT[dtype],
                                                   out.stride(0), R, C, _stream()), 'istvt_cast2d')
        else:
            out = cast(w2, dtype)
        self.insert(key, (w,), _versions((w,)), out, wt, grouped=wt is not None)
        return out

    def weight_cat_as(self, ws, dtype: torch.dtype) -> Tensor:
        """[w_0; w_1; ...] stacked along the output dimension as ONE line-aligned GEMM operand in the compute dtype: the
        parameters stay separate (state dict, optimizer), the operand copy is cached until one of them is modified.
        TemporalResidualAttention's [to_qk | to_v] (module.py:182-183): one 728 -> 1536 GEMM instead of two.  For bf16 the
        operand of the input-gradient GEMM ([K, sum N_i], k-contiguous W^T) comes out of the same passes over the fp32
        weights."""
        ws = tuple(ws)
        key = ('cat', tuple(id(w) for w in ws))
        ver = _versions(ws)
        e = self.entries.get(key)
        if e is not None and all(r() is w for r, w in zip(e.refs, ws)) and e.version == ver and e.out.dtype == dtype:
            return e.out
        K = ws[0].shape[1]
        if any(w.dim() != 2 or w.shape[1] != K for w in ws):
            raise RuntimeError('weight_cat_as: the weights must be 2-D with one input width')
        R = sum(w.shape[0] for w in ws)
        dev = ws[0].device
        out = empty_rows(R, K, dtype, dev, K % 8 == 0)
        fused_t = (dtype == torch.bfloat16 and all(w.dtype == torch.float32 and w.shape[0] % 8 == 0 and w.shape[0] >= G256_MIN
                                                    for w in ws) and K >= G256_MIN and K % 8 == 0)
        wt = empty_rows(K, R, dtype, dev) if fused_t else None
        r0 = 0
        for w in ws:
            w2 = _c(w.detach())
            n = w2.shape[0]
            if fused_t:
                es = out.element_size()
                _lib.check(_lib.lib().istvt_cast_transpose(w2.data_ptr(), K, out.data_ptr() + r0 * out.stride(0) * es, out.stride(0),
                                                           wt.data_ptr() + r0 * es, wt.stride(0), n, K, _stream()),
                           'istvt_cast_transpose')
            else:
                out[r0:r0 + n].copy_(w2)
            r0 += n
        self.insert(key, ws, ver, out, wt, grouped=fused_t)
        return out

    def derived(self, key, w: Tensor, builder):
        """builder(w) -> Tensor, cached until `w` changes (its version counter, or a raw-pointer writer's epoch).  Layouts that
        are built with a few torch ops (the stem's tap-major depthwise weights, conv1 / conv2 in GEMM form): rebuilt, like
        the operand copies, by refresh_stale_operands(), i.e. right behind the optimizer step when a fused optimizer drives
        the loop, instead of at the head of the next forward pass (where a loop that syncs every step has the GPU waiting
        for the host)."""
        e = self.entries.get(('derived', key))
        ver = _versions((w,))
        if e is not None and e.refs[0]() is w and e.version == ver:
            return e.out
        return self.insert(('derived', key), (w,), ver, builder(w), builder=builder).out

    def _transposed_operand(self, w: Tensor) -> Tensor:
        """w^T of an already-cast GEMM operand.  Of a cached copy: kept in (and refreshed with) that copy's entry.  Of any
        other tensor: cached for as long as that tensor lives."""
        e = self.by_out.get(id(w))
        if e is None or e.out is not w:
            e = self.entries.get(('loose', id(w)))
            if e is None or e.refs[0]() is not w:
                e = self.insert(('loose', id(w)), (w,), None, None)
        if e.wt is None:
            wt = empty_rows(w.shape[1], w.shape[0], w.dtype, w.device)        # line-aligned rows for the DMA-staged GEMM
            wt.copy_(w.t())
            e.wt = wt
        return e.wt

    # -- refresh ---------------------------------------------------------------------------------------------------------------
    def _refresh_derived(self) -> int:
        n = 0
        for key, e in list(self.entries.items()):
            if e.kind != 'derived':
                continue
            w = e.refs[0]()
            if w is None:
                self.drop(key)
            elif e.version != _versions((w,)):
                if static_addresses():
                    # captured HIP graphs hold the ADDRESS of the layout (parallel.StepGraphs): rebuilt in place
                    e.out.copy_(e.builder(w))
                    e.version = _versions((w,))
                else:
                    # a FRESH tensor (never in place): whatever a live autograd graph still holds of the old layout stays intact
                    self.insert(key, (w,), _versions((w,)), e.builder(w), builder=e.builder)
                n += 1
        return n

    def _refresh_plain_copies(self) -> int:
        """static-address mode: the cached copies that are NOT (operand, transpose) pairs of the grouped refresh -- plain casts
        (weight_as without padding or of a narrow weight), padded casts without a fused transpose, stacked operands without
        one, each with its lazily made transpose (_transposed_operand) if it has one -- re-made into the buffers they already
        live in.  A handful per model (the head's Linear, narrow 1x1 convolutions)."""
        n = 0
        for e in list(self.entries.values()):
            if e.grouped or e.kind not in COPIES:
                continue                                    # pairs: the grouped refresh
            ws = [r() for r in e.refs]
            if any(w is None for w in ws) or _versions(ws) == e.version:
                continue
            r0 = 0
            for w in ws:
                w2 = w.detach()
                if w2.dim() != 2:
                    w2 = w2.reshape(w2.shape[0], -1)
                e.out[r0:r0 + w2.shape[0]].copy_(w2)        # casts on the way; `out` may be a row-padded view
                r0 += w2.shape[0]
            if e.wt is not None:
                e.wt.copy_(e.out.t())
            e.version = _versions(ws)
            n += 1
        return n

    def refresh_stale_operands(self) -> int:
        """Re-cast, in one grouped launch (istvt_cast_transpose_group), the bf16 operand copies (W and W^T) of every weight
        that changed since they were made -- i.e. of all of them after an optimizer step.  The models call this at the start
        of a forward pass; without it the same work happens lazily, one launch per weight (84 per step at depth 12, each far
        shorter than the ~5 us a launch occupies the queue for).  Returns the number of weights re-cast."""
        import ctypes as C
        self._refresh_derived()
        static = static_addresses()
        if static:
            self._refresh_plain_copies()
        todo = []
        for key, e in list(self.entries.items()):
            if not e.grouped:
                continue
            ws = [r() for r in e.refs]
            if any(w is None for w in ws):
                self.drop(key)
                continue
            ver = _versions(ws)
            if e.version != ver:
                # Rewritten IN PLACE only when nothing but the cache holds the operand or its transpose.  A live autograd graph
                # that saved them (ctx attributes or save_for_backward of RepChainFn / StemFn / LinearFn: forward A ->
                # optimizer step -> forward B -> backward A) must still find forward A's weights: those copies are left alone
                # -- dropped from the cache, so the next use makes fresh ones -- and die with the graph.
                if not static and self.held(e):
                    self.drop(key)
                    continue
                todo.append((e, ws, ver))
        if not todo:
            return 0
        srcs, ins, ldi, outs, ldo, outts, ldt, Rs, Cs = [], [], [], [], [], [], [], [], []
        for e, ws, ver in todo:
            out, wt = e.out, e.wt
            es, r0 = out.element_size(), 0
            for w in ws:
                w2 = _c(w.detach().reshape(w.shape[0], -1))
                srcs.append(w2)                       # kept alive until the launch is enqueued
                n, K = w2.shape
                ins.append(w2.data_ptr()); ldi.append(K)
                outs.append(out.data_ptr() + r0 * out.stride(0) * es); ldo.append(out.stride(0))
                outts.append(wt.data_ptr() + r0 * es); ldt.append(wt.stride(0))
                Rs.append(n); Cs.append(K)
                r0 += n
        n = len(ins)
        PA, LA, IA = C.c_void_p * n, C.c_long * n, C.c_int * n
        _lib.check(_lib.lib().istvt_cast_transpose_group(n, PA(*ins), LA(*ldi), PA(*outs), LA(*ldo), PA(*outts), LA(*ldt),
                                                         IA(*Rs), IA(*Cs), _stream()), 'istvt_cast_transpose_group')
        for e, ws, ver in todo:
            e.version = ver
        return n


cache = WeightCache()       # the live one
weight_as = cache.weight_as
weight_cat_as = cache.weight_cat_as
derived = cache.derived
refresh_stale_operands = cache.refresh_stale_operands
_transposed_operand = cache._transposed_operand
_refresh_derived = cache._refresh_derived
_refresh_plain_copies = cache._refresh_plain_copies
