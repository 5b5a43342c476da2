"""Guard bands for the kernel checks: where does a kernel WRITE?

Inside ``with guarded() as calls:`` every tensor that ``torch.empty``, ``torch.empty_like``, ``torch.zeros`` or
``torch.zeros_like`` hands out on the chosen device (so also ops.empty_rows / zeros_rows / _same_rows) is a slice of a
larger flat buffer ``[head guard | body | tail guard]`` that this module owns.  Guards, and the body of an ``empty``
allocation, hold a fixed bit pattern per dtype (a NaN with a recognisable payload for the float types, so a kernel that
reads a guard poisons its result).  At exit the device is synchronised and every allocation is verified:

1. guards     head and tail are bit-identical to the sentinel;
2. rectangle  (``empty``, >= 2 dimensions) the elements that no longer hold the sentinel are all rows x columns [0, D) of
              the last dimension for ONE D: a pad column written in some rows, or an element inside the live rectangle
              left unwritten, breaks that -- without knowing D;
3. expect(t)  t is a declared output: the live elements of its allocation are exactly the elements of the view(s) declared
              (catches pad columns filled in ALL rows, which rule 2 takes for a wider rectangle);
4. place(t)   t is an input, copied into a guarded buffer (with pad=True behind sentinel pad columns): body, pads and
              guards must come back bit-identical -- no kernel uses an input as scratch;
5. calls      ``istvt_amd._lib._lib`` is a thin proxy for the duration; the set that guarded() yields holds the names of
              the istvt_* entry points that were called.

What this cannot see: a READ past an allocation that never reaches a result; a stray write further away than one guard
(256 rows / 4 KiB); a write of the sentinel's own bits; and, in uint8 / integer planes, a legitimate value equal to the
sentinel (0xA5) reads as unwritten.
"""
import contextlib
import os
import sys

import torch

GUARD_BYTES = 4096      # the least a guard holds
GUARD_ROWS = 256        # ... and, from two dimensions on, this many rows: the largest tile edge in csrc (T256)
ALIGN = 256             # every guard is a multiple of this many bytes: the body keeps the raw allocation's alignment

# dtype -> (integer view dtype, sentinel as that integer)
SENTINEL = {
    torch.float32: (torch.int32, 0x7FA5A5A5),
    torch.bfloat16: (torch.int16, 0x7FA5),
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
    torch.uint8: (torch.uint8, 0xA5),
    torch.int32: (torch.int32, 0x5AA5A5A5),
    torch.int64: (torch.int64, 0x5AA5A5A5A5A5A5A5),
}

# ---- waivers -------------------------------------------------------------------------------------------
# RECTANGLE_WAIVERS: `empty` allocations that are legitimately written in part; keyed by the allocating site
# ('file.py:function'); rule 1 (guards) still holds for them.
RECTANGLE_WAIVERS = {
    'stem.py:__init__': 'BNState pack [4][C]: filled row by row by the host (a check sets only the rows its kernel reads)',
    'gpu_checks.py:conv_dense_check': 'conv1 / conv2 weight-gradient slab workspaces allocated by the check: a 33^2 or 77^2 '
                                      'input has fewer chunks than the library has slabs (declared outputs of that check are '
                                      'held to rule 3 all the same)',
    'ops.py:_conv1_wgrad_ws': 'the same conv1 slab workspace, allocated by the wrapper',
    'frames.py:_u8_out': 'byte images: every value is legitimate, so a pixel equal to the uint8 sentinel reads as unwritten',
    'ops.py:relevance_overlay_u8': 'byte image (see frames.py:_u8_out)',
}
# (No kernel writes pad columns on purpose, so there is no table of pad-write waivers: the invariant in _common.py holds.)
# INPLACE_WAIVERS: placed inputs that a kernel overwrites as documented behaviour: place(t, inplace=<key>); the guards
# of such a buffer are still verified.
INPLACE_WAIVERS = {
    'optimizer.param': 'fused optimizers update the flat parameter vector in place',
    'optimizer.grad': 'fused optimizers may zero the gradient in place (zero_grad flag)',
    'optimizer.state': 'momentum / moment buffers are updated in place',
    'accumulator': 'gradient / statistics accumulators: kernels add onto what the buffer holds',
    'output.prefilled': 'an output buffer the check pre-fills and the kernel overwrites (out= forms, raw C ABI calls)',
}


class GuardViolation(AssertionError):
    def __init__(self, kind, index, row, col, message):
        super().__init__(message)
        self.kind, self.index, self.row, self.col = kind, index, row, col


class _Record:
    __slots__ = ('flat', 'ints', 'ge', 'n', 'shape', 'dtype', 'kind', 'site', 'views', 'snap', 'live_cols', 'inplace')

    def body_ints(self):
        return self.ints[self.ge:self.ge + self.n]


class _LibProxy:
    """calls go to the real ctypes handle; the names of the istvt_* entry points called are remembered"""

    def __init__(self, real, names):
        object.__setattr__(self, '_real', real)
        object.__setattr__(self, '_names', names)

    def __getattr__(self, name):
        fn = getattr(object.__getattribute__(self, '_real'), name)
        if not name.startswith('istvt_'):
            return fn
        names = object.__getattribute__(self, '_names')

        def call(*args):
            names.add(name)
            return fn(*args)
        return call


_ACTIVE = None
_HERE = os.path.abspath(__file__)


def _site():
    f = sys._getframe(2)
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.abspath(fn) != _HERE and os.sep + 'torch' + os.sep not in fn and 'contextlib' not in fn:
            return '%s:%s' % (os.path.basename(fn), f.f_code.co_name)
        f = f.f_back
    return '?'


def guard_elems(shape, dtype):
    """elements in each guard of an allocation of this shape: max(4096 bytes, 256 rows) rounded up to 256 bytes"""
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = GUARD_BYTES
    if len(shape) >= 2:
        nbytes = max(nbytes, GUARD_ROWS * shape[-1] * es)
    nbytes = -(-nbytes // ALIGN) * ALIGN
    return nbytes // es


class Guard:
    def __init__(self, device='cuda'):
        self.devtype = torch.device(device).type
        self.records = []
        self.by_storage = {}
        self.calls = set()
        self._orig = {}

    # -------------------------------------------------------------------------------- allocation
    def _wants(self, device, dtype):
        if dtype is None:
            dtype = torch.get_default_dtype()
        if dtype not in SENTINEL:
            return None
        devtype = 'cpu' if device is None else torch.device(device).type
        return dtype if devtype == self.devtype else None

    def _alloc(self, shape, dtype, device, kind, site):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        ge = guard_elems(shape, dtype)
        itype, sent = SENTINEL[dtype]
        r = _Record()
        r.flat = self._orig['empty']((ge + n + ge,), dtype=dtype, device=device)
        r.ints = r.flat.view(itype)
        r.ints.fill_(sent)
        r.ge, r.n, r.shape, r.dtype, r.kind, r.site = ge, n, shape, dtype, kind, site
        r.views, r.snap, r.live_cols, r.inplace = [], None, None, None
        body = r.flat[ge:ge + n].view(shape)
        if kind == 'zeros':
            body.zero_()
        self.records.append(r)
        self.by_storage[r.flat.untyped_storage().data_ptr()] = r
        return body, r

    @staticmethod
    def _shape_of(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        if not args or not all(isinstance(a, int) and not isinstance(a, bool) for a in args):
            return None
        return tuple(args)

    def _new(self, kind):
        orig = self._orig[kind]

        def fn(*args, **kw):
            shape = self._shape_of(args)
            extra = set(kw) - {'dtype', 'device', 'requires_grad'}
            if shape is None or extra or kw.get('requires_grad') or 0 in shape or len(shape) == 0:
                return orig(*args, **kw)
            dtype = self._wants(kw.get('device'), kw.get('dtype'))
            if dtype is None:
                return orig(*args, **kw)
            return self._alloc(shape, dtype, kw.get('device'), kind, _site())[0]
        fn.__wrapped__ = orig
        return fn

    def _new_like(self, kind):
        orig = self._orig[kind + '_like']

        def fn(t, *args, **kw):
            extra = set(kw) - {'dtype', 'device'}
            if args or extra or not torch.is_tensor(t) or t.numel() == 0 or t.dim() == 0 or not t.is_contiguous():
                return orig(t, *args, **kw)
            device = kw.get('device') if kw.get('device') is not None else t.device
            dtype = self._wants(device, kw.get('dtype') if kw.get('dtype') is not None else t.dtype)
            if dtype is None:
                return orig(t, *args, **kw)
            return self._alloc(t.shape, dtype, device, kind, _site())[0]
        fn.__wrapped__ = orig
        return fn

    # -------------------------------------------------------------------------------- declarations
    def _record_of(self, t):
        return self.by_storage.get(t.untyped_storage().data_ptr())

    def expect(self, *ts):
        for t in ts:
            if t is None:
                continue
            r = self._record_of(t)
            if r is None:
                raise AssertionError('expect(): a tensor of shape %s, dtype %s is not a guarded allocation'
                                     % (tuple(t.shape), t.dtype))
            if t.dtype != r.dtype:
                raise AssertionError('expect(): a %s view of a %s allocation' % (t.dtype, r.dtype))
            r.views.append((tuple(t.shape), tuple(t.stride()), t.storage_offset() - r.ge))
        return ts[0] if len(ts) == 1 else ts

    def place(self, t, pad=False, ld=None, inplace=None):
        if not torch.is_tensor(t) or t.dtype not in SENTINEL or t.device.type != self.devtype or t.numel() == 0:
            return t
        if inplace is not None and inplace not in INPLACE_WAIVERS:
            raise KeyError('place(inplace=%r): not in guard.INPLACE_WAIVERS' % (inplace,))
        if pad:
            M, D = t.shape
            ld = ld if ld is not None else -(-D // 64) * 64 + 64
            body, r = self._alloc((M, ld), t.dtype, t.device, 'place', _site())
            v = body[:, :D]
            r.live_cols = D
        else:
            body, r = self._alloc(tuple(t.shape), t.dtype, t.device, 'place', _site())
            v = body
            r.live_cols = t.shape[-1] if t.dim() else 1
        v.copy_(t.detach())
        r.inplace = inplace
        r.snap = r.body_ints().clone()
        return v

    def resnap(self, *ts):
        """the host changed a placed input on purpose (the check plants values): remember the new contents"""
        for t in ts:
            r = self._record_of(t)
            if r is not None and r.kind == 'place':
                r.snap = r.body_ints().clone()

    # -------------------------------------------------------------------------------- verification
    def _fail(self, r, kind, idx, what=''):
        ld = r.shape[-1] if r.shape else 1
        row, col = idx // ld, idx % ld
        raise GuardViolation(kind, idx, row, col,
                             'guard violation [%s]%s: %s allocation of shape %s, dtype %s, made in %s; first offending flat '
                             'index %d (from the start of the body) = row %d, column %d of rows of %d elements'
                             % (kind, what, r.kind, r.shape, r.dtype, r.site, idx, row, col, ld))

    @staticmethod
    def _first(mask):
        return int(torch.nonzero(mask.reshape(-1))[0]) if bool(mask.any()) else -1

    def verify(self):
        for r in self.records:
            sent = SENTINEL[r.dtype][1]
            i = self._first(r.ints[:r.ge] != sent)
            if i >= 0:
                self._fail(r, 'head', i - r.ge)
            i = self._first(r.ints[r.ge + r.n:] != sent)
            if i >= 0:
                self._fail(r, 'tail', r.n + i)
            body = r.body_ints()
            if r.kind == 'place':
                if r.inplace is None:
                    i = self._first(body != r.snap)
                    if i >= 0:
                        self._fail(r, 'input changed' if i % r.shape[-1] < r.live_cols else 'pad', i, ' (placed input)')
                elif len(r.shape) >= 2 and r.live_cols < r.shape[-1]:
                    i = self._first(body.view(-1, r.shape[-1])[:, r.live_cols:] != sent)
                    if i >= 0:
                        w = r.shape[-1] - r.live_cols
                        self._fail(r, 'pad', (i // w) * r.shape[-1] + r.live_cols + i % w, ' (placed in-place buffer)')
                continue
            if r.kind != 'empty':
                continue
            live = body != sent
            if r.views:
                want = torch.zeros((r.n,), dtype=torch.bool, device=live.device)
                for size, stride, off in r.views:
                    want.as_strided(size, stride, off).fill_(True)
                i = self._first(live & ~want)
                if i >= 0:
                    self._fail(r, 'pad', i, ' (written outside the declared output)')
                i = self._first(want & ~live)
                if i >= 0:
                    self._fail(r, 'hole', i, ' (declared output element never written)')
            elif len(r.shape) >= 2 and r.site not in RECTANGLE_WAIVERS:
                ld = r.shape[-1]
                live2 = live.view(-1, ld)
                nrows = live2.shape[0]
                owned = live2.sum(0) * 2 > nrows                   # a column belongs to the rectangle if most rows wrote it
                i = self._first(live2 & ~owned)
                if i >= 0:
                    self._fail(r, 'pad', i, ' (a column written in a minority of rows)')
                i = self._first(~live2 & owned)
                if i >= 0:
                    self._fail(r, 'hole', i, ' (an element inside the written rectangle never written)')
                cols = torch.nonzero(owned).reshape(-1)
                if cols.numel() and int(cols[-1]) + 1 != cols.numel():
                    self._fail(r, 'hole', self._first(~owned), ' (a whole column inside the written rectangle never written)')


def active():
    return _ACTIVE


def expect(*ts):
    """declare returned tensors as outputs (identity outside guarded())"""
    if _ACTIVE is None:
        return ts[0] if len(ts) == 1 else ts
    return _ACTIVE.expect(*ts)


def place(t, pad=False, ld=None, inplace=None):
    """move an input into a guarded buffer (identity outside guarded())"""
    return t if _ACTIVE is None else _ACTIVE.place(t, pad, ld, inplace)


def resnap(*ts):
    if _ACTIVE is not None:
        _ACTIVE.resnap(*ts)


@contextlib.contextmanager
def guarded(device='cuda', lib_module=None):
    """-> the set of istvt_* entry points called while the context is active (filled as they are called).
    lib_module: the istvt_amd._lib module (None: no entry-point record, e.g. in the harness's own CPU tests)."""
    global _ACTIVE
    if _ACTIVE is not None:
        raise RuntimeError('guarded() does not nest')
    g = Guard(device)
    names = ('empty', 'zeros', 'empty_like', 'zeros_like')
    g._orig = {k: getattr(torch, k) for k in names}
    real = None
    if lib_module is not None:
        real = lib_module.lib()
    try:
        torch.empty, torch.zeros = g._new('empty'), g._new('zeros')
        torch.empty_like, torch.zeros_like = g._new_like('empty'), g._new_like('zeros')
        if real is not None:
            lib_module._lib = _LibProxy(real, g.calls)
        _ACTIVE = g
        yield g.calls
        _ACTIVE = None
        if g.devtype == 'cuda' and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        for k in names:                       # (verification allocates: with the real callables)
            setattr(torch, k, g._orig[k])
        g.verify()
    finally:
        _ACTIVE = None
        for k in names:
            setattr(torch, k, g._orig[k])
        if real is not None:
            lib_module._lib = real
        g.records, g.by_storage = [], {}
