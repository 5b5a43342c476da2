"""The guard-band harness (tests/guard.py) on the CPU: every kind of violation, planted with ordinary torch indexing on
the harness's own buffers, is reported with its kind and position; a clean run reports nothing; the patched callables come
back; and every pointer-taking entry point of the C ABI is accounted for in one of three tables."""
import os
import re

import pytest
import torch

import guard as G

DTYPES = [torch.float32, torch.bfloat16, torch.uint8]
IDS = ['f32', 'bf16', 'u8']
M, D, LD = 5, 24, 40            # a [5, 24] view of rows of 40 elements


def _val(dtype):
    return 3 if dtype == torch.uint8 else 1.5


def _kernel(buf, dtype, rows=M, cols=D):
    """what a correct kernel does: writes rows x [0, cols)"""
    buf[:rows, :cols] = _val(dtype)


def _run(dtype, plant, declare=False, device='cpu'):
    """allocate [M, LD] through the patched torch.empty, write the [M, D] rectangle, plant; -> the violation or None"""
    try:
        with G.guarded(device=device):
            buf = torch.empty((M, LD), dtype=dtype, device=device)
            rec = G.active().records[-1]
            assert buf.data_ptr() == rec.flat.data_ptr() + rec.ge * buf.element_size()
            _kernel(buf, dtype)
            if declare:
                G.expect(buf[:, :D])
            plant(buf, rec)
    except G.GuardViolation as e:
        return e
    return None


@pytest.mark.parametrize('device', ['cpu'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_clean_run_reports_nothing(dtype, device):
    assert _run(dtype, lambda buf, rec: None, device=device) is None
    assert _run(dtype, lambda buf, rec: None, declare=True, device=device) is None


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_write_before_the_body(dtype):
    def plant(buf, rec):
        rec.flat[rec.ge - 1] = _val(dtype)
    e = _run(dtype, plant)
    assert e is not None and e.kind == 'head' and e.index == -1 and (e.row, e.col) == (-1, LD - 1), e
    assert str((M, LD)) in str(e) and str(dtype) in str(e)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_write_after_the_body(dtype):
    def plant(buf, rec):
        rec.flat[rec.ge + rec.n] = _val(dtype)
    e = _run(dtype, plant)
    assert e is not None and e.kind == 'tail' and e.index == M * LD and (e.row, e.col) == (M, 0), e


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_write_200_rows_after_the_body(dtype):
    """inside the row-scaled guard (256 rows), beyond a fixed 4 KiB one at this row length for float32"""
    def plant(buf, rec):
        assert rec.ge >= 256 * LD
        rec.flat[rec.ge + rec.n + 200 * LD + 7] = _val(dtype)
    e = _run(dtype, plant)
    assert e is not None and e.kind == 'tail' and e.index == (M + 200) * LD + 7 and (e.row, e.col) == (M + 200, 7), e


@pytest.mark.parametrize('declare', [False, True])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pad_column_in_the_last_row(dtype, declare):
    def plant(buf, rec):
        buf[M - 1, D + 3] = _val(dtype)
    e = _run(dtype, plant, declare)
    assert e is not None and e.kind == 'pad' and e.index == (M - 1) * LD + D + 3 and (e.row, e.col) == (M - 1, D + 3), e


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pad_column_in_every_row_needs_expect(dtype):
    def plant(buf, rec):
        buf[:, D] = _val(dtype)
    assert _run(dtype, plant) is None                      # rule 2 takes it for a rectangle of D + 1 columns
    e = _run(dtype, plant, declare=True)
    assert e is not None and e.kind == 'pad' and e.index == D and (e.row, e.col) == (0, D), e


@pytest.mark.parametrize('declare', [False, True])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_unwritten_element_in_the_last_row(dtype, declare):
    def plant(buf, rec):
        rec.ints[rec.ge + (M - 1) * LD + 5] = G.SENTINEL[dtype][1]
    e = _run(dtype, plant, declare)
    assert e is not None and e.kind == 'hole' and e.index == (M - 1) * LD + 5 and (e.row, e.col) == (M - 1, 5), e


def _placed(dtype, plant, pad):
    src = (torch.arange(M * D) % 7).view(M, D).to(dtype)
    try:
        with G.guarded(device='cpu'):
            x = G.place(src, pad=pad, ld=LD)
            rec = G.active().records[-1]
            assert torch.equal(x, src) and x.stride(0) == (LD if pad else D)
            plant(x, rec)
    except G.GuardViolation as e:
        return e
    return None


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_placed_input_changed(dtype):
    assert _placed(dtype, lambda x, rec: None, True) is None
    assert _placed(dtype, lambda x, rec: None, False) is None

    def body(x, rec):
        x[2, 3] = 9
    e = _placed(dtype, body, True)
    assert e is not None and e.kind == 'input changed' and e.index == 2 * LD + 3 and (e.row, e.col) == (2, 3), e
    e = _placed(dtype, body, False)
    assert e is not None and e.kind == 'input changed' and e.index == 2 * D + 3 and (e.row, e.col) == (2, 3), e

    def pad(x, rec):
        rec.flat[rec.ge + 4 * LD + D + 1] = _val(dtype)
    e = _placed(dtype, pad, True)
    assert e is not None and e.kind == 'pad' and e.index == 4 * LD + D + 1 and (e.row, e.col) == (4, D + 1), e

    def tail(x, rec):
        rec.flat[rec.ge + rec.n + 1] = _val(dtype)
    e = _placed(dtype, tail, True)
    assert e is not None and e.kind == 'tail' and e.index == M * LD + 1, e


def test_placed_pads_hold_the_sentinel_and_inplace_buffers_may_change():
    with G.guarded(device='cpu'):
        x = G.place(torch.ones((M, D)), pad=True, ld=LD)
        rec = G.active().records[-1]
        assert bool(rec.flat[rec.ge:rec.ge + rec.n].view(M, LD)[:, D:].isnan().all())
        acc = G.place(torch.zeros((D,)), inplace='accumulator')
        acc += 1.0
        del x
    with pytest.raises(KeyError):
        with G.guarded(device='cpu'):
            G.place(torch.zeros((D,)), inplace='no such waiver')


def test_zeros_body_is_zero_and_its_guards_are_checked():
    with G.guarded(device='cpu'):
        z = torch.zeros((M, LD), dtype=torch.bfloat16)
        like = torch.zeros_like(z)
        assert float(z.abs().max()) == 0.0 and float(like.abs().max()) == 0.0
        assert len(G.active().records) == 2
        z[1, 2] = 1.0                                     # accumulating into a zeroed buffer is no violation
    with pytest.raises(G.GuardViolation) as ei:
        with G.guarded(device='cpu'):
            z = torch.zeros((M, LD), dtype=torch.bfloat16)
            rec = G.active().records[-1]
            rec.flat[rec.ge + rec.n + 2] = 1.0
    assert ei.value.kind == 'tail' and ei.value.index == M * LD + 2


def test_one_dimensional_and_like_allocations():
    with G.guarded(device='cpu'):
        v = torch.empty((100,), dtype=torch.float32)
        rec = G.active().records[-1]
        assert rec.ge * 4 == 4096                         # a 1-D tensor: 4096 bytes on each side
        w = torch.empty_like(v)
        assert G.active().records[-1] is not rec and bool(w.isnan().all()) and bool(v.isnan().all())
        v.fill_(1.0)
        w.fill_(2.0)
        G.expect(v, w)
    with pytest.raises(G.GuardViolation) as ei:
        with G.guarded(device='cpu'):
            v = torch.empty((100,), dtype=torch.float32)
            v[:99] = 1.0
            G.expect(v)
    assert ei.value.kind == 'hole' and ei.value.index == 99
    with pytest.raises(AssertionError, match='not a guarded allocation'):
        with G.guarded(device='cpu'):
            G.expect(torch.ones((3,)))


def test_what_is_not_guarded_passes_through():
    with G.guarded(device='cpu'):
        n = len(G.active().records)
        a = torch.empty((3, 4), dtype=torch.float16)                      # a dtype the harness does not know
        b = torch.empty((3, 4), dtype=torch.float32, pin_memory=False)    # an unusual keyword
        c = torch.empty((0, 4))                                           # nothing to guard
        d = torch.empty_like(torch.ones((4, 6))[:, :3])                   # not contiguous
        e = torch.empty((3, 4), device='meta')                            # another device
        assert len(G.active().records) == n
        assert a.dtype == torch.float16 and b.shape == (3, 4) and c.numel() == 0 and d.shape == (4, 3) and e.is_meta
    with G.guarded(device='cuda'):                                         # the device filter: CPU tensors pass
        torch.empty((3, 4))
        assert len(G.active().records) == 0


def test_callables_are_restored_also_after_an_exception():
    orig = (torch.empty, torch.zeros, torch.empty_like, torch.zeros_like)
    with G.guarded(device='cpu'):
        assert torch.empty is not orig[0] and torch.zeros_like is not orig[3]
    assert (torch.empty, torch.zeros, torch.empty_like, torch.zeros_like) == orig
    with pytest.raises(ZeroDivisionError):
        with G.guarded(device='cpu'):
            1 / 0
    assert (torch.empty, torch.zeros, torch.empty_like, torch.zeros_like) == orig
    assert _run(torch.float32, lambda buf, rec: buf.__setitem__((0, D + 1), 1.0)) is not None
    assert (torch.empty, torch.zeros, torch.empty_like, torch.zeros_like) == orig and G.active() is None
    with pytest.raises(RuntimeError, match='does not nest'):
        with G.guarded(device='cpu'):
            with G.guarded(device='cpu'):
                pass
    assert (torch.empty, torch.zeros, torch.empty_like, torch.zeros_like) == orig and G.active() is None


@pytest.mark.parametrize('shape', [(M, LD), (1003, 728), (3, 7, 2), (100,)])
@pytest.mark.parametrize('dtype', DTYPES + [torch.float64, torch.int32, torch.int64], ids=IDS + ['f64', 'i32', 'i64'])
def test_body_keeps_the_alignment_of_the_raw_allocation(dtype, shape):
    with G.guarded(device='cpu'):
        t = torch.empty(shape, dtype=dtype)
        rec = G.active().records[-1]
        assert t.data_ptr() % 256 == rec.flat.data_ptr() % 256
        es = t.element_size()
        want = 4096 if len(shape) < 2 else max(4096, 256 * shape[-1] * es)
        assert rec.ge * es == -(-want // 256) * 256 and (rec.ge * es) % 256 == 0
        t.fill_(1)


def test_entry_point_record():
    class FakeLib:
        def istvt_something(self):
            return 0

        def istvt_looked_up_only(self):
            return 2

        def other(self):
            return 1

    class FakeModule:
        _lib = FakeLib()

        @classmethod
        def lib(cls):
            return cls._lib
    real = FakeModule._lib
    with G.guarded(device='cpu', lib_module=FakeModule) as calls:
        assert FakeModule._lib is not real
        FakeModule.lib().istvt_looked_up_only                             # a look-up is not a call
        assert FakeModule.lib().istvt_something() == 0 and FakeModule.lib().other() == 1
    assert calls == {'istvt_something'} and FakeModule._lib is real


# ---- completeness: every pointer-taking entry point has had a decision made about it ---------------------------------
def test_every_pointer_taking_entry_point_is_accounted_for():
    import ctypes

    import gpu_checks
    from istvt_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    guarded_here = set()
    for names in gpu_checks.EXPECTED_CALLS.values():
        guarded_here.update(names)
    assert guarded_here <= set(_lib.SIGNATURES), guarded_here - set(_lib.SIGNATURES)
    for name, (path, test, reason) in gpu_checks.GUARDED_ELSEWHERE.items():
        full = os.path.join(root, path)
        assert os.path.exists(full), (name, path)
        src = open(full).read()
        assert re.search(r'^def %s\(' % re.escape(test), src, re.M), (name, path, test)
        assert reason and name in _lib.SIGNATURES
    for name, reason in gpu_checks.NOT_A_WRITER.items():
        assert reason and name in _lib.SIGNATURES, name
    undecided = []
    for name, argtypes in _lib.SIGNATURES.items():
        if ctypes.c_void_p not in argtypes:
            continue
        if not (name in guarded_here or name in gpu_checks.GUARDED_ELSEWHERE or name in gpu_checks.NOT_A_WRITER):
            undecided.append(name)
    assert not undecided, 'entry points with pointer arguments and no guard decision: %s' % undecided
    # every guarded registration has its expected entry points, and every table entry a registration
    registered = {n for n, _ in gpu_checks.guarded_entries()}
    assert registered == set(gpu_checks.EXPECTED_CALLS), registered ^ set(gpu_checks.EXPECTED_CALLS)
    for table in (G.RECTANGLE_WAIVERS, G.INPLACE_WAIVERS):
        assert all(isinstance(v, str) and v for v in table.values())
