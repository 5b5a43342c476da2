"""PNG windows (DESIGN.md "PNG windows") on a real MI355X, through the C ABI: the batch and the bank entry against the
definition clips.png_bank_window_host, byte for byte -- windows, moved boxes, origins, sizes and statuses -- and the crop of the
windows through the moved boxes against the crop of the whole decode through the boxes, the same kernel on both sides; a device
index with repeats, -1 and n and device boxes; a file without the flag, faults a box touches and faults it does not, boxes
outside their images; doctored device tables; a first stream beyond 2^32 bytes; guards; the drawn entry and
ops.draw_clips(window=True); ops.decode_frames(window=True); the profile records; the -3 lists.  PNG is lossless: no tolerance
anywhere.  Every table, box and row that goes to a device here comes from tests/png_window_cases.py and was walked first by
tools/png_window_check.cpp, the same csrc/png_window.h on the host (tests/test_png_window_cpu.py builds it plain; DESIGN.md has
its run under AddressSanitizer and UBSan)."""
import pytest
import torch

import guard
import png_bank_cases as K
import png_window_cases as Wn

pytestmark = pytest.mark.gpu
NAMES = ('windows', 'moved boxes', 'sizes', 'status', 'origin')


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _want(ref):
    """png_bank_window_host's (windows, sizes, status, origin, moved) in the order the device call hands them back"""
    windows, sizes, status, origin, moved = ref
    return windows, moved, sizes, status, origin


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g.cpu(), w), '%s: %s differ' % (what, name)


def _record(ops, call):
    ops.kernel_profile = []
    try:
        out = call()
        return out, [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None


def _dev(rows):
    return torch.tensor(rows, dtype=torch.int32, device='cuda')


def test_the_batch(pkg):
    from istvt_amd import clips, ops
    named, bank = Wn.files(clips), Wn.bank(clips)
    batch = clips.png_batch([f for _, f, _ in named], bands='index', alone=True)
    boxes = Wn.batch_boxes(clips)
    want = _want(Wn.reference(clips, 'batch', bank, list(range(bank.n)), boxes, bank.Hmax, bank.Wmax))
    assert want[3].tolist() == [0] * bank.n
    host = torch.tensor(boxes, dtype=torch.int32)
    (got, record) = _record(ops, lambda: ops.png_decode_window_u8(batch, host, rows=bank.Hmax))
    assert record == ['png_decode_window_u8']
    _same(got, want, 'host boxes')
    _same(ops.png_decode_window_u8(batch, host.cuda(), rows=bank.Hmax), want, 'device boxes')
    # rows=None with host boxes: the smallest window that fits them
    small, need = ops.png_decode_window_u8(batch, host), Wn.batch_rows(clips)
    assert tuple(small[0].shape) == (bank.n, need, bank.Wmax, 3) and need < bank.Hmax
    _same(small, _want(clips.png_bank_window_host(bank, list(range(bank.n)), boxes, need)), 'the smallest window')
    # the crop of the windows through the moved boxes is the crop of the whole frames through the boxes: the same kernel
    frames = ops.png_decode_u8(batch, checked=True)[0]
    for S in (8, 16):
        sel = [i for i, b in enumerate(boxes) if max(b[2], b[3]) <= 8 * S]
        assert len(sel) >= 8
        a = ops.crop_resize_u8(got[0][sel].contiguous(), got[1][sel].contiguous(), S, checked=True)
        assert torch.equal(a, ops.crop_resize_u8(frames[sel].contiguous(), host[sel], S)), S


def test_the_bank(pkg):
    """every box at every band edge; a tight window on a wider canvas; faults touched and untouched, a file without the flag,
    indices outside the bank and boxes outside their images; doctored tables: index and boxes on the device"""
    from istvt_amd import clips, ops
    seen = set()
    for name, bank, index, boxes, rows, Wc in Wn.device_calls(clips):
        want = _want(Wn.reference(clips, 'call_' + name, bank, index, boxes, rows, Wc))
        for dtype in (torch.int32, torch.int64):
            (got, record) = _record(ops, lambda: ops.png_decode_window_u8(bank, _dev(boxes), index=torch.tensor(index, dtype=dtype, device='cuda'),
                                                                           rows=rows, canvas_w=Wc))
            assert record == ['png_decode_bank_window_u8']
            _same(got, want, '%s %s' % (name, dtype))
        seen |= set(want[3].tolist())
        if name == 'tight':
            assert 12 in want[3].tolist() and want[3].tolist().count(0) > 50
        if name.startswith('doctored'):
            assert want[3].tolist() == [9, 0, 9] and want[2][0].tolist() == [0, 0]
    assert {0, 6, 8, 9, 10, 11, 12} <= seen and len(seen) == 8
    # host index and host boxes go the same way, checked by name first
    bank = Wn.bank(clips)
    index, boxes, _ = Wn.places(clips)
    got = ops.png_decode_window_u8(bank, torch.tensor(boxes, dtype=torch.int32), index=index, rows=bank.Hmax)
    _same(got, _want(Wn.reference(clips, 'call_all', bank, index, boxes, bank.Hmax, bank.Wmax)), 'host tables')
    sel = [j for j, b in enumerate(boxes) if max(b[2], b[3]) <= 128]
    cut = [boxes[j] for j in sel]
    a = ops.decode_frames(bank, 16, _dev(cut), index=_dev([index[j] for j in sel]), window=True)
    assert torch.equal(a, ops.decode_frames(bank, 16, torch.tensor(cut, dtype=torch.int32), index=[index[j] for j in sel]))


def test_beyond_2_32_bytes(pkg):
    from istvt_amd import clips, ops
    bank = Wn.small_bank(clips, 2 ** 32 + 16)
    assert min(K.base_of(r) for r in bank.images.tolist()) >= 2 ** 32 + 16
    index, boxes, rows = Wn.BEYOND
    want = _want(clips.png_bank_window_host(bank, index, boxes, rows))
    assert want[3].tolist() == [0] * 4 + [8, 8, 0]
    _same(ops.png_decode_window_u8(bank, _dev(boxes), index=_dev(index), rows=rows), want, 'beyond 2^32')


def test_guards(pkg):
    """out, scratch, sizes and status between sentinel guards, the tables placed as inputs; every byte of out and every word of
    the moved boxes and origins written (two fills); of the scratch nothing beyond the layout, no slot without a band and no
    byte behind a window's rows; with out and buffers nothing is allocated"""
    from istvt_amd import _lib, clips, ops
    for name, bank, index, boxes, rows, Wc in [c for c in Wn.device_calls(clips) if c[0] in ('tight', 'faults', 'doctored_wrong_out')]:
        want = _want(Wn.reference(clips, 'call_' + name, bank, index, boxes, rows, Wc))
        m = len(index)
        need = clips.png_window_scratch_bytes(bank, m, rows)
        wb, ws = clips.png_window_bands(bank, rows), clips.png_window_stride(bank, rows)
        for fill in (0xA5, 0x5A):
            with guard.guarded(lib_module=_lib) as calls:
                dev = bank.on(torch.device('cuda', torch.cuda.current_device()))
                keep = (dev.data, dev.images, dev.segments)
                dev.data, dev.images, dev.segments = (guard.place(t) for t in keep)
                idx, bx = guard.place(_dev(index)), guard.place(_dev(boxes))
                out = guard.place(torch.full((m, rows, Wc, 3), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
                scratch = guard.place(torch.full((need + 64,), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
                sizes = torch.empty((m, 2), dtype=torch.int32, device='cuda')
                status = torch.empty((m,), dtype=torch.int32, device='cuda')
                try:
                    got = ops.png_decode_window_u8(bank, bx, index=idx, rows=rows, canvas_w=Wc, out=out, buffers=(scratch, sizes, status))
                finally:
                    dev.data, dev.images, dev.segments = keep
            assert calls == {'istvt_png_decode_bank_window_u8'} and got[0] is out and got[2] is sizes and got[3] is status
            _same(got, want, '%s fill %x' % (name, fill))
            host = scratch.cpu()
            assert bool((host[need:] == fill).all()), 'the scratch behind the layout was written'
            word = int.from_bytes(bytes([fill] * 4), 'little', signed=True)
            slots = host[m * ws:m * ws + 4 * m * wb].view(torch.int32).view(m, wb)
            for j in range(m):
                touched = 0
                if int(want[3][j]) not in (8, 9, 11, 12):
                    H, W, bpp, R, count, _ = clips._png_window_files(bank)[index[j]]
                    plan = clips.png_window_plan(H, R, count, boxes[j], rows, wb, W)
                    touched = plan[1] - plan[0] + 1
                    used = (plan[3] - plan[2]) * (1 + W * bpp)
                    assert bool((host[j * ws + used:(j + 1) * ws] == fill).all()), 'place %d: the scratch behind its rows was written' % j
                else:
                    assert bool((host[j * ws:(j + 1) * ws] == fill).all()), 'place %d: a place with a status was inflated' % j
                assert slots[j, touched:].tolist() == [word] * (wb - touched), 'place %d: a slot without a band was written' % j
    # nothing is allocated
    name, bank, index, boxes, rows, Wc = Wn.device_calls(clips)[0]
    m = len(index)
    idx, bx = _dev(index), _dev(boxes)
    out = torch.empty((m, rows, Wc, 3), dtype=torch.uint8, device='cuda')
    buffers = (torch.empty((clips.png_window_scratch_bytes(bank, m, rows),), dtype=torch.uint8, device='cuda'),
               torch.empty((m, 2), dtype=torch.int32, device='cuda'), torch.empty((m,), dtype=torch.int32, device='cuda'))
    ops.png_decode_window_u8(bank, bx, index=idx, rows=rows, canvas_w=Wc, out=out, buffers=buffers)
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    got = ops.png_decode_window_u8(bank, bx, index=idx, rows=rows, canvas_w=Wc, out=out, buffers=buffers)
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
    assert got[1].untyped_storage().data_ptr() == buffers[0].untyped_storage().data_ptr() == got[4].untyped_storage().data_ptr()
    _same(got, _want(Wn.reference(clips, 'call_' + name, bank, index, boxes, rows, Wc)), 'the caller\'s buffers')


def test_drawn_and_draw_clips(pkg):
    """png_decode_bank_window_drawn_u8 equals the draw, then the definition; draw_clips(window=True) gives the bytes of
    draw_clips for the same plan and step, all stages run: 2 clips of 3 frames"""
    from istvt_amd import clips, ops
    S = 16
    bank, args = Wn.drawn_case(clips)
    pa, pb = clips.BatchPlan(bank, **args).on('cuda'), clips.BatchPlan(bank, **args).on('cuda')
    assert pa.thr_jpeg > 0 and pa.thr_perturb > 0
    rows = clips.png_window_rows(bank, pa.max_side)
    assert rows < bank.Hmax
    for step in (0, 1):
        d = clips.batch_draw_host(pa, step)
        pa.seek(step)
        (got, record) = _record(ops, lambda: ops.png_decode_bank_window_drawn_u8(bank, pa))
        assert record == ['png_decode_bank_window_drawn_u8'] and got[5].index.cpu().tolist() == d.index.tolist()
        assert tuple(got[0].shape) == (6, rows, bank.Wmax, 3) and got[3].tolist() == [0] * 6
        _same(got[:5], _want(clips.png_bank_window_host(bank, d.index, d.boxes, rows)), 'drawn, step %d' % step)
        pa.seek(step), pb.seek(step)
        (a, record) = _record(ops, lambda: ops.draw_clips(bank, pa, S, window=True))
        assert record[0] == 'png_decode_bank_window_drawn_u8' and {'crop_resize_u8', 'jpeg_roundtrip_u8', 'perturb_u8'} <= set(record)
        (b, record) = _record(ops, lambda: ops.draw_clips(bank, pb, S))
        assert record[0] == 'png_decode_bank_alone_drawn_u8' and {'crop_resize_u8', 'jpeg_roundtrip_u8', 'perturb_u8'} <= set(record)
        assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b)) and bool(a[0].any()) and pa.step == pb.step == step + 1


def test_profile_records(pkg):
    """the three new names (the drawn one: test_drawn_and_draw_clips); the existing calls record what they did"""
    from istvt_amd import clips, ops
    bank = Wn.small_bank(clips)
    boxes = torch.tensor(Wn.PROFILE_BOXES, dtype=torch.int32)
    batch = clips.png_batch(bank.headers, bands='index', alone=True)
    (_, record) = _record(ops, lambda: ops.png_decode_window_u8(batch, boxes))
    assert record == ['png_decode_window_u8']
    (_, record) = _record(ops, lambda: ops.png_decode_window_u8(bank, boxes, index=[0, 1, 2]))
    assert record == ['png_decode_bank_window_u8']
    # a bank with boxes or an index on the device and no rows: refused by name, nothing launched
    for kw in (dict(boxes=boxes.cuda(), index=[0, 1, 2]), dict(boxes=boxes, index=_dev([0, 1, 2])), dict(boxes=boxes.cuda(), index=_dev([0, 1, 2]))):
        with pytest.raises(ValueError, match=r'png_decode_window_u8: boxes or an index on the device are not read here: say rows='):
            _record(ops, lambda: ops.png_decode_window_u8(bank, kw['boxes'], index=kw['index']))
    (_, record) = _record(ops, lambda: ops.png_decode_u8(batch, checked=True))
    assert record == ['png_decode_alone_u8']
    (_, record) = _record(ops, lambda: ops.png_decode_bank_u8(bank, [0, 1, 2]))
    assert record == ['png_decode_bank_alone_u8']
    (a, record) = _record(ops, lambda: ops.decode_frames(batch, 16, boxes))
    assert record == ['png_decode_alone_u8', 'crop_resize_u8']
    (b, record) = _record(ops, lambda: ops.decode_frames(batch, 16, boxes, window=True))
    assert record == ['png_decode_window_u8', 'crop_resize_u8'] and torch.equal(a, b)
    (a, record) = _record(ops, lambda: ops.decode_frames(bank, 16, boxes, index=[0, 1, 2]))
    assert record == ['png_decode_bank_alone_u8', 'crop_resize_u8']
    (b, record) = _record(ops, lambda: ops.decode_frames(bank, 16, boxes, index=[0, 1, 2], window=True))
    assert record == ['png_decode_bank_window_u8', 'crop_resize_u8'] and torch.equal(a, b) and bool(a.any())


def test_the_entries_refuse_before_any_launch(pkg):
    """the -3 list of each entry, once each, from scalars"""
    from istvt_amd import _lib, clips
    assert Wn.entries_refuse(clips, _lib) > 40
