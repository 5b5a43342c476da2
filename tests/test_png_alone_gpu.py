"""PNG bands that stand alone (DESIGN.md "PNG bands that stand alone") on a real MI355X: one mixed batch through
ops.png_decode_u8 against the definition clips.png_decode_alone_host, byte for byte, eager, captured in a graph and between
guards; the device writer against clips.png_encode_files_host(index=True, alone=True); the round trip; an alone bank by index,
with indices outside it, doctored band rows and a first stream beyond 2^32 bytes; the drawn entry and ops.draw_clips; the
profile records.  PNG is lossless: no tolerance anywhere.  Every flagged file and every doctored row that goes to a device here
comes from tests/png_alone_cases.py and was walked first by tools/png_alone_check.cpp, the same csrc/png_alone.h on the host
(tests/test_png_alone_cpu.py builds it plain; DESIGN.md has its run under AddressSanitizer and UBSan)."""
import numpy as np
import pytest
import torch

import guard
import png_alone_cases as A
import png_bank_cases as K
import png_encode_cases as C

pytestmark = pytest.mark.gpu
CANVAS = (133, 77)
S = 16


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def mixed(pkg, golden_dir):
    """(the named files of the mixed batch, [(frame, status)] of the definition, the batch)"""
    from istvt_amd import clips
    named = A.mixed_files(clips, golden_dir)
    return named, A.reference(clips, named), clips.png_batch([f for _, f in named], bands='index', alone=True)


def _expect(refs, index, canvas):
    """frames, sizes and statuses of the definition on a canvas: places outside the list are zero with status 8"""
    frames = torch.zeros((len(index), canvas[0], canvas[1], 3), dtype=torch.uint8)
    sizes, status = torch.zeros((len(index), 2), dtype=torch.int32), torch.zeros(len(index), dtype=torch.int32)
    for j, i in enumerate(index):
        if 0 <= i < len(refs):
            f, s = refs[i]
            frames[j, :f.shape[0], :f.shape[1]] = f
            sizes[j, 0], sizes[j, 1], status[j] = f.shape[0], f.shape[1], s
        else:
            status[j] = 8
    return frames, sizes, status


def _equal(got, want):
    return all(torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want))


def _record(ops, call):
    ops.kernel_profile = []
    try:
        out = call()
        return out, [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None


def test_one_mixed_batch(pkg, mixed):
    """flagged files at R of 1, 5, 8, 16, 64 and 100, an indexed file without the flag, a PIL file, the lying files and a
    damaged band in one call on a canvas larger than every image, `out` prefilled: frames, margins, sizes and statuses"""
    from istvt_amd import clips, ops
    named, refs, batch = mixed
    n = batch.n
    want = _expect(refs, list(range(n)), CANVAS)
    assert want[2].tolist().count(10) == 3 and {0, 6, 10} < set(want[2].tolist()) and batch.alone.tolist().count(0) == 2
    assert max(r[7] for r in batch.images.tolist()) == 64 and int(batch.bands.shape[0]) > 100
    out = torch.full((n,) + CANVAS + (3,), 0xA5, dtype=torch.uint8, device='cuda')
    buffers = (torch.full((batch.scratch_bytes,), 0xA5, dtype=torch.uint8, device='cuda'),
               torch.full((n, 2), -7, dtype=torch.int32, device='cuda'), torch.full((n,), -7, dtype=torch.int32, device='cuda'))
    (got, record) = _record(ops, lambda: ops.png_decode_u8(batch, canvas=CANVAS, out=out, checked=True, buffers=buffers))
    assert record == ['png_decode_alone_u8'] and got[0] is out and got[1] is buffers[1] and got[2] is buffers[2]
    for i, (name, _) in enumerate(named):
        assert int(got[2][i]) == int(want[2][i]), name
        assert torch.equal(got[0][i].cpu(), want[0][i]), name
    assert _equal(got, want)
    # a sequence of bytes and the crop follow the batch
    assert _equal(ops.png_decode_u8(batch, checked=True), _expect(refs, list(range(n)), (130, 70)))
    (cut, record) = _record(ops, lambda: ops.decode_frames(batch, 2 * S))         # 8 x 32 holds the 130 rows of the tallest
    assert record[0] == 'png_decode_alone_u8'
    assert torch.equal(cut, ops.crop_resize_u8(got[0][:, :130, :70].contiguous(), clips.whole_boxes(batch.sizes), 2 * S))
    # the same call captured in a graph and replayed into refilled buffers
    eager = [t.clone() for t in got]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_decode_u8(batch, canvas=CANVAS, out=out, checked=True, buffers=buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.png_decode_u8(batch, canvas=CANVAS, out=out, checked=True, buffers=buffers)
    for fill in (1, 2):
        out.fill_(fill)
        buffers[0].fill_(fill)
        buffers[1].fill_(-1)
        buffers[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert _equal((out, buffers[1], buffers[2]), eager), fill


def test_guards(pkg, mixed):
    """out, scratch, sizes and status between sentinel guards; the uploaded tables placed as inputs; every element of out
    written (two sentinel fills); of the scratch nothing but each file's filtered rows and the band status words"""
    from istvt_amd import _lib, clips, ops
    named, refs, batch = mixed
    n = batch.n
    want = _expect(refs, list(range(n)), CANVAS)
    band_statuses = sum((clips.png_inflate_bands_host(clips.png_parse(f))[1] for _, f in named), [])
    assert len(band_statuses) == int(batch.bands.shape[0])
    for fill in (0xA5, 0x5A):
        with guard.guarded(lib_module=_lib) as calls:
            dev = batch.on(torch.device('cuda', torch.cuda.current_device()))
            keep = (dev.data, dev.images, dev.bands, dev.alone)
            dev.data, dev.images, dev.bands, dev.alone = (guard.place(t) for t in keep)
            out = guard.place(torch.full((n,) + CANVAS + (3,), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            scratch = guard.place(torch.full((batch.scratch_bytes,), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            sizes = torch.empty((n, 2), dtype=torch.int32, device='cuda')
            status = torch.empty((n,), dtype=torch.int32, device='cuda')
            try:
                got = ops.png_decode_u8(batch, canvas=CANVAS, out=out, checked=True, buffers=(scratch, sizes, status))
            finally:
                dev.data, dev.images, dev.bands, dev.alone = keep
        assert calls == {'istvt_png_decode_alone_u8'} and got[0] is out
        assert _equal(got, want), fill
        host = scratch.cpu()
        rows = host[:n * batch.raw_stride].view(n, batch.raw_stride)
        for i, (h, w, _, bpp) in enumerate(r[:4] for r in batch.images.tolist()):
            assert bool((rows[i, h * (1 + w * bpp):] == fill).all()), 'file %d: the scratch behind its rows was written' % i
        assert host[n * batch.raw_stride:].view(torch.int32).tolist() == band_statuses


def test_the_device_writer(pkg):
    from istvt_amd import clips, ops
    for H, W, ch, R in A.DEVICE_WRITER:
        frames = np.stack([C.smooth(H, W, ch, 30 + j).reshape(H, W, ch) for j in range(2)] + [C.noise(H, W, ch, 9).reshape(H, W, ch)])
        x = torch.from_numpy(frames).cuda()
        for filters in C.FILTERS:
            want = clips.png_encode_files_host(frames, R, filters, index=True, alone=True)
            (files, record) = _record(ops, lambda: ops.png_encode_u8(x, R, filters, index=True, alone=True))
            assert record == ['png_encode_alone_u8'] and files.geometry.alone is True
            assert files.status.tolist() == [0] * 3 and files.files() == want, (H, W, ch, R, filters)
        (plain, record) = _record(ops, lambda: ops.png_encode_u8(x, R, index=True))
        assert record == ['png_encode_indexed_u8'] and plain.files() == clips.png_encode_files_host(frames, R, index=True)
    x = torch.from_numpy(np.stack([C.smooth(29, 29, 3, j) for j in range(3)])).cuda()
    boxes = torch.tensor([[0, 0, 29, 29]] * 3, dtype=torch.int32)
    made = ops.encode_frames(x, 24, boxes, format='png', band_rows=8, index=True, alone=True)
    assert made.files() == clips.png_encode_files_host(ops.crop_resize_u8(x, boxes, 24).cpu(), 8, index=True, alone=True)


def test_round_trip(pkg):
    """encode alone on the device, a bank from files(), decode by index: the source pixels"""
    from istvt_amd import clips, ops
    x = torch.from_numpy(np.stack([C.smooth(45, 37, 3, 60 + j) for j in range(5)])).cuda()
    files = ops.png_encode_u8(x, 8, index=True, alone=True).files()
    assert all(clips.png_parse(f).alone for f in files)
    bank = clips.png_bank(files, alone=True)
    index = [4, 0, 2, 2, 1, 3]
    (got, record) = _record(ops, lambda: ops.png_decode_bank_u8(bank, torch.tensor(index, device='cuda')))
    assert record == ['png_decode_bank_alone_u8'] and got[2].tolist() == [0] * 6 and torch.equal(got[0], x[index])
    batch = ops.png_decode_u8(clips.png_batch(files, bands='index', alone=True), checked=True)
    assert batch[2].tolist() == [0] * 5 and torch.equal(batch[0], x)


@pytest.fixture(scope='module')
def banked(pkg):
    from istvt_amd import clips
    bank = A.alone_bank(clips)
    return bank, [clips.png_decode_alone_host(hd, return_status=True) for hd in bank.headers]


def test_the_bank(pkg, banked):
    from istvt_amd import clips, ops
    bank, refs = banked
    n, canvas = bank.n, (bank.Hmax, bank.Wmax)
    assert bank.band_max == 64 and bank.images[:, 9].tolist() == [1] * 10 + [0, 0]
    for name, index in K.index_shapes(n):
        want = _expect(refs, index, canvas)
        for dtype in (torch.int32, torch.int64):
            assert _equal(ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=dtype, device='cuda')), want), (name, dtype)
        if name == 'repeats':
            assert _equal(want, clips.png_bank_decode_host(bank, index))
    index = [3, -1, 0, n, n - 1, n + 1, n - 2]
    got = ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=torch.int32, device='cuda'), canvas=(131, 75))
    assert got[2].tolist() == [0, 8, 0, 8, 0, 8, 0] and _equal(got, _expect(refs, index, (131, 75)))
    # the lying files and the damaged band in a bank: the definition's statuses, sizes kept, frames zeroed
    named = [(nm, f) for nm, f, _ in A.lying_files(clips)] + [('damaged_band', A.damaged_file(clips))]
    liars = clips.png_bank([f for _, f in named] + [bank_file for bank_file in A.bank_files(clips)[:2]], alone=True)
    index = list(range(liars.n))
    got, want = ops.png_decode_bank_u8(liars, index), clips.png_bank_decode_host(liars, index)
    assert want[2].tolist()[:3] == [10, 10, 10] and want[1][0].tolist() == [36, 25] and _equal(got, want)
    # band rows of a flagged file that differ from what png_bank built: status 9 at their places only
    for name, bad, place in A.doctored(clips, bank):
        index = [place, (place + 1) % n, place, -1, (place + 2) % n, n]
        got = ops.png_decode_bank_u8(bad, torch.tensor(index, dtype=torch.int32, device='cuda'))
        want = _expect(refs, index, canvas)
        for j in (0, 2):
            want[0][j].zero_(), want[1][j].zero_()
            want[2][j] = 9
        assert _equal(got, want) and _equal(got, clips.png_bank_decode_host(bad, index)), name


def test_beyond_2_32_bytes(pkg):
    from istvt_amd import clips, ops
    files = [f for _, f in A.alone_files(clips)[1:4]]
    bank = clips.png_bank(files, first_byte=2 ** 32 + 16, alone=True)
    assert min(K.base_of(r) for r in bank.images.tolist()) >= 2 ** 32 + 16
    index = [2, 0, 1, 1, -1, 3]
    want = clips.png_bank_decode_host(bank, index)
    assert want[2].tolist() == [0] * 4 + [8, 8]
    assert _equal(ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=torch.int32, device='cuda')), want)


def test_drawn_and_draw_clips(pkg):
    """png_decode_bank_alone_drawn_u8 equals the draw, then the decode; draw_clips from an alone bank equals draw_clips from a
    bank of the same frames written without alone, bit for bit: both are lossless"""
    from istvt_amd import clips, ops
    frames = [C.smooth(40 + 3 * j, 48 - 2 * j, 3, 80 + j) for j in range(7)]
    alone = clips.png_bank([clips.png_encode_banded_host(f, 8, index=True, alone=True) for f in frames], alone=True)
    plain = clips.png_bank([clips.png_encode_banded_host(f, 8, index=True) for f in frames])
    assert alone.sizes == plain.sizes and alone.images[:, 9].tolist() == [1] * 7
    base = torch.tensor([[0, 0, h, w] for h, w in alone.sizes], dtype=torch.int32)
    args = dict(videos=[(0, 4, 0), (4, 3, 1)], T=3, B=4, base=base, K=16, seed=77)
    pa, pp = clips.BatchPlan(alone, **args).on('cuda'), clips.BatchPlan(plain, **args).on('cuda')
    for step in (0, 1):
        d = clips.batch_draw_host(pa, step)
        pa.seek(step)
        (got, record) = _record(ops, lambda: ops.png_decode_bank_drawn_u8(alone, pa))
        assert record == ['png_decode_bank_alone_drawn_u8'] and got[3].index.cpu().tolist() == d.index.tolist()
        assert _equal(got[:3], ops.png_decode_bank_u8(alone, d.index)) and got[2].tolist() == [0] * 12
        assert _equal(got[:3], clips.png_bank_decode_host(alone, d.index))
        pa.seek(step), pp.seek(step)
        a, b = ops.draw_clips(alone, pa, S), ops.draw_clips(plain, pp, S)
        assert _equal(a, b) and bool(a[0].any()) and pa.step == pp.step == step + 1


def test_profile_records(pkg, mixed):
    """the three new names; a batch or bank without the flag still records the old ones"""
    from istvt_amd import clips, ops
    named, _, batch = mixed
    files = [f for _, f in named[:4]]
    (_, record) = _record(ops, lambda: ops.png_decode_u8(clips.png_batch(files, bands='index', alone=True), checked=True))
    assert record == ['png_decode_alone_u8']
    (_, record) = _record(ops, lambda: ops.png_decode_u8(clips.png_batch(files, bands='index'), checked=True))
    assert record == ['png_decode_bands_u8']
    (_, record) = _record(ops, lambda: ops.png_decode_u8(files))
    assert record == ['png_decode_u8']
    old, new = clips.png_bank(files), clips.png_bank(files, alone=True)
    plan_old, plan_new = (clips.BatchPlan(b, [(0, 4, 0)], T=2, B=2, jpeg=None, perturb=None).on('cuda') for b in (old, new))
    (a, record) = _record(ops, lambda: ops.png_decode_bank_u8(old, [1, 3]))
    assert record == ['png_decode_bank_u8']
    (b, record) = _record(ops, lambda: ops.png_decode_bank_u8(new, [1, 3]))
    assert record == ['png_decode_bank_alone_u8'] and _equal(a, b)                # flagged files in a bank without alone: the same pixels
    (_, record) = _record(ops, lambda: ops.png_decode_bank_drawn_u8(old, plan_old))
    assert record == ['png_decode_bank_drawn_u8']
    (_, record) = _record(ops, lambda: ops.png_decode_bank_drawn_u8(new, plan_new))
    assert record == ['png_decode_bank_alone_drawn_u8']
