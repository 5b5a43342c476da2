"""PNG bank (DESIGN.md "PNG bank") on a real MI355X: ops.png_decode_bank_u8 against ops.png_decode_u8 on the files the index
names and against the definition clips.png_bank_decode_host, byte for byte (PNG is lossless: no tolerance anywhere); indices
outside the bank; damaged and lying files, doctored device rows and where the call writes; a captured graph; the drawn decode
and ops.draw_clips; ops.decode_frames; banks whose streams lie beyond 2^31 and 2^32 bytes.  Every table row and every stream
that goes to a device here comes from tests/png_bank_cases.py and was passed first by tools/png_bank_check.cpp, the same
csrc/png_bank.h and csrc/png_inflate.h on the host (tests/test_png_bank_cpu.py builds it plain; DESIGN.md has its run under
AddressSanitizer and UBSan)."""
import pytest
import torch

import png_bank_cases as K
from test_jpeg_split_gpu import Guarded

pytestmark = pytest.mark.gpu
S = 16


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def banked(pkg):
    from istvt_amd import clips
    return K.fixture_files(clips), K.fixture_bank(clips), K.reference(clips)


def _draw(refs, index, n, canvas):
    """the definition's result for `index` from the per-file results: places outside [0, n) are zero with status 8"""
    frames = torch.zeros((len(index), canvas[0], canvas[1], 3), dtype=torch.uint8)
    sizes, status = torch.zeros((len(index), 2), dtype=torch.int32), torch.zeros(len(index), dtype=torch.int32)
    for j, i in enumerate(index):
        if 0 <= i < n:
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


def test_index_semantics(pkg, banked):
    from istvt_amd import clips, ops
    files, bank, refs = banked
    n = bank.n
    for name, index in K.index_shapes(n):
        want = _draw(refs, index, n, (130, 111))
        batch = ops.png_decode_u8(clips.png_batch([files[i] for i in index], bands='index'), canvas=(130, 111), checked=True)
        assert _equal(batch, want), name
        for dtype in (torch.int32, torch.int64):
            for device in ('cuda', 'cpu'):
                got = ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=dtype, device=device))
                assert tuple(got[0].shape) == (len(index), 130, 111, 3) and got[0].is_cuda       # the bank's largest image
                assert _equal(got, want), (name, dtype, device)
        if name == 'repeats':
            assert _equal(want, clips.png_bank_decode_host(bank, index))
    (got, record) = _record(ops, lambda: ops.png_decode_bank_u8(bank, [2, 1], canvas=(131, 113)))
    assert record == ['png_decode_bank_u8'] and _equal(got, _draw(refs, [2, 1], n, (131, 113)))


def test_indices_outside_the_bank(pkg, banked):
    from istvt_amd import clips, ops
    files, bank, refs = banked
    n = bank.n
    index = [3, -1, 0, n, n - 1, n + 1, n - 2]                     # the JPEG bank test's, with its two high places at ours
    want = _draw(refs, index, n, (130, 111))
    assert want[2].tolist() == [0, 8, 0, 8, 0, 8, 0] and want[1][1].tolist() == [0, 0] and int(want[0][3].max()) == 0
    for dtype in (torch.int32, torch.int64):
        assert _equal(ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=dtype, device='cuda')), want)
    low = [K.INT_MIN, 1, K.INT_MAX]
    assert _equal(ops.png_decode_bank_u8(bank, torch.tensor(low, dtype=torch.int32, device='cuda')), _draw(refs, low, n, (130, 111)))
    wide = [2 ** 32 + 3, 5, -2 ** 40, 2 ** 31, -2 ** 31 - 1]       # values no int32 holds: 2^32 + 3 is not file 3
    got = ops.png_decode_bank_u8(bank, torch.tensor(wide, dtype=torch.int64, device='cuda'))
    assert _equal(got, _draw(refs, wide, n, (130, 111))) and got[2].tolist() == [8, 0, 8, 8, 8]
    assert _equal(got, clips.png_bank_decode_host(bank, wide))
    with pytest.raises(ValueError, match=r'png_decode: file 0 is damaged \(status 8: the index is outside the bank\)'):
        clips.check_png_status(got[2])


def test_damaged_files_doctored_rows_and_what_the_call_leaves_alone(pkg, banked):
    from istvt_amd import clips, ops
    files, bank = K.damaged_files(clips), K.damaged_bank(clips)
    n = bank.n
    index = [1, 0, n - 1, 3, -1, n - 3, 5, n, 7, 1, 9, 11, 13, n - 2]
    sound = [j for j, i in enumerate(index) if 0 <= i < n]
    canvas = (37, 27)
    want = ops.png_decode_u8([files[index[j]] for j in sound], canvas=canvas, bands='index')
    assert len(set(want[2].tolist())) >= 5 and 0 in want[2].tolist()
    m = len(index)
    idx = torch.tensor(index, dtype=torch.int32, device='cuda')
    results = []
    for fill in (0xFF, 0x00):
        out = Guarded((m,) + canvas + (3,), torch.uint8, 1)
        scratch = Guarded((clips.png_bank_scratch_bytes(bank, m),), torch.uint8)
        sizes, status = Guarded((m, 2), torch.int32), Guarded((m,), torch.int32)
        assert out.t.data_ptr() % 2 == 1
        scratch.t.fill_(fill)
        out.t.fill_(0x5A)
        got = ops.png_decode_bank_u8(bank, idx, canvas=canvas, out=out.t, buffers=(scratch.t, sizes.t, status.t))
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.t.data_ptr()
        assert out.intact() and scratch.intact() and sizes.intact() and status.intact(), fill
        results.append([t.cpu().clone() for t in got])
    assert _equal(results[0], results[1])
    frames, sizes, status = results[0]
    assert torch.equal(frames[sound], want[0].cpu()) and torch.equal(sizes[sound], want[1].cpu())
    assert torch.equal(status[sound], want[2].cpu())
    assert status[[4, 7]].tolist() == [8, 8] and sizes[[4, 7]].tolist() == [[0, 0], [0, 0]] and int(frames[[4, 7]].max()) == 0
    assert _equal(results[0], clips.png_bank_decode_host(bank, index, canvas))
    # the bank's tables and bytes on the device are as they were uploaded
    dev = bank.on(idx.device)
    assert torch.equal(dev.images.cpu(), bank.images) and torch.equal(dev.segments.cpu(), bank.bands)
    assert torch.equal(dev.data.cpu(), bank.data)
    # a scratch one byte short and a canvas smaller than the bank's largest image are refused
    small = torch.empty(clips.png_bank_scratch_bytes(bank, m) - 1, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='png_decode_bank_u8: buffers = '):
        ops.png_decode_bank_u8(bank, idx, buffers=(small, results[0][1].cuda(), results[0][2].cuda()))
    with pytest.raises(ValueError, match='png_decode_bank_u8: the canvas must hold every image of the bank'):
        ops.png_decode_bank_u8(bank, idx, canvas=(35, 25))
    # device rows that differ from what png_bank built: status 9 at their places, every other place as it was
    _, good, refs = banked
    n = good.n
    names = []
    for name, bad, place in K.doctored(clips, good):
        index = [place, (place + 1) % n, place, -1, (place + 2) % n, n]
        got = ops.png_decode_bank_u8(bad, torch.tensor(index, dtype=torch.int32, device='cuda'))
        want = _draw(refs, index, n, (130, 111))
        for j in (0, 2):
            want[0][j].zero_(), want[1][j].zero_()
            want[2][j] = 9
        assert _equal(got, want), name
        assert _equal(got, clips.png_bank_decode_host(bad, index)), name
        names.append(name)
    assert len(names) == 11
    with pytest.raises(ValueError, match=r"status 9: the bank's row for this place"):
        clips.check_png_status(got[2])


def test_captured_in_a_graph(pkg, banked):
    """one call with out= and buffers= captured on one stream and replayed on three contents of the same index tensor: a
    call that synchronised, allocated or read the index on the host could not be captured, or would replay the first draw"""
    from istvt_amd import clips, ops
    files, bank, refs = banked
    n, m = bank.n, 9
    g = torch.Generator().manual_seed(9)
    draws = [torch.randint(0, n, (m,), generator=g).tolist() for _ in range(3)] + [[n, 4, -1] + [6] * (m - 3)]
    idx = torch.tensor(draws[0], dtype=torch.int32, device='cuda')
    out = torch.zeros((m, 130, 111, 3), dtype=torch.uint8, device='cuda')
    buffers = (torch.empty(clips.png_bank_scratch_bytes(bank, m), dtype=torch.uint8, device='cuda'),
               torch.zeros((m, 2), dtype=torch.int32, device='cuda'), torch.zeros((m,), dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.png_decode_bank_u8(bank, idx, out=out, buffers=buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.png_decode_bank_u8(bank, idx, out=out, buffers=buffers)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                      # captured, not run
    for draw in draws[1:]:
        idx.copy_(torch.tensor(draw, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert _equal((out, buffers[1], buffers[2]), _draw(refs, draw, n, (130, 111))), draw


def _plan_args(bank):
    base = torch.tensor([[0, 0, min(h, 8 * S), min(w, 8 * S)] for h, w in bank.sizes], dtype=torch.int32)
    return dict(videos=[(0, 6, 0), (6, 7, 1)], T=3, B=4, base=base, K=16, seed=77)


def _chain(clips, ops, bank, plan, step):
    """the input side of a step from the definition's host tables through the calls that take such tables"""
    d = clips.batch_draw_host(plan, step)
    B, T = plan.B, plan.T
    frames, _, status = ops.png_decode_bank_u8(bank, d.index)
    u8 = ops.crop_resize_u8(frames, d.boxes, S)
    if plan.thr_jpeg:
        u8 = ops.jpeg_roundtrip_u8(u8, d.quality)
    u8 = u8.view(B, T, S, S, 3)
    if plan.thr_perturb:
        u8 = ops.perturb_u8(u8, d.perturb, plan.taps, plan.seed)
    return u8.cpu(), d.view, d.label, status.cpu()


def _mixed(d):
    """some clips recompressed and some not, some perturbed and some not"""
    q, k = d.quality.view(-1, 3)[:, 0], d.perturb[:, 0]
    return 0 < int((q > 0).sum()) < len(q) and 0 < int((k > 0).sum()) < len(k)


def test_drawn(pkg, banked):
    from istvt_amd import clips, ops
    files, bank, refs = banked
    args = _plan_args(bank)
    plan = clips.BatchPlan(bank, **args)
    assert plan.thr_jpeg > 0 and plan.thr_perturb > 0               # all stages run
    first = next(s for s in range(500) if _mixed(clips.batch_draw_host(plan, s)) and _mixed(clips.batch_draw_host(plan, s + 1)))
    wants = [_chain(clips, ops, bank, plan, first + i) for i in range(3)]
    assert not torch.equal(wants[0][0], wants[1][0])
    plan.seek(first).on('cuda')
    for i in range(2):                                               # two steps: the decode, then the whole input side
        d = clips.batch_draw_host(plan, first + i)
        (got, record) = _record(ops, lambda: ops.png_decode_bank_drawn_u8(bank, plan))
        assert record == ['png_decode_bank_drawn_u8'] and tuple(got[0].shape) == (12, 130, 111, 3)
        assert _equal(got[:3], _draw(refs, d.index.tolist(), bank.n, (130, 111))) and got[3].index.cpu().tolist() == d.index.tolist()
        plan.seek(first + i)
        u8, view, label, status = ops.draw_clips(bank, plan, S)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (4, 3, S, S, 3)
        assert _equal((u8, view, label, status), wants[i]) and plan.step == first + i + 1
    other = clips.BatchPlan(bank.sizes[:11], [(0, 5, 0)], T=3, B=4).on('cuda')
    with pytest.raises(ValueError, match='png_decode_bank_drawn_u8: the plan was built for a bank of 11 places, this one has 13'):
        ops.png_decode_bank_drawn_u8(bank, other)
    # captured: every replay gives the next step's batch
    out = torch.zeros((4, 3, S, S, 3), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.draw_clips(bank, plan, S, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    plan.seek(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        u8, view, label, status = ops.draw_clips(bank, plan, S, out=out)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and plan.step == first and u8.data_ptr() == out.data_ptr()
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert _equal((out, view, label, status), wants[i]), i
        assert plan.step == first + i + 1


def test_the_crop(pkg):
    from istvt_amd import clips, ops
    files, bank = K.damaged_files(clips), K.damaged_bank(clips)
    n = bank.n
    index = [0, 3, n - 2, 0, 5]
    batch = clips.png_batch([files[i] for i in index], bands='index')
    got = ops.decode_frames(bank, S, index=torch.tensor(index, device='cuda'))
    assert tuple(got.shape) == (5, S, S, 3) and torch.equal(got, ops.decode_frames(batch, S)) and bool(got[0].any())
    boxes = torch.tensor([[1, 2, 15, 12]] * 5, dtype=torch.int32)
    assert torch.equal(ops.decode_frames(bank, S, boxes, index=index), ops.decode_frames(batch, S, boxes))
    out = ops.decode_frames(bank, S, index=[0, n, -1])               # a place outside the bank is black
    assert torch.equal(out[0], got[0]) and not bool(out[1:].any())
    assert not bool(ops.decode_frames(bank, S, boxes[:3], index=[n, 0, -1])[[0, 2]].any())


@pytest.mark.parametrize('first_byte', [2 ** 31 + 4096, 2 ** 32 + 16], ids=['2^31+4096', '2^32+16'])
def test_beyond_2_31_bytes(pkg, first_byte):
    """three small files behind first_byte bytes that are allocated, never written and never read: every byte offset of the
    bank's files is beyond what an int32 holds"""
    from istvt_amd import clips, ops
    files = K.small_files(clips)
    bank = clips.png_bank(files, first_byte=first_byte)
    assert min(K.base_of(r) for r in bank.images.tolist()) >= first_byte and bank.first_byte + bank.nbytes > 2 ** 31
    index = [2, 0, 1, 1, 0, 2, 2, -1, 3]
    want = clips.png_bank_decode_host(bank, index)
    assert want[2].tolist() == [0] * 7 + [8, 8]
    got = ops.png_decode_bank_u8(bank, torch.tensor(index, dtype=torch.int32, device='cuda'))
    assert int(bank.on(got[0].device).data.numel()) == first_byte + bank.nbytes
    assert _equal(got, want)
    assert _equal(want, clips.png_bank_decode_host(clips.png_bank(files), index))
    bank._on.clear()
    del got
    torch.cuda.empty_cache()
