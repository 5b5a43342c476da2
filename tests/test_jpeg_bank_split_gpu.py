"""The split decode of a JPEG bank (DESIGN.md "JPEG bank, split") on a real MI355X: a bank with a split against the same bank
without one, byte for byte -- frames, sizes, status and the coefficients in the scratch; the state rows at their stride per
drawn segment against the host model clips.jpeg_split_host; row-restart and restart-less files of all four layouts in one
bank; indices outside, empty places and damaged files; what the call writes and what it leaves alone (sentinels around every
buffer, a scratch filled with FF and with 00); the device ingest with and without a bound on the segment length; the drawn
decode and draw_clips, eager and as a replayed graph of one chain.  tools/jpeg_bank_split_check.cpp, the same row arithmetic
and plan under AddressSanitizer and UBSan on the host, has passed before the kernel ran on a device with the second
addressing: DESIGN.md has the command and its counts."""
import os
import re

import numpy as np
import pytest
import torch

from test_jpeg_split_cpu import _smooth
from test_jpeg_split_gpu import Guarded

pytestmark = pytest.mark.gpu

S = 16


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def j2(golden_dir):
    return np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))


@pytest.fixture(scope='module')
def sound(pkg, j2):
    from istvt_amd import clips
    return clips.jpeg_bank([bytes(j2['file_' + n]) for n in j2['names'].tolist()])


@pytest.fixture(scope='module')
def mixed(pkg, golden_dir):
    """row-restart and restart-less encoder files of all four layouts and every ninth recorded layout file, in one bank"""
    from istvt_amd import clips
    j3 = np.load(os.path.join(golden_dir, 'J3_jpeg_layouts.npz'))
    files = [clips.jpeg_encode_host(_smooth(33, 50, 20 + k), 40 + 7 * k, restart_interval=(0, 'row')[k % 2], layout=layout)
             for k, layout in enumerate(clips.JPEG_LAYOUTS + clips.JPEG_LAYOUTS[::-1])]
    files += [bytes(j3['file_' + n]) for n in j3['names'].tolist()[::9]]
    bank = clips.jpeg_bank(files, 'all')
    assert bank.seg_max > 1 and set(bank.images[:, 19].tolist()) == {0, 1, 2} and 1 in bank.images[:, 17].tolist()
    return bank


def _buffers(clips, bank, m, fill=0x11):
    return (torch.full((clips.jpeg_bank_scratch_bytes(bank, m),), fill, dtype=torch.uint8, device='cuda'),
            torch.empty((m, 2), dtype=torch.int32, device='cuda'), torch.empty((m,), dtype=torch.int32, device='cuda'))


def _default(clips, ops, bank, index):
    """the bank's call without a split -> (frames, sizes, status, the coefficients of its scratch)"""
    plain = bank.with_split(None)
    m = len(index)
    bufs = _buffers(clips, plain, m)
    got = ops.jpeg_decode_indexed_u8(plain, index, buffers=bufs)
    return got + (bufs[0][:128 * m * bank.block_stride],)


def _same_as_default(clips, ops, bank, index, want, what=None):
    """the split bank's call against `want` of _default -> its scratch"""
    m = len(index)
    bufs = _buffers(clips, bank, m)
    got = ops.jpeg_decode_indexed_u8(bank, index, buffers=bufs)
    for name, g, w in zip(('frames', 'sizes', 'status', 'coefficients'), got + (bufs[0][:128 * m * bank.block_stride],), want):
        assert torch.equal(g, w), (what, bank.split, name)
    return bufs[0]


def test_same_bytes_as_the_default_bank_call(pkg, sound):
    """All sound recorded files at chunk 16 and 128, and at 160: the set's longest segment (a noise fixture of one segment)
    makes more than 64 chunks of 128 bytes, so the third size is the one that takes the 64-lane kernel."""
    from istvt_amd import clips, ops
    n = sound.n
    banks = [sound.with_split(c) for c in (16, 128, 160)]
    assert [b.chunk_rows for b in banks] == [256, -(-sound.seg_bytes_max // 128), -(-sound.seg_bytes_max // 160)]
    assert banks[0].chunk_rows > 64 and banks[1].chunk_rows > 64 and banks[2].chunk_rows <= 64      # 256 lanes, 256, 64
    g = torch.Generator().manual_seed(5)
    draws = {'arange': list(range(n)), 'reversed': list(range(n))[::-1], 'all equal': [7] * 9, 'one': [n - 1],
             'random': torch.randint(0, n, (37,), generator=g).tolist()}
    assert len(set(draws['random'])) < 37
    ops.kernel_profile = []
    try:
        for name, index in draws.items():
            want = _default(clips, ops, sound, torch.tensor(index, dtype=torch.int32, device='cuda'))
            assert not bool(want[2].any())
            for dtype in (torch.int32, torch.int64):
                for bank in banks:
                    _same_as_default(clips, ops, bank, torch.tensor(index, dtype=dtype, device='cuda'), want, (name, dtype))
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == (['jpeg_decode_indexed_u8'] + ['jpeg_decode_indexed_split_u8'] * 6) * 5
    # a host list is uploaded, as for the default call
    got = ops.jpeg_decode_indexed_u8(banks[1], draws['random'])
    assert all(torch.equal(a, b) for a, b in zip(got, ops.jpeg_decode_indexed_u8(sound, draws['random'])))


def test_state_rows(pkg):
    """Encoder files without restart markers at 4:2:0 and 4:4:4 behind a row-restart file, so that seg_max > 1 and no file
    starts at byte 0 of the bank: rows (j * seg_max + s) * chunk_rows + lane, lane < S, are the host model's, rebased to the
    file's place in the bank.  The 4:4:4 scan is longer than 256 chunks of 16 bytes: there the chunk grows."""
    from istvt_amd import clips, ops
    data = [clips.jpeg_encode_host(_smooth(24, 40, 3), 75, '420', 'row'), clips.jpeg_encode_host(_smooth(64, 80, 1), 75, '420', 0),
            clips.jpeg_encode_host(_smooth(64, 80, 1), 90, '444', 0)]
    headers = [clips.jpeg_parse(d) for d in data]
    assert [len(h.segments) for h in headers] == [2, 1, 1] and headers[2].segments[0][1] - headers[2].segments[0][0] > 256 * 16
    plain = clips.jpeg_bank(headers)
    index = [2, 0, 1, 2]
    m = len(index)
    want = _default(clips, ops, plain, torch.tensor(index, device='cuda'))
    assert not bool(want[2].any())
    for chunk in (16, 32, 64):
        bank = plain.with_split(chunk)
        R = bank.chunk_rows
        assert R == min(256, -(-bank.seg_bytes_max // chunk)) and (chunk != 16 or R == 256)
        scratch = _same_as_default(clips, ops, bank, torch.tensor(index, device='cuda'), want)
        at = clips.jpeg_bank_scratch_bytes(plain, m)
        at = -(-at // 16) * 16
        rows = scratch[at:].view(torch.int32).view(m * bank.seg_max, R, 8).cpu()
        for i in set(index):
            host = clips.jpeg_split_host(headers[i], chunk)
            shift = int(plain.segments[int(plain.images[i, 16]), 1]) - headers[i].segments[0][0]
            for j in (j for j, v in enumerate(index) if v == i):
                for s, seg in enumerate(host.segments):
                    expect = torch.tensor(seg.rows, dtype=torch.int32)
                    expect[:, 0] += shift
                    assert len(seg.rows) == clips.jpeg_split_chunks(headers[i].segments[s][1] - headers[i].segments[s][0], chunk)[1] <= R
                    assert torch.equal(rows[j * bank.seg_max + s, :len(seg.rows)], expect), (chunk, i, j, s)
        assert chunk != 16 or len(clips.jpeg_split_host(headers[2], 16).segments[0].rows) < 256      # capped: the chunk grew


def test_a_mixed_bank(pkg, mixed):
    from istvt_amd import clips, ops
    n, seg_max = mixed.n, mixed.seg_max
    index = list(range(n)) + [3, 0, n - 1, 3]
    m = len(index)
    idx = torch.tensor(index, device='cuda')
    want = _default(clips, ops, mixed, idx)
    assert not bool(want[2].any())
    real = mixed.images[:, 17][index]
    for chunk in (16, 128):
        bank = mixed.with_split(chunk)
        scratch = _same_as_default(clips, ops, bank, idx, want)
        words = scratch[192 * m * bank.block_stride:][:4 * (m * seg_max + m)].view(torch.int32).cpu()
        seg_status = words[:m * seg_max].view(m, seg_max)
        padded = torch.arange(seg_max).view(1, -1) >= real.view(-1, 1)
        assert bool(padded.any()) and bool((seg_status[padded] == 2).all()) and bool((seg_status[~padded] == 0).all())
        assert not bool(words[m * seg_max:].any())
    assert torch.equal(ops.decode_frames(mixed.with_split(32), S, index=index), ops.decode_frames(mixed, S, index=index))


def test_statuses(pkg, j2):
    from istvt_amd import clips, ops
    # the three damaged recorded files and one cut in the middle of its scan between sound neighbours; indices outside
    pick = ['24x40_s2_q75', 'damaged_cut', '17x33_s0_q95', 'damaged_code', '33x70_s2_q75_rb1', 'damaged_run', '16x16_s2_q30']
    whole = bytes(j2['file_33x70_s2_q75'])
    hd = clips.jpeg_parse(whole)
    assert len(hd.segments) == 1
    cut = whole[:hd.segments[0][0] + (hd.segments[0][1] - hd.segments[0][0]) * 3 // 5]
    data = [bytes(j2['file_' + k]) for k in pick] + [cut, bytes(j2['file_24x40_s2_q75'])]
    plain = clips.jpeg_bank(data)
    n = len(data)
    index = list(range(n)) + [-1, 3, n, 1, 2 ** 31 - 1]
    idx = torch.tensor(index, dtype=torch.int64, device='cuda')
    want = _default(clips, ops, plain, idx)
    assert want[2].tolist() == [0, 1, 0, 2, 0, 3, 0, 1, 0, 4, 2, 4, 1, 4]
    for chunk in (16, 37, 128):
        _same_as_default(clips, ops, plain.with_split(chunk), idx, want)
    # an empty place of an ingested bank: the encoder refused quality -3
    frames = torch.stack([_smooth(16, 16, s) for s in (7, 8, 9)]).cuda()
    jf = ops.jpeg_encode_u8(frames, torch.tensor([80, -3, 50], dtype=torch.int32, device='cuda'), restart_interval=0, layout='grey',
                            checked=True)
    ingested = clips.JpegBank.from_encoded(jf)
    idx = torch.tensor([2, 1, 0, 1, 3], device='cuda')
    want = _default(clips, ops, ingested, idx)
    assert want[2].tolist() == [0, 5, 0, 5, 4]
    assert ingested.seg_bytes_max is None and ingested.with_split(16).chunk_rows == 256
    for chunk in (16, 64):
        _same_as_default(clips, ops, ingested.with_split(chunk), idx, want)


def test_guards_and_a_scratch_that_held_anything(pkg, mixed):
    from istvt_amd import clips, ops
    bank = mixed.with_split(32)
    n = bank.n
    index = [5, 0, n, 9, 5, -1, n - 1, 2, 7]
    m = len(index)
    idx = torch.tensor(index, dtype=torch.int32, device='cuda')
    canvas = (bank.Hmax + 1, bank.Wmax + 3)
    want = ops.jpeg_decode_indexed_u8(mixed, idx, canvas=canvas)
    assert want[2].tolist() == [0, 0, 4, 0, 0, 4, 0, 0, 0]
    results = []
    for fill in (0xFF, 0x00):
        out = Guarded((m,) + canvas + (3,), torch.uint8, 1)
        scratch = Guarded((clips.jpeg_bank_scratch_bytes(bank, m),), torch.uint8)
        sizes, status = Guarded((m, 2), torch.int32), Guarded((m,), torch.int32)
        assert out.t.data_ptr() % 2 == 1
        scratch.t.fill_(fill)
        out.t.fill_(0x5A)
        got = ops.jpeg_decode_indexed_u8(bank, idx, canvas=canvas, out=out.t, buffers=(scratch.t, sizes.t, status.t))
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.t.data_ptr() and got[1] is sizes.t and got[2] is status.t
        assert out.intact() and scratch.intact() and sizes.intact() and status.intact(), fill
        results.append([t.cpu().clone() for t in got])
    for a, b, w in zip(results[0], results[1], want):
        assert torch.equal(a, b) and torch.equal(a, w.cpu())
    # the scratch of the bank without a split is too small for the split layout, and the refusal says so
    small = _buffers(clips, mixed, m)
    assert small[0].numel() < clips.jpeg_bank_scratch_bytes(bank, m)
    with pytest.raises(RuntimeError, match=r'buffers = \(uint8 scratch of %d bytes for the split layout \(bank.split = 32: %d state '
                                           r'rows per segment\)' % (clips.jpeg_bank_scratch_bytes(bank, m), bank.chunk_rows)):
        ops.jpeg_decode_indexed_u8(bank, idx, buffers=small)
    ops.jpeg_decode_indexed_u8(mixed, idx, buffers=small)           # the default call takes them
    # the entry itself refuses its scalars before any launch
    import ctypes
    from istvt_amd import _lib
    d = bank.on(idx.device)
    big = _buffers(clips, bank, m)
    out = torch.full((m, bank.Hmax, bank.Wmax, 3), 0xA5, dtype=torch.uint8, device='cuda')
    args = _lib.JpegDecodeArgs(
        bytes=d.data.data_ptr(), nbytes=bank.nbytes, images=d.images.data_ptr(), images_host=idx.data_ptr(),
        segments=d.segments.data_ptr(), segments_host=None, qtabs=d.qtabs.data_ptr(), htabs=d.htabs.data_ptr(),
        scratch=big[0].data_ptr(), scratch_bytes=big[0].numel(), out=out.data_ptr(), sizes=big[1].data_ptr(),
        status=big[2].data_ptr(), stream=None, n=bank.n, nseg=bank.nseg, nq=bank.nq, nh=bank.nh, Hc=bank.Hmax, Wc=bank.Wmax)
    entry = _lib.lib().istvt_jpeg_decode_indexed_split_u8
    geometry = (m, bank.seg_max, bank.block_stride, bank.Hmax, bank.Wmax)
    R = bank.chunk_rows
    for scalars in ((15, R, bank.seg_bytes_max), (32, 0, bank.seg_bytes_max), (32, 257, bank.seg_bytes_max),
                    (32, R + 1, bank.seg_bytes_max)):       # the last: more rows than the scratch holds
        assert entry(ctypes.byref(args), *geometry, *scalars) == -3, scalars
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert entry(ctypes.byref(args), *geometry, 32, R, bank.seg_bytes_max) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.jpeg_decode_indexed_u8(mixed, idx)[0])


def test_ingest(pkg):
    from istvt_amd import clips, ops
    frames = torch.stack([_smooth(40, 56, 30 + k) for k in range(5)]).cuda()
    quality = torch.tensor([60, 92, 75, 92, 35], dtype=torch.int32)
    jf = ops.jpeg_encode_u8(frames, quality, restart_interval=0)
    n = len(quality)
    bank = clips.JpegBank.from_encoded(jf).with_split(64)
    assert bank.split == 64 and bank.seg_bytes_max is None and bank.chunk_rows == 256 and bank.seg_max == 1
    got = ops.jpeg_decode_indexed_u8(bank, torch.arange(n, device='cuda'))
    files = jf.files()
    want = ops.jpeg_decode_u8(files)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and not bool(want[2].any())
    # a bound one byte below the longest scan: exactly the places with a longer scan are refused, by the plan
    lengths = [hd.segments[0][1] - hd.segments[0][0] for hd in map(clips.jpeg_parse, files)]
    longest = max(lengths)
    over = [v == longest for v in lengths]
    assert 0 < sum(over) < n
    bounded = clips.JpegBank.from_encoded(jf, seg_bytes_max=longest - 1).with_split(64)
    assert bounded.seg_bytes_max == longest - 1 and bounded.chunk_rows == -(-(longest - 1) // 64) < 256
    index = [0, 1, 2, 3, 4, 1, 0]
    m = len(index)
    out = Guarded((m, 40, 56, 3), torch.uint8, 1)
    scratch = Guarded((clips.jpeg_bank_scratch_bytes(bounded, m),), torch.uint8)
    sizes, status = Guarded((m, 2), torch.int32), Guarded((m,), torch.int32)
    scratch.t.fill_(0xEE)
    frames_b, sizes_b, status_b = ops.jpeg_decode_indexed_u8(bounded, torch.tensor(index, device='cuda'), out=out.t,
                                                             buffers=(scratch.t, sizes.t, status.t))
    torch.cuda.synchronize()
    assert out.intact() and scratch.intact() and sizes.intact() and status.intact()
    assert status_b.tolist() == [5 if over[i] else 0 for i in index]
    for j, i in enumerate(index):
        if over[i]:
            assert int(frames_b[j].max()) == 0 and sizes_b[j].tolist() == [0, 0]
        else:
            assert torch.equal(frames_b[j], want[0][i]) and sizes_b[j].tolist() == [40, 56]
    # no state row of a refused place is written
    at = -(-clips.jpeg_bank_scratch_bytes(bounded.with_split(None), m) // 16) * 16
    rows = scratch.t[at:].view(m, bounded.chunk_rows * 32)
    for j, i in enumerate(index):
        assert bool((rows[j] == 0xEE).all()) == over[i], j
    exact = clips.JpegBank.from_encoded(jf, seg_bytes_max=longest).with_split('auto')
    assert exact.split == (128 if longest > clips.JPEG_SPLIT_AUTO_BYTES else None)
    assert all(torch.equal(g, w) for g, w in zip(ops.jpeg_decode_indexed_u8(exact, torch.arange(n, device='cuda')), want))


@pytest.fixture(scope='module')
def banked(pkg):
    """test_batch_draw_gpu's bank with the restart intervals 0, 'row', 0: 12 host-encoded files, places 0..4 of 24 x 40 and
    5..11 of 17 x 33, place 7 emptied -> (bank, its split twin, the arguments of a plan over its two videos)"""
    from istvt_amd import clips
    files = [clips.jpeg_encode_host(_smooth(*((24, 40) if i < 5 else (17, 33)), 60 + i), 70 + 2 * i,
                                    restart_interval=(0, 'row', 0)[i % 3]) for i in range(12)]
    bank = clips.jpeg_bank(files)
    bank.images[7, 17] = 0
    base = [[0, 0, h, w] for h, w in bank.sizes]
    base[2], base[9] = [3, 5, 18, 30], [1, 2, 15, 20]
    split = bank.with_split(16)
    assert split.images is bank.images and split.seg_max > 1
    return bank, split, dict(videos=[(0, 5, 0), (5, 7, 1)], T=3, B=6, base=torch.tensor(base, dtype=torch.int32), K=16, seed=77)


def test_decode_drawn(pkg, banked):
    from istvt_amd import clips, ops
    bank, split, args = banked
    plan = clips.BatchPlan(bank, **args)
    step = next(s for s in range(500) if 7 in clips.batch_draw_host(plan, s).index.tolist())
    plan.seek(step).on('cuda')
    d = clips.batch_draw_host(plan, step)
    ops.kernel_profile = []
    try:
        frames, sizes, status, draw = ops.jpeg_decode_drawn_u8(split, plan)
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_decode_drawn_split_u8'] and plan.step == step + 1
    want = ops.jpeg_decode_indexed_u8(bank, d.index)
    assert torch.equal(draw.index.cpu(), d.index) and tuple(frames.shape) == (18, 24, 40, 3)
    assert torch.equal(frames, want[0]) and torch.equal(sizes, want[1]) and torch.equal(status, want[2])
    assert set(status.cpu().tolist()) == {0, 5}


def _dot_edges(path):
    text = open(path).read()
    return re.findall(r'"?([\w.]+)"?\s*->\s*"?([\w.]+)"?', text), text


def test_draw_clips_eager_and_as_a_graph(pkg, banked, tmp_path):
    from istvt_amd import clips, ops
    bank, split, args = banked
    plan = clips.BatchPlan(bank, **args)
    s = 4
    plan.seek(s).on('cuda')
    wants = [[t.cpu().clone() for t in ops.draw_clips(bank, plan, S)] for _ in range(3)]       # steps s, s + 1, s + 2
    assert plan.step == s + 3 and not torch.equal(wants[0][0], wants[1][0])
    plan.seek(s)
    for i in range(2):                                              # eager, at two steps
        got = ops.draw_clips(split, plan, S)
        assert all(torch.equal(g.cpu(), w) for g, w in zip(got, wants[i])), i
    out = torch.zeros((6, 3, S, S, 3), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.draw_clips(split, plan, S, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    plan.seek(s)
    graph = torch.cuda.CUDAGraph(keep_graph=True)                   # the captured graph stays, for the dump below
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        u8, view, label, status = ops.draw_clips(split, plan, S, out=out)
    graph.instantiate()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and plan.step == s and u8.data_ptr() == out.data_ptr()      # captured, not run
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = (out.cpu(), view.cpu(), label.cpu(), status.cpu())
        assert all(torch.equal(g, w) for g, w in zip(got, wants[i])), i
        assert plan.step == s + i + 1
    dot = str(tmp_path / 'draw_clips_graph.dot')
    graph.debug_dump(dot)
    edges, text = _dot_edges(dot)
    nodes = {a for e in edges for a in e}
    assert len(nodes) >= 5, text                                    # the draw, the plan, the split kernel, IDCT, canvas at least
    assert len(edges) == len(nodes) - 1, text
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges), text   # no fork, no join
