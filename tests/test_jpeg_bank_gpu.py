"""The JPEG bank (DESIGN.md "JPEG bank") on a real MI355X: ops.jpeg_decode_indexed_u8 against the default call on the files
the index names and against the definition clips.jpeg_bank_decode_host, byte for byte; indices outside the bank; a damaged
file; what the call writes and what it leaves alone (sentinel bytes around every buffer, a scratch filled with ones and
with zeros); a captured graph replayed on changed index contents; the device ingest of the encoder's result against the
host parse of the same files; banks joined on the device; the crop.  tools/jpeg_bank_check.cpp, csrc/jpeg_bank_scan.h under
AddressSanitizer and UBSan on the host, has passed before any of these kernels ran on a device: DESIGN.md has the command
and its counts."""
import itertools

import pytest
import torch

from test_jpeg_split_cpu import _smooth
from test_jpeg_split_gpu import Guarded

pytestmark = pytest.mark.gpu

CANVAS = (40, 64)


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def mixed(pkg):
    """24 host-encoded files: four sizes x four layouts, restart interval 0, 1 and 'row', standard and optimised tables ->
    (files, their bank, the definition's frames, sizes and status of every file on CANVAS: decoded on the host once)"""
    from istvt_amd import clips
    sizes = ((8, 8), (17, 23), (40, 24), (33, 64))
    files = []
    for k, ((h, w), layout) in enumerate(itertools.product(sizes, clips.JPEG_LAYOUTS)):
        files.append(clips.jpeg_encode_host(_smooth(h, w, 10 + k), 55 + 2 * k, restart_interval=(0, 1, 'row')[k % 3],
                                            optimize=k % 2 == 1, layout=layout))
    for k, ((h, w), layout) in enumerate(list(itertools.product(sizes, clips.JPEG_LAYOUTS))[1::2]):
        files.append(clips.jpeg_encode_host(_smooth(h, w, 40 + k), 90, restart_interval=('row', 0, 1)[k % 3],
                                            optimize=k % 2 == 0, layout=layout))
    assert len(files) == 24
    bank = clips.jpeg_bank(files, 'all')
    assert bank.seg_max == 40 and (bank.Hmax, bank.Wmax) == CANVAS and set(bank.images[:, 19].tolist()) == {0, 1, 2}
    ref = clips.jpeg_bank_decode_host(bank, list(range(len(files))), CANVAS)
    assert not bool(ref[2].any())
    return files, bank, ref


def _draw(ref, index, n):
    """the definition's result for `index` from the per-file result `ref`: places outside [0, n) are zero with status 4"""
    frames, sizes, status = ref
    idx = torch.as_tensor(index, dtype=torch.int64)
    ok = (idx >= 0) & (idx < n)
    at = idx.clamp(0, n - 1)
    keep = ok.view(-1, 1, 1, 1)
    return (frames[at] * keep, sizes[at] * ok.view(-1, 1).int(), torch.where(ok, status[at], torch.full_like(status[at], 4)))


def _equal(got, want):
    return all(torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want))


def test_index_semantics(pkg, mixed):
    from istvt_amd import ops
    files, bank, ref = mixed
    n = len(files)
    g = torch.Generator().manual_seed(5)
    draws = {'arange': list(range(n)), 'reversed': list(range(n))[::-1], 'all equal': [7] * 9, 'one': [n - 1],
             'random': torch.randint(0, n, (37,), generator=g).tolist()}
    assert len(set(draws['random'])) < 37
    for name, index in draws.items():
        want = ops.jpeg_decode_u8([files[i] for i in index], canvas=CANVAS, layouts='all')
        assert _equal(want, _draw(ref, index, n)), name             # the default call is the definition's, as it always was
        for dtype in (torch.int32, torch.int64):
            got = ops.jpeg_decode_indexed_u8(bank, torch.tensor(index, dtype=dtype, device='cuda'), canvas=CANVAS)
            assert got[0].dtype == torch.uint8 and tuple(got[0].shape) == (len(index),) + CANVAS + (3,)
            assert _equal(got, want), (name, dtype)
    # a host list and a host tensor are uploaded; the default canvas is the bank's largest image
    for index in (draws['random'], torch.tensor(draws['random'], dtype=torch.int32)):
        assert _equal(ops.jpeg_decode_indexed_u8(bank, index), _draw(ref, draws['random'], n))


def test_indices_outside_the_bank(pkg, mixed):
    from istvt_amd import clips, ops
    files, bank, ref = mixed
    n = len(files)
    index = [3, -1, 0, n, 23, n + 1, 22]
    want = _draw(ref, index, n)
    assert want[2].tolist() == [0, 4, 0, 4, 0, 4, 0] and want[1][1].tolist() == [0, 0] and int(want[0][3].max()) == 0
    for dtype in (torch.int32, torch.int64):
        assert _equal(ops.jpeg_decode_indexed_u8(bank, torch.tensor(index, dtype=dtype, device='cuda'), canvas=CANVAS), want)
    # values no int32 holds: 2^32 + 3 is not file 3
    wide = [2 ** 32 + 3, 5, -2 ** 40, 2 ** 31, -2 ** 31 - 1]
    got = ops.jpeg_decode_indexed_u8(bank, torch.tensor(wide, dtype=torch.int64, device='cuda'), canvas=CANVAS)
    assert _equal(got, _draw(ref, wide, n)) and got[2].tolist() == [4, 0, 4, 4, 4]
    assert _equal(got, clips.jpeg_bank_decode_host(bank, wide, CANVAS))
    with pytest.raises(ValueError, match=r'place 0 has status 4'):
        clips.check_jpeg_bank_status(got[2])


def test_a_damaged_file_and_what_the_call_leaves_alone(pkg, mixed):
    """A file cut in the middle of its scan among sound ones and indices outside the bank, decoded into buffers with
    sentinels around them, from a scratch filled with FF and with 00: its places report status 1 as the default call does,
    the same bytes come out both times, and nothing outside the buffers is written."""
    from istvt_amd import clips, ops
    files, _, _ = mixed
    hd = clips.jpeg_parse(files[14], 'all')                       # 33 x 64 at 4:2:2, a restart marker per MCU row
    assert (hd.H, hd.W) == (33, 64) and len(hd.segments) > 2
    cut = files[14][:(hd.segments[1][0] + hd.segments[1][1]) // 2]
    some = files[:6] + [cut] + files[20:]
    bank = clips.jpeg_bank(some, 'all')
    n = len(some)
    index = [6, 0, 9, 6, -1, 5, n, 7, 1]
    sound = [j for j, i in enumerate(index) if 0 <= i < n]
    want = ops.jpeg_decode_u8([some[index[j]] for j in sound], canvas=CANVAS, layouts='all')
    assert want[2].tolist() == [1, 0, 0, 1, 0, 0, 0]
    m = len(index)
    idx = torch.tensor(index, dtype=torch.int32, device='cuda')
    results = []
    for fill in (0xFF, 0x00):
        out = Guarded((m,) + CANVAS + (3,), torch.uint8, 1)
        scratch = Guarded((clips.jpeg_bank_scratch_bytes(bank, m),), torch.uint8)
        sizes, status = Guarded((m, 2), torch.int32), Guarded((m,), torch.int32)
        assert out.t.data_ptr() % 2 == 1
        scratch.t.fill_(fill)
        out.t.fill_(0x5A)
        got = ops.jpeg_decode_indexed_u8(bank, idx, canvas=CANVAS, out=out.t, buffers=(scratch.t, sizes.t, status.t))
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.t.data_ptr()
        assert out.intact() and scratch.intact() and sizes.intact() and status.intact(), fill
        results.append([t.cpu().clone() for t in got])
    assert _equal(results[0], results[1])
    frames, sizes, status = results[0]
    assert torch.equal(frames[sound], want[0].cpu()) and torch.equal(sizes[sound], want[1].cpu())
    assert torch.equal(status[sound], want[2].cpu())
    assert status.tolist() == [1, 0, 0, 1, 4, 0, 4, 0, 0] and sizes[4].tolist() == sizes[6].tolist() == [0, 0]
    assert int(frames[4].max()) == 0 and int(frames[6].max()) == 0
    assert _equal(results[0], clips.jpeg_bank_decode_host(bank, index, CANVAS))
    # a scratch one byte short and a canvas smaller than the bank's largest image are refused
    small = torch.empty(clips.jpeg_bank_scratch_bytes(bank, m) - 1, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='buffers = '):
        ops.jpeg_decode_indexed_u8(bank, idx, buffers=(small, results[0][1].cuda(), results[0][2].cuda()))
    with pytest.raises(ValueError, match='the canvas must hold every image of the bank'):
        ops.jpeg_decode_indexed_u8(bank, idx, canvas=(CANVAS[0] - 1, CANVAS[1]))


def test_captured_in_a_graph(pkg, mixed):
    """one call with out= and buffers= captured on one stream and replayed on three contents of the same index tensor: a
    call that synchronised or read the index on the host could not be captured, or would replay the first draw"""
    from istvt_amd import clips, ops
    files, bank, ref = mixed
    n, m = len(files), 12
    g = torch.Generator().manual_seed(9)
    draws = [torch.randint(0, n, (m,), generator=g).tolist() for _ in range(3)] + [[n, 4, -1] + [2] * (m - 3)]
    idx = torch.tensor(draws[0], dtype=torch.int32, device='cuda')
    out = torch.zeros((m,) + CANVAS + (3,), dtype=torch.uint8, device='cuda')
    buffers = (torch.empty(clips.jpeg_bank_scratch_bytes(bank, m), dtype=torch.uint8, device='cuda'),
               torch.zeros((m, 2), dtype=torch.int32, device='cuda'), torch.zeros((m,), dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.jpeg_decode_indexed_u8(bank, idx, canvas=CANVAS, out=out, buffers=buffers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.jpeg_decode_indexed_u8(bank, idx, canvas=CANVAS, out=out, buffers=buffers)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                      # captured, not run
    for draw in draws[1:]:
        idx.copy_(torch.tensor(draw, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert _equal((out, buffers[1], buffers[2]), _draw(ref, draw, n)), draw


def _noisy(h, w, seed):
    """a gradient under uniform noise of +-40: scans long enough to span tiles at 224 x 224"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    base = torch.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (h + w)], -1)
    return (base + torch.randint(-40, 41, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)


# (H, W, layout, restart interval, qualities, seeds); the seeds of the 224 x 224 call were picked on the host with
# clips.jpeg_encode_host, so that test_ingest's condition on its inputs holds
INGEST_CALLS = [(16, 16, '420', 1, (75, 0, 90, 35), (1, 2, 3, 4)), (16, 16, '444', 'row', (60, 95), (5, 6)),
                (16, 16, 'grey', 0, (80, 50, -3), (7, 8, 9)), (24, 40, '422', 1, (85, 40), (10, 11)),
                (24, 40, '420', 'row', (70, 99), (12, 13)), (24, 40, 'grey', 1, (65, 90), (14, 15)),
                (24, 40, '444', 0, (88,), (16,)), (224, 224, '444', 1, (95, 95, 95), (6, 13, 0))]


def _straddles(clips, files):
    """which boundaries the restart markers and the stuffed FF 00 pairs of the files lie across, counted from each scan's
    first byte as the device's lanes count them: {('rst' | 'ff', 16 | 4096)}"""
    found = set()
    for f in filter(None, files):
        hd = clips.jpeg_parse(f, 'all')
        begin, end = hd.segments[0][0], hd.segments[-1][1]
        rst = [e - begin for _, e in hd.segments[:-1]]
        ff = [p - begin for p in range(begin, end - 1) if f[p] == 0xFF and f[p + 1] == 0]
        for span in (clips.JPEG_SCAN_LANE_BYTES, clips.JPEG_SCAN_TILE_BYTES):
            found |= {('rst', span)} if any(r % span == span - 1 for r in rst) else set()
            found |= {('ff', span)} if any(r % span == span - 1 for r in ff) else set()
    return found


def test_ingest(pkg):
    from istvt_amd import clips, ops
    straddles = set()
    for H, W, layout, ri, quality, seeds in INGEST_CALLS:
        key = (H, W, layout, ri)
        frames = torch.stack([_noisy(H, W, s) for s in seeds]).cuda()
        jf = ops.jpeg_encode_u8(frames, torch.tensor(quality, dtype=torch.int32, device='cuda'), restart_interval=ri,
                                layout=layout, checked=True)
        bank = clips.JpegBank.from_encoded(jf)
        n = len(seeds)
        assert bank.n == n and bank.device == frames.device and bank.data is None and bank.sizes == [(H, W)] * n
        # only now the host looks: the files, parsed, are what the device tables must say
        files = jf.files(check=False)
        fine = [i for i, q in enumerate(quality) if q > 0]
        assert [bool(f) for f in files] == [q > 0 for q in quality]
        straddles |= _straddles(clips, files)
        batch = clips.jpeg_batch([files[i] for i in fine], 'all')
        dev = bank.on(frames.device)
        offsets = jf.offsets.cpu().tolist()
        images, segments, qtabs = dev.images.cpu(), dev.segments.cpu(), dev.qtabs.cpu()
        assert bank.seg_max == int(batch.images[:, 17].max()) and bank.block_stride >= int(batch.images[:, 18].max()), key
        assert tuple(segments.shape) == (n * bank.seg_max, 5) and torch.equal(dev.htabs.cpu(), batch.htabs), key
        for k, i in enumerate(fine):
            hd = clips.jpeg_parse(files[i], 'all')
            mine, theirs = images[i], batch.images[k]
            cols = [0, 1, 2, 3, 4, 17, 18, 19]                     # geometry, segment count, blocks, layout
            assert torch.equal(mine[cols], theirs[cols]) and torch.equal(mine[8:14], theirs[8:14]), (key, i)
            assert torch.equal(qtabs[mine[5:8].long()], batch.qtabs[theirs[5:8].long()]), (key, i)
            rows = segments[int(mine[16]):int(mine[16]) + int(mine[17])]
            want = batch.segments[int(theirs[16]):int(theirs[16]) + int(theirs[17])]
            assert torch.equal(rows[:, 3:], want[:, 3:]) and rows[:, 0].tolist() == [i] * len(rows), (key, i)
            # rebased to each file's start: the bank counts from the encoder's buffer, the batch from its packed scans
            assert (rows[:, 1:3] - offsets[i]).tolist() == [list(s) for s in hd.segments], (key, i)
            assert torch.equal(rows[:, 1:3] - rows[0, 1], want[:, 1:3] - want[0, 1]), (key, i)
        got = ops.jpeg_decode_indexed_u8(bank, torch.arange(n, device='cuda'))
        want = ops.jpeg_decode_u8([files[i] for i in fine], layouts='all')
        assert torch.equal(got[0][fine], want[0]) and torch.equal(got[1][fine], want[1]) and not bool(want[2].any()), key
        assert got[2].tolist() == [0 if q > 0 else 5 for q in quality], key
        for i in set(range(n)) - set(fine):
            assert int(images[i][17]) == 0 and int(got[0][i].max()) == 0 and got[1][i].tolist() == [0, 0], (key, i)
        if H <= 64:                                                 # (the host decoder takes seconds for a 224 x 224 file)
            assert _equal(got, clips.jpeg_bank_decode_host(files, list(range(n)), (H, W), layouts='all')), key
    # the condition on the inputs: a restart marker and a stuffed FF 00 across a lane's last byte and across a tile's
    assert straddles == {('rst', 16), ('rst', 4096), ('ff', 16), ('ff', 4096)}, straddles


def test_banks_joined_on_the_device(pkg):
    from istvt_amd import clips, ops
    a = torch.stack([_noisy(24, 40, s) for s in (21, 22, 23)]).cuda()
    b = torch.stack([_noisy(24, 40, s) for s in (24, 25)]).cuda()
    ja = ops.jpeg_encode_u8(a, torch.tensor([80, 55, 91], dtype=torch.int32), restart_interval='row', layout='422')
    jb = ops.jpeg_encode_u8(b, torch.tensor([70, 97], dtype=torch.int32), restart_interval=1, layout='grey')
    bank = clips.JpegBank.from_encoded(ja)
    with pytest.raises(RuntimeError, match="share memory with the bank's files"):      # the encoder's buffer is the bank's
        ops.jpeg_decode_indexed_u8(bank, [0], out=ja.data[:24 * 40 * 3].view(1, 24, 40, 3))
    bank.extend(clips.JpegBank.from_encoded(jb))
    assert bank.n == 5 and bank.seg_max == 15 and bank.nh == 6 and bank.nq == 10
    index = [4, 2, 3, 0, 1, 3, 5]
    got = ops.jpeg_decode_indexed_u8(bank, torch.tensor(index, device='cuda'))
    files = ja.files() + jb.files()
    want = ops.jpeg_decode_u8([files[i] for i in index[:-1]], layouts='all')
    assert _equal([t[:-1] for t in got], want) and got[2].tolist() == [0] * 6 + [4]
    # a host bank takes a device bank behind it, on that device
    host = clips.jpeg_bank(files[:2], 'all').extend(clips.JpegBank.from_encoded(jb))
    assert _equal(ops.jpeg_decode_indexed_u8(host, [3, 0, 2, 1]), ops.jpeg_decode_u8([files[i] for i in (4, 0, 3, 1)], layouts='all'))


def test_crop(pkg, mixed):
    from istvt_amd import ops
    files, bank, _ = mixed
    index = [23, 0, 5, 5, 14, 9]
    want = ops.decode_frames([files[i] for i in index], 16, layouts='all')
    for idx in (index, torch.tensor(index, device='cuda')):
        got = ops.decode_frames(bank, 16, index=idx)
        assert tuple(got.shape) == (6, 16, 16, 3) and torch.equal(got, want)
    boxes = torch.tensor([[0, 0, 8, 8]] * len(index), dtype=torch.int32)
    assert torch.equal(ops.decode_frames(bank, 16, boxes, index=index),
                       ops.decode_frames(clips_batch(files, index), 16, boxes))
    black = ops.decode_frames(bank, 16, index=[len(files), 3])
    assert int(black[0].max()) == 0 and torch.equal(black[1], ops.decode_frames([files[3]], 16, layouts='all')[0])


def clips_batch(files, index):
    from istvt_amd import clips
    return clips.jpeg_batch([files[i] for i in index], 'all')
