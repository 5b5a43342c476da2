"""PNG files out (DESIGN.md "PNG files out") on a real MI355X: ops.png_encode_u8 against the integer definition
clips.png_encode_files_host, byte for byte, on the shapes, filters, runs and tables of tests/png_encode_cases.py; the round trip
through ops.png_decode_u8; a capacity one byte short; caller's buffers and a captured graph; ops.encode_frames(format='png');
every refusal and the profile record."""
import numpy as np
import pytest
import torch

import png_encode_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def groups(pkg):
    """the cases batched where shape, band_rows and filters agree: [(names, frames uint8 (n, H, W[, C]), R, filters, the
    definition's files)]; computed once"""
    from istvt_amd import clips
    by = {}
    for name, frame, R, filters in C.all_cases():
        by.setdefault((frame.shape, R, filters), []).append((name, frame))
    out = []
    for (shape, R, filters), members in by.items():
        frames = np.stack([f for _, f in members])
        out.append(([n for n, _ in members], frames, R, filters, clips.png_encode_files_host(frames, R, filters)))
    return out


@pytest.fixture(scope='module')
def five(pkg):
    """5 frames of 33 x 40 RGB with different contents, so that every file has another length, and the definition's files"""
    from istvt_amd import clips
    frames = np.stack([C.smooth(33, 40, 3, 4), C.noise(33, 40, 3, 11), np.zeros((33, 40, 3), np.uint8), C.smooth(33, 40, 3, 12),
                       C.noise(33, 40, 3, 13) // 16])
    files = clips.png_encode_files_host(frames, 8, 'adaptive')
    assert len({len(f) for f in files}) == 5
    return frames, files


def _rgb(frame):
    """what ops.png_decode_u8 makes of a file of this frame: grey replicated, alpha dropped"""
    f = frame[:, :, None] if frame.ndim == 2 else frame
    return np.repeat(f, 3, 2) if f.shape[2] == 1 else f[:, :, :3]


def test_bytes_equal_the_definition(pkg, groups, five):
    from istvt_amd import clips, ops
    assert sum(len(g[0]) for g in groups) == len(C.all_cases()) == 60
    for names, frames, R, filters, want in groups:
        res = ops.png_encode_u8(torch.from_numpy(frames).cuda(), R, filters)
        assert isinstance(res, clips.PngFiles) and res.data.is_cuda and res.offsets.dtype == torch.int64
        got = res.files()
        for name, g, w in zip(names, got, want):
            assert g == w, '%s: %d bytes, the definition has %d' % (name, len(g), len(w))
        assert res.nbytes() == sum(len(w) for w in want) and res.status.tolist() == [0] * len(names)
    frames, want = five
    res = ops.png_encode_u8(torch.from_numpy(frames).cuda(), 8)
    assert res.files() == want and res.offsets.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    # clips (B, T, H, W, C): the files of the B T frames in order; grey as (n, H, W) and as (n, H, W, 1)
    clip = torch.from_numpy(frames[:4].reshape(2, 2, 33, 40, 3)).cuda()
    assert ops.png_encode_u8(clip, 8).files() == want[:4]
    grey = torch.from_numpy(frames[:, :, :, 0].copy()).cuda()
    gw = clips.png_encode_files_host(grey, 16, 'adaptive')
    assert ops.png_encode_u8(grey).files() == gw == ops.png_encode_u8(grey.unsqueeze(-1)).files()


def test_round_trip_through_the_decoder(pkg, groups):
    """every file of every case decoded by ops.png_decode_u8 in one call: status 0 and the frames"""
    from istvt_amd import ops
    files, refs = [], []
    for names, frames, R, filters, want in groups:
        files += want
        refs += [_rgb(f) for f in frames]
    got, sizes, status = ops.png_decode_u8(files)
    assert status.tolist() == [0] * len(files) and sizes.tolist() == [list(r.shape[:2]) for r in refs]
    got = got.cpu().numpy()
    for i, r in enumerate(refs):
        assert np.array_equal(got[i, :r.shape[0], :r.shape[1]], r), i


def _buffers(n, H, W, bpp, R, capacity, fill=0xA5):
    from istvt_amd import frames as F
    need = F.png_encode_scratch(n, H, W, bpp, R)[1]
    return (torch.full((capacity,), fill, dtype=torch.uint8, device='cuda'), torch.empty((need,), dtype=torch.uint8, device='cuda'),
            torch.empty((n + 1,), dtype=torch.int64, device='cuda'), torch.empty((n,), dtype=torch.int32, device='cuda'))


def test_capacity_one_byte_short(pkg, five):
    from istvt_amd import ops
    frames, want = five
    dev = torch.from_numpy(frames).cuda()
    total = sum(len(w) for w in want)
    buffers = _buffers(5, 33, 40, 3, 8, total - 1)
    res = ops.png_encode_u8(dev, 8, buffers=buffers)
    assert res.data is buffers[0] and res.status.tolist() == [0, 0, 0, 0, 1]
    assert res.nbytes() == total and res.offsets.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert res.files(check=False) == want[:4] + [b'']
    fits = total - len(want[4])
    assert bool((res.data[fits:] == 0xA5).all()), 'bytes behind the files that fit were written'
    with pytest.raises(ValueError, match=r'png_encode: file 4 has status 1 \(the file does not fit in data: offsets\[n\] is the capacity a '
                                         r'retry needs\)'):
        res.files()
    again = ops.png_encode_u8(dev, 8, capacity=res.nbytes())
    assert again.files() == want and tuple(again.data.shape) == (total,)
    # a middle file's true size still stands in offsets where everything behind the first file is short
    tight = ops.png_encode_u8(dev, 8, capacity=len(want[0]))
    assert tight.status.tolist() == [0, 1, 1, 1, 1] and tight.files(check=False)[0] == want[0] and tight.nbytes() == total


def test_callers_buffers_allocate_nothing(pkg, five):
    from istvt_amd import ops
    frames, want = five
    dev = torch.from_numpy(frames).cuda()
    buffers = _buffers(5, 33, 40, 3, 8, 5 * 8192)
    first = ops.png_encode_u8(dev, 8, buffers=buffers)
    assert first.files() == want
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    second = ops.png_encode_u8(dev, 8, buffers=buffers)
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
    assert second.data is buffers[0] and second.offsets is buffers[2] and second.status is buffers[3]
    # captured in a graph and replayed over other bytes: the same files
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_encode_u8(dev, 8, buffers=buffers)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.png_encode_u8(dev, 8, buffers=buffers)
    for t in buffers:
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    assert second.files() == want
    small = (buffers[0], buffers[1][:buffers[1].numel() - 1], buffers[2], buffers[3])
    with pytest.raises(RuntimeError, match=r'png_encode_u8: buffers = \(uint8 data \(capacity,\); uint8 scratch of %d bytes, 16-byte aligned; '
                                           r'int64 offsets \(6,\); int32 status \(5,\)\), contiguous on cuda' % buffers[1].numel()):
        ops.png_encode_u8(dev, 8, buffers=small)
    with pytest.raises(ValueError, match='png_encode_u8: capacity 7 and data of 40960 bytes disagree'):
        ops.png_encode_u8(dev, 8, capacity=7, buffers=buffers)
    with pytest.raises(RuntimeError, match='png_encode_u8: out may not share memory with the frames'):
        ops.png_encode_u8(dev, 8, buffers=(dev.view(-1),) + buffers[1:])


def test_encode_frames(pkg):
    from istvt_amd import clips, ops
    frames = torch.from_numpy(np.stack([C.smooth(64, 80, 3, 20 + i) for i in range(3)])).cuda()
    boxes = torch.tensor([[0, 0, 64, 80], [5, 7, 40, 33], [10, 20, 24, 24]], dtype=torch.int32)
    crops = ops.crop_resize_u8(frames, boxes, 24)
    got = ops.encode_frames(frames, 24, boxes=boxes, format='png')
    assert isinstance(got, clips.PngFiles) and got.files() == ops.png_encode_u8(crops).files()
    assert got.files() == clips.png_encode_files_host(crops.cpu(), 16, 'adaptive')
    assert ops.encode_frames(frames, 24, boxes=boxes, format='png', band_rows=5, filters=4).files() == ops.png_encode_u8(crops, 5, 4).files()
    M = clips.similarity_of_boxes(torch.tensor([[0, 0, 64, 64], [5, 7, 33, 33], [10, 20, 24, 24]], dtype=torch.int32), 24)
    assert ops.encode_frames(frames, 24, transforms=M, format='png').files() == ops.png_encode_u8(ops.warp_similarity_u8(frames, M, 24)).files()
    # 'jpeg', and no format at all, are the existing call
    want = ops.jpeg_encode_u8(crops, 80, '444', 'row', optimize=True).files()
    assert ops.encode_frames(frames, 24, boxes=boxes, quality=80, subsampling='444', optimize=True).files() == want
    assert ops.encode_frames(frames, 24, boxes=boxes, quality=80, subsampling='444', optimize=True, format='jpeg').files() == want
    assert isinstance(ops.encode_frames(frames, 24, boxes=boxes), clips.JpegFiles)
    for kw in (dict(quality=80), dict(optimize=True), dict(layout='grey'), dict(restart_interval=0), dict(subsampling='444'),
               dict(quality=90), dict(subsampling='420'), dict(restart_interval='row'), dict(optimize=False)):
        name = list(kw)[0]
        with pytest.raises(ValueError, match=r"encode_frames: %s= goes with format='jpeg'; format='png' takes band_rows= and filters=" % name):
            ops.encode_frames(frames, 24, boxes=boxes, format='png', **kw)
    with pytest.raises(ValueError, match=r"encode_frames: band_rows= and filters= go with format='png'"):
        ops.encode_frames(frames, 24, boxes=boxes, band_rows=8)
    with pytest.raises(ValueError, match=r"encode_frames: format is 'jpeg' or 'png', got 'webp'"):
        ops.encode_frames(frames, 24, boxes=boxes, format='webp')
    with pytest.raises(ValueError, match='encode_frames: boxes and transforms are two ways'):
        ops.encode_frames(frames, 24, format='png')


def test_refusals_and_the_record(pkg, five):
    from istvt_amd import clips, ops
    frames, want = five
    dev = torch.from_numpy(frames).cuda()
    ops.kernel_profile = []
    try:
        ops.png_encode_u8(dev, 8)
        record = [(r[0], r[3]) for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == [('png_encode_u8', dev.numel() + 3 * 5 * 33 * (1 + 40 * 3))]
    with pytest.raises(TypeError, match=r'png_encode_u8: frames must be uint8, got torch.float32'):
        ops.png_encode_u8(dev.float())
    with pytest.raises(RuntimeError, match=r'png_encode_u8 expects channels-last \(n, H, W, C\) or \(B, T, H, W, C\) uint8 input with C in '
                                           r'\(1, 3, 4\) \(grey also as \(n, H, W\)\), got \(5, 33, 40, 2\)'):
        ops.png_encode_u8(dev[..., :2].contiguous())
    with pytest.raises(RuntimeError, match=r'png_encode_u8 expects channels-last .* got \(40, 3\)'):
        ops.png_encode_u8(dev[0, 0])
    with pytest.raises(RuntimeError, match=r'png_encode_u8: empty input \(0, 33, 40, 3\)'):
        ops.png_encode_u8(dev[:0])
    with pytest.raises(RuntimeError, match='png_encode_u8: frames must be contiguous'):
        ops.png_encode_u8(dev[:, :, ::2])
    with pytest.raises(RuntimeError, match='istvt_amd: frames must be on a ROCm device'):
        ops.png_encode_u8(torch.from_numpy(frames))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match='png_encode_u8: band_rows is a count of rows of at least 1, got %r' % (bad,)):
            ops.png_encode_u8(dev, bad)
    for bad in (5, -1, 'paeth', None):
        with pytest.raises(ValueError, match=r"png_encode_u8: filters is 'adaptive' or one type 0..4 for every row, got %r" % (bad,)):
            ops.png_encode_u8(dev, 8, bad)
    with pytest.raises(ValueError, match='png_encode_u8: frames of at most 16384 x 16384, got 1 x 16385'):
        ops.png_encode_u8(torch.zeros((1, 1, 16385), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='png_encode_u8: the capacity must be positive, got 0'):
        ops.png_encode_u8(dev, 8, capacity=0)
    # a batch whose bound passes ISTVT_PNG_MAX_BYTES: refused from the shape alone, before the device is asked for
    big = torch.empty((40, 4096, 4096, 4), dtype=torch.uint8, device='meta')
    assert 40 * clips.png_encoded_bound(4096, 4096, 4, 16) > clips.PNG_MAX_BYTES
    with pytest.raises(ValueError, match=r'png_encode_u8: the files of a batch hold at most %d bytes, 40 frames of 4096 x 4096 x 4 can need '
                                         % clips.PNG_MAX_BYTES):
        ops.png_encode_u8(big)
