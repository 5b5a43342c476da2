"""PNG files (DESIGN.md "PNG files") on a real MI355X: ops.png_decode_u8 against the integer definition clips.png_decode_host,
byte for byte -- every filter type on every band edge in grey, RGB and RGBA files of five stream kinds; streams zlib does not
write; damaged streams between sound files; where the call writes (tests/guard.py); the front end, a captured graph and
ops.decode_frames; the committed files PIL wrote."""
import os

import numpy as np
import pytest
import torch

import guard
import png_streams as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def filter_set(pkg):
    """[(name, file, the definition's frame)] of the filter test: decoded on the host once"""
    from istvt_amd import clips
    out = []
    for name, f in P.filter_files(clips.png_encode_host):
        ref, status = clips.png_decode_host(f, return_status=True)
        assert status == 0
        out.append((name, f, ref))
    return out


@pytest.fixture(scope='module')
def base_file(pkg):
    """the 100 x 111 image of the special streams as zlib writes it, and its frame"""
    from istvt_amd import clips
    rows = np.array(P.lits(0, P.TOTAL), np.uint8).reshape(P.H, -1)
    frame = torch.from_numpy(rows[:, 1:].reshape(P.H, P.W, 3).copy())
    f = clips.png_encode_host(frame, level=6)
    assert torch.equal(clips.png_decode_host(f), frame)
    return f, frame


def _check_canvas(got, refs):
    """every image's region equals the definition and every byte outside is 0"""
    got = got.cpu()
    for i, ref in enumerate(refs):
        h, w = ref.shape[:2]
        bad = int((got[i, :h, :w] != ref).sum())
        assert bad == 0, 'image %d (%d x %d): %d of %d bytes differ' % (i, h, w, bad, ref.numel())
        assert int(got[i, h:].any()) == 0 and int(got[i, :, w:].any()) == 0, 'image %d: bytes outside %d x %d' % (i, h, w)


def test_filters_and_colour_types(pkg, filter_set):
    """20 files of 6 sizes x 3 colour types and 5 stream kinds in ONE call on a common canvas: mixed sizes, the zero fill, every
    filter type on row 0 and on rows 63, 64 and 128, and behind every other type"""
    from istvt_amd import clips, ops
    batch = clips.png_batch([f for _, f, _ in filter_set])
    assert {(r[2], r[3]) for r in batch.images.tolist()} == {(0, 1), (2, 3), (6, 4)}
    ops.kernel_profile = []
    try:
        got, sizes, status = ops.png_decode_u8(batch, checked=True)
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['png_decode_u8']
    assert tuple(got.shape) == (20, 130, 70, 3) and got.dtype == torch.uint8
    assert status.tolist() == [0] * 20 and sizes.tolist() == [list(r.shape[:2]) for _, _, r in filter_set]
    _check_canvas(got, [r for _, _, r in filter_set])
    clips.check_png_status(status)
    one, s1, st1 = ops.png_decode_u8([filter_set[10][1]])                     # a sequence of bytes, parsed and packed here
    assert torch.equal(one[0].cpu(), filter_set[10][2]) and s1.tolist() == [[65, 67]] and st1.tolist() == [0]


def test_streams_zlib_does_not_write(pkg):
    from istvt_amd import clips, ops
    special = P.special_streams()
    assert [n for n, _, _ in special] == ['len258_dist32768', 'dist1_len258', 'match_across_blocks', 'empty_stored_unaligned',
                                         'empty_final_fixed', 'dynamic_15bit', 'dynamic_single_distance', 'dynamic_no_distance',
                                         'repeat_across_sets']
    files = [clips.png_wrap(P.H, P.W, 2, P.zlib_wrap(raw, data)) for _, raw, data in special]
    refs = [torch.from_numpy(clips._png_unfilter(np.frombuffer(data, np.uint8).reshape(P.H, -1), 3).reshape(P.H, P.W, 3))
            for _, _, data in special]
    got, sizes, status = ops.png_decode_u8(files)
    assert status.tolist() == [0] * 9 and sizes.tolist() == [[P.H, P.W]] * 9
    _check_canvas(got, refs)


def test_damaged_streams(pkg, base_file):
    """Each damaged stream between two good files: its status, an all-zero frame, intact neighbours.  Every one of these
    streams has been decoded to that status by tools/png_inflate_check.cpp (the same csrc/png_inflate.h) under AddressSanitizer
    and UBSan on the host before it went to a device: DESIGN.md "PNG files" has the command and its result.  These are refusals."""
    from istvt_amd import clips, ops
    good, frame = base_file
    damaged = P.damaged_streams()
    files = [good]
    for _, raw, _ in damaged:
        files += [clips.png_wrap(P.H, P.W, 2, P.zlib_wrap(raw)), good]
    got, sizes, status = ops.png_decode_u8(files)
    assert status.tolist()[1::2] == [s for _, _, s in damaged] == [1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 6]
    assert status.tolist()[0::2] == [0] * 12 and sizes.tolist() == [[P.H, P.W]] * 23
    got = got.cpu()
    for i in range(23):
        if i % 2:
            assert not bool(got[i].any()), damaged[i // 2][0]
        else:
            assert torch.equal(got[i], frame), i
    with pytest.raises(ValueError, match=r'png_decode: file 1 is damaged \(status 1: the stream ends early\)'):
        clips.check_png_status(status)


def test_guards(pkg, filter_set):
    """out, scratch, sizes and status between sentinel guards; the uploaded tables placed as inputs; every element of out
    written (two sentinel fills); nothing of the scratch outside each file's H (1 + W bpp) bytes"""
    from istvt_amd import _lib, clips, ops
    pick = filter_set[::2] + filter_set[1:4]
    batch = clips.png_batch([f for _, f, _ in pick])
    n, canvas = batch.n, (131, 73)
    for fill in (0xA5, 0x5A):
        with guard.guarded(lib_module=_lib) as calls:
            dev = batch.on(torch.device('cuda', torch.cuda.current_device()))
            data, images = dev.data, dev.images
            dev.data, dev.images = guard.place(data), guard.place(images)
            out = guard.place(torch.full((n, canvas[0], canvas[1], 3), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            scratch = guard.place(torch.full((batch.scratch_bytes,), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            sizes = torch.empty((n, 2), dtype=torch.int32, device='cuda')
            status = torch.empty((n,), dtype=torch.int32, device='cuda')
            try:
                got, s, st = ops.png_decode_u8(batch, canvas=canvas, out=out, checked=True, buffers=(scratch, sizes, status))
            finally:
                dev.data, dev.images = data, images
        assert calls == {'istvt_png_decode_u8'} and got is out and s is sizes and st is status
        assert st.tolist() == [0] * n and s.tolist() == batch.images[:, :2].tolist()
        _check_canvas(got, [r for _, _, r in pick])
        rows = scratch.cpu().view(n, batch.raw_stride)
        for i, (h, w, _, bpp) in enumerate(r[:4] for r in batch.images.tolist()):
            assert bool((rows[i, h * (1 + w * bpp):] == fill).all()), 'file %d: the scratch behind its rows was written' % i


def test_front_end(pkg, filter_set, base_file):
    from istvt_amd import clips, ops
    good, frame = base_file
    files = [filter_set[9][1], good, filter_set[17][1]]
    refs = [filter_set[9][2], frame, filter_set[17][2]]
    batch = clips.png_batch(files)
    dev = torch.device('cuda', torch.cuda.current_device())
    # canvas= larger than the batch, out= and buffers=, checked=True
    out = torch.full((3, 140, 120, 3), 7, dtype=torch.uint8, device=dev)
    buffers = (torch.empty(batch.scratch_bytes, dtype=torch.uint8, device=dev), torch.empty((3, 2), dtype=torch.int32, device=dev),
               torch.empty(3, dtype=torch.int32, device=dev))
    got, sizes, status = ops.png_decode_u8(batch, canvas=(140, 120), out=out, checked=True, buffers=buffers)
    assert got is out and sizes is buffers[1] and status is buffers[2] and status.tolist() == [0, 0, 0]
    _check_canvas(got, refs)
    eager = got.clone()
    # captured in a graph and replayed twice: the eager bytes, nothing allocated in between
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_decode_u8(batch, canvas=(140, 120), out=out, checked=True, buffers=buffers)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.png_decode_u8(batch, canvas=(140, 120), out=out, checked=True, buffers=buffers)
    for fill in (1, 2):
        out.fill_(fill)
        buffers[0].fill_(fill)
        buffers[2].fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and buffers[2].tolist() == [0, 0, 0]
    # decode_frames takes a PngBatch: the decode and crop_resize_u8
    boxes = torch.tensor([[3, 5, 40, 50], [10, 20, 64, 64], [0, 0, 130, 9]], dtype=torch.int32)
    frames, _, _ = ops.png_decode_u8(batch, checked=True)
    assert torch.equal(ops.decode_frames(batch, 32, boxes), ops.crop_resize_u8(frames, boxes, 32))
    assert torch.equal(ops.decode_frames(batch, 32), ops.crop_resize_u8(frames, clips.whole_boxes(batch.sizes), 32))
    # refusals, by type and text
    with pytest.raises(RuntimeError, match=r'png_decode_u8: empty input \(no files\)'):
        ops.png_decode_u8([])
    with pytest.raises(ValueError, match=r'png_decode_u8: the canvas must hold every image \(130 x 111 at least, 16384 x 16384 at most\), '
                                         r'got 129 x 111'):
        ops.png_decode_u8(batch, canvas=(129, 111), checked=True)
    with pytest.raises(ValueError, match='got 130 x 16385'):
        ops.png_decode_u8(batch, canvas=(130, 16385), checked=True)
    small = (buffers[0][:batch.scratch_bytes - 1], buffers[1], buffers[2])
    with pytest.raises(RuntimeError, match=r'png_decode_u8: buffers = \(uint8 scratch of %d bytes, 16-byte aligned; int32 sizes \(3, 2\); '
                                           r'int32 status \(3,\)\), contiguous on cuda' % batch.scratch_bytes):
        ops.png_decode_u8(batch, checked=True, buffers=small)
    with pytest.raises(RuntimeError, match=r'png_decode_u8: out must be contiguous uint8 \(3, 130, 111, 3\)'):
        ops.png_decode_u8(batch, checked=True, out=out)
    tiny = clips.png_batch([filter_set[0][1]])                               # 1 x 1, grey
    with pytest.raises(RuntimeError, match='png_decode_u8: out may not share memory with the uploaded files'):
        ops.png_decode_u8(tiny, checked=True, out=tiny.on(dev).data[:3].view(1, 1, 1, 3))
    with pytest.raises(RuntimeError, match='png_decode_u8: checked=True takes a clips.PngBatch'):
        ops.png_decode_u8(files, checked=True)
    with pytest.raises(TypeError, match='png_decode_u8 expects a sequence of files'):
        ops.png_decode_u8(files[0])


def test_committed_files(pkg, golden_dir):
    from istvt_amd import ops
    d = os.path.join(golden_dir, 'png')
    px = np.load(os.path.join(d, 'pixels.npz'))
    names = px['names'].tolist()
    files = [open(os.path.join(d, n + '.png'), 'rb').read() for n in names]
    got, sizes, status = ops.png_decode_u8(files)
    assert len(names) == 15 and status.tolist() == [0] * 15
    _check_canvas(got, [torch.from_numpy(px['rgb_' + n]) for n in names])
