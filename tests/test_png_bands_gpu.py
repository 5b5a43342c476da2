"""PNG files by their bands (DESIGN.md "PNG files by their bands") on a real MI355X: ops.png_decode_u8 on batches that carry
bands against the integer definitions, byte for byte -- our indexed files beside files without an index in one call; files
zlib wrote with a flush at every band edge; indexes that lie and damaged bands between sound files; where the call writes
(tests/guard.py); the device writer's index; the front end, a captured graph and ops.decode_frames.  Every band that goes to a
device here was decoded to its status first by tools/png_bands_check.cpp, the same csrc/png_inflate.h on the host
(tests/test_png_bands_cpu.py builds it plain; DESIGN.md has its run under AddressSanitizer and UBSan)."""
import pytest
import torch

import guard
import png_bands_cases as B
import png_encode_cases as C
import png_streams as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def mixed(pkg, golden_dir):
    """[(name, file, the sequential definition's frame)] of the mixed call: decoded on the host once"""
    from istvt_amd import clips
    files = B.mixed_files(clips) + B.pil_files(golden_dir) + [('ignored_index', B.ignored_index_file(clips))]
    out = []
    for name, f in files:
        ref, status = clips.png_decode_host(f, return_status=True)
        assert status == 0, name
        out.append((name, f, ref))
    return out


def _check_canvas(got, refs):
    """every image's region equals the definition and every byte outside is 0"""
    got = got.cpu()
    for i, ref in enumerate(refs):
        h, w = ref.shape[:2]
        bad = int((got[i, :h, :w] != ref).sum())
        assert bad == 0, 'image %d (%d x %d): %d of %d bytes differ' % (i, h, w, bad, ref.numel())
        assert int(got[i, h:].any()) == 0 and int(got[i, :, w:].any()) == 0, 'image %d: bytes outside %d x %d' % (i, h, w)


def _record(ops, call):
    ops.kernel_profile = []
    try:
        out = call()
        return out, [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None


def test_one_mixed_call(pkg, mixed):
    """grey, RGB and RGBA files of ours at band_rows 1, 8, 16 and 64 and H of 1, below R, R, one above a multiple of R and 130,
    files PIL wrote and a file whose index is ignored, on one canvas"""
    from istvt_amd import clips, ops
    files = [f for _, f, _ in mixed]
    batch = clips.png_batch(files, bands='index')
    rows = batch.bands.tolist()
    assert {(r[2], r[3]) for r in batch.images.tolist()} == {(0, 1), (2, 3), (6, 4)}
    assert {r[1] % 4 for r in rows} == {0, 1, 2, 3}                           # a band begins at any byte
    strides = [1 + r[1] * r[3] for r in batch.images.tolist()]
    assert any(r[4] == strides[r[0]] for r in rows)                           # a band of a single row
    assert {r[7] for r in batch.images.tolist()} >= {1, 3, 5, 9, 130} and len(rows) > 160
    (got, sizes, status), record = _record(ops, lambda: ops.png_decode_u8(batch, checked=True))
    assert record == ['png_decode_bands_u8']
    n = len(files)
    assert tuple(got.shape) == (n, 130, 111, 3) and got.dtype == torch.uint8
    assert status.tolist() == [0] * n and sizes.tolist() == [list(r.shape[:2]) for _, _, r in mixed]
    _check_canvas(got, [r for _, _, r in mixed])
    # a sequence of bytes with bands='index' is packed that way; without, and for a batch without bands, today's path and record
    (one, s1, st1), record = _record(ops, lambda: ops.png_decode_u8(files[3:6], bands='index'))
    assert record == ['png_decode_bands_u8'] and st1.tolist() == [0] * 3
    _check_canvas(one, [r for _, _, r in mixed[3:6]])
    (seq, _, st2), record = _record(ops, lambda: ops.png_decode_u8(clips.png_batch(files), checked=True))
    assert record == ['png_decode_u8'] and st2.tolist() == [0] * n and torch.equal(seq, got)
    (_, _, st3), record = _record(ops, lambda: ops.png_decode_u8(files[:2]))
    assert record == ['png_decode_u8'] and st3.tolist() == [0, 0]


def test_flush_files(pkg):
    """zlib's streams with a flush at every band edge and inside every band, hand-made indexes: stored, fixed and dynamic
    blocks, several per band, long matches"""
    from istvt_amd import clips, ops
    files = [f for _, f in B.flush_files(clips)]
    refs = []
    for f in files:
        ref, status = clips.png_decode_bands_host(f, return_status=True)
        assert status == 0 and clips.png_parse(f).bands is not None
        refs.append(ref)
    batch = clips.png_batch(files, bands='index')
    assert batch.bands.shape[0] == sum(-(-h // r) for (h, _, _, r) in ((37, 50, 3, 8), (20, 45, 1, 16), (66, 30, 4, 16), (33, 64, 3, 4),
                                                                      (19, 27, 1, 5), (48, 100, 3, 16), (130, 20, 4, 64)))
    got, sizes, status = ops.png_decode_u8(batch, checked=True)
    assert status.tolist() == [0] * len(files)
    _check_canvas(got, refs)


def test_lying_indexes_and_damaged_bands(pkg):
    """Each between two good files: the definition's status, an all-zero frame, intact neighbours.  These are refusals; every
    band of them has been decoded to its status by the host program first."""
    from istvt_amd import clips, ops
    good = clips.png_encode_banded_host(P.pattern(36, 25, 3, 91), 8, index=True)
    frame = clips.png_decode_host(good)
    cases = B.lying_files(clips)
    want = [clips.png_decode_bands_host(f, return_status=True)[1] for _, f, _ in cases]
    assert want[1:5] == [4, 7, 1, 5] and 0 not in want
    files = [good]
    for _, f, _ in cases:
        files += [f, good]
    got, sizes, status = ops.png_decode_u8(files, bands='index')
    assert status.tolist()[1::2] == want and status.tolist()[0::2] == [0] * (len(cases) + 1)
    assert sizes.tolist() == [[36, 25]] * len(files)
    got = got.cpu()
    for i in range(len(files)):
        if i % 2:
            assert not bool(got[i].any()), cases[i // 2][0]
        else:
            assert torch.equal(got[i], frame), i
    with pytest.raises(ValueError, match=r'png_decode: file 1 is damaged \(status %d: ' % want[0]):
        clips.check_png_status(status)
    # the sequential decoder takes the sync-flush file: its stream is sound
    _, _, st = ops.png_decode_u8([cases[1][1]])
    assert st.tolist() == [0]


def test_guards(pkg, mixed):
    """out, scratch, sizes and status between sentinel guards; the uploaded tables placed as inputs; every element of out
    written (two sentinel fills); of the scratch nothing but each file's H (1 + W bpp) bytes and the band status words"""
    from istvt_amd import _lib, clips, ops
    pick = mixed[::2] + mixed[1:4]
    batch = clips.png_batch([f for _, f, _ in pick], bands='index')
    n, canvas, nband = batch.n, (131, 113), int(batch.bands.shape[0])
    assert batch.scratch_bytes == n * batch.raw_stride + 4 * nband
    for fill in (0xA5, 0x5A):
        with guard.guarded(lib_module=_lib) as calls:
            dev = batch.on(torch.device('cuda', torch.cuda.current_device()))
            data, images, bands = dev.data, dev.images, dev.bands
            dev.data, dev.images, dev.bands = guard.place(data), guard.place(images), guard.place(bands)
            out = guard.place(torch.full((n, canvas[0], canvas[1], 3), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            scratch = guard.place(torch.full((batch.scratch_bytes,), fill, dtype=torch.uint8, device='cuda'), inplace='output.prefilled')
            sizes = torch.empty((n, 2), dtype=torch.int32, device='cuda')
            status = torch.empty((n,), dtype=torch.int32, device='cuda')
            try:
                got, s, st = ops.png_decode_u8(batch, canvas=canvas, out=out, checked=True, buffers=(scratch, sizes, status))
            finally:
                dev.data, dev.images, dev.bands = data, images, bands
        assert calls == {'istvt_png_decode_bands_u8'} and got is out and s is sizes and st is status
        assert st.tolist() == [0] * n and s.tolist() == batch.images[:, :2].tolist()
        _check_canvas(got, [r for _, _, r in pick])
        host = scratch.cpu()
        rows = host[:n * batch.raw_stride].view(n, batch.raw_stride)
        for i, (h, w, _, bpp) in enumerate(r[:4] for r in batch.images.tolist()):
            assert bool((rows[i, h * (1 + w * bpp):] == fill).all()), 'file %d: the scratch behind its rows was written' % i
        assert host[n * batch.raw_stride:].view(torch.int32).tolist() == [0] * nband


def test_device_encoder_writes_the_index(pkg):
    from istvt_amd import clips, ops
    dev = torch.device('cuda', torch.cuda.current_device())
    for ch in C.CHANNELS:
        for H, R, frames in B.encoder_frames(ch):
            x = torch.from_numpy(frames).to(dev)
            want = clips.png_encode_files_host(frames, R, index=True)
            (files, record) = _record(ops, lambda: ops.png_encode_u8(x, R, index=True))
            assert record == ['png_encode_indexed_u8'] and files.geometry.index is True
            assert files.status.tolist() == [0] * 3 and files.files() == want, (ch, H, R)
            assert files.offsets.tolist() == [sum(len(f) for f in want[:i]) for i in range(4)]
            # one byte short of the last file: status 1 for it, true offsets
            short = ops.png_encode_u8(x, R, index=True, capacity=sum(len(f) for f in want) - 1)
            assert short.status.tolist() == [0, 0, 1] and short.offsets.tolist() == files.offsets.tolist()
            assert short.files(check=False) == want[:2] + [b'']
            # without index: the bytes and the record of before
            (plain, record) = _record(ops, lambda: ops.png_encode_u8(x, R))
            assert record == ['png_encode_u8'] and plain.geometry.index is False
            assert plain.files() == clips.png_encode_files_host(frames, R)
            # and back, by the bands
            got, sizes, status = ops.png_decode_u8(files.files(), bands='index')
            assert status.tolist() == [0] * 3 and sizes.tolist() == [[H, 29]] * 3
            src = x.expand(3, H, 29, 3) if ch == 1 else x[..., :3]
            assert torch.equal(got, src), (ch, H, R)
    boxes = torch.tensor([[0, 0, 29, 29]] * 3, dtype=torch.int32)
    x = torch.from_numpy(B.encoder_frames(3)[2][2]).to(dev)
    made = ops.encode_frames(x, 24, boxes, format='png', band_rows=8, index=True)
    assert made.geometry.index is True and made.files() == clips.png_encode_files_host(ops.crop_resize_u8(x, boxes, 24).cpu(), 8, index=True)
    assert ops.encode_frames(x, 24, boxes, format='png', band_rows=8).files() == ops.encode_frames(x, 24, boxes, format='png', band_rows=8,
                                                                                                   index=False).files()


def test_front_end(pkg, mixed):
    from istvt_amd import clips, ops
    pick = [mixed[5], mixed[7], mixed[12], mixed[3]]                          # 130 x 9 RGBA, 40 x 111 RGB, a PIL file, 17 x 9 RGB
    files, refs = [f for _, f, _ in pick], [r for _, _, r in pick]
    batch = clips.png_batch(files, bands='index')
    plain = clips.png_batch(files)
    dev = torch.device('cuda', torch.cuda.current_device())
    n = len(files)
    # canvas= larger than the batch, out= and buffers=, checked=True
    out = torch.full((n, 140, 120, 3), 7, dtype=torch.uint8, device=dev)
    buffers = (torch.empty(batch.scratch_bytes, dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
    got, sizes, status = ops.png_decode_u8(batch, canvas=(140, 120), out=out, checked=True, buffers=buffers)
    assert got is out and sizes is buffers[1] and status is buffers[2] and status.tolist() == [0] * n
    _check_canvas(got, refs)
    eager = got.clone()
    # captured in a graph and replayed twice into refilled buffers: the eager bytes
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
        assert torch.equal(out, eager) and buffers[2].tolist() == [0] * n
    # decode_frames follows the batch: the decode and crop_resize_u8
    boxes = torch.tensor([[0, 0, 130, 9], [3, 5, 30, 50], [0, 0, 8, 8], [2, 1, 9, 7]], dtype=torch.int32)
    frames, _, _ = ops.png_decode_u8(batch, checked=True)
    (cut, record) = _record(ops, lambda: ops.decode_frames(batch, 32, boxes))
    assert record[0] == 'png_decode_bands_u8' and torch.equal(cut, ops.crop_resize_u8(frames, boxes, 32))
    assert torch.equal(ops.decode_frames(batch, 32), ops.crop_resize_u8(frames, clips.whole_boxes(batch.sizes), 32))
    (_, record) = _record(ops, lambda: ops.decode_frames(plain, 32, boxes))
    assert record[0] == 'png_decode_u8'
    # refusals, by type and text
    with pytest.raises(ValueError, match=r"png_decode_u8: bands is None or 'index', got 'rows'"):
        ops.png_decode_u8(files, bands='rows')
    with pytest.raises(ValueError, match=r"png_decode_u8: bands='index' with a clips.PngBatch that was packed without bands"):
        ops.png_decode_u8(plain, checked=True, bands='index')
    nband = int(batch.bands.shape[0])
    old = (buffers[0][:plain.scratch_bytes], buffers[1], buffers[2])           # the scratch of the same files without bands
    with pytest.raises(RuntimeError, match=r'png_decode_u8: a batch with bands needs a scratch of %d bytes: %d of filtered rows and a '
                                           r'status word for each of its %d bands, got %d'
                                           % (batch.scratch_bytes, plain.scratch_bytes, nband, plain.scratch_bytes)):
        ops.png_decode_u8(batch, checked=True, buffers=old)
    with pytest.raises(RuntimeError, match=r'png_decode_u8: buffers = \(uint8 scratch of %d bytes' % batch.scratch_bytes):
        ops.png_decode_u8(batch, checked=True, buffers=(buffers[0][:16], buffers[1], buffers[2]))
    x = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r"encode_frames: index= goes with format='png'"):
        ops.encode_frames(x, 8, torch.tensor([[0, 0, 16, 16]] * 2, dtype=torch.int32), index=True)
