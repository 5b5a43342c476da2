"""JPEG files (DESIGN.md "JPEG files") on a real MI355X: ops.jpeg_decode_u8 against the integer definition
clips.jpeg_decode_host, bit for bit, on PIL's files and on the host encoder's; what it writes and what it leaves alone
(sentinel bytes around every buffer it is given); damaged files; ops.decode_frames; the wrapper's refusals."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 4096                   # sentinel bytes on each side of a buffer


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def files(golden_dir):
    return np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))


@pytest.fixture(scope='module')
def sound(pkg, files):
    """[(name, bytes, the definition's frame)] of every sound fixture file: decoded on the host once"""
    from istvt_amd import clips
    out = []
    for name in files['names'].tolist():
        data = bytes(files['file_' + name])
        ref, status = clips.jpeg_decode_host(data, return_status=True)
        assert status == 0
        out.append((name, data, ref))
    return out


def _smooth(h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return torch.from_numpy(np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8))


class Guarded:
    """a buffer of `shape` with GUARD sentinel bytes on each side, `offset` bytes past an aligned address"""

    def __init__(self, shape, dtype, offset=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + n + 256,), SENTINEL, dtype=torch.uint8, device='cuda')
        self.lo = GUARD + (-self.raw.data_ptr() - GUARD) % 256 + offset
        self.hi = self.lo + n
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())


def _buffers(batch, canvas, out_offset=1):
    n = batch.n
    out = Guarded((n, canvas[0], canvas[1], 3), torch.uint8, out_offset)
    scratch = Guarded((batch.scratch_bytes,), torch.uint8)
    sizes, status = Guarded((n, 2), torch.int32), Guarded((n,), torch.int32)
    return out, scratch, sizes, status


def _check_canvas(got, refs):
    """every image's region equals the definition and every byte outside is 0"""
    got = got.cpu()
    for i, ref in enumerate(refs):
        h, w = ref.shape[:2]
        bad = int((got[i, :h, :w] != ref).sum())
        assert bad == 0, 'image %d (%d x %d): %d of %d bytes differ' % (i, h, w, bad, ref.numel())
        assert int(got[i, h:].any()) == 0 and int(got[i, :, w:].any()) == 0, 'image %d: bytes outside %d x %d' % (i, h, w)


def test_single_files(pkg, sound):
    from istvt_amd import ops
    for name, data, ref in sound:
        frames, sizes, status = ops.jpeg_decode_u8([data])
        h, w = ref.shape[:2]
        assert tuple(frames.shape) == (1, h, w, 3) and frames.dtype == torch.uint8, name
        assert sizes.dtype == torch.int32 and sizes.tolist() == [[h, w]] and status.tolist() == [0], name
        bad = int((frames[0].cpu() != ref).sum())
        assert bad == 0, '%s: %d of %d bytes differ' % (name, bad, ref.numel())


def test_mixed_batch(pkg, sound):
    """all sound files in one call on a 48 x 72 canvas: sizes, subsamplings, table sets and restart intervals mixed"""
    from istvt_amd import clips, ops
    batch = clips.jpeg_batch([d for _, d, _ in sound])
    assert batch.qtabs.shape[0] > 8 and batch.htabs.shape[0] > 8 and batch.segments.shape[0] > 2 * batch.n
    out, scratch, sizes, status = _buffers(batch, (48, 72))
    assert out.t.data_ptr() % 2 == 1
    source = batch.on(out.t.device).data.clone()
    ops.kernel_profile = []
    try:
        got, s, st = ops.jpeg_decode_u8(batch, canvas=(48, 72), out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t))
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_decode_u8']
    assert got is out.t and s is sizes.t and st is status.t
    _check_canvas(got, [r for _, _, r in sound])
    assert s.tolist() == [list(r.shape[:2]) for _, _, r in sound] and not bool(st.any())
    assert out.intact() and scratch.intact() and sizes.intact() and status.intact()
    assert torch.equal(batch.on(out.t.device).data, source)
    first = got.clone()
    scratch.t.fill_(0x3C)                                         # nothing may depend on what the scratch held
    again, _, _ = ops.jpeg_decode_u8(batch, canvas=(48, 72), checked=True, buffers=(scratch.t, sizes.t, status.t))
    assert torch.equal(again, first) and scratch.intact()


def test_damaged_files(pkg, files, sound):
    """The three damaged files between sound ones.  tools/jpeg_entropy_check.cpp (the same csrc/jpeg_entropy.h under
    AddressSanitizer and UBSan on the host) has passed on these bytes, cut at every length and with flipped bits, before this
    ran on a device for the first time: DESIGN.md "JPEG files" has the command and its result."""
    from istvt_amd import clips, ops
    pick = {n: (d, r) for n, d, r in sound if n in ('24x40_s2_q75', '17x33_s0_q95', '33x70_s2_q75_rb1', '16x16_s2_q30')}
    order = ['24x40_s2_q75', 'damaged_cut', '17x33_s0_q95', 'damaged_code', '33x70_s2_q75_rb1', 'damaged_run', '16x16_s2_q30']
    data = [pick[k][0] if k in pick else bytes(files['file_' + k]) for k in order]
    want = dict(zip(files['damaged'].tolist(), files['damaged_status'].tolist()))
    batch = clips.jpeg_batch(data)
    out, scratch, sizes, status = _buffers(batch, (33, 70), out_offset=3)
    got, s, st = ops.jpeg_decode_u8(batch, out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t))
    assert st.tolist() == [want.get(k, 0) for k in order] == [0, 1, 0, 2, 0, 3, 0]
    assert s.tolist() == [[24, 40], [24, 40], [17, 33], [24, 40], [33, 70], [24, 40], [16, 16]]
    host = got.cpu()
    for i, k in enumerate(order):
        if k in pick:
            h, w = pick[k][1].shape[:2]
            assert torch.equal(host[i, :h, :w], pick[k][1]), k
            assert int(host[i, h:].any()) == 0 and int(host[i, :, w:].any()) == 0, k
        else:
            assert int(host[i, 24:].any()) == 0 and int(host[i, :, 40:].any()) == 0, k
    assert out.intact() and scratch.intact() and sizes.intact() and status.intact()
    with pytest.raises(ValueError, match='file 1 is damaged'):
        clips.check_jpeg_status(st)


@pytest.mark.parametrize('ri', [1, 2, 5])
def test_encoder_files_with_many_segments(pkg, ri):
    """33 x 70 from clips.jpeg_encode_host: 15 MCUs at 4:2:0 and 45 at 4:4:4 in restart intervals of 1, 2 and 5 -- many lanes
    per image, the DC prediction reset in each, a last interval that is shorter"""
    from istvt_amd import clips, ops
    x = _smooth(33, 70, 3370)
    data = [clips.jpeg_encode_host(x, q, sub, ri) for sub in ('420', '444') for q in (40, 95)]
    batch = clips.jpeg_batch(data)
    assert batch.segments.shape[0] == 2 * (-(-15 // ri)) + 2 * (-(-45 // ri))
    got, _, st = ops.jpeg_decode_u8(batch, checked=True)
    assert st.tolist() == [0, 0, 0, 0]
    refs = [clips.jpeg_decode_host(d) for d in data]
    _check_canvas(got, refs)
    assert torch.equal(refs[0], clips.jpeg_roundtrip_host(x[None], 40, '420')[0])


def test_decode_frames(pkg, sound):
    from istvt_amd import clips, ops
    names = ['48x48_s2_q75', '33x70_s0_q75_rr1', '24x40_s2_q30', '17x33_s2_q75_opt']
    pick = {n: (d, r) for n, d, r in sound}
    canvas = torch.zeros((4, 48, 70, 3), dtype=torch.uint8)
    for i, k in enumerate(names):
        h, w = pick[k][1].shape[:2]
        canvas[i, :h, :w] = pick[k][1]
    boxes = torch.tensor([[4, 6, 40, 36], [1, 30, 32, 40], [0, 0, 24, 40], [3, 2, 13, 30]], dtype=torch.int32)
    got = ops.decode_frames([pick[k][0] for k in names], 16, boxes)
    assert tuple(got.shape) == (4, 16, 16, 3)
    assert torch.equal(got, ops.crop_resize_u8(canvas.cuda(), boxes, 16))
    whole = ops.decode_frames([pick[k][0] for k in names], 16)
    sizes = [pick[k][1].shape[:2] for k in names]
    assert torch.equal(whole, ops.crop_resize_u8(canvas.cuda(), clips.whole_boxes(sizes), 16))


def test_wrapper_refusals(pkg, sound):
    """each of them before any launch: a sentinel-filled `out` stays as it is"""
    from istvt_amd import clips, ops
    data = [d for n, d, _ in sound if n in ('24x40_s2_q75', '17x33_s0_q95')]
    batch = clips.jpeg_batch(data)
    with pytest.raises(ValueError, match='canvas must hold every image .24 x 40 at least'):
        ops.jpeg_decode_u8(batch, canvas=(24, 39))
    with pytest.raises(ValueError, match='canvas'):
        ops.jpeg_decode_u8(data, canvas=(23, 40))
    out = torch.full((2, 24, 41, 3), SENTINEL, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='out must be contiguous uint8 .2, 24, 40, 3.'):
        ops.jpeg_decode_u8(batch, out=out)
    with pytest.raises(RuntimeError, match='out must be contiguous uint8'):
        ops.jpeg_decode_u8(batch, out=out[:, :, :40])
    # out on top of the uploaded files
    dev = batch.on(out.device)
    big = torch.full((2 * 24 * 40 * 3 + batch.nbytes,), SENTINEL, dtype=torch.uint8, device='cuda')
    big[100:100 + batch.nbytes] = dev.data[:batch.nbytes]
    dev.data = big[100:100 + batch.nbytes]
    with pytest.raises(RuntimeError, match='out may not share memory with the uploaded files'):
        ops.jpeg_decode_u8(batch, out=big[:2 * 24 * 40 * 3].view(2, 24, 40, 3))
    with pytest.raises(RuntimeError, match='empty'):
        ops.jpeg_decode_u8([])
    with pytest.raises(RuntimeError, match='checked=True takes a clips.JpegBatch'):
        ops.jpeg_decode_u8(data, checked=True)
    with pytest.raises(TypeError):
        ops.jpeg_decode_u8(data[0])
    with pytest.raises(RuntimeError, match='buffers'):
        ops.jpeg_decode_u8(batch, buffers=(torch.empty(16, dtype=torch.uint8, device='cuda'),
                                           torch.empty((2, 2), dtype=torch.int32, device='cuda'),
                                           torch.empty((2,), dtype=torch.int32, device='cuda')))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((big[:100] == SENTINEL).all())
    # and the entry itself: a canvas smaller than an image, bad counts
    import ctypes
    from istvt_amd import _lib
    fresh = clips.jpeg_batch(data)
    d = fresh.on(out.device)
    scratch = torch.empty((fresh.scratch_bytes,), dtype=torch.uint8, device='cuda')
    sizes, status = torch.empty((2, 2), dtype=torch.int32, device='cuda'), torch.empty((2,), dtype=torch.int32, device='cuda')
    ok = dict(bytes=d.data.data_ptr(), nbytes=fresh.nbytes, images=d.images.data_ptr(), images_host=fresh.images.data_ptr(),
              segments=d.segments.data_ptr(), segments_host=fresh.segments.data_ptr(), qtabs=d.qtabs.data_ptr(),
              htabs=d.htabs.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), out=out.data_ptr(),
              sizes=sizes.data_ptr(), status=status.data_ptr(), stream=None, n=2, nseg=2, nq=int(fresh.qtabs.shape[0]),
              nh=int(fresh.htabs.shape[0]), Hc=24, Wc=41)
    for change in (dict(Wc=39), dict(Hc=23), dict(n=0), dict(nseg=1), dict(nseg=3), dict(nq=1), dict(nh=2), dict(nbytes=10),
                   dict(scratch_bytes=scratch.numel() - 1), dict(scratch=scratch.data_ptr() + 8), dict(images_host=None),
                   dict(out=None), dict(status=None)):
        args = _lib.JpegDecodeArgs(**dict(ok, **change))
        assert _lib.lib().istvt_jpeg_decode_u8(ctypes.byref(args)) == -3, change
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
