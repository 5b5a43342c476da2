"""JPEG files without restart markers on a real MI355X: ops.jpeg_decode_u8(..., split=chunk) against the default
call and the integer definition clips.jpeg_decode_host, byte for byte; the state rows it leaves in the scratch against the
host model clips.jpeg_split_host; damaged files; what it writes and what it leaves alone (sentinel bytes around every buffer
it is given, which is this entry's guard duty); its refusals.  tools/jpeg_entropy_split_check.cpp, the same
csrc/jpeg_entropy_split.h under AddressSanitizer and UBSan on the host, has passed on the fixture files, cut at every length
and with flipped bits, before the kernel ran on a device for the first time: DESIGN.md has the command and its result."""
import os

import numpy as np
import pytest
import torch

from test_jpeg_split_cpu import _smooth, stuffed_boundaries

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


def _buffers(batch, canvas, scratch_bytes, out_offset=1):
    n = batch.n
    out = Guarded((n, canvas[0], canvas[1], 3), torch.uint8, out_offset)
    scratch = Guarded((scratch_bytes,), torch.uint8)
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


def _same_as_default(ops, batch, chunk, canvas=None):
    """the split call against the default call: frames, sizes, status and the coefficients in the scratch -> the split
    call's (frames, status, scratch)"""
    from istvt_amd import clips
    plan = clips.jpeg_split_plan(batch, chunk)
    n = batch.n
    bufs = [(torch.full((nb,), fill, dtype=torch.uint8, device='cuda'), torch.empty((n, 2), dtype=torch.int32, device='cuda'),
             torch.empty((n,), dtype=torch.int32, device='cuda')) for nb, fill in ((batch.scratch_bytes, 0x11), (plan.scratch_bytes, 0xEE))]
    want, ws, wst = ops.jpeg_decode_u8(batch, canvas=canvas, checked=True, buffers=bufs[0])
    got, gs, gst = ops.jpeg_decode_u8(batch, canvas=canvas, checked=True, buffers=bufs[1], split=chunk)
    assert torch.equal(got, want) and torch.equal(gs, ws) and torch.equal(gst, wst), chunk
    assert torch.equal(bufs[1][0][:128 * batch.blocks], bufs[0][0][:128 * batch.blocks]), chunk    # the coefficients
    return got, gst, bufs[1][0]


@pytest.mark.parametrize('chunk', [16, 128])
def test_all_sound_files_in_one_batch(pkg, sound, chunk):
    from istvt_amd import clips, ops
    batch = clips.jpeg_batch([d for _, d, _ in sound])
    got, st, _ = _same_as_default(ops, batch, chunk, canvas=(48, 72))
    _check_canvas(got, [r for _, _, r in sound])
    assert not bool(st.any())


@pytest.mark.parametrize('sub,q', [('420', 75), ('444', 90)])
def test_encoder_files_without_restarts_and_their_states(pkg, sub, q):
    """64 x 80 from clips.jpeg_encode_host, one segment: the state rows equal the host model's.  The 4:4:4 scan is longer than
    256 chunks of 16 bytes, so there the chunk grows; at chunk 64 the 4:2:0 file takes several rounds."""
    from istvt_amd import clips, ops
    data = clips.jpeg_encode_host(_smooth(64, 80, 1), q, sub, 0)
    ref = clips.jpeg_decode_host(data)
    hd = clips.jpeg_parse(data)
    batch = clips.jpeg_batch([hd])
    (begin, end), = hd.segments
    assert sub == '420' or end - begin > 256 * 16
    for chunk in (16, 32, 64):
        got, st, scratch = _same_as_default(ops, batch, chunk)
        _check_canvas(got, [ref])
        assert st.tolist() == [0]
        plan, host = clips.jpeg_split_plan(batch, chunk), clips.jpeg_split_host(hd, chunk)
        assert plan.row0 == [0] and plan.count == [len(host.segments[0].states)] and plan.chunk == [host.segments[0].chunk]
        rows = scratch[plan.states_at:plan.states_at + 32 * plan.count[0]].view(torch.int32).view(-1, 8).cpu()
        want = torch.tensor(host.segments[0].rows, dtype=torch.int32)
        want[:, 0] -= begin                                       # the batch holds the scan alone
        assert torch.equal(rows, want), (chunk, int((rows != want).any(1).nonzero()[0]))
        assert chunk != 64 or sub != '420' or host.rounds >= 2


def test_boundaries_on_stuffed_zeros(pkg, files, sound):
    from istvt_amd import clips, ops
    found = stuffed_boundaries(clips, files)
    assert found
    pick = {n: (d, r) for n, d, r in sound}
    for name in sorted({n for n, _ in found}):
        chunks = [c for n, c in found if n == name]
        batch = clips.jpeg_batch([pick[name][0]])
        for chunk in (chunks[0], chunks[-1]):
            got, st, _ = _same_as_default(ops, batch, chunk)
            _check_canvas(got, [pick[name][1]])
            assert st.tolist() == [0]


def test_mixed_restart_intervals(pkg):
    """row-restart, every-MCU-restart and restart-less files in one batch"""
    from istvt_amd import clips, ops
    x = _smooth(33, 70, 3370)
    data = [clips.jpeg_encode_host(x, 75, '420', 'row'), clips.jpeg_encode_host(x, 90, '444', 1),
            clips.jpeg_encode_host(x, 75, '420', 0), clips.jpeg_encode_host(x[:17, :33], 40, '444', 0),
            clips.jpeg_encode_host(x, 95, '444', 'row')]
    batch = clips.jpeg_batch(data)
    refs = [clips.jpeg_decode_host(d) for d in data]
    for chunk in (16, 48):
        got, st, _ = _same_as_default(ops, batch, chunk)
        _check_canvas(got, refs)
        assert not bool(st.any())


def test_damaged_files_between_sound_ones(pkg, files, sound):
    from istvt_amd import clips, ops
    pick = {n: (d, r) for n, d, r in sound if n in ('24x40_s2_q75', '17x33_s0_q95', '33x70_s2_q75_rb1', '16x16_s2_q30')}
    order = ['24x40_s2_q75', 'damaged_cut', '17x33_s0_q95', 'damaged_code', '33x70_s2_q75_rb1', 'damaged_run', '16x16_s2_q30',
             'truncated', '24x40_s2_q75']
    whole = bytes(files['file_33x70_s2_q75'])                     # one segment
    hd = clips.jpeg_parse(whole)
    assert len(hd.segments) == 1
    truncated = whole[:hd.segments[0][0] + (hd.segments[-1][1] - hd.segments[0][0]) * 3 // 5]       # no EOI: the scan ends early
    named = dict(truncated=truncated)
    data = [pick[k][0] if k in pick else named.get(k) or bytes(files['file_' + k]) for k in order]
    want = [clips.jpeg_decode_host(d, return_status=True)[1] for d in data]
    recorded = dict(zip(files['damaged'].tolist(), files['damaged_status'].tolist()))
    assert want == [recorded.get(k, 0) for k in order[:7]] + [1, 0] == [0, 1, 0, 2, 0, 3, 0, 1, 0]
    batch = clips.jpeg_batch(data)
    for chunk in (16, 37, 128):
        assert [clips.jpeg_split_host(d, chunk).status for d in data] == want
        got, st, _ = _same_as_default(ops, batch, chunk)
        assert st.tolist() == want
        host = got.cpu()
        for i, k in enumerate(order):
            if k in pick:
                h, w = pick[k][1].shape[:2]
                assert torch.equal(host[i, :h, :w], pick[k][1]), k
            else:
                h, w = (33, 70) if k == 'truncated' else (24, 40)
            assert int(host[i, h:].any()) == 0 and int(host[i, :, w:].any()) == 0, k


def test_guards_and_a_scratch_that_held_anything(pkg, sound):
    from istvt_amd import clips, ops
    batch = clips.jpeg_batch([d for _, d, _ in sound])
    plan = clips.jpeg_split_plan(batch, 32)
    out, scratch, sizes, status = _buffers(batch, (48, 72), plan.scratch_bytes)
    assert out.t.data_ptr() % 2 == 1
    source = batch.on(out.t.device).data.clone()
    ops.kernel_profile = []
    try:
        scratch.t.fill_(0xC3)
        got, s, st = ops.jpeg_decode_u8(batch, canvas=(48, 72), out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t),
                                        split=32)
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_decode_split_u8']
    assert got is out.t and s is sizes.t and st is status.t
    _check_canvas(got, [r for _, _, r in sound])
    assert s.tolist() == [list(r.shape[:2]) for _, _, r in sound] and not bool(st.any())
    assert out.intact() and scratch.intact() and sizes.intact() and status.intact()
    assert torch.equal(batch.on(out.t.device).data, source)
    first, front = got.clone(), scratch.t[:192 * batch.blocks + 4 * batch.segments.shape[0]].clone()
    rows = [scratch.t[plan.states_at + 32 * r0:plan.states_at + 32 * (r0 + c)].clone() for r0, c in zip(plan.row0, plan.count)]
    scratch.t.fill_(0x3C)                                         # nothing may depend on what the scratch held
    again, _, st2 = ops.jpeg_decode_u8(batch, canvas=(48, 72), checked=True, buffers=(scratch.t, sizes.t, status.t), split=32)
    assert torch.equal(again, first) and not bool(st2.any()) and scratch.intact()
    assert torch.equal(scratch.t[:front.numel()], front)
    for r0, c, want in zip(plan.row0, plan.count, rows):
        assert torch.equal(scratch.t[plan.states_at + 32 * r0:plan.states_at + 32 * (r0 + c)], want)


def test_refusals(pkg, sound):
    """each of them before any launch: a sentinel-filled `out` stays as it is"""
    import ctypes
    from istvt_amd import _lib, clips, ops
    data = [d for n, d, _ in sound if n in ('24x40_s2_q75', '17x33_s0_q95')]
    batch = clips.jpeg_batch(data)
    out = torch.full((2, 24, 40, 3), SENTINEL, dtype=torch.uint8, device='cuda')
    for bad in (8, 1.5, 'row', True, 0, -16):
        with pytest.raises(ValueError, match='split is None, .auto. or a chunk size'):
            ops.jpeg_decode_u8(batch, out=out, split=bad)
        with pytest.raises(ValueError, match='split'):
            ops.decode_frames(data, 16, split=bad)
    plan = clips.jpeg_split_plan(batch, 16)
    assert plan.scratch_bytes > batch.scratch_bytes
    small = (torch.empty((batch.scratch_bytes,), dtype=torch.uint8, device='cuda'),
             torch.empty((2, 2), dtype=torch.int32, device='cuda'), torch.empty((2,), dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='buffers = .uint8 scratch of %d bytes' % plan.scratch_bytes):
        ops.jpeg_decode_u8(batch, out=out, buffers=small, split=16)
    ops.jpeg_decode_u8(batch, buffers=small)                      # the default call takes them
    # the entry itself
    d = batch.on(out.device)
    scratch = torch.empty((plan.scratch_bytes,), dtype=torch.uint8, device='cuda')
    ok = dict(bytes=d.data.data_ptr(), nbytes=batch.nbytes, images=d.images.data_ptr(), images_host=batch.images.data_ptr(),
              segments=d.segments.data_ptr(), segments_host=batch.segments.data_ptr(), qtabs=d.qtabs.data_ptr(),
              htabs=d.htabs.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), out=out.data_ptr(),
              sizes=small[1].data_ptr(), status=small[2].data_ptr(), stream=None, n=2, nseg=2, nq=int(batch.qtabs.shape[0]),
              nh=int(batch.htabs.shape[0]), Hc=24, Wc=40)
    entry = _lib.lib().istvt_jpeg_decode_split_u8
    for change, chunk in ((dict(), 15), (dict(), 0), (dict(scratch_bytes=plan.scratch_bytes - 1), 16), (dict(Wc=39), 16),
                          (dict(nseg=3), 16), (dict(scratch=scratch.data_ptr() + 8), 16), (dict(status=None), 16),
                          (dict(scratch_bytes=clips.jpeg_split_plan(batch, 128).scratch_bytes), 16)):
        assert entry(ctypes.byref(_lib.JpegDecodeArgs(**dict(ok, **change))), chunk) == -3, (change, chunk)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert entry(ctypes.byref(_lib.JpegDecodeArgs(**ok)), 16) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.jpeg_decode_u8(batch)[0])


def test_decode_frames_passes_the_split_on(pkg, sound):
    from istvt_amd import ops
    pick = {n: d for n, d, _ in sound}
    data = [pick[k] for k in ('48x48_s2_q75', '33x70_s0_q75_rr1', '24x40_s2_q30', '17x33_s2_q75_opt')]
    from istvt_amd import clips
    long_file = clips.jpeg_encode_host(_smooth(64, 80, 1), 90, '444', 0)
    short = max(e - b for d in data for b, e in clips.jpeg_parse(d).segments)
    assert short <= clips.JPEG_SPLIT_AUTO_BYTES < max(e - b for b, e in clips.jpeg_parse(long_file).segments)
    want, want_long = ops.decode_frames(data, 32), ops.decode_frames(data + [long_file], 32)
    ops.kernel_profile = []
    try:
        got = ops.decode_frames(data, 32, split=16)
        auto = ops.decode_frames(data, 32, split='auto')          # no segment long enough: the default path
        auto_long = ops.decode_frames(data + [long_file], 32, split='auto')
        record = [r[0] for r in ops.kernel_profile if r[0].startswith('jpeg_decode')]
    finally:
        ops.kernel_profile = None
    assert torch.equal(got, want) and torch.equal(auto, want) and torch.equal(auto_long, want_long)
    assert record == ['jpeg_decode_split_u8', 'jpeg_decode_u8', 'jpeg_decode_split_u8']
