"""JPEG files out with optimised Huffman tables (DESIGN.md "JPEG files out, optimised tables") on a real MI355X:
ops.jpeg_encode_u8(optimize=True) against clips.jpeg_encode_files_host(optimize=True), every comparison equality of all bytes;
flat frames; the frame whose table runs the length limiting; mixed qualities with an empty file between sound ones; a
capacity one byte short; more than 64 restart intervals in one image; what the entry writes and what it leaves alone (sentinel
bytes around every buffer); its refusals; the decoder on the device's files; and optimize=False as it was."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                   # sentinel bytes on each side of a buffer
SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (24, 40))
QUALITIES = (30, 75, 95, 100)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'J4_jpeg_optimize.npz')


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _smooth(h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return torch.from_numpy(np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8))


_HOST = {}


def _host(key, x, q, sub, ri, optimize=True):
    """clips.jpeg_encode_host, once per case of the module: the definition is pure Python"""
    from istvt_amd import clips
    k = (key, q, sub, ri, optimize)
    if k not in _HOST:
        _HOST[k] = clips.jpeg_encode_host(x, q, sub, ri, optimize=optimize)
    return _HOST[k]


def _differ(got, want):
    return [(i, len(g), len(w), next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), -1))
            for i, (g, w) in enumerate(zip(got, want)) if g != w]


@pytest.mark.parametrize('ri', [0, 'row', 1, 5])
@pytest.mark.parametrize('sub', ['420', '444'])
def test_equals_the_host_definition(pkg, sub, ri):
    """every size, four frames per call with the four qualities as the per-frame table: four header lengths per call"""
    from istvt_amd import clips, ops
    q = torch.tensor(QUALITIES, dtype=torch.int32)
    for h, w in SIZES:
        x = torch.stack([_smooth(h, w, 1000 * h + 10 * w + i) for i in range(4)])
        want = [_host((h, w, i), x[i], QUALITIES[i], sub, ri) for i in range(4)]
        res = ops.jpeg_encode_u8(x.cuda(), q, sub, ri, capacity=4 * (3 * h * w + 1024), optimize=True)
        assert isinstance(res, clips.JpegFiles) and res.status.tolist() == [0, 0, 0, 0], (h, w)
        got = res.files()
        assert got == want, ((h, w), _differ(got, want))
        assert res.nbytes() == sum(len(f) for f in want) and res.offsets[0].item() == 0
    assert len({len(f) - len(_host((24, 40, i), x[i], QUALITIES[i], sub, ri, False)) for i, f in enumerate(want)}) > 1


@pytest.mark.parametrize('name', ['zero', 'grey', 'step'])
def test_flat_frames(pkg, name):
    """tables of one or two codes: a frame of one colour has one DC category per table after the first block and EOB alone"""
    from istvt_amd import clips, ops
    x = torch.zeros((24, 40, 3), dtype=torch.uint8)
    if name == 'grey':
        x += 128
    elif name == 'step':
        x[:, 16:] = 200
    for sub, ri in (('420', 'row'), ('444', 0)):
        want = _host(name, x, 75, sub, ri)
        hd = clips.jpeg_parse(want)
        assert all(len(ac[1]) <= 2 for _, ac in hd.huffman[1:]) and len(hd.huffman[1][1][1]) == 1     # chroma: EOB alone
        if name != 'step':
            assert all(len(dc[1]) <= 2 and len(ac[1]) == 1 for dc, ac in hd.huffman)
        res = ops.jpeg_encode_u8(x[None].cuda(), 75, sub, ri, capacity=4096, optimize=True)
        assert res.status.tolist() == [0] and res.files() == [want], (sub, ri, _differ(res.files(), [want]))


def test_the_length_limited_table(pkg):
    """the recorded 224 x 224 4:4:4 frame whose chroma AC table has code lengths of 17 before T.81 K.2 folds them"""
    from istvt_amd import clips, ops
    golden = np.load(GOLDEN)
    name = str(golden['limit'])
    x = torch.from_numpy(golden['frame_' + name])
    want = _host(name, x, 95, '444', 0)
    assert clips.jpeg_parse(want).huffman == clips.jpeg_parse(bytes(golden['file_' + name])).huffman      # PIL's tables
    assert clips.jpeg_parse(want).huffman[1][1][0][15] > 0
    res = ops.jpeg_encode_u8(x[None].cuda(), 95, '444', 0, optimize=True)
    assert res.status.tolist() == [0]
    got = res.files()
    assert got == [want], _differ(got, [want])


def test_mixed_qualities_and_an_empty_file(pkg):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(24, 40, 2440 + i) for i in range(5)])
    q = [30, 100, 0, 75, -3]
    want = [_host(('mixed', i), x[i], q[i], '420', 'row') if q[i] > 0 else b'' for i in range(5)]
    heads = {clips.jpeg_parse(f).segments[0][0] for f in want if f}
    assert len(heads) > 1                                         # header lengths differ: the offsets carry them
    res = ops.jpeg_encode_u8(x.cuda(), torch.tensor(q, dtype=torch.int32).cuda(), checked=True, optimize=True)
    assert res.status.tolist() == [0, 0, 2, 0, 2]
    assert res.offsets.tolist() == [0] + list(np.cumsum([len(f) for f in want]))
    assert res.files(check=False) == want


def test_a_capacity_one_byte_short(pkg):
    """status 1 for the file that does not fit, the true sizes in offsets, not a byte of it written, its neighbours whole"""
    from istvt_amd import ops
    x = torch.stack([_smooth(24, 40, 2440 + i) for i in range(3)])
    qs = (30, 100, 60)
    want = [_host(('mixed', i), x[i], qs[i], '420', 'row') for i in range(2)] + [_host(('short', 2), x[2], 60, '420', 'row')]
    q = torch.tensor(qs, dtype=torch.int32)
    sizes = [len(f) for f in want]
    out = torch.full((sum(sizes) - 1,), 0xA5, dtype=torch.uint8, device='cuda')
    res = ops.jpeg_encode_u8(x.cuda(), q, out=out, optimize=True)
    assert res.status.tolist() == [0, 0, 1] and res.offsets.tolist() == [0, sizes[0], sum(sizes[:2]), sum(sizes)]
    assert bytes(out[:sum(sizes[:2])].cpu().numpy()) == want[0] + want[1] and bool((out[sum(sizes[:2]):] == 0xA5).all())
    assert res.files(check=False) == want[:2] + [b'']
    again = ops.jpeg_encode_u8(x.cuda(), q, capacity=res.nbytes(), optimize=True)
    assert again.status.tolist() == [0, 0, 0] and again.files() == want


def test_more_than_64_restart_intervals(pkg):
    """8 x 600 at interval 1: 75 intervals at 4:4:4 for the 64 lanes of an image's workgroup, and the RSTm numbering wraps"""
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(8, 600, 8600 + i) for i in range(2)])
    for sub, segments in (('444', 75), ('420', 38)):
        want = [_host(('wide', i), x[i], 85, sub, 1) for i in range(2)]
        assert len(clips.jpeg_parse(want[0]).segments) == segments
        res = ops.jpeg_encode_u8(x.cuda(), 85, sub, 1, optimize=True)
        assert res.status.tolist() == [0, 0] and res.files() == want, _differ(res.files(), want)


class Guarded:
    """a buffer of `shape` with GUARD sentinel bytes on each side, `offset` bytes past an aligned address"""

    def __init__(self, shape, dtype, fill, offset=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.fill = fill
        self.raw = torch.full((2 * GUARD + n + 256,), fill, dtype=torch.uint8, device='cuda')
        self.lo = GUARD + (-self.raw.data_ptr() - GUARD) % 256 + offset
        self.hi = self.lo + n
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.hi:] == self.fill).all())


@pytest.mark.parametrize('sub,ri', [('420', 'row'), ('444', 2)])
def test_guard_bands_and_refusals(pkg, sub, ri):
    """`data` (at an odd address), the scratch, offsets and status between 4 KiB of sentinel bytes, with two different fills:
    every byte of data[:offsets[n]] is written, every byte behind keeps the fill, no band is touched, the frames stay; an
    image whose quality is <= 0 sits between the sound ones.  Then what the entry refuses before any launch."""
    from istvt_amd import _lib, clips, frames as F
    n, H, W = 4, 33, 70
    x = torch.stack([_smooth(H, W, 3370 + i) for i in range(n)])
    q = [75, 95, 0, 30]
    want = b''.join(_host(('guard', i), x[i], q[i], sub, ri) for i in range(n) if q[i] > 0)
    step = clips.JPEG_SUBSAMPLINGS[sub]
    mcus = (-(-H // (8 * step))) * (-(-W // (8 * step)))
    r = clips.jpeg_restart_interval(ri, W, sub)
    blocks, segments = n * mcus * (step * step + 2), n * -(-mcus // r)
    need = F.jpeg_encode_scratch_bytes(blocks, segments, n, True)
    assert need == 128 * blocks + 16 * segments + 3344 * n
    dev = x.cuda()
    qdev = torch.tensor(q, dtype=torch.int32).cuda()
    header, hlen = F._jpeg_header_on(dev.device, H, W, sub, r)
    results = []
    for fill in (0xA5, 0x3C):
        data = Guarded((len(want) + 777,), torch.uint8, fill, offset=1)
        scratch = Guarded((need,), torch.uint8, fill)
        offsets, status = Guarded((n + 1,), torch.int64, fill), Guarded((n,), torch.int32, fill)
        assert data.t.data_ptr() % 2 == 1 and scratch.t.data_ptr() % 16 == 0
        F._jpeg_encode_launch(dev, dev.numel(), qdev, header, hlen, scratch.t, data.t, offsets.t, status.t, n, H, W, step, r, True)
        torch.cuda.synchronize()
        assert status.t.tolist() == [0, 0, 2, 0] and offsets.t[-1].item() == len(want)
        assert bytes(data.t[:len(want)].cpu().numpy()) == want
        assert bool((data.t[len(want):] == fill).all())
        assert data.intact() and scratch.intact() and offsets.intact() and status.intact()
        row = scratch.t[128 * blocks + 16 * segments + 2 * 3344:][:3344]
        assert bool((row == fill).all())                          # the row of the image without a file is not written
        results.append(data.t[:len(want)].clone())
    assert torch.equal(results[0], results[1]) and torch.equal(dev.cpu(), x)
    args = dict(frames=dev.data_ptr(), total=dev.numel(), quality=qdev.data_ptr(), header=header.data_ptr(), header_bytes=hlen,
                scratch=scratch.t.data_ptr(), scratch_bytes=need, data=data.t.data_ptr(), capacity=data.t.numel(),
                offsets=offsets.t.data_ptr(), status=status.t.data_ptr(), stream=None, n=n, H=H, W=W,
                subsampling=2 if sub == '420' else 0, restart_interval=r, dqt0=25, dqt1=94)
    dht = clips.JPEG_HEADER_DHT
    data.t.fill_(0x77)
    entry = _lib.lib().istvt_jpeg_encode_opt_u8
    for change in (dict(scratch_bytes=need - 1), dict(scratch_bytes=128 * blocks + 16 * segments), dict(scratch=scratch.t.data_ptr() + 8),
                   dict(n=0), dict(H=0), dict(W=16385), dict(subsampling=1), dict(restart_interval=-1), dict(restart_interval=65536),
                   dict(capacity=-1), dict(total=dev.numel() - 1), dict(header=None), dict(header_bytes=100), dict(dqt1=60),
                   dict(data=None), dict(offsets=None), dict(status=None), dict(quality=None), dict(data=dev.data_ptr() + 10),
                   dict(offsets=offsets.t.data_ptr() + 4)):
        assert entry(ctypes.byref(_lib.JpegEncodeArgs(**dict(args, **change))), *dht) == -3, change
    for bad in ((dht[0], dht[0]), (157, dht[1]), (dht[0], hlen + 1), (dht[1], dht[0]), (-1, dht[1])):
        assert entry(ctypes.byref(_lib.JpegEncodeArgs(**args)), *bad) == -3, bad
    torch.cuda.synchronize()
    assert bool((data.t == 0x77).all()) and torch.equal(dev.cpu(), x)


@pytest.mark.parametrize('sub', ['420', '444'])
def test_the_decoder_on_the_devices_files(pkg, sub):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(33, 70, 70 + i) for i in range(4)]).cuda()
    q = torch.tensor([30, 75, 95, 100], dtype=torch.int32)
    opt, std = ops.jpeg_encode_u8(x, q, sub, optimize=True), ops.jpeg_encode_u8(x, q, sub)
    assert opt.nbytes() < std.nbytes()
    frames, sizes, status = ops.jpeg_decode_u8(opt.files())
    assert status.tolist() == [0, 0, 0, 0] and sizes.tolist() == [[33, 70]] * 4
    assert torch.equal(frames, ops.jpeg_decode_u8(std.files())[0]) and torch.equal(frames, ops.jpeg_roundtrip_u8(x, q, sub))
    crops = ops.encode_frames(x, 24, boxes=clips.whole_boxes([(33, 70)] * 4), quality=80, optimize=True)
    host = clips.jpeg_encode_files_host(ops.crop_resize_u8(x, clips.whole_boxes([(33, 70)] * 4), 24).cpu(), 80, optimize=True)
    assert crops.files() == host


def test_the_default_is_as_it_was(pkg):
    """optimize=False: the bytes of the call without the argument, and the one record it made before"""
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(24, 40, 240 + i) for i in range(3)])
    q = torch.tensor([30, 75, 95], dtype=torch.int32)
    ops.kernel_profile = []
    try:
        plain = ops.jpeg_encode_u8(x.cuda(), q).files()
        off = ops.jpeg_encode_u8(x.cuda(), q, optimize=False).files()
        on = ops.jpeg_encode_u8(x.cuda(), q, optimize=True).files()
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_encode_u8', 'jpeg_encode_u8', 'jpeg_encode_opt_u8']
    assert plain == off == clips.jpeg_encode_files_host(x, q) and on == clips.jpeg_encode_files_host(x, q, optimize=True)
    default = ops.jpeg_encode_u8(x.cuda(), q, optimize=True)
    assert default.data.numel() == 3 * (24 * 40 * 3 + clips.jpeg_header_bound(24, 40, '420', 'row'))
    with pytest.raises(ValueError, match='jpeg_encode_u8: optimize'):
        ops.jpeg_encode_u8(x.cuda(), q, optimize=1)
