"""JPEG files out (DESIGN.md "JPEG files out") on a real MI355X: ops.jpeg_encode_u8 against the integer definition
clips.jpeg_encode_host, byte for byte; the coder's paths that smooth images miss; files that do not fit; what the call writes
and what it leaves alone (sentinel bytes around every buffer it is given); the loop through ops.jpeg_decode_u8;
ops.encode_frames; VideoScorer.render_explanation(jpeg_quality=); the statuses of a device quality table; the entry's own
refusals."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                   # sentinel bytes on each side of a buffer
SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (24, 40), (33, 70), (48, 48))       # the sizes of the J2 fixture
QUALITIES = (30, 75, 95, 100)


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


def _noise():
    """the 40 x 56 uniform noise of tests/golden/make_jpeg_files_golden.py"""
    return torch.from_numpy(np.random.default_rng(4056).integers(0, 256, (40, 56, 3), dtype=np.uint8))


_HOST = {}


def _host(key, x, q, sub, ri):
    """clips.jpeg_encode_host, once per (key, q, sub, ri) of the module: the definition is pure Python"""
    from istvt_amd import clips
    k = (key, q, sub, ri)
    if k not in _HOST:
        _HOST[k] = clips.jpeg_encode_host(x, q, sub, ri)
    return _HOST[k]


def _coefficients(x, q, sub):
    """what jpeg_encode_host codes: per component int32 (blocks, 64) in zig-zag order, blocks in plane order"""
    from istvt_amd import clips
    qt, zz = clips.jpeg_quant_tables(q), torch.tensor(clips.JPEG_ZIGZAG)
    out = []
    for c, p in enumerate(clips._jpeg_planes_in(x[None], clips.JPEG_SUBSAMPLINGS[sub])):
        k = clips._jpeg_quantise(p, qt[min(c, 1)][None])[0].permute(0, 2, 1, 3)
        out.append(k.reshape(-1, 64)[:, zz])
    return out


def _longest_coded_run(coef):
    """the longest run of zeros in front of a non-zero AC coefficient"""
    best = 0
    for c in coef:
        for blk in c.tolist():
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                else:
                    best, run = max(best, run), 0
    return best


def _differ(got, want):
    return [(i, len(g), len(w), next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), -1))
            for i, (g, w) in enumerate(zip(got, want)) if g != w]


@pytest.mark.parametrize('ri', [0, 1, 2, 5, 'row'])
@pytest.mark.parametrize('sub', ['420', '444'])
def test_equals_the_host_definition(pkg, sub, ri):
    """every size of the fixture, four frames per call with the four qualities as the per-frame table"""
    from istvt_amd import clips, ops
    q = torch.tensor(QUALITIES, dtype=torch.int32)
    for h, w in SIZES:
        x = torch.stack([_smooth(h, w, 1000 * h + 10 * w + i) for i in range(4)])
        want = [_host((h, w, i), x[i], QUALITIES[i], sub, ri) for i in range(4)]
        # (the default capacity, 3 bytes per pixel + the header, is less than a 1 x 1 file: a whole MCU is coded)
        res = ops.jpeg_encode_u8(x.cuda(), q, sub, ri, capacity=4 * (3 * h * w + 1024))
        assert isinstance(res, clips.JpegFiles) and res.data.is_cuda and res.offsets.dtype == torch.int64
        assert res.status.tolist() == [0, 0, 0, 0], (h, w)
        got = res.files()
        assert got == want, ((h, w), _differ(got, want))
        assert res.nbytes() == sum(len(f) for f in want) and res.offsets[0].item() == 0
    if sub == '444' and ri == 1:                                  # 36 segments: the RSTm numbering wraps past 7 four times
        hd = clips.jpeg_parse(got[1])
        assert len(hd.segments) == 36 and got[1].count(b'\xff\xd7') >= 4


def test_per_frame_qualities(pkg):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(24, 40, 240 + i) for i in range(6)])
    q = torch.tensor([30, 75, 95, 100, 1, 50], dtype=torch.int32)
    want = clips.jpeg_encode_files_host(x, q)
    assert len({f[25:89] for f in want}) == 6                     # six different luminance tables
    ops.kernel_profile = []
    try:
        got = ops.jpeg_encode_u8(x.cuda(), q).files()
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_encode_u8']
    assert got == want, _differ(got, want)


def test_clips_share_their_quality(pkg):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(16, 24, 1624 + i) for i in range(6)]).view(2, 3, 16, 24, 3)
    q = torch.tensor([40, 90], dtype=torch.int32)
    res = ops.jpeg_encode_u8(x.cuda(), q, '444', 2)
    want = clips.jpeg_encode_files_host(x, q, '444', 2)
    assert len(res) == 6 and res.files() == want
    assert want[0] == clips.jpeg_encode_host(x[0, 0], 40, '444', 2) and want[5] == clips.jpeg_encode_host(x[1, 2], 90, '444', 2)


def _special(name):
    yy, xx = np.mgrid[0:40, 0:56]

    def grey(a):
        return torch.from_numpy(a.clip(0, 255).astype(np.uint8))[..., None].repeat(1, 1, 3).contiguous()
    if name == 'noise':
        return _noise(), 100, '444'
    if name == 'blocks':                                          # black and white 8 x 8 blocks
        return grey(((yy // 8 + xx // 8) % 2) * 255), 100, '444'
    if name == 'pixels':                                          # a checkerboard of single pixels
        return grey(((yy + xx) % 2) * 255), 100, '420'
    if name == 'zero':
        return torch.zeros((40, 56, 3), dtype=torch.uint8), 75, '420'
    return grey(128 + ((yy + xx) % 2) * 40 + xx), 50, '444'        # 'ripple': a faint pixel checkerboard on a ramp


@pytest.mark.parametrize('name', ['noise', 'blocks', 'pixels', 'zero', 'ripple'])
def test_paths_that_smooth_images_miss(pkg, name):
    """each input is looked at on the host first: the coefficients jpeg_encode_host codes do take the path in question"""
    from istvt_amd import ops
    x, q, sub = _special(name)
    coef = _coefficients(x, q, sub)
    every = torch.cat(coef)
    host = _host(name, x, q, sub, 'row')
    if name == 'noise':                                           # long codes, and many FF bytes to stuff
        assert int(every[:, 1:].abs().max()) > 127 and host.count(b'\xff\x00') > 40 and len(host) > x.numel()
        assert bool((every[:, 63] != 0).all())
    elif name == 'blocks':                                        # DC differences in category 11, nothing else
        dc = coef[0][:, 0]
        assert int((dc[1:] - dc[:-1]).abs().max()) >= 1024 and int(every[:, 1:].abs().max()) == 0
    elif name == 'pixels':                                        # AC values in category 10, a coded last coefficient
        assert int(every[:, 1:].abs().max()) >= 512 and int((every[:, 63] != 0).sum()) > 0
    elif name == 'zero':                                          # DC and EOB in every block
        assert int(every[:, 1:].abs().max()) == 0 and len(set(coef[0][:, 0].tolist())) == 1
    else:                                                         # runs past 16 and 32 (ZRL), then a coded last coefficient: no EOB
        assert _longest_coded_run(coef) >= 48 and int((every[:, 63] != 0).sum()) > 0
    for ri in ('row', 0):
        res = ops.jpeg_encode_u8(x[None].cuda(), q, sub, ri, capacity=16384)
        want = [_host(name, x, q, sub, ri)]
        assert res.status.tolist() == [0]
        assert res.files() == want, (ri, _differ(res.files(), want))


def test_a_file_that_does_not_fit(pkg):
    """40 x 56 uniform noise at quality 100, 4:4:4: 9783 bytes against 6720 raw ones and a default capacity of 7349"""
    from istvt_amd import clips, ops
    x = _noise()
    want = _host('noise', x, 100, '444', 'row')
    assert len(want) == 9783 and x.numel() == 6720
    out = torch.full((6720 + 629,), 0xA5, dtype=torch.uint8, device='cuda')
    res = ops.jpeg_encode_u8(x[None].cuda(), 100, '444', out=out)
    assert res.data is out and res.status.tolist() == [1] and res.offsets.tolist() == [0, 9783] and res.nbytes() == 9783
    assert bool((out == 0xA5).all())                              # not one byte of it is written
    with pytest.raises(ValueError, match='file 0 has status 1 .*does not fit'):
        res.files()
    assert res.files(check=False) == [b'']
    default = ops.jpeg_encode_u8(x[None].cuda(), 100, '444')
    assert default.data.numel() == 6720 + len(clips.jpeg_header(40, 56, 100, '444', 'row')) and default.status.tolist() == [1]
    again = ops.jpeg_encode_u8(x[None].cuda(), 100, '444', capacity=int(res.offsets[-1]))
    assert again.status.tolist() == [0] and again.files() == [want] and again.data.numel() == 9783
    # a batch whose buffer holds only the first file
    smooth = _smooth(40, 56, 4056)
    first = _host('smooth4056', smooth, 100, '444', 'row')
    batch = torch.stack([smooth, x, smooth]).cuda()
    out = torch.full((len(first) + 5000,), 0x5A, dtype=torch.uint8, device='cuda')
    res = ops.jpeg_encode_u8(batch, 100, '444', out=out)
    assert res.status.tolist() == [0, 1, 1]
    assert res.offsets.tolist() == [0, len(first), len(first) + 9783, 2 * len(first) + 9783]
    assert bytes(out[:len(first)].cpu().numpy()) == first and bool((out[len(first):] == 0x5A).all())
    assert res.files(check=False) == [first, b'', b'']


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
def test_guard_bands(pkg, sub, ri):
    """`data` (at an odd address), the scratch, offsets and status between 4 KiB of sentinel bytes, with two different fills:
    every byte of data[:offsets[n]] is written, every byte behind keeps the fill, no band is touched, the frames stay"""
    from istvt_amd import clips, frames as F
    n, H, W = 3, 33, 70
    x = torch.stack([_smooth(H, W, 3370 + i) for i in range(n)])
    q = [75, 95, 30]
    want = b''.join(_host(('guard', i), x[i], q[i], sub, ri) for i in range(n))
    step = clips.JPEG_SUBSAMPLINGS[sub]
    mcus = (-(-H // (8 * step))) * (-(-W // (8 * step)))
    r = clips.jpeg_restart_interval(ri, W, sub)
    blocks, segments = n * mcus * (step * step + 2), n * -(-mcus // r)
    dev = x.cuda()
    qdev = torch.tensor(q, dtype=torch.int32).cuda()
    header, hlen = F._jpeg_header_on(dev.device, H, W, sub, r)
    results = []
    for fill in (0xA5, 0x3C):
        data = Guarded((len(want) + 777,), torch.uint8, fill, offset=1)
        scratch = Guarded((128 * blocks + 16 * segments,), torch.uint8, fill)
        offsets, status = Guarded((n + 1,), torch.int64, fill), Guarded((n,), torch.int32, fill)
        assert data.t.data_ptr() % 2 == 1 and scratch.t.data_ptr() % 16 == 0
        F._jpeg_encode_launch(dev, dev.numel(), qdev, header, hlen, scratch.t, data.t, offsets.t, status.t, n, H, W, step, r)
        torch.cuda.synchronize()
        assert status.t.tolist() == [0, 0, 0] and offsets.t[-1].item() == len(want)
        assert bytes(data.t[:len(want)].cpu().numpy()) == want
        assert bool((data.t[len(want):] == fill).all())
        assert data.intact() and scratch.intact() and offsets.intact() and status.intact()
        results.append(data.t[:len(want)].clone())
    assert torch.equal(results[0], results[1]) and torch.equal(dev.cpu(), x)
    # one byte less of scratch, or a scratch off its alignment: refused before any launch
    args = dict(frames=dev.data_ptr(), total=dev.numel(), quality=qdev.data_ptr(), header=header.data_ptr(), header_bytes=hlen,
                scratch=scratch.t.data_ptr(), scratch_bytes=scratch.t.numel(), data=data.t.data_ptr(), capacity=data.t.numel(),
                offsets=offsets.t.data_ptr(), status=status.t.data_ptr(), stream=None, n=n, H=H, W=W,
                subsampling=2 if sub == '420' else 0, restart_interval=r, dqt0=25, dqt1=94)
    from istvt_amd import _lib
    data.t.fill_(0x77)
    for change in (dict(scratch_bytes=scratch.t.numel() - 1), dict(scratch=scratch.t.data_ptr() + 8), dict(n=0), dict(H=0),
                   dict(W=16385), dict(subsampling=1), dict(restart_interval=-1), dict(restart_interval=65536), dict(capacity=-1),
                   dict(total=dev.numel() - 1), dict(header=None), dict(header_bytes=100), dict(dqt1=60), dict(dqt1=hlen - 63),
                   dict(data=None), dict(offsets=None), dict(status=None), dict(quality=None),
                   dict(data=dev.data_ptr() + 10), dict(offsets=offsets.t.data_ptr() + 4)):
        assert _lib.lib().istvt_jpeg_encode_u8(ctypes.byref(_lib.JpegEncodeArgs(**dict(args, **change)))) == -3, change
    torch.cuda.synchronize()
    assert bool((data.t == 0x77).all()) and torch.equal(dev.cpu(), x)


@pytest.mark.parametrize('sub', ['420', '444'])
def test_the_loop_closes_on_the_device(pkg, sub):
    from istvt_amd import ops
    x = torch.stack([_smooth(33, 70, 70 + i) for i in range(3)] + [_smooth(33, 70, 99)]).cuda()
    q = torch.tensor([30, 75, 95, 100], dtype=torch.int32)
    files = ops.jpeg_encode_u8(x, q, sub)
    frames, sizes, status = ops.jpeg_decode_u8(files.files())
    assert status.tolist() == [0, 0, 0, 0] and sizes.tolist() == [[33, 70]] * 4
    assert torch.equal(frames, ops.jpeg_roundtrip_u8(x, q, sub))
    again, _, _ = ops.jpeg_decode_u8(files)                        # the JpegFiles itself
    assert torch.equal(again, frames)


def test_crop_and_encode(pkg):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(64, 96, 6496 + i) for i in range(3)])
    boxes = torch.tensor([[4, 6, 40, 36], [1, 30, 62, 60], [0, 0, 64, 96]], dtype=torch.int32)
    res = ops.encode_frames(x.cuda(), 24, boxes=boxes, quality=80)
    want = clips.jpeg_encode_files_host(clips.crop_resize_host(x, boxes, 24), 80)
    assert res.files() == want
    M = clips.similarity_of_boxes(torch.tensor([[4, 6, 40, 40], [1, 30, 62, 62], [0, 16, 64, 64]], dtype=torch.int32), 24)
    warped = ops.encode_frames(x.cuda(), 24, transforms=M, quality=60, subsampling='444', restart_interval=0)
    crops = ops.warp_similarity_u8(x.cuda(), M, 24).cpu()
    assert warped.files() == clips.jpeg_encode_files_host(crops, 60, '444', 0)
    assert torch.equal(ops.decode_frames(res, 24), ops.decode_frames(want, 24))


def test_rendered_explanations_leave_as_files(pkg):
    """the geometry of tests/test_paste_gpu.py: 120 x 160 frames, crops of side 96, XceptionVidTr(num_frames=4, grid=6,
    depth=1); maps and weights that paste something"""
    from istvt_amd import clips, video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    n, side = 4, 96
    model = XceptionVidTr(num_frames=4, grid=6, depth=1).cuda()
    x = torch.stack([_smooth(120, 160, 120160 + i) for i in range(n)])
    boxes = torch.tensor([[10 + 5 * i, 15 + 9 * i, 70 + i, 80 + 2 * i] for i in range(n)], dtype=torch.int32)
    gen = torch.Generator().manual_seed(5)
    maps = torch.randn((n, 36), generator=gen).cuda()
    ex = video.VideoExplanation(None, None, maps, maps, torch.rand((n,), generator=gen).cuda(), torch.zeros(n).cuda(),
                                torch.ones(n, dtype=torch.int32).cuda())
    scorer = video.VideoScorer(model, side=side, frame_batch=3)
    plain = scorer.render_explanation(x, ex, boxes=boxes)
    assert plain.dtype == torch.uint8 and not torch.equal(plain.cpu(), x)
    res = scorer.render_explanation(x, ex, boxes=boxes, jpeg_quality=75)
    assert isinstance(res, clips.JpegFiles) and res.status.tolist() == [0] * n
    assert res.files() == clips.jpeg_encode_files_host(plain.cpu(), 75, '420', 'row')
    assert res.nbytes() < plain.numel() // 4


def test_device_table_statuses(pkg):
    from istvt_amd import clips, ops
    x = torch.stack([_smooth(24, 40, 2440 + i) for i in range(4)])
    q = torch.tensor([75, 0, 90, -3], dtype=torch.int32)
    res = ops.jpeg_encode_u8(x.cuda(), q.cuda(), checked=True)
    a, c = clips.jpeg_encode_host(x[0], 75, '420', 'row'), clips.jpeg_encode_host(x[2], 90, '420', 'row')
    assert res.status.tolist() == [0, 2, 0, 2]
    assert res.offsets.tolist() == [0, len(a), len(a), len(a) + len(c), len(a) + len(c)]
    assert res.files(check=False) == [a, b'', c, b'']
    with pytest.raises(ValueError, match='file 1 has status 2 .*quality <= 0'):
        res.files()
    over = ops.jpeg_encode_u8(x[:1].cuda(), torch.tensor([250], dtype=torch.int32).cuda(), checked=True)     # counts as 100
    assert over.files() == [clips.jpeg_encode_host(x[0], 100, '420', 'row')]
    with pytest.raises(RuntimeError, match='a device quality table is taken with checked=True only'):
        ops.jpeg_encode_u8(x.cuda(), q.cuda())
    with pytest.raises(RuntimeError, match='out may not share memory with the frames'):
        d = x.cuda()
        ops.jpeg_encode_u8(d, 50, out=d.view(-1)[100:5000])
    with pytest.raises(RuntimeError, match='out must be contiguous uint8'):
        ops.jpeg_encode_u8(x.cuda(), 50, out=torch.empty((10, 10), dtype=torch.uint8, device='cuda'))
