"""JPEG files out in the layouts 4:2:2 and greyscale (DESIGN.md "JPEG files out, 4:2:2 and greyscale") on a real MI355X:
ops.jpeg_encode_u8(layout=) against clips.jpeg_encode_files_host(layout=), every comparison equality of all bytes, with the
Annex K.3 tables and with every file's own; the sizes at which the coefficient kernel can go wrong (an odd width, a second
luma block wholly outside the frame, a third tile that holds one MCU and a replicated half); clip batches; what the entry
writes and what it leaves alone (sentinel bytes around every buffer); its statuses and refusals; the decoder on the device's
files, a mixed batch of all four layouts included; the recorded files of tests/golden/J5_jpeg_encode_layouts.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                   # sentinel bytes on each side of a buffer
SIZES = {'422': ((1, 1), (8, 16), (8, 17), (9, 47), (17, 33), (24, 40), (16, 130), (33, 70)),
         'grey': ((1, 1), (8, 8), (9, 47), (17, 33), (16, 130), (33, 70))}
QUALITIES = (30, 75, 95, 100)
CODES = {'422': 1, 'grey': 2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'J5_jpeg_encode_layouts.npz')


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


_FRAMES, _HOST = {}, {}


def _frames(h, w):
    """four frames of a size, shared by the tests of the module"""
    if (h, w) not in _FRAMES:
        _FRAMES[(h, w)] = torch.stack([_smooth(h, w, 1000 * h + 10 * w + i) for i in range(4)])
    return _FRAMES[(h, w)]


def _host(h, w, i, q, layout, ri, optimize):
    """clips.jpeg_encode_host(layout=) of frame i of a size, once per case of the module: the definition is pure Python"""
    from istvt_amd import clips
    k = (h, w, i, q, layout, ri, optimize)
    if k not in _HOST:
        _HOST[k] = clips.jpeg_encode_host(_frames(h, w)[i], q, restart_interval=ri, optimize=optimize, layout=layout)
    return _HOST[k]


def _differ(got, want):
    return [(i, len(g), len(w), next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), -1))
            for i, (g, w) in enumerate(zip(got, want)) if g != w]


@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('ri', ['row', 0, 1, 3, 65535])
@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_equals_the_host_definition(pkg, layout, ri, optimize):
    """every size, four frames per call with the four qualities as the per-frame table"""
    from istvt_amd import clips, ops
    q = torch.tensor(QUALITIES, dtype=torch.int32)
    for h, w in SIZES[layout]:
        want = [_host(h, w, i, QUALITIES[i], layout, ri, optimize) for i in range(4)]
        res = ops.jpeg_encode_u8(_frames(h, w).cuda(), q, restart_interval=ri, capacity=4 * (3 * h * w + 1024), optimize=optimize,
                                 layout=layout)
        assert isinstance(res, clips.JpegFiles) and res.status.tolist() == [0, 0, 0, 0], (h, w)
        got = res.files()
        assert got == want, ((h, w), _differ(got, want))
        assert res.nbytes() == sum(len(f) for f in want) and res.offsets[0].item() == 0


@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_a_clip_batch_with_per_clip_qualities(pkg, layout):
    from istvt_amd import clips, ops
    x = torch.cat([_frames(17, 33), _frames(17, 33).flip(1)]).view(2, 4, 17, 33, 3).contiguous()
    q = torch.tensor([30, 95], dtype=torch.int32)
    for optimize in (False, True):
        want = clips.jpeg_encode_files_host(x, q, optimize=optimize, layout=layout)
        res = ops.jpeg_encode_u8(x.cuda(), q, optimize=optimize, layout=layout)
        assert res.status.tolist() == [0] * 8 and res.files() == want, _differ(res.files(), want)
        assert res.data.numel() == 8 * (17 * 33 * 3 + clips.jpeg_header_bound(17, 33, restart_interval='row', layout=layout))


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


@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('layout,ri', [('422', 'row'), ('grey', 2)])
def test_guard_bands_and_refusals(pkg, layout, ri, optimize):
    """Frames, header and quality table as well as `data` (at an odd address), the scratch, offsets and status lie between 4
    KiB of sentinel bytes, with two different fills: every byte of data[:offsets[n]] is written, every byte behind keeps the
    fill, no band is touched, the inputs stay; an image whose quality is <= 0 (status 2, an empty file) sits between the
    sound ones.  Then what the entry refuses before any launch."""
    from istvt_amd import _lib, clips, frames as F
    n, H, W = 4, 33, 70
    x = _frames(H, W)
    q = [75, 95, 0, 30]
    want = b''.join(_host(H, W, i, q[i], layout, ri, optimize) for i in range(n) if q[i] > 0)
    mh, mv = clips.JPEG_LAYOUT_FACTORS[layout][0]
    mcus = (-(-H // (8 * mv))) * (-(-W // (8 * mh)))
    r = clips.jpeg_restart_interval(ri, W, layout=layout)
    assert r == (5 if layout == '422' else 2) and mcus == (25 if layout == '422' else 45)
    blocks, segments = n * mcus * (4 if layout == '422' else 1), n * -(-mcus // r)
    need = F.jpeg_encode_scratch_bytes(blocks, segments, n, optimize)
    assert need == 128 * blocks + 16 * segments + (3344 * n if optimize else 0)
    head = clips.jpeg_header(H, W, 50, restart_interval=r, layout=layout)
    results = []
    for fill in (0xA5, 0x3C):
        dev, qdev = Guarded((n, H, W, 3), torch.uint8, fill, offset=3), Guarded((n,), torch.int32, fill)
        header = Guarded((len(head),), torch.uint8, fill, offset=1)
        dev.t.copy_(x), qdev.t.copy_(torch.tensor(q, dtype=torch.int32)), header.t.copy_(torch.frombuffer(bytearray(head), dtype=torch.uint8))
        data = Guarded((len(want) + 777,), torch.uint8, fill, offset=1)
        scratch = Guarded((need,), torch.uint8, fill)
        offsets, status = Guarded((n + 1,), torch.int64, fill), Guarded((n,), torch.int32, fill)
        assert data.t.data_ptr() % 2 == 1 and scratch.t.data_ptr() % 16 == 0
        F._jpeg_encode_launch(dev.t, dev.t.numel(), qdev.t, header.t, len(head), scratch.t, data.t, offsets.t, status.t, n, H, W, mh, r,
                              optimize, layout)
        torch.cuda.synchronize()
        assert status.t.tolist() == [0, 0, 2, 0] and offsets.t[-1].item() == len(want)
        assert offsets.t[2].item() == offsets.t[3].item()
        assert bytes(data.t[:len(want)].cpu().numpy()) == want
        assert bool((data.t[len(want):] == fill).all())
        assert all(b.intact() for b in (data, scratch, offsets, status, dev, qdev, header))
        assert torch.equal(dev.t.cpu(), x) and qdev.t.tolist() == q and bytes(header.t.cpu().numpy()) == head
        results.append(data.t[:len(want)].clone())
    assert torch.equal(results[0], results[1])
    args = dict(frames=dev.t.data_ptr(), total=dev.t.numel(), quality=qdev.t.data_ptr(), header=header.t.data_ptr(),
                header_bytes=len(head), scratch=scratch.t.data_ptr(), scratch_bytes=need, data=data.t.data_ptr(),
                capacity=data.t.numel(), offsets=offsets.t.data_ptr(), status=status.t.data_ptr(), stream=None, n=n, H=H, W=W,
                subsampling=0, restart_interval=r, dqt0=25, dqt1=94)
    code = CODES[layout]
    dht = clips.jpeg_header_dht(layout) if optimize else (0, 0)
    data.t.fill_(0x77)
    entry = _lib.lib().istvt_jpeg_encode_layout_u8
    for change in (dict(subsampling=1), dict(subsampling=2), dict(scratch_bytes=need - 1), dict(scratch=scratch.t.data_ptr() + 8),
                   dict(data=dev.t.data_ptr() + 10), dict(n=0), dict(H=0), dict(W=16385), dict(restart_interval=-1),
                   dict(restart_interval=65536), dict(capacity=-1), dict(total=dev.t.numel() - 1), dict(header=None),
                   dict(header_bytes=100), dict(dqt1=60), dict(offsets=offsets.t.data_ptr() + 4)):
        assert entry(ctypes.byref(_lib.JpegEncodeArgs(**dict(args, **change))), code, *dht) == -3, change
    for bad in (0, 3, -1):
        assert entry(ctypes.byref(_lib.JpegEncodeArgs(**args)), bad, *dht) == -3, bad
    d0, d1 = clips.jpeg_header_dht(layout)
    for bad in ((d1, d0), (d0, d0), (157, d1), (d0, len(head) + 1), (-1, d1), (0, d1), (d0, 0)):
        assert entry(ctypes.byref(_lib.JpegEncodeArgs(**args)), code, *bad) == -3, bad
    torch.cuda.synchronize()
    assert bool((data.t == 0x77).all()) and torch.equal(dev.t.cpu(), x)


@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_statuses(pkg, layout):
    """a capacity one byte short: status 1, not a byte of that file written, the true size in offsets[n]; a quality <= 0 with
    checked=True: status 2 and an empty file"""
    from istvt_amd import ops
    x = _frames(17, 33)[:3]
    qs = (30, 100, 75)
    for optimize in (False, True):
        want = [_host(17, 33, i, qs[i], layout, 'row', optimize) for i in range(3)]
        sizes = [len(f) for f in want]
        out = torch.full((sum(sizes) - 1,), 0xA5, dtype=torch.uint8, device='cuda')
        res = ops.jpeg_encode_u8(x.cuda(), torch.tensor(qs, dtype=torch.int32), out=out, optimize=optimize, layout=layout)
        assert res.status.tolist() == [0, 0, 1] and res.offsets.tolist() == [0, sizes[0], sum(sizes[:2]), sum(sizes)]
        assert bytes(out[:sum(sizes[:2])].cpu().numpy()) == want[0] + want[1] and bool((out[sum(sizes[:2]):] == 0xA5).all())
        assert res.files(check=False) == want[:2] + [b'']
        again = ops.jpeg_encode_u8(x.cuda(), torch.tensor(qs, dtype=torch.int32), capacity=res.nbytes(), optimize=optimize, layout=layout)
        assert again.status.tolist() == [0, 0, 0] and again.files() == want
        empty = ops.jpeg_encode_u8(x.cuda(), torch.tensor([30, -1, 0], dtype=torch.int32).cuda(), checked=True, optimize=optimize,
                                   layout=layout)
        assert empty.status.tolist() == [0, 2, 2] and empty.files(check=False) == [want[0], b'', b'']
        assert empty.offsets.tolist() == [0, sizes[0], sizes[0], sizes[0]]


@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_the_decoder_on_the_devices_files(pkg, layout):
    """the device's files decode, on the device, to what the definition's decoder makes of the definition's files; 'row'
    files hold one segment per MCU row, ceil(H / 8) in both layouts"""
    from istvt_amd import clips, ops
    H, W = 33, 70
    q = torch.tensor(QUALITIES, dtype=torch.int32)
    for optimize in (False, True):
        files = ops.jpeg_encode_u8(_frames(H, W).cuda(), q, optimize=optimize, layout=layout).files()
        assert all(len(clips.jpeg_parse(f, layouts='all').segments) == -(-H // 8) for f in files)
        assert all(clips.jpeg_parse(f, layouts='all').layout == layout for f in files)
        frames, sizes, status = ops.jpeg_decode_u8(files, layouts='all')
        assert status.tolist() == [0, 0, 0, 0] and sizes.tolist() == [[H, W]] * 4
        want = torch.stack([clips.jpeg_decode_host(_host(H, W, i, QUALITIES[i], layout, 'row', optimize), layouts='all') for i in range(4)])
        assert torch.equal(frames.cpu(), want)
    if layout == 'grey':
        assert torch.equal(want[..., 0], want[..., 1]) and torch.equal(want[..., 0], want[..., 2])
    crops = ops.encode_frames(_frames(H, W).cuda(), 24, boxes=clips.whole_boxes([(H, W)] * 4), quality=80, optimize=True, layout=layout)
    host = clips.jpeg_encode_files_host(ops.crop_resize_u8(_frames(H, W).cuda(), clips.whole_boxes([(H, W)] * 4), 24).cpu(), 80,
                                        optimize=True, layout=layout)
    assert crops.files() == host


def test_a_mixed_batch_of_all_four_layouts(pkg):
    from istvt_amd import clips, ops
    x = _frames(17, 33)
    files = []
    for layout in clips.JPEG_LAYOUTS:
        files += ops.jpeg_encode_u8(x[:2].cuda(), 75, optimize=layout in ('444', 'grey'), layout=layout).files()
    assert [clips.jpeg_parse(f, layouts='all').layout for f in files] == ['420', '420', '444', '444', '422', '422', 'grey', 'grey']
    frames, sizes, status = ops.jpeg_decode_u8(files, layouts='all')
    assert status.tolist() == [0] * 8 and sizes.tolist() == [[17, 33]] * 8
    assert torch.equal(frames.cpu(), torch.stack([clips.jpeg_decode_host(f, layouts='all') for f in files]))
    assert torch.equal(frames[:2], ops.jpeg_roundtrip_u8(x[:2].cuda(), 75, '420'))


def test_the_recorded_files(pkg):
    """J5: the definition's files, whose scans are PIL's where libjpeg writes no dummy block (the recipe asserted it)"""
    from istvt_amd import ops
    golden = np.load(GOLDEN)
    names = [str(n) for n in golden['names']]
    assert len(names) == 160 and len(golden['pil_equal']) == 128
    groups = {}
    for name in names:
        size, layout, q = name.split('_')[:3]
        groups.setdefault((size, layout, '_rr1' in name, name.endswith('_opt')), []).append((int(q[1:]), name))
    assert len(groups) == 80
    for (size, layout, rows, optimize), members in groups.items():
        x = torch.from_numpy(golden['frame_' + size])
        q = torch.tensor([m[0] for m in members], dtype=torch.int32)
        res = ops.jpeg_encode_u8(x[None].repeat(len(members), 1, 1, 1).cuda(), q, restart_interval='row' if rows else 0,
                                 capacity=len(members) * (x.numel() + 1024), optimize=optimize, layout=layout)
        want = [bytes(golden['file_' + m[1]]) for m in members]
        assert res.status.tolist() == [0] * len(members) and res.files() == want, (size, layout, rows, optimize)


def test_the_old_names_and_the_profile_record(pkg):
    """layout='420' / '444' is the subsampling of that name, by the same entry; the new layouts record their own"""
    from istvt_amd import clips, ops
    x = _frames(24, 40)[:3]
    q = torch.tensor([30, 75, 95], dtype=torch.int32)
    ops.kernel_profile = []
    try:
        plain = ops.jpeg_encode_u8(x.cuda(), q).files()
        named = ops.jpeg_encode_u8(x.cuda(), q, layout='420').files()
        full = ops.jpeg_encode_u8(x.cuda(), q, layout='444', optimize=True).files()
        new = [ops.jpeg_encode_u8(x.cuda(), q, layout=layout, optimize=optimize).files()
               for layout in ('422', 'grey') for optimize in (False, True)]
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_encode_u8', 'jpeg_encode_u8', 'jpeg_encode_opt_u8'] + ['jpeg_encode_layout_u8'] * 4
    assert plain == named == clips.jpeg_encode_files_host(x, q)
    assert full == clips.jpeg_encode_files_host(x, q, '444', optimize=True)
    assert new[0] == clips.jpeg_encode_files_host(x, q, layout='422') and new[3] == clips.jpeg_encode_files_host(x, q, optimize=True, layout='grey')
    assert sum(map(len, new[2])) < sum(map(len, plain)) < sum(map(len, new[0]))       # greyscale is the smallest file
