"""4:2:2 and greyscale JPEG files (DESIGN.md "JPEG layouts") on a real MI355X: ops.jpeg_decode_u8(..., layouts='all'), by the
default call and by the split, against the integer definition clips.jpeg_decode_host and the bytes PIL recorded, byte for
byte; layouts mixed in one batch with the files of tests/golden/J2_jpeg_files.npz; the state rows against
clips.jpeg_split_host; damaged files; what is written and what is left alone (sentinel bytes around every buffer); the
refusals.  tools/jpeg_entropy_check.cpp and tools/jpeg_entropy_split_check.cpp, the same two headers under AddressSanitizer
and UBSan on the host, have passed on the J2 and J3 files, cut at every length and with flipped bits, before the changed
kernels ran on a device for the first time: DESIGN.md has the commands and their counts."""
import os

import numpy as np
import pytest
import torch

from test_jpeg_split_cpu import _smooth
from test_jpeg_split_gpu import SENTINEL, _buffers, _check_canvas, _same_as_default

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def files(golden_dir):
    return np.load(os.path.join(golden_dir, 'J3_jpeg_layouts.npz'))


def _sound(clips, npz, layouts):
    out = []
    for name in npz['names'].tolist():
        data = bytes(npz['file_' + name])
        ref, status = clips.jpeg_decode_host(data, return_status=True, layouts=layouts)
        assert status == 0 and np.array_equal(ref.numpy(), npz['rgb_' + name]), name
        out.append((name, data, ref))
    return out


@pytest.fixture(scope='module')
def sound(pkg, files):
    """[(name, bytes, the definition's frame, which is PIL's)] of every sound J3 file: decoded on the host once"""
    from istvt_amd import clips
    return _sound(clips, files, 'all')


@pytest.fixture(scope='module')
def mixed(pkg, golden_dir, sound):
    """all 102 J2 files and all J3 files interleaved: neighbouring lanes and consecutive IDCT workgroups hold different
    layouts -> (the [(name, bytes, frame)] list, its JpegBatch)"""
    from istvt_amd import clips
    old = _sound(clips, np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz')), clips.JPEG_LAYOUTS_DEFAULT)
    assert len(old) == 102
    order = [f for pair in zip(old, sound) for f in pair] + sound[len(old):]
    batch = clips.jpeg_batch([d for _, d, _ in order], layouts='all')
    codes = batch.images[:, 19].tolist()
    assert {0, 1, 2} == set(codes) and all(a != b for a, b in zip(codes[:204], codes[1:204]))
    return order, batch


def test_single_files(pkg, sound):
    from istvt_amd import clips, ops
    for name, data, ref in sound:
        batch = clips.jpeg_batch([data], layouts='all')
        h, w = ref.shape[:2]
        out, scratch, sizes, status = _buffers(batch, (h, w), batch.scratch_bytes)
        assert out.t.data_ptr() % 2 == 1
        got = []
        for fill in (None, 0x3C, 0xFF):                           # nothing may depend on what the scratch held
            if fill is not None:
                scratch.t.fill_(fill)
            frames, s, st = ops.jpeg_decode_u8(batch, out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t))
            assert s.tolist() == [[h, w]] and st.tolist() == [0], name
            assert out.intact() and scratch.intact() and sizes.intact() and status.intact(), name
            got.append(frames.cpu().clone())
        bad = int((got[0][0] != ref).sum())
        assert bad == 0, '%s: %d of %d bytes differ' % (name, bad, ref.numel())
        assert torch.equal(got[1], got[0]) and torch.equal(got[2], got[0]), name
        frames, s, st = ops.jpeg_decode_u8([data], layouts='all')            # and as files, with the wrapper's own buffers
        assert torch.equal(frames.cpu()[0], ref) and s.tolist() == [[h, w]] and st.tolist() == [0], name


def test_mixed_batch(pkg, mixed):
    from istvt_amd import ops
    order, batch = mixed
    out, scratch, sizes, status = _buffers(batch, (48, 72), batch.scratch_bytes)
    ops.kernel_profile = []
    try:
        got, s, st = ops.jpeg_decode_u8(batch, canvas=(48, 72), out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t))
        record = [r[0] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert record == ['jpeg_decode_u8']
    _check_canvas(got, [r for _, _, r in order])
    assert s.tolist() == [list(r.shape[:2]) for _, _, r in order] and not bool(st.any())
    assert out.intact() and scratch.intact() and sizes.intact() and status.intact()
    as_files, _, _ = ops.jpeg_decode_u8([d for _, d, _ in order], canvas=(48, 72), layouts='all')
    assert torch.equal(as_files, got)


@pytest.mark.parametrize('chunk', [16, 128])
def test_mixed_batch_split(pkg, mixed, chunk):
    from istvt_amd import clips, ops
    order, batch = mixed
    got, st, scratch = _same_as_default(ops, batch, chunk, canvas=(48, 72))
    _check_canvas(got, [r for _, _, r in order])
    assert not bool(st.any())
    plan = clips.jpeg_split_plan(batch, chunk)
    segments = batch.segments.tolist()
    rows = scratch[plan.states_at:plan.states_at + 32 * plan.rows].view(torch.int32).view(-1, 8).cpu()
    seen = set()
    for i, (name, data, _) in enumerate(order):
        if '_s' in name:
            continue                                              # a J2 file: tests/test_jpeg_split_gpu.py has its rows
        hd = clips.jpeg_parse(data, 'all')
        host = clips.jpeg_split_host(hd, chunk)
        seg0 = int(batch.images[i, 16])
        for k, (seg, (begin, _)) in enumerate(zip(host.segments, hd.segments)):
            s = seg0 + k
            assert plan.count[s] == len(seg.states) and plan.chunk[s] == seg.chunk, (name, k)
            want = torch.tensor(seg.rows, dtype=torch.int32)
            want[:, 0] += segments[s][1] - begin                  # the batch holds the scans end to end
            assert torch.equal(rows[plan.row0[s]:plan.row0[s] + plan.count[s]], want), (name, k)
            seen.update((hd.layout, r[2]) for r in seg.rows)
    assert seen == {('422', 0), ('422', 1), ('422', 2), ('422', 3), ('grey', 0)}
    noise = [n for n, _, _ in order].index('noise40x56_422_q100')
    _, begin, end, _, _ = segments[int(batch.images[noise, 16])]
    assert chunk != 16 or (end - begin > 256 * 16 and plan.chunk[int(batch.images[noise, 16])] > 16)      # the lane cap


def test_small_files_run_the_64_lane_workgroup(pkg, sound):
    from istvt_amd import clips, ops
    pick = [(n, d, r) for n, d, r in sound if n.split('_')[0] in ('1x1', '8x8', '9x15', '8x17', '16x16')]
    batch = clips.jpeg_batch([d for _, d, _ in pick], layouts='all')
    plan = clips.jpeg_split_plan(batch, 16)
    assert len(pick) == 5 * 14 and 1 < max(plan.count) <= 64
    got, st, _ = _same_as_default(ops, batch, 16)
    _check_canvas(got, [r for _, _, r in pick])
    assert not bool(st.any())


@pytest.mark.parametrize('ri', [1, 2, 5])
def test_encoder_files(pkg, ri):
    from istvt_amd import clips, ops
    data = [clips.jpeg_encode_layout_host(_smooth(h, w, 100 * h + w), q, layout, ri)
            for h, w in ((24, 40), (33, 70)) for layout, q in (('422', 40), ('grey', 95), ('422', 95), ('grey', 40))]
    refs = [clips.jpeg_decode_host(d, layouts='all') for d in data]
    batch = clips.jpeg_batch(data, layouts='all')
    mcus = [3 * 3, 3 * 5, 3 * 3, 3 * 5, 5 * 5, 5 * 9, 5 * 5, 5 * 9]
    assert batch.images[:, 17].tolist() == [-(-m // ri) for m in mcus]
    got, _, st = ops.jpeg_decode_u8(batch, checked=True)
    _check_canvas(got, refs)
    assert not bool(st.any())
    got, st, _ = _same_as_default(ops, batch, 16)
    _check_canvas(got, refs)
    assert not bool(st.any())


def test_damaged_files(pkg, files, sound, golden_dir):
    """The three damaged 4:2:2 files, each between a sound greyscale and a sound 4:2:0 neighbour.  Recorded files whose decode
    is bounded by construction and ran under the sanitizers on the CPU first."""
    from istvt_amd import clips, ops
    j2 = np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))
    grey = next((d, r) for n, d, r in sound if n == '33x70_grey_q75_rb1')
    d420 = bytes(j2['file_24x40_s2_q75'])
    r420 = clips.jpeg_decode_host(d420)
    names = files['damaged'].tolist()
    want = files['damaged_status'].tolist()
    assert sorted(want) == [1, 2, 3]
    data, refs, expect = [grey[0]], [grey[1]], [0]
    for name, status in zip(names, want):
        bad = bytes(files['file_' + name])
        assert clips.jpeg_decode_host(bad, True, 'all')[1] == status
        data += [bad, d420, grey[0]]
        refs += [None, r420, grey[1]]
        expect += [status, 0, 0]
    batch = clips.jpeg_batch(data, layouts='all')
    for chunk in (None, 16):
        need = batch.scratch_bytes if chunk is None else clips.jpeg_split_plan(batch, chunk).scratch_bytes
        out, scratch, sizes, status = _buffers(batch, (33, 70), need, out_offset=3)
        got, s, st = ops.jpeg_decode_u8(batch, out=out.t, checked=True, buffers=(scratch.t, sizes.t, status.t), split=chunk)
        assert st.tolist() == expect, chunk
        host = got.cpu()
        for i, ref in enumerate(refs):
            h, w = (24, 40) if ref is None else ref.shape[:2]
            assert s[i].tolist() == [h, w]
            assert ref is None or torch.equal(host[i, :h, :w], ref), (chunk, i)
            assert int(host[i, h:].any()) == 0 and int(host[i, :, w:].any()) == 0, (chunk, i)
        assert out.intact() and scratch.intact() and sizes.intact() and status.intact(), chunk
    with pytest.raises(ValueError, match='file 1 is damaged'):
        clips.check_jpeg_status(st)


def test_decode_frames(pkg, sound):
    from istvt_amd import clips, ops
    names = ['48x48_422_q75', '33x70_grey_q75_rr1', '24x40_422_q30', '17x33_grey_q75_opt']
    pick = {n: (d, r) for n, d, r in sound}
    canvas = torch.zeros((4, 48, 70, 3), dtype=torch.uint8)
    for i, k in enumerate(names):
        h, w = pick[k][1].shape[:2]
        canvas[i, :h, :w] = pick[k][1]
    boxes = torch.tensor([[4, 6, 40, 36], [1, 30, 32, 40], [0, 0, 24, 40], [3, 2, 13, 30]], dtype=torch.int32)
    data = [pick[k][0] for k in names]
    got = ops.decode_frames(data, 16, boxes, layouts='all')
    assert tuple(got.shape) == (4, 16, 16, 3)
    assert torch.equal(got, ops.crop_resize_u8(canvas.cuda(), boxes, 16))
    assert torch.equal(ops.decode_frames(data, 16, boxes, split=16, layouts=('422', 'grey')), got)
    sizes = [pick[k][1].shape[:2] for k in names]
    assert torch.equal(ops.decode_frames(data, 16, layouts='all'), ops.crop_resize_u8(canvas.cuda(), clips.whole_boxes(sizes), 16))


def test_refusals(pkg, sound):
    """each of them before any launch: a sentinel-filled `out` stays as it is"""
    import ctypes
    from istvt_amd import _lib, clips, ops
    f422 = next(d for n, d, _ in sound if n == '24x40_422_q75')
    fgrey = next(d for n, d, _ in sound if n == '24x40_grey_q75')
    out = torch.full((1, 24, 40, 3), SENTINEL, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='jpeg_parse: sampling 2x1/1x1/1x1'):
        ops.jpeg_decode_u8([f422], out=out)
    with pytest.raises(ValueError, match='jpeg_parse: sampling 2x1/1x1/1x1'):
        ops.decode_frames([f422], 16)
    with pytest.raises(ValueError, match='jpeg_parse: 1 component '):
        ops.jpeg_decode_u8([fgrey], out=out)
    with pytest.raises(ValueError, match='jpeg_parse: sampling 2x1/1x1/1x1'):
        ops.jpeg_decode_u8([f422], out=out, layouts=('420', '444', 'grey'))
    with pytest.raises(ValueError, match='jpeg_batch: layouts '):
        ops.jpeg_decode_u8([f422], out=out, layouts='422')
    # the entry itself
    batch = clips.jpeg_batch([f422], layouts='all')
    assert batch.images[0].tolist()[:5] == [24, 40, 2, 3, 3] and batch.images[0, 18:].tolist() == [36, 1]
    d = batch.on(out.device)
    plan = clips.jpeg_split_plan(batch, 16)
    scratch = torch.empty((plan.scratch_bytes,), dtype=torch.uint8, device='cuda')
    sizes, status = torch.empty((1, 2), dtype=torch.int32, device='cuda'), torch.empty((1,), dtype=torch.int32, device='cuda')

    def args(images):
        dev = images.cuda()
        keep.append(dev)
        return _lib.JpegDecodeArgs(
            bytes=d.data.data_ptr(), nbytes=batch.nbytes, images=dev.data_ptr(), images_host=images.data_ptr(),
            segments=d.segments.data_ptr(), segments_host=batch.segments.data_ptr(), qtabs=d.qtabs.data_ptr(),
            htabs=d.htabs.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), out=out.data_ptr(),
            sizes=sizes.data_ptr(), status=status.data_ptr(), stream=None, n=1, nseg=1, nq=int(batch.qtabs.shape[0]),
            nh=int(batch.htabs.shape[0]), Hc=24, Wc=40)
    keep = []
    # an unknown layout code; a code its chroma step does not go with; a 4:2:2 row with the two MCU rows 4:2:0 has, with
    # its own block count and with one that fits them; a 4:2:0 row with 4:2:2's counts
    for change in ({19: 3}, {19: -1}, {19: 2}, {2: 1}, {4: 2}, {4: 2, 18: 24}, {19: 0}):
        images = batch.images.clone()
        for at, value in change.items():
            images[0, at] = value
        assert _lib.lib().istvt_jpeg_decode_u8(ctypes.byref(args(images))) == -3, change
        assert _lib.lib().istvt_jpeg_decode_split_u8(ctypes.byref(args(images)), 16) == -3, change
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert _lib.lib().istvt_jpeg_decode_u8(ctypes.byref(args(batch.images.clone()))) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.jpeg_decode_u8(batch)[0])
