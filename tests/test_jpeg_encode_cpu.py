"""JPEG files out (DESIGN.md "JPEG files out") without a device: the header and the 'row' restart interval factored out of
clips.jpeg_encode_host, the batch definition, clips.JpegFiles on host tensors, the refusals of ops.jpeg_encode_u8 that need
no device, and the entry point's aliases."""

import numpy as np
import pytest
import torch



@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def _smooth(h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return torch.from_numpy(np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8))


@pytest.mark.parametrize('sub', ['420', '444'])
@pytest.mark.parametrize('ri', [0, 2])
def test_header_then_scan_is_the_file(clips, sub, ri):
    x = _smooth(17, 33, 1733)
    data = clips.jpeg_encode_host(x, 75, sub, ri)
    head = clips.jpeg_header(17, 33, 75, sub, ri)
    assert data[:len(head)] == head and head[:2] == b'\xff\xd8' and head[-14:-12] == b'\xff\xda'
    hd = clips.jpeg_parse(data)
    assert hd.segments[0][0] == len(head) and hd.restart_interval == ri
    # the two tables lie where JPEG_HEADER_DQT says, in zig-zag order; nothing else depends on the quality
    other = clips.jpeg_header(17, 33, 30, sub, ri)
    differ = {i for i in range(len(head)) if head[i] != other[i]}
    lo0, lo1 = clips.JPEG_HEADER_DQT
    assert differ and differ <= set(range(lo0, lo0 + 64)) | set(range(lo1, lo1 + 64))
    zz = torch.tensor(clips.JPEG_ZIGZAG)
    q = clips.jpeg_quant_tables(75).reshape(2, 64)
    assert list(head[lo0:lo0 + 64]) == q[0][zz].tolist() and list(head[lo1:lo1 + 64]) == q[1][zz].tolist()
    assert (b'\xff\xdd' in head) == (ri != 0)


def test_restart_interval(clips):
    f = clips.jpeg_restart_interval
    assert f('row', 33, '420') == 3 and f('row', 33, '444') == 5 and f('row', 1, '420') == 1 and f('row', 224, '420') == 14
    assert f(0, 33) == 0 and f(65535, 33) == 65535 and f(7, 33, '444') == 7
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match='restart interval'):
            f(bad, 33)
    with pytest.raises(ValueError, match="'row'"):
        f('column', 33)
    with pytest.raises(ValueError, match='subsampling'):
        f('row', 33, '422')


@pytest.mark.parametrize('sub', ['420', '444'])
def test_row_files(clips, sub):
    """'row' is the interval of one MCU row; the parser finds one segment per MCU row; decoding gives the round trip"""
    step = 16 if sub == '420' else 8
    for (h, w), q in (((33, 70), 75), ((17, 33), 95), ((8, 8), 30)):
        x = _smooth(h, w, h * 100 + w)
        mx = -(-w // step)
        data = clips.jpeg_encode_host(x, q, sub, 'row')
        assert data == clips.jpeg_encode_host(x, q, sub, mx)
        hd = clips.jpeg_parse(data)
        assert hd.restart_interval == mx and len(hd.segments) == -(-h // step) and hd.eoi
        got, status = clips.jpeg_decode_host(data, return_status=True)
        assert status == 0 and torch.equal(got, clips.jpeg_roundtrip_host(x[None], q, sub)[0])


def test_files_host(clips):
    frames = torch.stack([_smooth(24, 40, s) for s in range(4)])
    q = torch.tensor([30, 75, 95, 100], dtype=torch.int32)
    files = clips.jpeg_encode_files_host(frames, q, '420', 'row')
    assert files == [clips.jpeg_encode_host(frames[i], int(q[i]), '420', 3) for i in range(4)]
    assert clips.jpeg_encode_files_host(frames, 50, '444', 0) == [clips.jpeg_encode_host(f, 50, '444', 0) for f in frames]
    both = clips.jpeg_encode_files_host(frames.view(2, 2, 24, 40, 3), torch.tensor([30, 95], dtype=torch.int32))
    assert both == [clips.jpeg_encode_host(frames[i], (30, 30, 95, 95)[i], '420', 'row') for i in range(4)]
    for bad in (0, 101, torch.tensor([50, 0, 50, 50], dtype=torch.int32)):
        with pytest.raises(ValueError, match='quality'):
            clips.jpeg_encode_files_host(frames, bad)
    with pytest.raises(ValueError):
        clips.jpeg_encode_files_host(frames.float(), 50)


def test_jpeg_files_on_host_tensors(clips):
    parts = [b'abc', b'', b'defgh']
    data = torch.frombuffer(bytearray(b''.join(parts) + b'\xa5' * 5), dtype=torch.uint8)
    offsets = torch.tensor([0, 3, 3, 8], dtype=torch.int64)
    jf = clips.JpegFiles(data, offsets, torch.zeros(3, dtype=torch.int32))
    assert len(jf) == 3 and jf.nbytes() == 8 and jf.files() == parts
    names = {1: 'does not fit', 2: 'quality <= 0', 3: 'outside the categories'}
    for status, name in names.items():
        bad = clips.JpegFiles(data, offsets, torch.tensor([0, status, 0], dtype=torch.int32))
        with pytest.raises(ValueError, match='file 1 has status %d .*%s' % (status, name)):
            bad.files()
        assert name in clips.JPEG_ENCODE_STATUS[status]
    # status 1: the offsets hold the true sizes, beyond the capacity; what was written is handed over with check=False
    short = clips.JpegFiles(data[:5], torch.tensor([0, 3, 3, 80], dtype=torch.int64), torch.tensor([0, 2, 1], dtype=torch.int32))
    assert short.nbytes() == 80 and short.files(check=False) == [b'abc', b'', b'']
    with pytest.raises(ValueError, match='file 1 has status 2'):
        short.files()
    with pytest.raises(ValueError):
        clips.JpegFiles(data, offsets, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        clips.JpegFiles(data, offsets.int(), torch.zeros(3, dtype=torch.int32))


def test_a_batch_takes_jpeg_files(clips):
    x = _smooth(16, 16, 5)
    f = [clips.jpeg_encode_host(x, 75, '420', 'row'), clips.jpeg_encode_host(x, 40, '420', 'row')]
    data = torch.frombuffer(bytearray(f[0] + f[1]), dtype=torch.uint8)
    jf = clips.JpegFiles(data, torch.tensor([0, len(f[0]), len(f[0]) + len(f[1])], dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    a, b = clips.jpeg_batch(jf), clips.jpeg_batch(f)
    assert a.n == 2 and torch.equal(a.data, b.data) and torch.equal(a.images, b.images) and torch.equal(a.segments, b.segments)


def test_refusals_that_need_no_device(clips):
    from istvt_amd import ops
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match='jpeg_encode_u8: frames must be uint8'):
        ops.jpeg_encode_u8(x.float(), 50)
    for bad in (x[0], x[..., :2], x.view(2, 16, 24 * 3)):
        with pytest.raises(RuntimeError, match='jpeg_encode_u8 expects channels-last'):
            ops.jpeg_encode_u8(bad, 50)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.jpeg_encode_u8(x[:, :, ::2], 50)
    for bad in (0, 101, torch.tensor([50, 0], dtype=torch.int32), torch.tensor([101, 50], dtype=torch.int32)):
        with pytest.raises(ValueError, match='quality'):
            ops.jpeg_encode_u8(x, bad)
    with pytest.raises(ValueError, match='quality must have shape'):
        ops.jpeg_encode_u8(x, torch.tensor([50], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='a device quality table is taken with checked=True only'):
        ops.jpeg_encode_u8(x, torch.empty((2,), dtype=torch.int32, device='meta'))
    with pytest.raises(ValueError, match="subsampling must be '420' or '444'"):
        ops.jpeg_encode_u8(x, 50, '422')
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match='restart interval must lie in .0, 65535.'):
            ops.jpeg_encode_u8(x, 50, restart_interval=bad)
    with pytest.raises(RuntimeError, match='must be on a ROCm device'):
        ops.jpeg_encode_u8(x, 50)                                # sound arguments on the host: no fallback
    with pytest.raises(ValueError, match='pass one of them'):
        ops.encode_frames(x, 8)


def test_render_explanation_refuses_nv12_with_a_quality():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    scorer = video.VideoScorer(model, side=4, pixel_format='nv12')
    with pytest.raises(ValueError, match="pixel_format='nv12' with jpeg_quality is not supported"):
        scorer.render_explanation(torch.zeros((2, 12, 8), dtype=torch.uint8), None, jpeg_quality=75)
    rgb = video.VideoScorer(model, side=4)
    for bad in (0, 101, 75.0, True):
        with pytest.raises(ValueError, match='jpeg_quality must be an int in .1, 100.'):
            rgb.render_explanation(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), None, jpeg_quality=bad)
    import inspect
    assert inspect.signature(video.VideoScorer.render_explanation).parameters['jpeg_quality'].default is None


def test_entry_point_declared_and_bound(clips):
    from istvt_amd import frames, ops
    # (header, table, argument block and library: test_abi_cpu.py)
    assert ops.jpeg_encode_u8 is frames.jpeg_encode_u8 and ops.encode_frames is frames.encode_frames
    assert max(len(line) for line in frames.jpeg_encode_u8.__doc__.splitlines()) <= 128


def test_pil_decodes_a_row_file_to_the_definition(clips):
    Image = pytest.importorskip('PIL.Image')
    import io
    for sub in ('420', '444'):
        x = _smooth(33, 70, 7)
        data = clips.jpeg_encode_host(x, 75, sub, 'row')
        pil = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        assert np.array_equal(pil, clips.jpeg_decode_host(data).numpy())
