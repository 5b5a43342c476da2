"""JPEG files out in the layouts 4:2:2 and greyscale (DESIGN.md "JPEG files out, 4:2:2 and greyscale") without a device:
clips.jpeg_encode_host(layout=) against clips.jpeg_encode_layout_host and against the recorded files
(tests/golden/J5_jpeg_encode_layouts.npz; no PIL needed here), the 'row' interval, the places of the header's tables, the
header bound, the optimised form's defining properties, the refusals that need no device, the entry's declaration, and
tools/jpeg_entropy_layout_check.cpp, built plain, on the recorded scans."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SIZES = ((1, 1), (8, 8), (8, 17), (9, 47), (17, 33), (16, 130))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'J5_jpeg_encode_layouts.npz'))


def _smooth(h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return torch.from_numpy(np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8))


@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_the_standard_form_is_jpeg_encode_layout_host(clips, layout):
    for h, w in SIZES:
        x = _smooth(h, w, 100 * h + w)
        for q, ri in ((30, 0), (75, 1), (95, 3), (100, 65535)):
            assert clips.jpeg_encode_host(x, q, restart_interval=ri, layout=layout) == clips.jpeg_encode_layout_host(x, q, layout, ri)
        row = clips.jpeg_restart_interval('row', w, layout=layout)
        assert clips.jpeg_encode_host(x, 75, restart_interval='row', layout=layout) == clips.jpeg_encode_layout_host(x, 75, layout, row)


def test_the_old_names_are_the_subsamplings(clips):
    x = _smooth(17, 33, 1733)
    for sub in ('420', '444'):
        for optimize in (False, True):
            assert clips.jpeg_encode_host(x, 75, layout=sub, optimize=optimize) == clips.jpeg_encode_host(x, 75, sub, optimize=optimize)
        assert clips.jpeg_header(17, 33, 75, layout=sub, restart_interval='row') == clips.jpeg_header(17, 33, 75, sub, 'row')
        assert clips.jpeg_header_bound(17, 33, layout=sub) == clips.jpeg_header_bound(17, 33, sub)
        assert clips.jpeg_restart_interval('row', 33, layout=sub) == clips.jpeg_restart_interval('row', 33, sub)


def test_row_is_one_mcu_row(clips):
    f = clips.jpeg_restart_interval
    assert f('row', 33, layout='422') == 3 and f('row', 33, layout='grey') == 5 and f('row', 1, layout='422') == 1
    assert f('row', 224, layout='422') == 14 and f('row', 224, layout='grey') == 28 and f(7, 33, layout='grey') == 7
    for layout in ('422', 'grey'):
        for (h, w), q in (((33, 70), 75), ((17, 33), 95), ((8, 8), 30)):
            hd = clips.jpeg_parse(clips.jpeg_encode_host(_smooth(h, w, h * 100 + w), q, restart_interval='row', layout=layout), layouts='all')
            assert hd.layout == layout and hd.restart_interval == f('row', w, layout=layout) and len(hd.segments) == -(-h // 8) and hd.eoi


@pytest.mark.parametrize('layout', ['420', '444', '422', 'grey'])
@pytest.mark.parametrize('ri', [0, 2])
def test_the_places_of_the_headers_tables(clips, layout, ri):
    head = clips.jpeg_header(17, 33, 75, restart_interval=ri, layout=layout)
    d0, d1 = clips.jpeg_header_dht(layout)
    assert (d0, d1) == ((171, 603) if layout == 'grey' else clips.JPEG_HEADER_DHT) and clips.JPEG_HEADER_DHT == (177, 609)
    at, kinds = d0, []
    while at < d1:                                                # four DHT segments, one behind the other, fill [d0, d1)
        assert head[at:at + 2] == b'\xff\xc4'
        kinds.append(head[at + 4])
        at += 2 + ((head[at + 2] << 8) | head[at + 3])
    assert at == d1 and kinds == [0x00, 0x01, 0x10, 0x11]
    assert head[d1:d1 + 2] == (b'\xff\xdd' if ri else b'\xff\xda') and head[d0 - (13 if layout == 'grey' else 19):][:2] == b'\xff\xc0'
    lo0, lo1 = clips.JPEG_HEADER_DQT                              # in front of SOF0: the same places in every layout
    zz = torch.tensor(clips.JPEG_ZIGZAG)
    qt = clips.jpeg_quant_tables(75).reshape(2, 64)
    assert list(head[lo0:lo0 + 64]) == qt[0][zz].tolist() and list(head[lo1:lo1 + 64]) == qt[1][zz].tolist()
    x = _smooth(17, 33, 1733)
    for optimize in (False, True):
        data = clips.jpeg_encode_host(x, 75, restart_interval=ri, optimize=optimize, layout=layout)
        assert data[:d0] == head[:d0] and data[d0:d0 + 2] == b'\xff\xc4'
        begin = clips.jpeg_parse(data, layouts='all').segments[0][0]
        assert data[begin - (len(head) - d1):begin] == head[d1:]
        assert begin <= clips.jpeg_header_bound(17, 33, restart_interval=ri, layout=layout) == len(head)


@pytest.mark.parametrize('layout', ['422', 'grey'])
def test_the_optimised_form(clips, layout):
    """the same pixels from no more bytes; the tables of the frame's own counts; an empty pair of id-1 tables for 'grey'"""
    for (h, w), q, ri in (((9, 47), 30, 0), ((17, 33), 75, 'row'), ((16, 130), 100, 3)):
        x = _smooth(h, w, 100 * h + w)
        std = clips.jpeg_encode_host(x, q, restart_interval=ri, layout=layout)
        opt = clips.jpeg_encode_host(x, q, restart_interval=ri, optimize=True, layout=layout)
        assert len(opt) < len(std)
        assert torch.equal(clips.jpeg_decode_host(opt, layouts='all'), clips.jpeg_decode_host(std, layouts='all'))
        hs, ho = clips.jpeg_parse(std, layouts='all'), clips.jpeg_parse(opt, layouts='all')
        assert ho.huffman != hs.huffman and ho.restart_interval == hs.restart_interval and len(ho.segments) == len(hs.segments)
        d0 = clips.jpeg_header_dht(layout)[0]
        if layout == 'grey':                                      # DC 0 | DC 1, empty: 19 bytes and no values
            first = 2 + ((opt[d0 + 2] << 8) | opt[d0 + 3])
            assert opt[d0 + first:d0 + first + 21] == b'\xff\xc4\x00\x13\x01' + bytes(16)


def test_the_recorded_files(clips, golden):
    names = [str(n) for n in golden['names']]
    assert len(names) == 160 and len(golden['pil_equal']) == 128 and set(map(str, golden['pil_equal'])) <= set(names)
    dummy = {n.split('_')[0] for n in names if n not in set(map(str, golden['pil_equal']))}
    assert dummy == {'8x8', '17x33', '24x40', '33x70'}            # 4:2:2 with 0 < W % 16 <= 8: libjpeg's dummy block
    for name in names:
        size, layout, q = name.split('_')[:3]
        x = torch.from_numpy(golden['frame_' + size])
        ours = clips.jpeg_encode_host(x, int(q[1:]), restart_interval='row' if '_rr1' in name else 0, optimize=name.endswith('_opt'),
                                      layout=layout)
        assert ours == bytes(golden['file_' + name]), name


def test_files_host(clips):
    frames = torch.stack([_smooth(24, 40, s) for s in range(4)])
    q = torch.tensor([30, 75, 95, 100], dtype=torch.int32)
    for layout, row in (('422', 3), ('grey', 5)):
        files = clips.jpeg_encode_files_host(frames, q, layout=layout)
        assert files == [clips.jpeg_encode_layout_host(frames[i], int(q[i]), layout, row) for i in range(4)]
        both = clips.jpeg_encode_files_host(frames.view(2, 2, 24, 40, 3), torch.tensor([30, 95], dtype=torch.int32), optimize=True, layout=layout)
        assert both == [clips.jpeg_encode_host(frames[i], (30, 30, 95, 95)[i], restart_interval='row', optimize=True, layout=layout)
                        for i in range(4)]


def test_refusals_that_need_no_device(clips):
    from istvt_amd import ops
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 8, 8]] * 2, dtype=torch.int32)
    for bad in ('411', 'gray', 1, ('422',)):
        with pytest.raises(ValueError, match="jpeg_encode_u8: layout must be one of '420', '444', '422', 'grey', got"):
            ops.jpeg_encode_u8(x, 50, layout=bad)
        with pytest.raises(ValueError, match='jpeg_encode_u8: layout must be one of'):
            ops.encode_frames(x, 8, boxes=boxes, layout=bad)
        with pytest.raises(ValueError, match='jpeg_encode_host: layout must be one of'):
            clips.jpeg_encode_host(x[0], 50, layout=bad)
        with pytest.raises(ValueError, match='jpeg_header: layout must be one of'):
            clips.jpeg_header(16, 24, 50, layout=bad)
        with pytest.raises(ValueError, match='jpeg_restart_interval: layout must be one of'):
            clips.jpeg_restart_interval('row', 24, layout=bad)
    for layout in ('422', 'grey', '420', '444'):
        text = "layout='%s' takes the place of subsampling: leave subsampling at its default, got '444'" % layout
        with pytest.raises(ValueError, match='jpeg_encode_u8: ' + text):
            ops.jpeg_encode_u8(x, 50, '444', layout=layout)
        with pytest.raises(ValueError, match='jpeg_encode_u8: ' + text):
            ops.encode_frames(x, 8, boxes=boxes, subsampling='444', layout=layout)
        with pytest.raises(ValueError, match='jpeg_encode_host: ' + text):
            clips.jpeg_encode_host(x[0], 50, '444', layout=layout)
        with pytest.raises(ValueError, match='jpeg_header: ' + text):
            clips.jpeg_header_bound(16, 24, '444', layout=layout)
        with pytest.raises(ValueError, match='jpeg_encode_host: ' + text):
            clips.jpeg_encode_files_host(x, 50, '444', layout=layout)
    with pytest.raises(ValueError, match="subsampling must be '420' or '444', got '422'"):      # the name stays refused there
        ops.jpeg_encode_u8(x, 50, '422')
    for layout in ('422', 'grey'):
        for bad in (-1, 65536):
            with pytest.raises(ValueError, match='restart interval must lie in .0, 65535.'):
                ops.jpeg_encode_u8(x, 50, restart_interval=bad, layout=layout)
        with pytest.raises(ValueError, match='quality'):
            ops.jpeg_encode_u8(x, 0, layout=layout)
        with pytest.raises(RuntimeError, match='must be on a ROCm device'):
            ops.jpeg_encode_u8(x, 50, layout=layout)              # sound arguments on the host: no fallback


def test_entry_point_declared_and_bound(clips):
    import ctypes

    from istvt_amd import _lib, frames
    assert _lib.SIGNATURES['istvt_jpeg_encode_layout_u8'] == [ctypes.POINTER(_lib.JpegEncodeArgs), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert hasattr(_lib.lib(), 'istvt_jpeg_encode_layout_u8')
    assert clips.JPEG_LAYOUT_CODES['422'] == 1 and clips.JPEG_LAYOUT_CODES['grey'] == 2
    for fn in (frames.jpeg_encode_u8, frames.encode_frames, clips.jpeg_encode_host, clips.jpeg_encode_files_host, clips.jpeg_header,
               clips.jpeg_header_bound, clips.jpeg_restart_interval):
        assert inspect.signature(fn).parameters['layout'].default is None, fn.__name__
    assert 'layout' not in inspect.signature(clips.jpeg_roundtrip_host).parameters
    assert max(len(line) for line in frames.jpeg_encode_u8.__doc__.splitlines()) <= 128
    key = (16, 24, '420', 0, 'cpu', 'grey')
    frames._JPEG_HEADERS.pop(key, None)
    header, hlen = frames._jpeg_header_on(torch.device('cpu'), 16, 24, '420', 0, 'grey')
    assert key in frames._JPEG_HEADERS and hlen == len(clips.jpeg_header(16, 24, 50, layout='grey')) == header.numel()
    assert hlen + 10 == frames._jpeg_header_on(torch.device('cpu'), 16, 24, '420', 0)[1]      # SOF0 and SOS name one component


def test_the_host_tool_builds_and_passes(tmp_path):
    """tools/jpeg_entropy_layout_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it) on the
    recorded scans"""
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'jpeg_entropy_layout_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'jpeg_entropy_layout_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), os.path.join(GOLDEN, 'J5_jpeg_encode_layouts_scans.txt')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == 'ok', r.stdout + r.stderr
    assert 'scans: 16 of 16 equal' in r.stdout and len(r.stdout.splitlines()) == 4
