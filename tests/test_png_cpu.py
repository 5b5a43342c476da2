"""PNG files (DESIGN.md "PNG files") without a device: clips.png_decode_host against PIL's recorded pixels of the files PIL
wrote (tests/golden/png); the host writer and every filter type on every row position; every refusal of clips.png_parse; IDAT
splits; the pure-Python inflate against zlib; the plain build of tools/png_inflate_check.cpp on the vectors the definition
writes, the damaged streams among them; the batch's layout; the ABI row."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_streams as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def golden(golden_dir):
    d = os.path.join(golden_dir, 'png')
    px = np.load(os.path.join(d, 'pixels.npz'))
    return [(n, open(os.path.join(d, n + '.png'), 'rb').read(), px['rgb_' + n]) for n in px['names'].tolist()]


def test_pil_files(clips, golden):
    assert len(golden) == 15
    kinds = set()
    for name, data, rgb in golden:
        hd = clips.png_parse(data)
        kinds.add((hd.colour_type, hd.bpp))
        assert (hd.H, hd.W) == rgb.shape[:2] and hd.raw_bytes == hd.H * (1 + hd.W * hd.bpp), name
        got, status = clips.png_decode_host(data, return_status=True)
        assert status == 0 and got.dtype == torch.uint8 and np.array_equal(got.numpy(), rgb), name
    assert kinds == {(0, 1), (2, 3), (6, 4)}


def test_every_filter_on_every_row(clips):
    """5 x 5 rows: file k has type (r + k) % 5 on row r, so every type stands on every row, first row included"""
    for ch in P.CHANNELS:
        x = P.pattern(5, 7, ch, 7 + ch)
        want = np.repeat(x[:, :, None], 3, 2) if ch == 1 else x[:, :, :3]
        seen = set()
        for k in range(5):
            filters = [(r + k) % 5 for r in range(5)]
            data = clips.png_encode_host(x, filters=filters)
            hd = clips.png_parse(data)
            rows = np.frombuffer(zlib.decompress(hd.data, -15), np.uint8).reshape(5, -1)
            assert rows[:, 0].tolist() == filters
            seen.update(enumerate(filters))
            assert np.array_equal(clips.png_decode_host(data).numpy(), want), (ch, k)
        assert len(seen) == 25
    # a tensor is taken as an array is; the default is type 0 on every row; a one-pixel image
    t = torch.from_numpy(P.pattern(3, 4, 3, 1))
    assert torch.equal(clips.png_decode_host(clips.png_encode_host(t)), t)
    assert clips.png_decode_host(clips.png_encode_host(np.array([[200]], np.uint8), filters=[4])).tolist() == [[[200] * 3]]
    with pytest.raises(ValueError, match=r'png_encode_host: filters holds one type 0..4 per row \(3 rows\)'):
        clips.png_encode_host(t, filters=[0, 5, 0])
    with pytest.raises(ValueError, match='png_encode_host: a uint8'):
        clips.png_encode_host(t.float())


def test_stream_kinds_and_idat_splits(clips):
    x = P.pattern(9, 11, 3, 3)
    first = {0: 0, 1: 1, 2: 2}                                     # BTYPE of the first block: stored, fixed, dynamic
    for (level, strategy), kind in zip(P.KINDS[:3], (0, 1, 2)):
        hd = clips.png_parse(clips.png_encode_host(x, level=level, strategy=strategy))
        assert (hd.data[0] >> 1) & 3 == first[kind]
    whole = clips.png_encode_host(x, filters=[4] * 9)
    for k in (1, 2, 3, 7):
        split = clips.png_encode_host(x, filters=[4] * 9, idat=k)
        assert split.count(b'IDAT') == -(-(len(clips.png_parse(whole).data) + 6) // k) and split != whole
        assert clips.png_parse(split).data == clips.png_parse(whole).data
        assert np.array_equal(clips.png_decode_host(split).numpy(), x)


def _chunk(kind, body):
    return len(body).to_bytes(4, 'big') + kind + body + zlib.crc32(kind + body).to_bytes(4, 'big')


def _file(ihdr=None, idat=True, iend=True, extra=b'', stream=None, H=2, W=3, depth=8, ct=2, lace=0):
    body = (W.to_bytes(4, 'big') + H.to_bytes(4, 'big') + bytes([depth, ct, 0, 0, lace])) if ihdr is None else ihdr
    stream = zlib.compress(bytes(H * (1 + 3 * W))) if stream is None else stream
    return (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', body) + extra + (_chunk(b'IDAT', stream) if idat else b'')
            + (_chunk(b'IEND', b'') if iend else b''))


def test_refusals(clips):
    good = _file()
    assert clips.png_parse(good).H == 2 and clips.png_decode_host(good).shape == (2, 3, 3)
    # ancillary chunks, and a PLTE in an RGB file, are skipped
    assert clips.png_parse(_file(extra=_chunk(b'tEXt', b'a\0b') + _chunk(b'PLTE', bytes(9)) + _chunk(b'gAMA', bytes(4)))).W == 3
    z = zlib.compress(bytes(8))
    cases = [
        (b'\x89PNX' + good[4:], 'the file does not start with the PNG signature'),
        (_file(depth=16), '16-bit samples are not decoded'),
        (_file(depth=4, ct=0), '4-bit samples are not decoded'),
        (_file(depth=1, ct=0), '1-bit samples are not decoded'),
        (_file(ct=3), r'palette images \(colour type 3\) are not decoded'),
        (_file(ct=4), r'grey \+ alpha images \(colour type 4\) are not decoded'),
        (_file(lace=1), 'Adam7 interlaced files are not decoded'),
        (good[:45] + bytes([good[45] ^ 1]) + good[46:], 'chunk IDAT at byte 33 has a bad CRC-32'),
        (_file(iend=False), 'the file has no IEND'),
        (_file(idat=False), 'the file has no IDAT'),
        (_file(H=0), r'sides of 1..16384, got 0 x 3'),
        (_file(W=0), r'sides of 1..16384, got 2 x 0'),
        (_file(H=16385), r'sides of 1..16384, got 16385 x 3'),
        (_file(W=16385), r'sides of 1..16384, got 2 x 16385'),
        (_file(stream=b'\x79\x9c' + z[2:]), 'a bad zlib header'),             # method 9
        (_file(stream=b'\x88\x1c' + z[2:]), 'a bad zlib header'),             # a 64 KiB window
        (_file(stream=b'\x78\xbb' + z[2:]), 'a bad zlib header'),             # a preset dictionary
        (_file(stream=b'\x78\x9d' + z[2:]), 'a bad zlib header'),             # the check bits
        (_file(extra=_chunk(b'ABCD', b'')), 'critical chunk ABCD is not known'),
        (good[:-5], 'reaches past the end of the file'),
        (_file(ct=0, extra=_chunk(b'PLTE', bytes(9)), stream=zlib.compress(bytes(2 * 4))), r'a PLTE chunk in a grey file'),
        (good[:-12] + _chunk(b'tEXt', b'a\0b') + _chunk(b'IDAT', b'') + good[-12:], 'IDAT chunks at byte %d that do not follow one another' % (len(good) - 12 + 15)),
    ]
    for data, text in cases:
        with pytest.raises(ValueError, match='png_parse: .*' + text):
            clips.png_parse(data)
    with pytest.raises(ValueError, match='png_batch: an empty batch'):
        clips.png_batch([])
    with pytest.raises(ValueError, match='png_parse: .*Adam7'):
        clips.png_batch([good, _file(lace=1)])


def test_python_inflate_equals_zlib(clips):
    """on every valid stream of the GPU tests: the files of the filter test and the streams zlib does not write"""
    files = P.filter_files(clips.png_encode_host)
    assert len(files) == 20
    for name, f in files:
        hd = clips.png_parse(f)
        out, status = clips._png_inflate(hd.data, hd.raw_bytes)
        assert status == 0 and bytes(out) == zlib.decompress(hd.data, -15), name
    special = P.special_streams()
    assert len(special) == 9
    for name, raw, data in special:
        out, status = clips._png_inflate(raw, P.TOTAL)
        assert status == 0 and bytes(out) == data == zlib.decompress(raw, -15), name
        frame, status = clips.png_decode_host(clips.png_wrap(P.H, P.W, 2, P.zlib_wrap(raw, data)), return_status=True)
        want = clips._png_unfilter(np.frombuffer(data, np.uint8).reshape(P.H, -1), 3).reshape(P.H, P.W, 3)
        assert status == 0 and np.array_equal(frame.numpy(), want), name


def test_damaged_streams(clips):
    damaged = P.damaged_streams()
    assert [s for _, _, s in damaged] == [1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 6]
    for name, raw, want in damaged:
        frame, status = clips.png_decode_host(clips.png_wrap(P.H, P.W, 2, P.zlib_wrap(raw)), return_status=True)
        assert status == want and tuple(frame.shape) == (P.H, P.W, 3) and not bool(frame.any()), name
    # zlib decodes the one-code literal tree; the definition's status is its own inflate's, as the device's is
    name, raw, want = damaged[6]
    assert name == 'one_code_literal_tree' and want == 3 and len(zlib.decompress(raw, -15)) == P.TOTAL
    with pytest.raises(ValueError, match=r'png_decode: file 1 is damaged \(status 4: a distance beyond the bytes produced\)'):
        clips.check_png_status(torch.tensor([0, 4, 1], dtype=torch.int32))
    clips.check_png_status(torch.zeros(3, dtype=torch.int32))
    assert sorted(clips.PNG_STATUS) == [1, 2, 3, 4, 5, 6]


def test_the_checker_built_plain(clips, tmp_path):
    """csrc/png_inflate.h on the host, one lane, against the definition on 91 vectors; DESIGN.md "PNG files" records the same
    program's run under AddressSanitizer and UBSan"""
    from istvt_amd import build
    vectors = tmp_path / 'png_vectors.txt'
    done = P.write_vectors(str(vectors), clips)
    assert len(done) == 91 and {s for _, s in done} == {0, 1, 2, 3, 4, 5}
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_inflate_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_inflate_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'png_inflate_check: 91 cases agree', r.stdout + r.stderr
    # the check can fail: a vector with another status
    lines = vectors.read_text().splitlines()
    name, status, rest = lines[0].split(' ', 2)
    (tmp_path / 'wrong.txt').write_text('%s %d %s\n' % (name, 4, rest))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'status 0, the definition has 4' in r.stdout


def test_batch_layout(clips, golden):
    files = [d for _, d, _ in golden[:4]] + [clips.png_encode_host(P.pattern(1, 1, 3, 0))]
    b = clips.png_batch(files)
    heads = [clips.png_parse(f) for f in files]
    assert b.n == 5 and b.images.dtype == torch.int32 and tuple(b.images.shape) == (5, clips.PNG_IMAGE_INTS)
    assert b.sizes == [(h.H, h.W) for h in heads]
    assert b.raw_stride % 16 == 0 and 0 <= b.raw_stride - max(h.raw_bytes for h in heads) < 16
    assert b.scratch_bytes == 5 * b.raw_stride and b.raw_bytes == sum(h.raw_bytes for h in heads)
    data = bytes(b.data.numpy().tobytes())
    assert b.nbytes == len(data) and b.nbytes % 16 == 0
    for row, h in zip(b.images.tolist(), heads):
        assert row[:4] == [h.H, h.W, h.colour_type, h.bpp] and row[4] % 16 == 0 and row[6:] == [0, 0]
        assert data[row[4]:row[5]] == h.data
    assert clips.png_batch(heads).images.tolist() == b.images.tolist()      # parsed files are taken as they are


def test_entry_point_declared_and_bound(clips):
    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        text = fh.read()
    assert H.defines(text)['ISTVT_PNG_IMAGE_INTS'] == clips.PNG_IMAGE_INTS == 8
    assert H.defines(text)['ISTVT_PNG_MAX_BYTES'] == clips.PNG_MAX_BYTES == 2 ** 31 - 4096
    assert H.prototypes(text)['istvt_png_decode_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'raw_stride')]
    assert _lib.SIGNATURES['istvt_png_decode_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs), ctypes.c_int]
    assert ctypes.c_void_p not in _lib.SIGNATURES['istvt_png_decode_u8']
    assert ops.png_decode_u8 is frames.png_decode_u8 and ops.decode_frames is frames.decode_frames
    assert _lib.lib().istvt_png_decode_u8(None, 16) == -3                    # no block: refused, nothing launched
    args = _lib.JpegDecodeArgs(n=1, Hc=8, Wc=8)
    assert _lib.lib().istvt_png_decode_u8(ctypes.byref(args), 16) == -3      # null pointers
    # the refusals that need no device
    with pytest.raises(RuntimeError, match='png_decode_u8: empty input'):
        ops.png_decode_u8([])
    with pytest.raises(TypeError, match='png_decode_u8 expects a sequence of files'):
        ops.png_decode_u8(b'\x89PNG')
    with pytest.raises(RuntimeError, match='png_decode_u8: checked=True takes a clips.PngBatch'):
        ops.png_decode_u8([b''], checked=True)
    batch = clips.png_batch([clips.png_encode_host(P.pattern(4, 4, 3, 0))])
    for kw in (dict(split=128), dict(split='auto'), dict(layouts='all')):
        with pytest.raises(ValueError, match='decode_frames: split= and layouts= go with JPEG files; a clips.PngBatch takes neither'):
            ops.decode_frames(batch, 32, **kw)
